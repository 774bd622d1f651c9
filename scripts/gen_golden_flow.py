"""Writes tests/golden/flow.npz from the reference's own detectron2/geometry/camera.py (run on the CPU, unmodified): img_to_points into
points_to_img, the way its view_synthesis chains them (L172-180).

Usage: python scripts/gen_golden_flow.py   (needs the reference checkout named by oracle.ref_harness; not used on the GPU machine)

Two cases, B = 2, 10 x 16, float32, the inputs of tests/flow_ref.py's conventions (depth in [2, 60] m, |t + m| <= 1.5 m, rotations <= 3 degrees):
  rigid_*   one translation per sample                    (t [B,3,1])
  motion_*  a per-pixel translation t + m                 (t [B,3,H*W], the sum formed in float32)
Arrays per case: depth [B,1,H,W], K [B,3,3], T [B,4,4], motion [B,3,H,W] (motion case), and what the reference computed from them:
points [B,3,H,W] = img_to_points(depth, inv_intrinsics(K), 0), KR = K R, Kt = K t, and points_to_img(points, KR, Kt) = coords [B,H,W,2],
Z [B,H,W,1], mask [B,H,W,1].
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness  # noqa: E402
import flow_ref as FR  # noqa: E402

B, H, W = 2, 10, 16


def main():
    ref_harness.load()
    C = importlib.import_module("detectron2.geometry.camera")
    rng = np.random.default_rng(24)
    out = {}
    for case in ("rigid", "motion"):
        depth = torch.from_numpy(rng.uniform(2.0, 60.0, (B, 1, H, W)).astype(np.float32))
        K = torch.from_numpy(FR.intrinsics(B, H, W))
        T = torch.from_numpy(np.stack([FR.pose([1.0, -2.5, 0.5], [0.2, -0.05, -1.0]), FR.pose([-0.5, 3.0, -1.0], [-0.3, 0.1, 0.9])]))
        R, t = T[:, :3, :3].contiguous(), T[:, :3, 3:].contiguous()
        rec = dict(depth=depth, K=K, T=T)
        if case == "motion":
            rec["motion"] = torch.from_numpy(rng.uniform(-0.23, 0.23, (B, 3, H, W)).astype(np.float32))
            t = t + rec["motion"].view(B, 3, H * W)
        points = C.img_to_points(depth, C.inv_intrinsics(K), torch.zeros(B, 3, 1))
        KR, Kt = K.bmm(R), K.bmm(t)
        coords, Z, mask = C.points_to_img(points, KR, Kt)
        rec.update(points=points, KR=KR, Kt=Kt, coords=coords, Z=Z, mask=mask)
        out.update({f"{case}_{k}": v.numpy() for k, v in rec.items()})
    path = os.path.join(ROOT, "tests", "golden", "flow.npz")
    np.savez(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes): " + ", ".join(f"{k} {v.shape}" for k, v in out.items()))


if __name__ == "__main__":
    main()

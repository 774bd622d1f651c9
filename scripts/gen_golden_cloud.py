"""Writes tests/golden/cloud.npz from the reference's own detectron2/geometry/camera.py (run on the CPU, unmodified).

Usage: python scripts/gen_golden_cloud.py   (needs the reference checkout named by oracle.ref_harness; not used on the GPU machine)

B = 2, 5 x 7, float32.  Arrays:
  K, K_inv              intrinsics [B,3,3] with a non-zero skew and a last row that is not (0, 0, 1) -- inv_intrinsics leaves those entries alone
  grid                  image_grid(B, 5, 7, float32, cpu) [B,3,5,7]
  depth, R, t1, tp      the inputs of img_to_points: depth [B,1,5,7], a general R [B,3,3], t [B,3,1] and t [B,3,35]
  points_t1, points_tp  img_to_points(depth, R, t1 / tp) [B,3,5,7]
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402

B, H, W = 2, 5, 7


def main():
    ref_harness.load()
    C = importlib.import_module("detectron2.geometry.camera")
    g = torch.Generator().manual_seed(20)
    K = torch.tensor([[[721.5, 0.3, 3.2], [0.0, 715.25, 2.4], [0.0, 0.0, 1.0]], [[500.0, -0.7, 2.9], [0.1, 480.5, 1.6], [0.2, 0.0, 1.5]]])
    depth = torch.rand(B, 1, H, W, generator=g) * 60 + 1
    R = torch.randn(B, 3, 3, generator=g)
    t1 = torch.randn(B, 3, 1, generator=g)
    tp = torch.randn(B, 3, H * W, generator=g)
    out = dict(K=K, K_inv=C.inv_intrinsics(K), grid=C.image_grid(B, H, W, torch.float32, torch.device("cpu")), depth=depth, R=R, t1=t1, tp=tp,
               points_t1=C.img_to_points(depth, R, t1), points_tp=C.img_to_points(depth, R, tp))
    path = os.path.join(ROOT, "tests", "golden", "cloud.npz")
    np.savez(path, **{k: v.numpy() for k, v in out.items()})
    print(f"wrote {path}: " + ", ".join(f"{k} {tuple(v.shape)}" for k, v in out.items()))


if __name__ == "__main__":
    main()

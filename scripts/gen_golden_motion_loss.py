"""Writes tests/golden/motion_loss.npz from the reference's own loss code (run on the CPU, unmodified).

Usage: python scripts/gen_golden_motion_loss.py   (needs the reference checkout named by oracle.ref_harness; not used on the GPU machine)

Every case of tests/motion_loss_init.py CASES = (size, C1, C2, depth_l1_w) runs MotionLearningModel.rgbd_consistency_loss (unbound, on a namespace that
carries the loss weights and WeightedSSIM(C1, C2)) for frame 1 -> 2 and motion_consistency_loss on its coords / occlusion mask, in fp32 (the golden
values) and in fp64 (their error bars).  The objective is the sum of all returned losses.  Contents (arrays and name lists only):
  case{k}_{rgb_l1_loss,ssim_loss,depth_l1_loss,rot_error,trans_error}   fp32 losses
  case{k}_coords, _dpw                       coords_A_in_B / depth_proximity_weight (small size: full; 128 x 416: the rows motion_loss_init.FULL_ROWS);
                                             like g_t21 they do not depend on (C1, C2, depth_l1_w) and are kept for the first case of each size only
  case{k}_occ, _occ_shape                    np.packbits of the occlusion mask
  case{k}_g_{depth,t12,t21,R12,R21}          fp32 gradients (maps of the 128 x 416 cases: the rows FULL_ROWS), case{k}_gn_*: their norms
  case{k}_d_*                                the reference's own fp32-vs-fp64 difference of each of the above (tensors: max |a - b| / max |b|;
                                             losses and norms: |a - b| / |b|)
Asserted here: the occlusion mask of the two runs differs on at most 0.1 % of the pixels, and at most 0.1 % of the elements of a gradient map differ by
more than 3e-3 * max (the caps the GPU tests apply to the HIP path)."""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness  # noqa: E402
import motion_loss_init as MI  # noqa: E402

LOSSES = ("rgb_l1_loss", "ssim_loss", "depth_l1_loss", "rot_error", "trans_error")
GRADS = ("depth", "t12", "t21", "R12", "R21")


def rel_t(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


def run(ML, MLoss, SS, inp, C1, C2, dl1_w, dt):
    v = {k: x.detach().clone().to(dt) for k, x in inp.items()}
    for k in ("depth1", "t12", "t21", "R12", "R21"):
        v[k].requires_grad_(True)
    ns = types.SimpleNamespace(depth_l1_loss_w=dl1_w, ssim_loss_w=MI.SSIM_W, ssim=SS.WeightedSSIM(C1, C2))
    o = ML.MotionLearningModel.rgbd_consistency_loss(ns, v["frame1"], v["frame2"], v["depth1"], v["depth2"], v["K"], v["R12"], v["t12"])
    rot, trans = MLoss.motion_consistency_loss(o["coords_A_in_B"], o["occlusion_mask"], v["R12"], v["R21"], v["t12"], v["t21"])
    o["rot_error"], o["trans_error"] = rot, trans
    sum(o[k] for k in LOSSES if k in o).backward()
    res = {k: o[k].detach() for k in LOSSES if k in o}
    res.update(coords=o["coords_A_in_B"].detach(), occ=o["occlusion_mask"].detach(), dpw=o["depth_proximity_weight"].detach())
    res.update(g_depth=v["depth1"].grad, g_t12=v["t12"].grad, g_t21=v["t21"].grad, g_R12=v["R12"].grad, g_R21=v["R21"].grad)
    return res


def main():
    ref_harness.load()
    SS = importlib.import_module("detectron2.modeling.losses.ssim_loss")
    MLoss = importlib.import_module("detectron2.modeling.losses.motion_loss")
    ML = importlib.import_module("detectron2.modeling.meta_arch.MotionLearning")
    out = {}
    for ci, (size, C1, C2, dl1_w) in enumerate(MI.CASES):
        N, H, W = MI.SIZES[size]
        inp = MI.inputs(N, H, W)
        a, b = run(ML, MLoss, SS, inp, C1, C2, dl1_w, torch.float32), run(ML, MLoss, SS, inp, C1, C2, dl1_w, torch.float64)
        p = f"case{ci}_"
        rows = (lambda t, dim: t) if size == "small" else (lambda t, dim: t.index_select(dim, torch.tensor(MI.FULL_ROWS)))
        for k in LOSSES:
            if k in a:
                out[p + k] = np.float64(a[k].item())
                out[p + "d_" + k] = np.float64(abs(a[k].item() - b[k].item()) / abs(b[k].item()))
        flips = float((a["occ"] != b["occ"].float()).double().mean())
        assert flips <= 1e-3, (ci, flips)
        out[p + "occ"] = np.packbits(a["occ"].numpy().astype(np.uint8).reshape(-1))
        out[p + "occ_shape"] = np.array(a["occ"].shape)
        shared = ci == MI.first_case(size)        # coords, the weight and the t21 gradient do not depend on (C1, C2, depth_l1_w): kept once per size
        out[p + "d_coords"], out[p + "d_dpw"] = np.float64(rel_t(a["coords"], b["coords"])), np.float64(rel_t(a["dpw"], b["dpw"]))
        if shared:
            out[p + "coords"], out[p + "dpw"] = rows(a["coords"], 1).numpy(), rows(a["dpw"], 2).numpy()
        worst = 0.0
        for k in GRADS:
            ga, gb = a["g_" + k], b["g_" + k]
            off = float(((ga.double() - gb).abs() > 3e-3 * gb.abs().max()).double().mean())
            worst = max(worst, off)
            assert off <= 1e-3, (ci, k, off)
            if shared or k != "t21":
                out[p + "g_" + k] = (rows(ga, 2) if ga.dim() == 4 else ga).numpy()
            out[p + "d_g_" + k] = np.float64(rel_t(ga, gb))
            na, nb = ga.double().norm().item(), gb.norm().item()
            out[p + "gn_" + k], out[p + "d_gn_" + k] = np.float64(na), np.float64(abs(na - nb) / nb)
        print(f"case {ci} {size} C1={C1} C2={C2} dl1_w={dl1_w}: occ {100 * a['occ'].mean().item():.1f} % flips {flips:.1e} off-tolerance grads {worst:.1e} "
              + " ".join(f"d_{k} {out[p + 'd_' + k]:.1e}" for k in LOSSES if p + k in out)
              + " " + " ".join(f"d_g_{k} {out[p + 'd_g_' + k]:.1e} d_gn_{k} {out[p + 'd_gn_' + k]:.1e}" for k in GRADS))
    path = os.path.join(ROOT, "tests", "golden", "motion_loss.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

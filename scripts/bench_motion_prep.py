"""pair_prep (sde_motion_prep_fwd / _bwd) alone at the reference setting: N = 32 (batch 16, both directions), 128x416 -> 128x416, fp32, with a motion field,
with and without scale_normalize, plus dilate_mask (d = 8).  Runs each a few times; meant to be run under a kernel trace for the per-kernel times
(rocprofv3 --kernel-trace --stats -- python scripts/bench_motion_prep.py), and prints event-timed ms per forward + backward as one JSON line.

    python scripts/bench_motion_prep.py [--reps R] [--b B] [--height H] [--width W]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--b", type=int, default=16)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=416)
    a = ap.parse_args()
    from simpledepthestimation_amd.hip import motion_loss as HM
    N, H, W = 2 * a.b, a.height, a.width
    g = torch.Generator().manual_seed(0)
    depth = (torch.rand(N, 1, H, W, generator=g) * 30 + 2).cuda().requires_grad_(True)
    motion = (torch.randn(N, 3, H, W, generator=g) * 0.2).cuda().requires_grad_(True)
    t_pose = (torch.randn(N, 3, generator=g) * 0.3).cuda().requires_grad_(True)
    mask = (torch.rand(N, 1, H, W, generator=g) > 0.9).float().cuda()
    cot = {k: torch.randn(N, c, H, W, generator=g).cuda() for k, c in (("depth_r", 1), ("depth_n", 1), ("t", 3), ("m_norm", 3), ("t_sw", 3))}
    line = {"workload": "pair_prep", "n": N, "size": [H, W], "reps": a.reps}
    for normalize in (False, True):
        def step():
            o = HM.pair_prep(depth, motion, t_pose, None, (H, W), normalize)
            outs = [o[k] for k in cot if not (k == "depth_n" and not normalize)]
            torch.autograd.backward(outs, [cot[k] for k in cot if not (k == "depth_n" and not normalize)])
        for _ in range(3):
            step()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            step()
        e1.record()
        torch.cuda.synchronize()
        line["normalize" if normalize else "plain"] = {"fwd_bwd_ms": round(e0.elapsed_time(e1) / a.reps, 4)}
    HM.dilate_mask(mask, 8)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        HM.dilate_mask(mask, 8)
    e1.record()
    torch.cuda.synchronize()
    line["dilate_d8_ms"] = round(e0.elapsed_time(e1) / a.reps, 4)
    print(json.dumps(line))


if __name__ == "__main__":
    main()

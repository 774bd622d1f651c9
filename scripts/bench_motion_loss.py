"""The MotionLearning loss stack at the reference setting: batch 16 in both directions stacked along the batch (N = 32), 128x416, fp32, C1 = inf, C2 = 9e-6,
SSIM weight 3, depth-L1 weight 1, per-pixel motion field; forward + backward of RGB-D consistency + motion consistency + motion smoothness + sparsity.
Prints one JSON line.

    python scripts/bench_motion_loss.py [--reps R] [--runs K] [--b B] [--height H] [--width W] [--no-profile]

Two implementations of the same math on the same device: "hip" (this package's fused kernels) and "torch" (tests/motion_loss_ref.py, the plain-torch
composition, in fp32).  Per implementation: ms per call (median over K runs of the mean of R warm calls, events), and from one profiled call the
summed GPU kernel time and the number of kernel launches; for "hip" the launches of the package's own kernels are listed by name.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

INF = float("inf")
SSIM_W, DL1_W, C1, C2 = 3.0, 1.0, INF, 9e-6


def make(B, H, W):
    import motion_loss_init as MI
    v = {k: x.cuda() for k, x in MI.inputs(B, H, W).items()}
    cat = lambda a, b: torch.cat([v[a], v[b]], 0).contiguous()
    s = {"fA": cat("frame1", "frame2"), "fB": cat("frame2", "frame1"), "dA": cat("depth1", "depth2"), "dB": cat("depth2", "depth1"), "K": cat("K", "K"),
         "R": cat("R12", "R21"), "t": cat("t12", "t21")}
    for k in ("dA", "R", "t"):
        s[k].requires_grad_(True)
    return s


def step(impl, s):
    for k in ("dA", "R", "t"):
        s[k].grad = None
    if impl == "hip":
        from simpledepthestimation_amd.modeling import losses as ML
        o = ML.rgbd_consistency_loss(s["fA"], s["fB"], s["dA"], s["dB"], s["K"], s["R"], s["t"], depth_l1_w=DL1_W, ssim_w=SSIM_W, C1=C1, C2=C2)
        mcl, smooth, sparse = ML.motion_consistency_loss, ML.motion_smoothness_loss_fn, ML.motion_sparsity_loss_fn
    else:
        import motion_loss_ref as REF
        o = REF.rgbd_consistency_loss(s["fA"], s["fB"], s["dA"], s["dB"], s["K"], s["R"], s["t"], DL1_W, SSIM_W, C1, C2)
        mcl, smooth, sparse = REF.motion_consistency_loss, REF.motion_smoothness_loss_fn, REF.motion_sparsity_loss_fn
    # the inverse-direction fields of the stacked batch are the same tensors with the halves swapped: both get gradients, as in the model
    N = s["t"].shape[0]
    tinv, Rinv = torch.cat([s["t"][N // 2:], s["t"][:N // 2]], 0), torch.cat([s["R"][N // 2:], s["R"][:N // 2]], 0)
    rot, trans = mcl(o["coords_A_in_B"], o["occlusion_mask"], s["R"], Rinv, s["t"], tinv)
    loss = o["rgb_l1_loss"] + o["ssim_loss"] + o["depth_l1_loss"] + rot + trans + smooth(s["t"]) + sparse(s["t"])
    loss.backward()
    return loss


def _time(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def profile(fn):
    from torch.profiler import ProfilerActivity, profile as prof
    fn(); torch.cuda.synchronize()
    with prof(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as p:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in p.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    names = {}
    for e in ev:
        names[e.name] = names.get(e.name, 0) + 1
    own = {k.split("(anonymous namespace)::")[1].split("(")[0]: n for k, n in names.items() if k.startswith("(anonymous namespace)::")}
    return {"gpu_kernel_ms": round(sum(e.device_time for e in ev) / 1e3, 3), "launches": len(ev), "package_kernels": own}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--b", type=int, default=16)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=416)
    ap.add_argument("--no-profile", action="store_true")
    a = ap.parse_args()
    s = make(a.b, a.height, a.width)
    line = {"workload": "motion_loss_stack", "n": 2 * a.b, "size": [a.height, a.width], "C1": "inf", "C2": C2, "ssim_w": SSIM_W, "depth_l1_w": DL1_W, "reps": a.reps,
            "runs": a.runs}
    for impl in ("hip", "torch"):
        times = [_time(lambda: step(impl, s), a.reps) for _ in range(a.runs)]
        loss = step(impl, s)
        torch.cuda.synchronize()
        line[impl] = {"fwd_bwd_ms": round(statistics.median(times), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3), "loss": float(loss),
                      "finite": bool(all(torch.isfinite(s[k].grad).all() for k in ("dA", "R", "t")))}
        if not a.no_profile:
            try:
                line[impl].update(profile(lambda: step(impl, s)))
            except Exception as e:       # the timing above stands without the profiler
                line[impl]["profile_error"] = repr(e)[:200]
    line["speedup"] = round(line["torch"]["fwd_bwd_ms"] / line["hip"]["fwd_bwd_ms"], 2)
    print(json.dumps(line))


if __name__ == "__main__":
    main()

"""GoogleMotionNet (projects/MotionLearning/configs/Base.yaml's pose net) forward + backward at the reference setting: N = 32 (batch 16 in both
frame orders), 128x416, bf16, GROUP_NORM off and on, eager.  Prints one JSON line.

    python scripts/bench_motion.py [--reps R] [--runs K] [--n N] [--dtype bf16|fp32] [--no-kernels] [--no-tail-levels] [--steps-only S]

Per configuration: the median over K runs of the mean of R warm forward + backward calls (events).  Also times every new kernel on its largest
map (refiner0: 8 skip channels at 128x416, the field resized from 64x208) with the bytes it must move at least, and, per refiner level, the
pointwise tail (forward + backward) next to the same arithmetic on the convolution engine (cat -> 1x1 conv -> add).
--steps-only S: just S forward + backward calls of the GROUP_NORM-off network (for a kernel trace).
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


def make(n, H, W, dtype, group_norm):
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.modeling.pose_net import build_pose_net
    cfg = get_cfg()
    pn = cfg.MODEL.POSE_NET
    pn.NAME, pn.GROUP_NORM, pn.SCALE_CONSTRAIN, cfg.MODEL.COMPUTE_DTYPE = "GoogleMotionNet", group_norm, "clip_ste", dtype
    torch.manual_seed(0)
    net = build_pose_net(cfg).cuda().train()
    g = torch.Generator().manual_seed(0)
    x = torch.rand(n, 8, H, W, generator=g).cuda().requires_grad_(True)
    return net, x


def step(net, x):
    net.zero_grad(set_to_none=True)
    x.grad = None
    out = net({"pose_net_input": x})
    (out["motion_pred"].sum() + out["pose_pred"].sum()).backward()
    return out


def _time(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3      # microseconds


def _entry(shape, us, nbytes):
    return {"shape": list(shape), "us": round(us, 1), "GBps": round(nbytes / us / 1e3, 1)}


def time_kernels(n, H, W, dtype):
    from simpledepthestimation_amd.hip import motion as HM
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    es = 2 if dt == torch.bfloat16 else 4
    P = n * H * W
    res = {}
    field = torch.randn(n, H // 2, W // 2, 4, device="cuda").requires_grad_(True)
    skip = torch.randn(n, H, W, 8, device="cuda").to(dt).requires_grad_(True)
    Cx = 16 if es == 2 else 12
    with torch.no_grad():
        us = _time(lambda: HM.resize_cat(field, skip, 8))
    res["resize_cat_fwd"] = _entry(skip.shape, us, P * (8 * es + Cx * es + 16) + field.numel() * 4)
    xa, xb, up = HM.resize_cat(field, skip, 8)
    ga, gb, gu = torch.randn_like(xa), torch.randn_like(xb), torch.randn_like(up)
    us = _time(lambda: torch.autograd.grad((xa, xb, up), (field, skip), (ga, gb, gu), retain_graph=True))
    res["resize_cat_bwd"] = _entry(skip.shape, us, P * (2 * Cx * es + 16 + 8 * es) + field.numel() * 4)
    o1, o2 = (torch.randn(n, H, W, 8, device="cuda").to(dt).requires_grad_(True) for _ in range(2))
    w3 = torch.randn(3, 16, 1, 1, device="cuda").requires_grad_(True)
    upd = up.detach().requires_grad_(True)
    with torch.no_grad():
        us = _time(lambda: HM.refiner_tail(o1, o2, w3, upd))
    res["tail_fwd"] = _entry(o1.shape, us, P * (16 * es + 32))
    out = HM.refiner_tail(o1, o2, w3, upd)
    go = torch.randn_like(out)
    us = _time(lambda: torch.autograd.grad(out, (o1, o2, w3, upd), go, retain_graph=True))
    res["tail_bwd"] = _entry(o1.shape, us, P * (16 + 32 * es))
    scale = torch.full((), 0.01, device="cuda", requires_grad=True)
    weight = torch.ones(1, device="cuda")
    f0 = out.detach().requires_grad_(True)
    for mask in (True, False):
        with torch.no_grad():
            us = _time(lambda: HM.motion_head(f0, scale, weight, mask))
        res[f"head_fwd_mask{int(mask)}"] = _entry(f0.shape, us, P * ((32 if mask else 16) + 12 + int(mask)))
        mp = HM.motion_head(f0, scale, weight, mask)
        gm = torch.randn_like(mp)
        us = _time(lambda: torch.autograd.grad(mp, (f0, scale), gm, retain_graph=True))
        res[f"head_bwd_mask{int(mask)}"] = _entry(f0.shape, us, P * (12 + 16 + 16 + int(mask)))
    img = torch.rand(n, 8, H, W, device="cuda").requires_grad_(True)
    pa, pb = HM.prep_input_grad(img, dt)
    g1, g2 = torch.randn_like(pa), torch.randn_like(pb)
    us = _time(lambda: torch.autograd.grad((pa, pb), img, (g1, g2), retain_graph=True))
    res["prep_input_bwd"] = _entry(img.shape, us, P * (16 * es + 32))
    return res


def time_tail_levels(n, H, W, dtype):
    """Per refiner level: pointwise tail against cat -> 1x1 conv on the engine -> add, forward + backward, microseconds."""
    from simpledepthestimation_amd.hip import bts as HB
    from simpledepthestimation_amd.hip import motion as HM
    from simpledepthestimation_amd.hip import nn as HN
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    res = {}
    h, w = H, W
    for level, mid in enumerate((8, 16, 32, 64, 128, 256, 512, 1024)):
        if level:
            h, w = (h + 1) // 2, (w + 1) // 2
        o1, o2 = (torch.randn(n, h, w, mid, device="cuda").to(dt).requires_grad_(True) for _ in range(2))
        w3 = (torch.randn(3, 2 * mid, 1, 1, device="cuda") / (2 * mid) ** 0.5).requires_grad_(True)
        up = torch.randn(n, h, w, 4, device="cuda").requires_grad_(True)
        go = torch.randn(n, h, w, 4, device="cuda")

        def pointwise():
            torch.autograd.grad(HM.refiner_tail(o1, o2, w3, up), (o1, o2, w3, up), go)

        def engine():
            y = HN.conv2d(HB.cat([(o1, mid), (o2, mid)]), w3)[..., :4].float() + up
            torch.autograd.grad(y, (o1, o2, w3, up), go)

        res[f"refiner{level}"] = {"map": [h, w], "mid": mid, "pointwise_us": round(_time(pointwise, 10), 1), "engine_us": round(_time(engine, 10), 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=416)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-tail-levels", action="store_true")
    ap.add_argument("--steps-only", type=int, default=0)
    a = ap.parse_args()
    if a.steps_only:
        net, x = make(a.n, a.height, a.width, a.dtype, False)
        for _ in range(a.steps_only):
            step(net, x)
        torch.cuda.synchronize()
        print(json.dumps({"workload": "google_motion_net", "steps": a.steps_only}))
        return
    line = {"workload": "google_motion_net", "dtype": a.dtype, "n": a.n, "size": [a.height, a.width], "graph": False, "reps": a.reps, "runs": a.runs}
    for gn in (False, True):
        net, x = make(a.n, a.height, a.width, a.dtype, gn)
        times = [_time(lambda: step(net, x), a.reps) / 1e3 for _ in range(a.runs)]
        out = step(net, x)
        torch.cuda.synchronize()
        key = "gn_on" if gn else "gn_off"
        line[key] = {"fwd_bwd_ms": round(statistics.median(times), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3),
                     "finite": bool(torch.isfinite(out["motion_pred"]).all() and torch.isfinite(x.grad).all())}
        del net, x, out
        torch.cuda.empty_cache()
    if not a.no_kernels:
        line["kernels"] = time_kernels(a.n, a.height, a.width, a.dtype)
    if not a.no_tail_levels:
        line["tail_levels"] = time_tail_levels(a.n, a.height, a.width, a.dtype)
    print(json.dumps(line))


if __name__ == "__main__":
    main()

"""GoogleResNet-18 (projects/MotionLearning/configs/resnet18.yaml's depth net, RandLayerNorm) trained supervised with SILog: bf16, bs 16,
128x416, hipGraph replay.  Prints one JSON line.

    python scripts/bench_google.py [--steps K] [--warmup W] [--bs B] [--dtype bf16|fp32] [--no-graph] [--no-kernels]

Also times, on the largest maps of that setting, the RandLayerNorm forward / backward (stem output: 64 x H/2 x W/2) and the bilinear x2
up-sampling forward / backward (the last decoder level: 32 -> 16 channels up to H x W), with the bytes each must move at least.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(bs, H, W, dtype, graph):
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.engine.trainer import supervised_trainer
    from simpledepthestimation_amd.modeling import build_model
    cfg = get_cfg()
    cfg.MODEL.META_ARCHITECTURE, cfg.MODEL.DEVICE, cfg.MODEL.COMPUTE_DTYPE = "SupDepthModel", "cuda:0", dtype
    cfg.MODEL.DEPTH_NET.NAME, cfg.MODEL.DEPTH_NET.ENCODER_NAME, cfg.MODEL.DEPTH_NET.NORM = "GoogleResNet", "18", "randLN"
    cfg.SOLVER.DEPTH_LR = 2e-4
    model = build_model(cfg).train()
    tr = supervised_trainer(model, cfg, use_graph=graph)
    g = torch.Generator().manual_seed(0)
    batch = {"img": torch.rand(bs, 3, H, W, generator=g).cuda(), "depth": (torch.rand(bs, 1, H, W, generator=g) * 79 + 1).cuda()}
    return model, tr, batch


def _time(fn, reps=20):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3      # microseconds


def time_kernels(bs, H, W, dtype):
    from simpledepthestimation_amd.hip import google as HG
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    es = 2 if dt == torch.bfloat16 else 4
    res = {}
    # RandLayerNorm + ReLU on the stem output
    y = torch.randn(bs, H // 2, W // 2, 64, device="cuda").to(dt).requires_grad_(True)
    gamma = torch.ones(64, device="cuda", requires_grad=True)
    beta = torch.zeros(64, device="cuda", requires_grad=True)
    z = torch.randn(2, bs, 64, device="cuda")
    s = torch.full((1,), 0.5, device="cuda")
    n = y.numel() * es
    with torch.no_grad():
        us = _time(lambda: HG.rand_layer_norm(y, gamma, beta, z, s, relu=True))
    res["randln_fwd"] = {"shape": list(y.shape), "us": round(us, 1), "GBps": round(3 * n / us / 1e3, 1)}       # read twice, write once
    out = HG.rand_layer_norm(y, gamma, beta, z, s, relu=True)
    go = torch.randn_like(out)
    us = _time(lambda: torch.autograd.grad(out, (y, gamma, beta), go, retain_graph=True))
    res["randln_bwd"] = {"shape": list(y.shape), "us": round(us, 1), "GBps": round(4 * n / us / 1e3, 1)}      # g, out, y in; dx out
    # bilinear x2 of the last decoder level: [B, H/2, W/2, 32] -> [B, H, W, 32]
    x = torch.randn(bs, H // 2, W // 2, 32, device="cuda").to(dt).requires_grad_(True)
    n = x.numel() * es
    with torch.no_grad():
        us = _time(lambda: HG.bilinear2(x))
    res["bilinear2_fwd"] = {"shape": list(x.shape), "us": round(us, 1), "GBps": round(5 * n / us / 1e3, 1)}     # read once, write 4x
    up = HG.bilinear2(x)
    gu = torch.randn_like(up)
    us = _time(lambda: torch.autograd.grad(up, x, gu, retain_graph=True))
    res["bilinear2_bwd"] = {"shape": list(x.shape), "us": round(us, 1), "GBps": round(5 * n / us / 1e3, 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bs", type=int, default=16)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=416)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    a = ap.parse_args()
    model, tr, batch = make(a.bs, a.height, a.width, a.dtype, not a.no_graph)
    for _ in range(a.warmup):
        out = tr.step(dict(batch))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        out = tr.step(dict(batch))
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    loss = float(out["silog_loss"].detach())
    line = {"workload": "google_resnet18_randln", "dtype": a.dtype, "bs": a.bs, "size": [a.height, a.width], "graph": not a.no_graph,
            "steps": a.steps, "ms_per_step": round(ms, 3), "images_per_s": round(a.bs * 1000.0 / ms, 1), "loss": loss, "finite": loss == loss}
    if not a.no_kernels:
        line["kernels"] = time_kernels(a.bs, a.height, a.width, a.dtype)
    print(json.dumps(line))


if __name__ == "__main__":
    main()

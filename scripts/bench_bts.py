"""BtsModel (projects/Supervised/configs/bts_r50.yaml) training step: bf16, bs 8, 352x704, hipGraph replay.  Prints one JSON line.

    python scripts/bench_bts.py [--steps K] [--warmup W] [--bs B] [--dtype bf16|fp32] [--no-graph]

Also times the dilated 3x3 convolutions of the decoder's DASPP (forward only, each d of 3/6/12/18/24 at the H/8 map, 256 -> 128 channels in
bts_r50) and reports their algorithmic TFLOP/s.
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
    cfg.MODEL.META_ARCHITECTURE, cfg.MODEL.DEVICE, cfg.MODEL.DATASET, cfg.MODEL.COMPUTE_DTYPE = "SupDepthModel", "cuda:0", "kitti", dtype
    cfg.MODEL.DEPTH_NET.NAME, cfg.MODEL.DEPTH_NET.ENCODER_NAME, cfg.MODEL.DEPTH_NET.BTS_SIZE = "BtsModel", "resnet50_bts", 512
    cfg.SOLVER.DEPTH_LR = 2e-4
    model = build_model(cfg).train()
    tr = supervised_trainer(model, cfg, use_graph=graph)
    g = torch.Generator().manual_seed(0)
    f = torch.full((bs,), 721.5377)
    K = torch.zeros(bs, 3, 3)
    K[:, 0, 0], K[:, 1, 1], K[:, 2, 2], K[:, 0, 2], K[:, 1, 2] = f, f, 1.0, W / 2, H / 2
    batch = {"img": torch.rand(bs, 3, H, W, generator=g).cuda(), "depth": (torch.rand(bs, 1, H, W, generator=g) * 79 + 1).cuda(), "intrinsics": K.cuda()}
    return model, tr, batch


def time_dilated(bs, H, W, dtype, reps=20):
    from simpledepthestimation_amd.hip import bts as HB
    from simpledepthestimation_amd.layers.hip_modules import HipConv2d
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    h, w = H // 8, W // 8
    conv = HipConv2d(256, 128, 3, 1, 1, bias=False).cuda()
    x = torch.randn(bs, h, w, 256, device="cuda").to(dt)
    res = {}
    with torch.no_grad():
        for d in (3, 6, 12, 18, 24):
            for _ in range(3):
                HB.dilated_conv3x3(conv, x, d)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                HB.dilated_conv3x3(conv, x, d)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / reps
            flops = 2.0 * bs * h * w * 128 * 256 * 9
            res[str(d)] = {"ms": round(ms, 4), "tflops": round(flops / ms / 1e9, 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--height", type=int, default=352)
    ap.add_argument("--width", type=int, default=704)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-dilated", action="store_true")
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
    line = {"workload": "bts_r50", "dtype": a.dtype, "bs": a.bs, "size": [a.height, a.width], "graph": not a.no_graph, "steps": a.steps,
            "ms_per_step": round(ms, 3), "images_per_s": round(a.bs * 1000.0 / ms, 1), "loss": loss, "finite": loss == loss}
    if not a.no_dilated:
        line["dilated_fwd"] = time_dilated(a.bs, a.height, a.width, a.dtype)
    print(json.dumps(line))


if __name__ == "__main__":
    main()

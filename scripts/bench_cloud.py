"""Point clouds from predictions: Supervised ResNet-50, bf16, the KBCrop chain, random 375 x 1242 uint8 frames, one frame at a time.

    stream            DepthPredictor.stream, graph replay, picture and depth downloaded (the route of scripts/bench_demo.py)
    stream_cloud      the same with cloud=dict(min_depth, max_depth, step): three more launches in the graph, count and the whole points buffer
                      (cap x 16 bytes) downloaded as well
    cloud_us          GPU time of one sde_depth_cloud call (its three launches) from a graph of --reps calls, on a uniform random prediction over
                      [0, vmax] (the range (min_depth, max_depth] then keeps the share printed as cloud_kept_share), and with every pixel kept
    present_us        one sde_depth_present launch measured the same way in the same session: the yardstick (7.0 us / 7.8 MB in profiles/demo_bench.txt)
    composed_cloud_us the same cloud from torch operators -- meshgrid, mask, nonzero, gather -- ending, like the kernel's route, with the count known
                      on the device and the records in a [cap,16] buffer; wall clock per call, because nonzero synchronises with the host

    python scripts/bench_cloud.py [--frames 200] [--warmup 20] [--reps 50] [--dtype bf16|fp32] [--encoder 50] [--step 1]

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 375, 1242
KITTI_K = np.array([[721.5377, 0, 609.5593], [0, 721.5377, 172.854], [0, 0, 1]], dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--encoder", default="50")
    ap.add_argument("--step", type=int, default=1)
    args = ap.parse_args()
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.engine.predictor import DepthPredictor
    from simpledepthestimation_amd.hip.cloud import RECORD, as_records, capacity, depth_cloud
    from simpledepthestimation_amd.hip.present import depth_present, device_maps
    from simpledepthestimation_amd.modeling import build_model
    dev = "cuda:0"
    cfg = get_cfg()
    cfg.MODEL.META_ARCHITECTURE, cfg.MODEL.DEPTH_NET.ENCODER_NAME, cfg.MODEL.DEVICE, cfg.MODEL.COMPUTE_DTYPE = "SupDepthModel", args.encoder, dev, args.dtype
    torch.manual_seed(0)
    model = build_model(cfg).eval()
    vmax = float(cfg.MODEL.MAX_DEPTH)
    rng = np.random.default_rng(0)
    pool = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(8)]
    frames = lambda n: (pool[i % len(pool)] for i in range(n))
    cloud = dict(min_depth=0.0, max_depth=vmax, step=args.step)          # what tools/demo.py passes for a config without MODEL.MIN_DEPTH
    cap = capacity(H, W, args.step)

    def timed(run, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(n)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    res = {"bench": "cloud", "model": f"SupDepthModel-R{args.encoder}", "dtype": args.dtype, "frame": [H, W], "frames": args.frames, "step": args.step,
           "capacity": cap, "points_bytes": cap * 16}
    graph = DepthPredictor(cfg, model=model, use_graph=True)
    run_a = lambda n: [r["canvas"][0, 0, 0] for r in graph.stream(frames(n))][-1]
    run_b = lambda n: [int(r["count"][0]) for r in graph.stream(frames(n), intrinsics=KITTI_K, cloud=cloud)][-1]
    run_a(args.warmup)
    run_b(args.warmup)
    fa, fb = [], []
    for _ in range(3):                                                   # alternating rounds: the two routes see the same neighbours
        fa.append(round(timed(run_a, args.frames), 2))
        fb.append(round(timed(run_b, args.frames), 2))
    res["stream_fps"], res["stream_cloud_fps"] = fa, fb
    res["stream_cloud_count"] = run_b(1)
    # the added download alone: cap x 16 bytes device -> pinned host on an otherwise idle device
    src = torch.empty((cap, 16), dtype=torch.uint8, device=dev)
    dst = torch.empty((cap, 16), dtype=torch.uint8).pin_memory()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dst.copy_(src, non_blocking=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(20):
        dst.copy_(src, non_blocking=True)
    e1.record()
    torch.cuda.synchronize()
    res["points_download_us"] = round(e0.elapsed_time(e1) * 1e3 / 20, 1)

    # the launches alone
    plan = graph.plan(H, W)
    ymap, xmap = device_maps(*plan.maps((plan.h, plan.w)), plan.h, plan.w, dev)
    fr = torch.from_numpy(pool[0])[None].to(dev)
    Kd = torch.from_numpy(KITTI_K)[None].to(dev)

    def graph_us(call):
        call()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(args.reps):
                call()
        g.replay()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        return round(a.elapsed_time(b) * 1e3 / args.reps, 2)

    pred_u = torch.rand(1, plan.h, plan.w, device=dev) * vmax
    pred_all = pred_u.clamp(min=1.0)
    out_p = depth_present(pred_u, ymap, xmap, vmax, 0.8, frame=fr)
    ws = torch.empty((1 << 16,), dtype=torch.int32, device=dev)
    for name, pred, lo in (("cloud", pred_u, 20.0), ("cloud_all_kept", pred_all, 0.0)):
        out_c = depth_cloud(pred, ymap, xmap, Kd, lo, vmax, args.step, frame=fr)
        torch.cuda.synchronize()
        kept = int(out_c[1][0])
        res[name + "_kept_share"] = round(kept / cap, 4)
        for _ in range(2):                                               # present and cloud interleaved
            res.setdefault("present_us", []).append(graph_us(lambda: depth_present(pred, ymap, xmap, vmax, 0.8, frame=fr, out=out_p)))
            res.setdefault(name + "_us", []).append(graph_us(lambda: depth_cloud(pred, ymap, xmap, Kd, lo, vmax, args.step, frame=fr, out=out_c, workspace=ws)))
        # bytes: the prediction is read twice per candidate (count and scatter), a kept candidate reads 3 B of colour and writes 16 B
        res[name + "_bytes"] = cap * 8 + kept * 19
    res["present_bytes"] = H * W * (4 + 3 + 3 + 3) + plan.h * plan.w * 4

    # the same cloud from torch operators
    ry, cx = ymap.long(), xmap.long()
    inside = (ry >= 0)[:, None] & (cx >= 0)[None, :]
    kinv = torch.tensor([1 / KITTI_K[0, 0], 1 / KITTI_K[1, 1], -KITTI_K[0, 2] / KITTI_K[0, 0], -KITTI_K[1, 2] / KITTI_K[1, 1]], device=dev)

    def composed(pred, lo):
        full = torch.where(inside, pred[0][ry.clamp(min=0)][:, cx.clamp(min=0)], torch.zeros((), device=dev))[::args.step, ::args.step]
        vs, us = torch.meshgrid(torch.arange(0, H, args.step, device=dev), torch.arange(0, W, args.step, device=dev), indexing="ij")
        keep = torch.isfinite(full) & (full > lo) & (full <= vmax)
        idx = keep.flatten().nonzero()[:, 0]                              # the host learns the count here
        d, u, v = full.flatten()[idx], us.flatten()[idx], vs.flatten()[idx]
        xyz = torch.stack([d * (kinv[0] * u + kinv[2]), d * (kinv[1] * v + kinv[3]), d], 1)
        rgba = torch.cat([fr[0, v, u], torch.full((idx.numel(), 1), 255, dtype=torch.uint8, device=dev)], 1)
        out = torch.empty((cap, 16), dtype=torch.uint8, device=dev)
        out[:idx.numel(), :12] = xyz.contiguous().view(torch.uint8).view(-1, 12)
        out[:idx.numel(), 12:] = rgba
        return out, idx.numel()

    for name, pred, lo in (("composed_cloud", pred_u, 20.0), ("composed_cloud_all_kept", pred_all, 0.0)):
        o, n = composed(pred, lo)
        k, c = depth_cloud(pred, ymap, xmap, Kd, lo, vmax, args.step, frame=fr)
        if n == int(c[0]):                                                # same pixels in the same order: z and the colours are copies
            a, b = as_records(o.cpu().numpy(), n), as_records(k[0], c[0])
            res[name + "_same_points"] = all(bool(np.array_equal(a[f], b[f])) for f in ("z", "red", "green", "blue", "alpha"))
        else:
            res[name + "_same_points"] = False
        for _ in range(5):
            composed(pred, lo)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            composed(pred, lo)
        torch.cuda.synchronize()
        res[name + "_us"] = round((time.perf_counter() - t0) * 1e6 / args.reps, 1)
    assert RECORD.itemsize == 16
    print(json.dumps(res))


if __name__ == "__main__":
    main()

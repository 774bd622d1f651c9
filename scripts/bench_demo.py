"""Inference throughput on camera frames: Supervised ResNet-50, bf16, the KBCrop chain, random 375 x 1242 uint8 frames, one frame at a time, every
route ending with the stacked frame / depth picture in host memory.

    composed   what the package offered before DepthPredictor: CPU chain (KBCrop, ToTensor), model(batch), torch gather through backward_maps on the
               device, download of the restored depth, colours by a numpy table lookup on the host
    predict    DepthPredictor.predict, eager, then canvas.cpu()
    stream     DepthPredictor.stream: graph replay, uploads and downloads on the copy stream

Frames per second over --frames frames after --warmup (wall clock between two synchronisations), and the GPU time of one sde_depth_present launch
(--reps launches back to back between two events) with the bytes it moves.

    python scripts/bench_demo.py [--frames 200] [--warmup 20] [--reps 50] [--dtype bf16|fp32] [--encoder 50]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--encoder", default="50")
    args = ap.parse_args()
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.data.preprocess import build_preprocess
    import simpledepthestimation_amd.data.preprocess.augmentation, simpledepthestimation_amd.data.preprocess.formating  # noqa: F401,E401
    from simpledepthestimation_amd.engine.predictor import DepthPredictor
    from simpledepthestimation_amd.evaluation.depth_evaluation import backward_maps
    from simpledepthestimation_amd.hip.present import depth_present, device_maps
    from simpledepthestimation_amd.modeling import build_model
    from simpledepthestimation_amd.utils.colormap import magma_u8
    dev = "cuda:0"
    cfg = get_cfg()
    cfg.MODEL.META_ARCHITECTURE, cfg.MODEL.DEPTH_NET.ENCODER_NAME, cfg.MODEL.DEVICE, cfg.MODEL.COMPUTE_DTYPE = "SupDepthModel", args.encoder, dev, args.dtype
    torch.manual_seed(0)
    model = build_model(cfg).eval()
    vmax, gamma, lut = float(cfg.MODEL.MAX_DEPTH), 0.8, magma_u8()
    rng = np.random.default_rng(0)
    pool = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(8)]
    frames = lambda n: (pool[i % len(pool)] for i in range(n))
    steps = [build_preprocess({"NAME": "KBCrop"}), build_preprocess({"NAME": "ToTensor"})]

    def composed(frame):
        data = {"img": frame, "metadata": {}}
        for s in steps:
            data = s.forward(data)
        with torch.no_grad():
            pred = model({"img": data["img"][None]})["depth_pred"].float()[0, 0]
        rows, cols = backward_maps(tuple(pred.shape), data["metadata"], ["KBCrop"])
        ry, cx = torch.from_numpy(rows).to(dev).long(), torch.from_numpy(cols).to(dev).long()
        full = (pred[ry.clamp(min=0)][:, cx.clamp(min=0)] * ((ry >= 0)[:, None] & (cx >= 0)[None, :])).cpu().numpy()
        idx = np.minimum(255, (np.maximum(full, 0) ** np.float32(gamma) / np.float32(vmax ** gamma) * 256).astype(np.int32))
        return np.concatenate([frame, lut[idx]], 0)

    def timed(run, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(n)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    res = {"bench": "demo", "model": f"SupDepthModel-R{args.encoder}", "dtype": args.dtype, "frame": [H, W], "frames": args.frames}
    run_a = lambda n: [composed(f) for f in frames(n)][-1]
    run_a(args.warmup)
    res["composed_fps"] = round(timed(run_a, args.frames), 2)
    eager = DepthPredictor(cfg, model=model, use_graph=False)
    run_b = lambda n: [eager.predict(f)["canvas"].cpu() for f in frames(n)][-1]
    run_b(args.warmup)
    res["predict_eager_fps"] = round(timed(run_b, args.frames), 2)
    graph = DepthPredictor(cfg, model=model, use_graph=True)
    run_c = lambda n: [r["canvas"][0, 0, 0] for r in graph.stream(frames(n))][-1]
    run_c(args.warmup)
    res["stream_graph_fps"] = round(timed(run_c, args.frames), 2)
    # the three routes show the same picture (the composed route's host powers may differ from the kernel's in the last bit at an index boundary)
    a, c = composed(pool[0]), next(iter(graph.stream(iter([pool[0]]))))["canvas"]
    res["pictures_differ_px"] = int(np.any(a != c, -1).sum())
    # model time alone (graph replay without present), for the share of the frame the rest takes
    run_d = lambda n: [graph.predict(f, present=False) for f in frames(n)][-1]
    run_d(args.warmup)
    res["predict_graph_no_present_fps"] = round(timed(run_d, args.frames), 2)
    # the present launch alone
    plan = graph.plan(H, W)
    pred = torch.rand(1, plan.h, plan.w, device=dev) * vmax
    ymap, xmap = device_maps(*plan.maps((plan.h, plan.w)), plan.h, plan.w, dev)
    fr = torch.from_numpy(pool[0])[None].to(dev)
    for name, kw in (("present_us", dict(frame=fr)), ("present_no_frame_us", dict(frame=None)), ("present_all_outputs_us", dict(frame=fr, want_u16=True))):
        o = depth_present(pred, ymap, xmap, vmax, gamma, **kw)
        # --reps launches captured into one graph: the replay is free of the host's launch path (~10 us per ctypes call, as long as the kernel)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(args.reps):
                depth_present(pred, ymap, xmap, vmax, gamma, out=o, **kw)
        g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        res[name] = round(e0.elapsed_time(e1) * 1e3 / args.reps, 2)
    px = H * W
    moved = px * (4 + 3 + 3 + 3) + plan.h * plan.w * 4          # depth out, colours out, frame in + out, the prediction read once
    res["present_bytes"] = moved
    res["present_gbps"] = round(moved / (res["present_us"] * 1e-6) / 1e9, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

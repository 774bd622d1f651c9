"""The TSDF volume seen from a camera (TsdfVolume.render, sde_tsdf_render: one launch, ray casting), on the volume the launch part of
scripts/bench_volume.py builds: --dims voxels of vmax / dims_z, one uniform random prediction over [2, vmax] integrated from the middle of the near
face.  Rendered from that pose at 192 x 640 and at 375 x 1242 with the KITTI intrinsics scaled to the size, near = 0, far = vmax, step = one voxel.

    render_us            GPU time of one launch (depth, normal and picture), from a graph of --reps launches replayed --replays times between two
                         events; depth_only_us the same launch without the two optional outputs.  The two are timed in alternating rounds in two
                         runs of --rounds rounds each: per run the medians and spread_pct, the largest (max - min) / median of either's rounds
    torch_us             the same depth and colour from torch operators: a dense march over the n samples, the tsdf through
                         torch.nn.functional.grid_sample (trilinear, voxel centres), validity as the trilinear sample of (weight >= 1) above 0.9999, the
                         colour through a nearest grid_sample; eager, --torch-reps runs between two events, two runs.  torch_agree_pct: pixels
                         whose hit / miss agrees with the kernel's and, on a hit, whose depth lies within 1e-3 of it (the operators round otherwise)
    hit_pct / samples_marched   what the launch does: pixels with a surface, and the mean over the rays of the index of the sample that hit + 1, or n
                         on a miss: an upper figure of the samples a ray visits, the ones skipped in front of and behind the grid are in it
    picture_agree_pct    pixels whose four colour bytes agree with the torch march's (its nearest sample rounds half to even)
    stream               PairPredictor.stream (MonoDepth2 ResNet-18, bf16, 375 x 1242 frames) with volume= against volume= + render= in the same
                         session, alternating rounds: windows per second of each, render_cost_pct the difference of the medians and spread_pct
                         the largest spread of either route's rounds; `resolved` says whether the difference exceeds that spread

    python scripts/bench_render.py [--reps 20] [--replays 5] [--rounds 5] [--frames 100] [--dims 256 256 128] [--out profiles/render_bench.txt]

Prints one JSON line per part and appends it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_mesh import build_volume  # noqa: E402
from bench_pairs import H, KITTI_K, NET_H, NET_W, W, make_cfg  # noqa: E402


def scaled_K(h, w):
    K = KITTI_K.copy()
    K[0] *= w / W
    K[1] *= h / H
    return K


def torch_render(vol, K, C, size, near, step, n):
    """Depth [H,W] and colour [H,W,4] by a dense march with torch operators; no normal."""
    import torch.nn.functional as F
    dev = vol.device
    h, w = size
    nx, ny, nz = vol.dims
    v, u = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32), indexing="ij")
    ray = torch.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], torch.ones_like(u)], -1)
    R, t = C[:3, :3], C[:3, 3]
    origin = torch.tensor(vol.origin, device=dev)
    dims = torch.tensor([nx, ny, nz], device=dev, dtype=torch.float32)
    tsdf = vol.tsdf[None, None]
    valid_src = (vol.weight >= 1).float()[None, None]
    colour = vol.rgba.permute(3, 0, 1, 2)[None].float()
    depth = torch.zeros((h, w), device=dev)
    g_hit = torch.zeros((h, w, 3), device=dev)
    live = torch.ones((h, w), dtype=torch.bool, device=dev)
    prev = torch.zeros((h, w), dtype=torch.bool, device=dev)
    tp = torch.zeros((h, w), device=dev)
    for i in range(n):
        s = near + i * step
        g = ((s * ray - t) @ R - origin) / vol.voxel - 0.5                 # R^T (p - t) as a row vector times R
        norm = (2 * g / (dims - 1) - 1)[None, None]                         # align_corners=True: voxel centres at -1 and 1
        inside = ((g >= 0) & (g < dims - 1)).all(-1)
        ti = F.grid_sample(tsdf, norm, mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0, 0]
        ok = inside & (F.grid_sample(valid_src, norm, mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0, 0] > 0.9999)
        hit = live & ok & prev & (tp > 0) & (ti <= 0)
        depth = torch.where(hit, (s - step) + step * (tp / (tp - ti)), depth)
        g_hit = torch.where(hit[..., None], g, g_hit)
        live = live & ~hit
        prev, tp = ok, torch.where(ok, ti, tp)
    norm = (2 * g_hit / (dims - 1) - 1)[None, None]
    pic = F.grid_sample(colour, norm, mode="nearest", padding_mode="zeros", align_corners=True)[0, :, 0].permute(1, 2, 0)
    pic[..., 3] = 255
    pic = torch.where((depth != 0)[..., None], pic, torch.zeros_like(pic)).to(torch.uint8)
    return depth, pic


def bench_launch(args, dev, vol, size):
    h, w = size
    K = torch.from_numpy(scaled_K(h, w)).to(dev)
    C = torch.eye(4, device=dev)
    out = vol.render(K, C, size)
    depth_only = vol.render(K, C, size, normals=False, picture=False)
    calls = {"render": lambda: vol.render(K, C, size, out=out), "depth_only": lambda: vol.render(K, C, size, normals=False, picture=False, out=depth_only)}
    graphs = {}
    for name, call in calls.items():
        call()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(args.reps):
                call()
        g.replay()
        graphs[name] = g

    def us(g):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.replays):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        return round(a.elapsed_time(b) * 1e3 / (args.reps * args.replays), 2)

    runs = []
    for _ in range(2):
        rounds = {k: [] for k in graphs}
        for _ in range(args.rounds):                                     # alternating: the two calls see the same neighbours
            for name in graphs:
                rounds[name].append(us(graphs[name]))
        med = {k: float(np.median(v)) for k, v in rounds.items()}
        runs.append({"render_us": rounds["render"], "depth_only_us": rounds["depth_only"], "render_median_us": med["render"],
                     "depth_only_median_us": med["depth_only"], "spread_pct": round(100 * max((max(v) - min(v)) / med[k] for k, v in rounds.items()), 2)})
    from simpledepthestimation_amd.hip.volume import check_render
    _, _, near, step, n = check_render(size, vol.min_depth, vol.max_depth, vol.voxel)
    torch_us = []
    for _ in range(2):
        torch_render(vol, K, C, size, near, step, n)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.torch_reps):
            td, tpic = torch_render(vol, K, C, size, near, step, n)
        b.record()
        torch.cuda.synchronize()
        torch_us.append(round(a.elapsed_time(b) * 1e3 / args.torch_reps, 1))
    d = out[0]
    hit, thit = d != 0, td != 0
    agree = (hit == thit) & (~hit | ((d - td).abs() <= 1e-3 * d.abs()))
    marched = torch.where(hit, (d - near) / step + 1, torch.full_like(d, float(n)))
    return {"bench": "render_launch", "dims": list(vol.dims), "size": [h, w], "samples": n, "reps": args.reps, "replays": args.replays, "runs": runs,
            "torch_us": torch_us, "torch_over_render": [round(t / r["render_median_us"], 1) for t, r in zip(torch_us, runs)],
            "torch_agree_pct": round(100 * float(agree.float().mean()), 2), "hit_pct": round(100 * float(hit.float().mean()), 2),
            "samples_marched": round(float(marched.mean()), 1), "picture_agree_pct": round(100 * float((out[2] == tpic).all(-1).float().mean()), 2)}


def bench_stream(args, dev):
    from simpledepthestimation_amd.engine.predictor import PairPredictor
    from simpledepthestimation_amd.hip.volume import TsdfVolume
    from simpledepthestimation_amd.modeling import build_model
    cfg = make_cfg("MonoDepth2", args.dtype, dev)
    torch.manual_seed(0)
    pair_p = PairPredictor(cfg, model=build_model(cfg).eval(), use_graph=True)
    rng = np.random.default_rng(0)
    pool = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(8)]
    frames = lambda n: (pool[i % len(pool)] for i in range(n))
    span = max(pair_p.offsets + (0,)) - min(pair_p.offsets + (0,))
    dims = tuple(args.dims)
    m = float(np.median(next(iter(pair_p.stream(frames(1 + span), KITTI_K, present=False)))["depth_net"]))
    voxel = 4 * m / dims[0]
    vol = TsdfVolume(dims, voxel, origin=(-dims[0] * voxel / 2, -dims[1] * voxel / 2, m / 4), min_depth=0.0, max_depth=1e6, device=dev)
    render = dict(normals=True, picture=True, min_weight=1, near=m / 8, far=m / 4 + dims[2] * voxel, step=voxel)

    def timed(run, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = run(k)
        torch.cuda.synchronize()
        return got / (time.perf_counter() - t0)

    run_v = lambda k: len([r["world_to_camera"][0, 0] for r in pair_p.stream(frames(k + span), KITTI_K, volume=vol)])
    hits = []
    run_r = lambda k: len([hits.append(float((r["model_depth"] != 0).mean())) for r in pair_p.stream(frames(k + span), KITTI_K, volume=vol, render=render)])
    run_v(args.warmup)
    run_r(args.warmup)
    fv, fr = [], []
    for _ in range(3):                                                   # alternating rounds: the two routes see the same neighbours
        fv.append(round(timed(run_v, args.frames), 2))
        fr.append(round(timed(run_r, args.frames), 2))
    mv, mr = float(np.median(fv)), float(np.median(fr))
    cost = 100 * (mv - mr) / mv
    spread = 100 * max((max(fv) - min(fv)) / mv, (max(fr) - min(fr)) / mr)
    return {"bench": "render_stream", "model": "MonoDepth2", "dtype": args.dtype, "frame": [H, W], "net": [NET_H, NET_W], "frames": args.frames, "dims": list(dims),
            "samples": int(np.ceil((np.float32(render["far"]) - np.float32(render["near"])) / np.float32(voxel))), "volume_stream_fps": fv,
            "render_stream_fps": fr, "render_cost_pct": round(cost, 2), "spread_pct": round(spread, 2), "resolved": bool(abs(cost) > spread),
            "ms_per_window_difference": round(1e3 / mr - 1e3 / mv, 3), "hit_pct_last_window": round(100 * hits[-1], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--dims", type=int, nargs=3, default=[256, 256, 128])
    ap.add_argument("--sizes", type=int, nargs="+", default=[192, 640, 375, 1242], help="H W pairs")
    ap.add_argument("--no-stream", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_render.py measures on the GPU; there is no CPU fallback"
    dev = "cuda:0"

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    vol = build_volume(tuple(args.dims), args.dtype, dev)
    for h, w in zip(args.sizes[::2], args.sizes[1::2]):
        emit(bench_launch(args, dev, vol, (h, w)))
    del vol
    if not args.no_stream:
        emit(bench_stream(args, dev))


if __name__ == "__main__":
    main()

"""A sequence's depth fused into a TSDF volume (PairPredictor.stream(..., volume=TsdfVolume(...)), hip/volume.py): the models, frames and sizes of
scripts/bench_pairs.py (MonoDepth2 and MotionLearning ResNet-18, bf16, random 375 x 1242 frames at 192 x 640, one window at a time).

    pair_stream_fps     windows per second of PairPredictor.stream as it is
    volume_stream_fps   the same stream with volume=, in alternating rounds in the same session; volume_cost_pct is the difference of the medians,
                        stream_spread_pct the largest spread of either route's rounds around its median.  The volume has --dims voxels; its edge
                        is set from the median m of the model's first prediction (a random-weight network has no scale one could know beforehand)
                        so that the grid spans 4 m sideways and reaches from m / 4 to beyond 2 m
    stream_touched      voxels with weight > 0 after the last round, of how many
    integrate_us        GPU time of one sde_tsdf_integrate launch from a graph of --reps launches into one volume (every launch keeps the same
                        voxels: the same traffic, whatever the weights have grown to), on a uniform random prediction over [2, vmax] seen
                        from the middle of the near face, voxels of vmax / dims_z
    integrate_touched   voxels that launch keeps, and integrate_coloured, those whose colour it also updates (sdf <= trunc)
    integrate_bytes     what the launch has to move, counted from those: 8 B read + 8 B written per kept voxel, 4 B + 4 B more per coloured one, the
                        prediction and the frame once; integrate_gbs is that over the time.  Voxels that are not kept move nothing from the volume
    compose_us          one sde_pose_compose launch (64 B read, 64 B written: launch latency)
    points_us           one sde_tsdf_points call (three launches) on the volume the integrate run left; points_bytes: 8 B per voxel and its three
                        neighbours (from cache) read twice, 4 B per tile written and read three times, 16 B per record; points_found the records

    python scripts/bench_volume.py [--frames 200] [--warmup 20] [--reps 50] [--dims 256 256 128] [--out profiles/volume_bench.txt]

Prints one JSON line per model and appends it to --out."""
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

from bench_pairs import H, KITTI_K, NET_H, NET_W, W, make_cfg  # noqa: E402


def bench(name, args, dev):
    from simpledepthestimation_amd.engine.predictor import PairPredictor
    from simpledepthestimation_amd.hip.present import device_maps
    from simpledepthestimation_amd.hip.volume import TsdfVolume, pose_compose
    from simpledepthestimation_amd.modeling import build_model
    cfg = make_cfg(name, args.dtype, dev)
    torch.manual_seed(0)
    model = build_model(cfg).eval()
    vmax = float(cfg.MODEL.MAX_DEPTH)
    rng = np.random.default_rng(0)
    pool = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(8)]
    frames = lambda n: (pool[i % len(pool)] for i in range(n))
    pair_p = PairPredictor(cfg, model=model, use_graph=True)
    span = max(pair_p.offsets + (0,)) - min(pair_p.offsets + (0,))
    dims = tuple(args.dims)
    m = float(np.median(next(iter(pair_p.stream(frames(1 + span), KITTI_K, present=False)))["depth_net"]))
    voxel = 4 * m / dims[0]
    vol = TsdfVolume(dims, voxel, origin=(-dims[0] * voxel / 2, -dims[1] * voxel / 2, m / 4), min_depth=0.0, max_depth=1e6, device=dev)

    def timed(run, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = run(k)
        torch.cuda.synchronize()
        return got / (time.perf_counter() - t0)

    run_p = lambda k: len([r["flow"][0, 0, 0, 0] for r in pair_p.stream(frames(k + span), KITTI_K)])          # k windows
    run_v = lambda k: len([r["world_to_camera"][0, 0] for r in pair_p.stream(frames(k + span), KITTI_K, volume=vol)])
    run_p(args.warmup)
    run_v(args.warmup)
    fp, fv = [], []
    for _ in range(3):                                                   # alternating rounds: the two routes see the same neighbours
        fp.append(round(timed(run_p, args.frames), 2))
        fv.append(round(timed(run_v, args.frames), 2))
    mp, mv = float(np.median(fp)), float(np.median(fv))
    res = {"bench": "volume", "model": name, "dtype": args.dtype, "frame": [H, W], "net": [NET_H, NET_W], "contexts": list(pair_p.offsets), "frames": args.frames,
           "dims": list(dims), "stream_voxel": round(voxel, 6), "pair_stream_fps": fp, "volume_stream_fps": fv, "volume_cost_pct": round(100 * (mp - mv) / mp, 2),
           "stream_spread_pct": round(100 * max((max(fp) - min(fp)) / mp, (max(fv) - min(fv)) / mv), 2),
           "stream_touched": [int((vol.weight > 0).sum()), int(vol.weight.numel())]}
    del vol

    # the launches alone
    plan = pair_p.plan(H, W)
    ymap, xmap = device_maps(*plan.maps((plan.h, plan.w)), plan.h, plan.w, dev)
    fr = torch.from_numpy(pool[0]).to(dev)
    Kd = torch.from_numpy(KITTI_K).to(dev)
    pred = torch.rand(1, plan.h, plan.w, device=dev) * (vmax - 2) + 2
    voxel = vmax / dims[2]
    vol = TsdfVolume(dims, voxel, min_depth=0.0, max_depth=vmax, device=dev)
    C = torch.eye(4, device=dev)
    T = torch.eye(4, device=dev)
    T[:3, 3] = torch.tensor([0.05, -0.02, -0.8], device=dev)
    T[0, 2], T[2, 0] = 0.02, -0.02

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

    vol.integrate(pred, ymap, xmap, Kd, C, frame=fr)
    kept, coloured = int((vol.weight > 0).sum()), int((vol.rgba[..., 3] == 255).sum())
    res["integrate_touched"], res["integrate_coloured"], res["voxels"] = kept, coloured, int(vol.weight.numel())
    res["integrate_us"] = [graph_us(lambda: vol.integrate(pred, ymap, xmap, Kd, C, frame=fr)) for _ in range(2)]
    res["integrate_bytes"] = kept * 16 + coloured * 8 + plan.h * plan.w * 4 + H * W * 3
    res["integrate_gbs"] = [round(res["integrate_bytes"] / us / 1e3, 1) for us in res["integrate_us"]]
    res["compose_us"] = [graph_us(lambda: pose_compose(T, C)) for _ in range(2)]
    C.copy_(torch.eye(4, device=dev))
    points, count = vol.points()
    ws = torch.empty(vol.workspace_numel(), dtype=torch.int32, device=dev)
    res["points_us"] = [graph_us(lambda: vol.points(out=(points, count), workspace=ws)) for _ in range(2)]
    found = int(count.item())
    res["points_found"], res["points_cap"] = found, int(points.shape[0])
    res["points_bytes"] = 2 * 8 * int(vol.weight.numel()) + 3 * 4 * ws.numel() + 16 * min(found, int(points.shape[0]))
    res["points_gbs"] = [round(res["points_bytes"] / us / 1e3, 1) for us in res["points_us"]]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--dims", type=int, nargs=3, default=[256, 256, 128])
    ap.add_argument("--models", nargs="+", default=["MonoDepth2", "MotionLearning"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_volume.py measures on the GPU; there is no CPU fallback"
    for name in args.models:
        line = json.dumps(bench(name, args, "cuda:0"))
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

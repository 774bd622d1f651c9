"""Ego-motion and flow from frame pairs: MonoDepth2 ResNet-18 (PoseNet, contexts at -1 and +1) and MotionLearning ResNet-18 (GoogleResNet +
GoogleMotionNet, context at +1), bf16, random 375 x 1242 uint8 frames resized to 192 x 640, one window at a time.

    depth_stream_fps  DepthPredictor.stream on the same model: graph replay, picture and depth downloaded (the route of scripts/bench_demo.py)
    pair_stream_fps   PairPredictor.stream: every frame of the window prepared, the pose network, sde_pair_flow and the flow's downloads on top
    pair_flow_us      GPU time of one sde_pair_flow launch over the model's n contexts (flow, validity, colours) from a graph of --reps launches,
                      on a uniform random prediction over [2, vmax] and a small pose; with the motion field for MotionLearning
    present_us        one sde_depth_present launch (depth, colours under the frame) measured the same way in the same session: the same gathers
    *_gbs             the bytes the launch has to move (counted from the shapes, below) over that time
    composed_flow_us  the same flow from the package's operators: the gather through the maps, img_to_points, points_to_img, minus the pixel grid

    python scripts/bench_pairs.py [--frames 200] [--warmup 20] [--reps 50] [--dtype bf16|fp32] [--out profiles/pair_bench.txt]

Prints one JSON line per model and appends it to --out.

    python scripts/bench_pairs.py --temporal [--out profiles/temporal_bench.txt]

measures the temporally fused depth instead (PairPredictor.stream(..., temporal=dict(alpha=0.5, tol=0.05)), hip/temporal.py):

    pair_stream_fps      windows per second of PairPredictor.stream as it is
    temporal_stream_fps  the same stream with temporal fusion, in alternating rounds in the same session; temporal_cost_pct is the difference of the
                         medians, stream_spread_pct the largest spread of either route's rounds around its median
    warp_fuse_us         GPU time of one sde_depth_warp_fuse call (three launches: fill, scatter, fuse) at the network's size from a graph of
                         --reps calls, on a uniform random previous depth over [2, vmax], a prediction within 3 % of it and a small pose; with
                         the motion field for MotionLearning
    warp_fuse_bytes      what the three launches move, from the shapes: 4 B z-buffer fill, 4 B previous depth (+ 12 B motion), 4 B z-buffer and
                         4 B prediction read, 4 B fused and 1 B state written per pixel, and one 4-byte atomic per pixel"""
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
NET_H, NET_W = 192, 640
KITTI_K = np.array([[721.5377, 0, 609.5593], [0, 721.5377, 172.854], [0, 0, 1]], dtype=np.float32)
MOTION_LOSS = {"NUM_SCALES": 1, "SSIM_WEIGHT": 3.0, "C1": "inf", "C2": 9e-6, "DEPTH_L1_WEIGHT": 0.0, "MOTION_SMOOTHNESS_WEIGHT": 1.0, "MOTION_SPARSITY_WEIGHT": 0.2,
               "ROT_CYCLE_WEIGHT": 1e-3, "TRANS_CYCLE_WEIGHT": 5e-2, "SCALE_NORMALIZE": False}


def make_cfg(name, dtype, dev):
    from simpledepthestimation_amd.config import get_cfg
    cfg = get_cfg()
    cfg.set_new_allowed(True)
    if name == "MonoDepth2":
        cfg.merge_from_other_cfg({"MODEL": {"META_ARCHITECTURE": "MonoDepth2Model", "POSE_NET": {"NAME": "PoseNet", "NUM_CONTEXTS": 2}}})
    else:
        cfg.merge_from_other_cfg({"MODEL": {"META_ARCHITECTURE": "MotionLearningModel", "DEPTH_NET": {"NAME": "GoogleResNet", "NORM": "randLN"},
                                            "POSE_NET": {"NAME": "GoogleMotionNet", "USE_DEPTH": True, "SCALE_CONSTRAIN": "clip_ste"}}, "LOSS": MOTION_LOSS})
    cfg.MODEL.DEPTH_NET.ENCODER_NAME, cfg.MODEL.DEVICE, cfg.MODEL.COMPUTE_DTYPE = "18", dev, dtype
    cfg.merge_from_other_cfg({"DATASETS": {"TEST": {"PREPROCESS": [{"NAME": "LoadImg"}, {"NAME": "Resize", "IMG_H": NET_H, "IMG_W": NET_W}, {"NAME": "ToTensor"}]}}})
    return cfg


def bench(name, args, dev):
    from simpledepthestimation_amd.engine.predictor import DepthPredictor, PairPredictor
    from simpledepthestimation_amd.geometry.camera import img_to_points, inv_intrinsics, points_to_img
    from simpledepthestimation_amd.hip.flow import pair_flow
    from simpledepthestimation_amd.hip.present import depth_present, device_maps
    from simpledepthestimation_amd.modeling import build_model
    cfg = make_cfg(name, args.dtype, dev)
    torch.manual_seed(0)
    model = build_model(cfg).eval()
    vmax = float(cfg.MODEL.MAX_DEPTH)
    rng = np.random.default_rng(0)
    pool = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(8)]
    frames = lambda n: (pool[i % len(pool)] for i in range(n))
    depth_p = DepthPredictor(cfg, model=model, use_graph=True)
    pair_p = PairPredictor(cfg, model=model, use_graph=True)
    n = pair_p.n
    span = max(pair_p.offsets + (0,)) - min(pair_p.offsets + (0,))

    def timed(run, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = run(k)
        torch.cuda.synchronize()
        return got / (time.perf_counter() - t0)

    run_d = lambda k: len([r["canvas"][0, 0, 0] for r in depth_p.stream(frames(k))])
    run_p = lambda k: len([r["flow"][0, 0, 0, 0] for r in pair_p.stream(frames(k + span), KITTI_K)])          # k windows
    run_d(args.warmup)
    run_p(args.warmup)
    fd, fp = [], []
    for _ in range(3):                                                   # alternating rounds: the two routes see the same neighbours
        fd.append(round(timed(run_d, args.frames), 2))
        fp.append(round(timed(run_p, args.frames), 2))
    res = {"bench": "pairs", "model": name, "dtype": args.dtype, "frame": [H, W], "net": [NET_H, NET_W], "contexts": list(pair_p.offsets), "frames": args.frames,
           "depth_stream_fps": fd, "pair_stream_fps": fp}

    # the launches alone
    plan = pair_p.plan(H, W)
    ymap, xmap = device_maps(*plan.maps((plan.h, plan.w)), plan.h, plan.w, dev)
    fr = torch.from_numpy(pool[0])[None].to(dev)
    Kd = torch.from_numpy(KITTI_K)[None].expand(n, 3, 3).contiguous().to(dev)
    pred = torch.rand(n, plan.h, plan.w, device=dev) * (vmax - 2) + 2
    T = torch.eye(4, device=dev).repeat(n, 1, 1)
    T[:, :3, 3] = torch.tensor([0.05, -0.02, -0.8], device=dev)
    T[:, 0, 2], T[:, 2, 0] = 0.02, -0.02
    motion = (torch.rand(n, 3, plan.h, plan.w, device=dev) - 0.5) * 0.2 if name != "MonoDepth2" else None

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

    out_f = pair_flow(pred, ymap, xmap, Kd, T, motion=motion, max_flow=0.05 * W)
    out_p = depth_present(pred[:1], ymap, xmap, vmax, 0.8, frame=fr)
    for _ in range(2):                                                   # the two kernels interleaved
        res.setdefault("present_us", []).append(graph_us(lambda: depth_present(pred[:1], ymap, xmap, vmax, 0.8, frame=fr, out=out_p)))
        res.setdefault("pair_flow_us", []).append(graph_us(lambda: pair_flow(pred, ymap, xmap, Kd, T, motion=motion, max_flow=0.05 * W, out=out_f)))
    # bytes from the shapes: every element of the prediction (and of the motion field) comes in once, every restored pixel goes out as 8 B of flow,
    # 1 B of validity and 3 B of colour; present: 4 B depth + 3 B colour + 3 B frame in / out per pixel
    res["pair_flow_bytes"] = n * (plan.h * plan.w * 4 * (4 if motion is not None else 1) + H * W * 12)
    res["present_bytes"] = H * W * (4 + 3 + 3 + 3) + plan.h * plan.w * 4
    res["pair_flow_gbs"] = [round(res["pair_flow_bytes"] / us / 1e3, 1) for us in res["pair_flow_us"]]
    res["present_gbs"] = [round(res["present_bytes"] / us / 1e3, 1) for us in res["present_us"]]

    # the same flow from the package's operators
    ry, cx = ymap.long(), xmap.long()
    inside = (ry >= 0)[:, None] & (cx >= 0)[None, :]
    Kinv = inv_intrinsics(Kd)
    KR, Kt = Kd.bmm(T[:, :3, :3]), Kd.bmm(T[:, :3, 3:])
    zero_t = torch.zeros(n, 3, 1, device=dev)
    grid = torch.stack(torch.meshgrid(torch.arange(W, device=dev, dtype=torch.float32), torch.arange(H, device=dev, dtype=torch.float32), indexing="xy"), -1)

    def composed():
        gather = lambda a: torch.where(inside, a[..., ry.clamp(min=0), :][..., cx.clamp(min=0)], torch.zeros((), device=dev))
        t = Kt if motion is None else Kd.bmm((T[:, :3, 3:, None] + gather(motion)).reshape(n, 3, H * W))
        coords, _, _ = points_to_img(img_to_points(gather(pred)[:, None].contiguous(), Kinv, zero_t), KR, t)
        return coords - grid

    diff = (composed() - out_f[0]).abs()[(out_f[1] & 1).bool()]
    res["composed_max_abs_diff_px"] = round(float(diff.max()), 6)
    for _ in range(5):
        composed()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(args.reps):
        composed()
    b.record()
    torch.cuda.synchronize()
    res["composed_flow_us"] = round(a.elapsed_time(b) * 1e3 / args.reps, 1)
    return res


def bench_temporal(name, args, dev):
    from simpledepthestimation_amd.engine.predictor import PairPredictor
    from simpledepthestimation_amd.hip.temporal import warp_fuse
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
    fuse = dict(alpha=0.5, tol=0.05)

    def timed(run, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = run(k)
        torch.cuda.synchronize()
        return got / (time.perf_counter() - t0)

    run_p = lambda k: len([r["flow"][0, 0, 0, 0] for r in pair_p.stream(frames(k + span), KITTI_K)])          # k windows
    run_t = lambda k: len([r["temporal_state"][0, 0] for r in pair_p.stream(frames(k + span), KITTI_K, temporal=fuse)])
    run_p(args.warmup)
    run_t(args.warmup)
    fp, ft = [], []
    for _ in range(3):                                                   # alternating rounds: the two routes see the same neighbours
        fp.append(round(timed(run_p, args.frames), 2))
        ft.append(round(timed(run_t, args.frames), 2))
    mp, mt = float(np.median(fp)), float(np.median(ft))
    res = {"bench": "temporal", "model": name, "dtype": args.dtype, "frame": [H, W], "net": [NET_H, NET_W], "contexts": list(pair_p.offsets), "frames": args.frames,
           "pair_stream_fps": fp, "temporal_stream_fps": ft, "temporal_cost_pct": round(100 * (mp - mt) / mp, 2),
           "stream_spread_pct": round(100 * max((max(fp) - min(fp)) / mp, (max(ft) - min(ft)) / mt), 2)}

    # the three launches alone, at the network's size
    plan = pair_p.plan(H, W)
    h, w = plan.h, plan.w
    Kd = torch.from_numpy(np.asarray(plan.intrinsics(KITTI_K), dtype=np.float32))[None].to(dev)
    prev = torch.rand(1, h, w, device=dev) * (vmax - 2) + 2
    cur = prev * (1 + (torch.rand(1, h, w, device=dev) - 0.5) * 0.06)
    T = torch.eye(4, device=dev)[None].clone()
    T[:, :3, 3] = torch.tensor([0.05, -0.02, -0.8], device=dev)
    T[:, 0, 2], T[:, 2, 0] = 0.02, -0.02
    motion = (torch.rand(1, 3, h, w, device=dev) - 0.5) * 0.2 if name != "MonoDepth2" else None
    fused, state, _ = warp_fuse(prev, cur, Kd, T, motion=motion)
    zbuf = torch.empty((1, h, w), dtype=torch.int32, device=dev)

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

    res["warp_fuse_us"] = [graph_us(lambda: warp_fuse(prev, cur, Kd, T, motion=motion, out=fused, zbuf=zbuf, state=state)) for _ in range(2)]
    res["warp_fuse_bytes"] = h * w * (4 + 4 + (12 if motion is not None else 0) + 4 + 4 + 4 + 4 + 1)
    res["warp_fuse_classes"] = torch.bincount(state.flatten().long() & 3, minlength=4).tolist()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--models", nargs="+", default=["MonoDepth2", "MotionLearning"])
    ap.add_argument("--temporal", action="store_true", help="measure the temporally fused stream against the plain one, and sde_depth_warp_fuse alone")
    ap.add_argument("--out", default=None, help="default: profiles/pair_bench.txt, profiles/temporal_bench.txt with --temporal")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "temporal_bench.txt" if args.temporal else "pair_bench.txt")
    assert torch.cuda.is_available(), "bench_pairs.py measures on the GPU; there is no CPU fallback"
    for name in args.models:
        line = json.dumps((bench_temporal if args.temporal else bench)(name, args, "cuda:0"))
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

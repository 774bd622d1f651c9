"""Frame-to-model tracking (TsdfVolume.track, sde_frame_align: two launches per iteration) on a volume that HAS a surface: a synthetic room -- two
side walls, floor, ceiling and a back wall, analytic z-depth -- integrated from three cameras into --dims voxels of --voxel.  The tracked frame
sees the room from a camera turned by half a degree and moved by a voxel against the predicted one, with a depth 3 % short.

    align_us             GPU time of ONE iteration (mode POSE | SCALE: accumulate + finish), from a graph of --reps iterations replayed --replays
                         times between two events, at 192 x 640 and at 375 x 1242 (KITTI intrinsics scaled to the size); render_us the render that
                         precedes the iterations of one tracked frame, the same way.  The two are timed in alternating rounds in two runs of
                         --rounds rounds each: per run the medians and spread_pct, the largest (max - min) / median of either's rounds
    torch_us             the same iteration composed from torch operators (the per-pixel stage as tensor arithmetic, the 31 sums as one
                         reduction, torch.linalg.solve in float64, the Cayley update): eager, --torch-reps runs between two events, two runs.
                         torch_agree: the largest difference between its D / scale and the kernel's after one iteration from the same state
    inlier_pct           pose and scale inliers of the first iteration, in per cent of the picture: the iteration that is timed has work to do
    bytes                what one iteration moves, counted from the shapes: 4 B of depth per pixel, 16 B of the model per kept pixel (an upper
                         figure: every pixel), the maps, the slab written once and read once
    stream               PairPredictor.stream (MonoDepth2 ResNet-18, bf16, 375 x 1242 frames) with volume= against volume= + track= in the same
                         session, alternating rounds: windows per second of each, track_cost_pct the difference of the medians and spread_pct the
                         largest spread of either route's rounds; `resolved` says whether the difference exceeds that spread
    --trace-only         runs --reps iterations per size and nothing else: the command a kernel trace is taken of, in a run of its own

    python scripts/bench_track.py [--reps 20] [--replays 5] [--rounds 5] [--frames 100] [--dims 256 128 256] [--voxel 0.05] [--out profiles/track_bench.txt]

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

from bench_pairs import H, KITTI_K, NET_H, NET_W, W, make_cfg  # noqa: E402
from bench_render import scaled_K  # noqa: E402

ROOM = (5.0, 1.5, 11.0)                           # half width, half height, the back wall's z: |x| <= 5, |y| <= 1.5, z <= 11


def pose(deg, t, dev):
    ax, ay, az = np.deg2rad(deg)
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rx @ Ry @ Rz, t
    return torch.from_numpy(T.astype(np.float32)).to(dev)


def room_depth(K, C, size):
    """The z-depth of the room's inside seen from the world -> camera pose C through K: float32 [H,W] on C's device."""
    h, w = size
    dev = C.device
    K64, C64 = K.double(), C.double()
    v, u = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float64), torch.arange(w, device=dev, dtype=torch.float64), indexing="ij")
    ray = torch.stack([(u - K64[0, 2]) / K64[0, 0], (v - K64[1, 2]) / K64[1, 1], torch.ones_like(u)], -1) @ C64[:3, :3]      # R^T ray, row-wise
    o = -(C64[:3, :3].T @ C64[:3, 3])
    best = torch.full((h, w), float("inf"), device=dev, dtype=torch.float64)
    for axis, c in ((0, ROOM[0]), (0, -ROOM[0]), (1, ROOM[1]), (1, -ROOM[1]), (2, ROOM[2])):
        s = (c - o[axis]) / ray[..., axis]
        best = torch.where((s > 1e-3) & (s < best), s, best)
    return best.float()


def build_room(args, dev, size):
    """-> (volume, K, the frame's depth, the predicted pose C): the room integrated from three cameras at `size`, and a frame to track."""
    from simpledepthestimation_amd.hip.present import device_maps
    from simpledepthestimation_amd.hip.volume import TsdfVolume
    dims = tuple(args.dims)
    vol = TsdfVolume(dims, args.voxel, origin=(-dims[0] * args.voxel / 2, -dims[1] * args.voxel / 2, 0.0), min_depth=0.1, max_depth=dims[2] * args.voxel,
                     colour=False, device=dev)
    h, w = size
    K = torch.from_numpy(scaled_K(h, w)).to(dev)
    ymap, xmap = device_maps(np.arange(h, dtype=np.int32), np.arange(w, dtype=np.int32), h, w, dev)
    for deg, t in (((0, 0, 0), (0, 0, 0)), ((0, 3, 0), (0.3, 0, 0)), ((1, -3, 0), (-0.3, 0.1, 0.2))):
        C = pose(deg, t, dev)
        vol.integrate(room_depth(K, C, size), ymap, xmap, K, C)
    C = pose((0.3, 0.5, -0.2), (0.05, -0.02, 0.1), dev)
    true = torch.linalg.inv(pose((0.3, -0.4, 0.2), (args.voxel, -0.5 * args.voxel, 0.8 * args.voxel), dev).double()) @ C.double()
    pred = (room_depth(K, true.float(), size) / 1.03).contiguous()
    return vol, K, pred, ymap, xmap, C


def torch_iteration(pred, K, depth, normal, D, s, lo, hi, dist_tol, scale_tol, damping):
    """One POSE | SCALE iteration from torch operators -> (D', s', pose inliers, scale inliers)."""
    h, w = pred.shape
    dev = pred.device
    v, u = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32), indexing="ij")
    fx, cx, fy, cy = K[0, 0], K[0, 2], K[1, 1], K[1, 2]
    keep = torch.isfinite(pred) & (pred > lo) & (pred <= hi)
    d = s * pred
    p = torch.stack([d * (u - cx) / fx, d * (v - cy) / fy, d], -1)
    q = p @ D[:3, :3].T + D[:3, 3]
    keep = keep & (q[..., 2] > 0)
    den = q[..., 2] + 1e-6
    ix, iy = torch.round((fx * q[..., 0] + cx * q[..., 2]) / den), torch.round((fy * q[..., 1] + cy * q[..., 2]) / den)
    keep = keep & (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
    at = (torch.where(keep, iy, 0).long() * w + torch.where(keep, ix, 0).long()).reshape(-1)
    m = depth.reshape(-1)[at].reshape(h, w)
    n = normal.reshape(-1, 3)[at].reshape(h, w, 3)
    keep = keep & (m > 0) & (n != 0).any(-1)
    g = torch.stack([m * (ix - cx) / fx, m * (iy - cy) / fy, m], -1)
    r = ((q - g) * n).sum(-1)
    inl = keep & (r.abs() <= dist_tol * m)
    J = torch.cat([torch.linalg.cross(q, n), n], -1).double() * inl[..., None]
    A = torch.einsum("hwi,hwj->ij", J, J)
    b = (J * (r.double() * inl)[..., None]).sum((0, 1))
    A = A + torch.diag(torch.diagonal(A)) * damping
    xi = torch.linalg.solve(A, -b)
    a = xi[:3] / 2
    ax = torch.zeros((3, 3), device=dev, dtype=torch.float64)
    ax[0, 1], ax[0, 2], ax[1, 0], ax[1, 2], ax[2, 0], ax[2, 1] = -a[2], a[1], a[2], -a[0], -a[1], a[0]
    T = torch.eye(4, device=dev, dtype=torch.float64)
    T[:3, :3] = ((1 - a @ a) * torch.eye(3, device=dev, dtype=torch.float64) + 2 * torch.outer(a, a) + 2 * ax) / (1 + a @ a)
    T[:3, 3] = xi[3:]
    rho = m / q[..., 2]
    sin = keep & ((rho - 1).abs() <= scale_tol)
    return (T @ D.double()).float(), s * (rho * sin).sum() / sin.sum(), inl.sum(), sin.sum()


def bench_launch(args, dev, size):
    from simpledepthestimation_amd.hip import align as AL
    h, w = size
    vol, K, pred, ymap, xmap, C = build_room(args, dev, size)
    state = AL.AlignState(size, dev)
    kw = dict(AL.DEFAULTS, min_depth=vol.min_depth, max_depth=vol.max_depth)
    out = (state.model_depth, state.model_normal, None)
    render = lambda: vol.render(K, C, size, normals=True, picture=False, out=out)
    align = lambda: AL.frame_align(pred, ymap, xmap, K, state.model_depth, state.model_normal, state, mode=AL.POSE | AL.SCALE, **kw)
    render()
    state.reset()
    align()
    first = state.info()
    td, ts, tin, tsin = torch_iteration(pred, K, state.model_depth, state.model_normal, torch.eye(4, device=dev), torch.ones((), device=dev), vol.min_depth,
                                        vol.max_depth, kw["dist_tol"], kw["scale_tol"], kw["damping"])
    agree = max(float((td - state.D).abs().max()), abs(float(ts) - first["scale"]))
    if args.trace_only:
        for _ in range(args.reps):
            align()
        torch.cuda.synchronize()
        return {"bench": "track_trace", "size": [h, w], "iterations": args.reps + 1}
    graphs = {}
    for name, call in (("align", align), ("render", render)):
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
                state.reset()
                rounds[name].append(us(graphs[name]))
        med = {k: float(np.median(v)) for k, v in rounds.items()}
        runs.append({"align_us": rounds["align"], "render_us": rounds["render"], "align_median_us": med["align"], "render_median_us": med["render"],
                     "spread_pct": round(100 * max((max(v) - min(v)) / med[k] for k, v in rounds.items()), 2)})
    last = state.info()
    torch_us = []
    D0, s0 = torch.eye(4, device=dev), torch.ones((), device=dev)
    for _ in range(2):
        torch_iteration(pred, K, state.model_depth, state.model_normal, D0, s0, vol.min_depth, vol.max_depth, kw["dist_tol"], kw["scale_tol"], kw["damping"])
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.torch_reps):
            torch_iteration(pred, K, state.model_depth, state.model_normal, D0, s0, vol.min_depth, vol.max_depth, kw["dist_tol"], kw["scale_tol"], kw["damping"])
        b.record()
        torch.cuda.synchronize()
        torch_us.append(round(a.elapsed_time(b) * 1e3 / args.torch_reps, 1))
    rows = AL.slab_rows(h, w)
    nbytes = {"depth": 4 * h * w, "model_upper": 16 * h * w, "maps": 4 * (h + w), "slab_written": 128 * rows, "slab_read": 128 * rows, "state": 2 * 160}
    return {"bench": "track_launch", "dims": list(vol.dims), "voxel": args.voxel, "size": [h, w], "reps": args.reps, "replays": args.replays, "runs": runs,
            "torch_us": torch_us, "torch_over_align": [round(t / r["align_median_us"], 1) for t, r in zip(torch_us, runs)], "torch_agree": agree,
            "inlier_pct": [round(100 * first["count"] / (h * w), 2), round(100 * first["scale_count"] / (h * w), 2)],
            "torch_inlier_pct": [round(100 * int(tin) / (h * w), 2), round(100 * int(tsin) / (h * w), 2)], "status_first_last": [first["status"], last["status"]],
            "hit_pct": round(100 * float((state.model_depth != 0).float().mean()), 2), "workgroups": rows, "bytes": nbytes, "bytes_total": sum(nbytes.values())}


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
    dims = tuple(args.stream_dims)
    m = float(np.median(next(iter(pair_p.stream(frames(1 + span), KITTI_K, present=False)))["depth_net"]))
    voxel = 4 * m / dims[0]
    vol = TsdfVolume(dims, voxel, origin=(-dims[0] * voxel / 2, -dims[1] * voxel / 2, m / 4), min_depth=0.0, max_depth=1e6, device=dev)
    track = dict(near=m / 8, far=m / 4 + dims[2] * voxel, step=voxel)

    def timed(run, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = run(k)
        torch.cuda.synchronize()
        return got / (time.perf_counter() - t0)

    run_v = lambda k: len([r["world_to_camera"][0, 0] for r in pair_p.stream(frames(k + span), KITTI_K, volume=vol)])
    seen = []
    run_t = lambda k: len([seen.append((r["track_status"], r["track_count"])) for r in pair_p.stream(frames(k + span), KITTI_K, volume=vol, track=track)])
    run_v(args.warmup)
    run_t(args.warmup)
    fv, ft = [], []
    for _ in range(3):                                                   # alternating rounds: the two routes see the same neighbours
        fv.append(round(timed(run_v, args.frames), 2))
        ft.append(round(timed(run_t, args.frames), 2))
    mv, mt = float(np.median(fv)), float(np.median(ft))
    cost = 100 * (mv - mt) / mv
    spread = 100 * max((max(fv) - min(fv)) / mv, (max(ft) - min(ft)) / mt)
    ok = sum(1 for s, _ in seen if s == 0)
    return {"bench": "track_stream", "model": "MonoDepth2", "dtype": args.dtype, "frame": [H, W], "net": [NET_H, NET_W], "frames": args.frames, "dims": list(dims),
            "samples": int(np.ceil((np.float32(track["far"]) - np.float32(track["near"])) / np.float32(voxel))), "iterations_per_window": 4,
            "volume_stream_fps": fv, "track_stream_fps": ft, "track_cost_pct": round(cost, 2), "spread_pct": round(spread, 2),
            "resolved": bool(abs(cost) > spread), "ms_per_window_difference": round(1e3 / mt - 1e3 / mv, 3),
            "windows_with_status_ok_pct": round(100 * ok / max(len(seen), 1), 1), "inliers_last_window": int(seen[-1][1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--dims", type=int, nargs=3, default=[256, 128, 256])
    ap.add_argument("--voxel", type=float, default=0.05)
    ap.add_argument("--stream-dims", type=int, nargs=3, default=[256, 256, 128])
    ap.add_argument("--sizes", type=int, nargs="+", default=[192, 640, 375, 1242], help="H W pairs")
    ap.add_argument("--no-stream", action="store_true")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_track.py measures on the GPU; there is no CPU fallback"
    dev = "cuda:0"

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if not args.trace_only:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    for h, w in zip(args.sizes[::2], args.sizes[1::2]):
        emit(bench_launch(args, dev, (h, w)))
    if not args.no_stream and not args.trace_only:
        emit(bench_stream(args, dev))


if __name__ == "__main__":
    main()

"""Raw LiDAR scans -> depth ground truth: what the projection costs per frame, and what it costs a training step.

    python scripts/bench_lidar.py [--out profiles/lidar_bench.txt] [--steps 60] [--workers 16] [--runs 2] [--only-frame | --only-feeds]

1. Per frame, 375 x 1242, one synthetic scan of 120 k points (64 rings over 360 degrees, 2-80 m), --runs runs each:
     published   generate_depth_map of monodepth2 / packnet-sfm as published: float64 numpy, np.round, sub2ind + Counter for the duplicates
     host twin   hip.lidar.lidar_depth_np: float32, np.minimum.at on the bit patterns
     kernel      sde_lidar_depth alone, points resident: one scan per call, and twelve scans per call (per frame)
     + upload    the same with the padded scan ([131072,3] fp32, pinned) copied host -> device in front of every call
2. Supervised ResNet-50, bf16, batch 12, 192 x 640, with the input side in the timed region -- bench.py --with-loader's arrangement (uint8 frames at
   375 x 1242 through DevicePrefetcher, resize + jitter kernels at the head of the step), taken as the parent's number and re-measured here --
   under four feeds of the `depth` entry, each in a child process of its own, --runs times in alternating order:
     resident      one batch resident on the device (bench.py without --with-loader)
     png           depth arrives as a finished fp32 [12,1,192,640] map (what LoadDepth hands over; bench.py --with-loader as it is)
     lidar_host    LidarDepth host mode: --workers loader workers run lidar_depth_np per frame into the 192 x 640 window, the map is uploaded as in `png`
     lidar_device  LidarDepth ON_DEVICE: padded scans [12,131072,3] are uploaded and DeviceImageAug projects them at the head of the step
   As in bench.py, decoding files (PNG frames, .bin scans) is not part of the measurement; the frames are the same pinned buffers in every feed.
   The depth window of the two lidar feeds is a 192 x 640 crop of the full image: Resize does not fold into a projection window, so the image
   side (resized) and the depth side (cropped) are two measurements sharing a step, not one coherent sample.

Writes the report to --out and prints it."""
import argparse
import json
import os
import subprocess
import sys
import time
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H_FULL, W_FULL, N_POINTS, CAP = 375, 1242, 120000, 131072
B, H, W, WINDOW = 12, 192, 640, (301, 150)              # the window's origin: inside the KBCrop region, where the scan lands
FEEDS = ("resident", "png", "lidar_host", "lidar_device")
# KITTI raw 2011_09_26: P_rect_02 @ R_rect_00 @ Tr_velo_to_cam, rounded to float32
PROJ = np.array([[6.0969543e+02, -7.2142157e+02, -1.2512581e+00, -1.2304182e+02],
                 [1.8038420e+02, 7.6447983e+00, -7.1965149e+02, -1.0101669e+02],
                 [9.9994534e-01, 1.2436534e-04, 1.0451303e-02, -2.6938692e-01]], np.float32)


def synthetic_scan(seed, n=N_POINTS):
    """A spinning 64-ring scanner: azimuth uniform over the circle, elevation uniform over +2 .. -24.9 degrees, range 2-80 m; [n,3] float32."""
    r = np.random.default_rng(seed)
    az, el, rg = r.uniform(-np.pi, np.pi, n), np.deg2rad(r.uniform(-24.9, 2.0, n)), r.uniform(2.0, 80.0, n) ** 0.5 * 80.0 ** 0.5
    return np.stack([rg * np.cos(el) * np.cos(az), rg * np.cos(el) * np.sin(az), rg * np.sin(el)], 1).astype(np.float32)


def published(velo, P_velo2im, im_shape, vel_depth=False):
    """generate_depth_map (monodepth2 kitti_utils.py) from the scan on: the published statements, float64."""
    velo = np.concatenate([velo.astype(np.float64), np.ones((len(velo), 1))], 1)
    velo = velo[velo[:, 0] >= 0, :]
    velo_pts_im = np.dot(P_velo2im.astype(np.float64), velo.T).T
    velo_pts_im[:, :2] = velo_pts_im[:, :2] / velo_pts_im[:, 2][..., np.newaxis]
    if vel_depth:
        velo_pts_im[:, 2] = velo[:, 0]
    velo_pts_im[:, 0] = np.round(velo_pts_im[:, 0]) - 1
    velo_pts_im[:, 1] = np.round(velo_pts_im[:, 1]) - 1
    val_inds = (velo_pts_im[:, 0] >= 0) & (velo_pts_im[:, 1] >= 0)
    val_inds = val_inds & (velo_pts_im[:, 0] < im_shape[1]) & (velo_pts_im[:, 1] < im_shape[0])
    velo_pts_im = velo_pts_im[val_inds, :]
    depth = np.zeros(im_shape[:2])
    depth[velo_pts_im[:, 1].astype(int), velo_pts_im[:, 0].astype(int)] = velo_pts_im[:, 2]
    inds = velo_pts_im[:, 1].astype(int) * im_shape[1] + velo_pts_im[:, 0].astype(int)
    dupe_inds = [item for item, count in Counter(inds).items() if count > 1]
    for dd in dupe_inds:
        pts = np.where(inds == dd)[0]
        depth[int(velo_pts_im[pts[0], 1]), int(velo_pts_im[pts[0], 0])] = velo_pts_im[pts, 2].min()
    depth[depth < 0] = 0
    return depth


def per_frame(a):
    import torch
    from simpledepthestimation_amd.hip.lidar import lidar_depth, lidar_depth_np
    dev = torch.device("cuda:0")
    scan = synthetic_scan(0)
    front = scan[scan[:, 0] >= 0]
    lines = [f"scan: {len(scan)} points, {len(front)} with x >= 0; frame {H_FULL} x {W_FULL}"]
    ref = published(scan, PROJ, (H_FULL, W_FULL))
    twin = lidar_depth_np(scan, PROJ, (0, 0), H_FULL, W_FULL)
    lines.append(f"non-zero pixels: published {int((ref != 0).sum())}, host twin {int((twin != 0).sum())}, occupancy differs at {int(((ref != 0) != (twin != 0)).sum())} "
                 f"(float32 against float64 rounding near k + 0.5)")

    def host_ms(fn, reps):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t0) / reps * 1e3

    padded = np.zeros((B, CAP, 3), np.float32)
    padded[:, :len(front)] = front
    pinned = torch.from_numpy(padded).pin_memory()
    pts = pinned.to(dev)
    cnt = torch.full((B,), len(front), dtype=torch.int32, device=dev)
    proj = torch.from_numpy(np.stack([PROJ] * B)).to(dev)
    org = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    out = torch.empty((B, 1, H_FULL, W_FULL), device=dev)
    got = lidar_depth(pts[:1], cnt[:1], proj[:1], org[:1], H_FULL, W_FULL, out=out[:1])[0, 0].cpu().numpy()
    lines.append(f"kernel against host twin: {'bit-equal' if np.array_equal(got, twin) else 'DIFFERENT'}")

    def dev_us(n, upload, reps=200):
        def call():
            if upload:
                pts[:n].copy_(pinned[:n], non_blocking=True)
            lidar_depth(pts[:n], cnt[:n], proj[:n], org[:n], H_FULL, W_FULL, out=out[:n])
        for _ in range(10):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3
    for run in range(a.runs):
        lines.append(f"run {run + 1}: published numpy {host_ms(lambda: published(scan, PROJ, (H_FULL, W_FULL)), 3):8.2f} ms/frame   "
                     f"host twin {host_ms(lambda: lidar_depth_np(scan, PROJ, (0, 0), H_FULL, W_FULL), 5):8.2f} ms/frame")
        k1, k12, u1, u12 = dev_us(1, False), dev_us(B, False), dev_us(1, True), dev_us(B, True)
        lines.append(f"run {run + 1}: kernel alone {k1:7.1f} us/call at 1 scan, {k12 / B:7.1f} us/frame at {B} per call   "
                     f"with upload ({CAP * 12 / 1e6:.2f} MB/frame) {u1:7.1f} us at 1 scan, {u12 / B:7.1f} us/frame at {B} per call")
    return lines


class _Scans:
    """lidar_host's dataset: item i = the host-mode depth map of one of eight scans in the training window, clipped at 80 m."""

    def __init__(self):
        self.scans = [synthetic_scan(s) for s in range(8)]

    def __len__(self):
        return 1 << 30

    def __getitem__(self, i):
        from simpledepthestimation_amd.hip.lidar import lidar_depth_np
        return lidar_depth_np(self.scans[i % 8], PROJ, WINDOW, H, W, max_depth=80.0)[None]


def run_feed(name, a):
    import torch
    it = None
    if name == "lidar_host":                # the workers are forked before this process opens the GPU
        loader = torch.utils.data.DataLoader(_Scans(), batch_size=B, num_workers=a.workers, collate_fn=lambda xs: torch.from_numpy(np.stack(xs, 0)))
        it = iter(loader)
        first = next(it)
    import bench as BM
    from simpledepthestimation_amd.data import DevicePrefetcher
    from simpledepthestimation_amd.data.device_aug import DeviceImageAug
    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    ns = argparse.Namespace(workload="sup_r50", dtype="bf16", no_graph=False, force_overlap=False, no_pose_stream=False)
    cfg, model, trainer = BM.build(ns, device)
    n_warm, res = 36, {}
    if name == "resident":
        batch = BM.synth_batch("SupDepthModel", B, H, W, 1000, device)
        step = lambda: trainer.step(batch)
    else:
        trainer.input_transform = DeviceImageAug(device)
        gen, nbytes = BM.host_loader("SupDepthModel", B, H, W, 2000, n_warm + a.steps)
        depth_bytes = B * H * W * 4
        if name == "lidar_host":
            def feed_gen():
                d = first
                for hb in gen:
                    hb["depth"] = d
                    yield hb
                    d = next(it)
        elif name == "lidar_device":
            front = [s[s[:, 0] >= 0] for s in (synthetic_scan(k) for k in range(B))]
            pts = np.zeros((B, CAP, 3), np.float32)
            for b, f in enumerate(front):
                pts[b, :len(f)] = f
            raw = {"lidar_points": torch.from_numpy(pts).pin_memory(), "lidar_count": torch.tensor([len(f) for f in front], dtype=torch.int32).pin_memory(),
                   "lidar_proj": torch.from_numpy(np.stack([PROJ] * B)).pin_memory(), "lidar_window": torch.tensor([[WINDOW[0], WINDOW[1], W, H]] * B, dtype=torch.int32),
                   "lidar_clip": torch.full((B,), 80.0), "lidar_flags": torch.full((B,), 2, dtype=torch.int32)}
            nbytes += sum(raw[k].numel() * raw[k].element_size() for k in ("lidar_points", "lidar_count", "lidar_proj")) + B * 8 - depth_bytes

            def feed_gen():
                for hb in gen:
                    hb.pop("depth")
                    hb.update(raw)
                    yield hb
        else:
            feed_gen = lambda: gen
        res["h2d_bytes_per_step"] = int(nbytes)
        feed = iter(DevicePrefetcher(feed_gen(), device))
        step = lambda: trainer.step(next(feed))
    for _ in range(n_warm):
        losses = step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        losses = step()
    torch.cuda.synchronize()
    res["ms_per_step"] = round((time.perf_counter() - t0) / a.steps * 1e3, 3)
    final = {k: float(v.item()) for k, v in losses.items()}
    assert all(np.isfinite(x) for x in final.values()), final
    res["loss"] = round(sum(final.values()), 5)
    del it
    return res


def feeds(a):
    lines, ms, info = [], {f: [] for f in FEEDS}, {}
    for run in range(a.runs):
        for name in FEEDS:
            cmd = [sys.executable, os.path.abspath(__file__), "--feed", name, "--steps", str(a.steps), "--workers", str(a.workers)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit, cwd=ROOT)
            if p.returncode != 0:               # a fault or an abort: nothing more is started on the device
                raise SystemExit(f"feed {name} ended with status {p.returncode}")
            r = json.loads(p.stdout.strip().splitlines()[-1])
            ms[name].append(r["ms_per_step"])
            info[name] = r
            print(f"# run {run + 1} {name}: {r}", file=sys.stderr, flush=True)
    lines.append(f"Supervised ResNet-50 bf16, batch {B}, {H} x {W}, {a.steps} timed steps behind 36 warm-up steps, {a.workers} loader workers; ms per step, {a.runs} runs each")
    for name in FEEDS:
        mb = f"{info[name]['h2d_bytes_per_step'] / 1e6:7.2f} MB uploaded per step" if "h2d_bytes_per_step" in info[name] else "nothing uploaded"
        lines.append(f"  {name:13s} " + "  ".join(f"{v:7.3f}" for v in ms[name]) + f"   mean {np.mean(ms[name]):7.3f}   {mb}")
    spread = max(max(v) - min(v) for v in ms.values())
    diff = float(np.mean(ms["lidar_device"]) - np.mean(ms["png"]))
    lines.append(f"  lidar_device - png = {diff:+.3f} ms/step; largest run-to-run spread of a feed {spread:.3f} ms: device mode "
                 + ("stays within" if abs(diff) <= spread else "lies outside") + " the run-to-run spread of the png feed's arrangement")
    lines.append(f"  lidar_host - png = {float(np.mean(ms['lidar_host']) - np.mean(ms['png'])):+.3f} ms/step")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lidar_bench.txt"))
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--only-frame", action="store_true")
    ap.add_argument("--only-feeds", action="store_true")
    ap.add_argument("--feed", choices=FEEDS + ("frame",), help="run this one feed (or the per-frame part) in this process and print its JSON line (what the parent starts)")
    ap.add_argument("--limit", type=float, default=300.0, help="seconds a feed's child process may take")
    a = ap.parse_args()
    a.workers = min(a.workers, 16)
    if a.feed:
        print(json.dumps(per_frame(a) if a.feed == "frame" else run_feed(a.feed, a)))
        return
    lines = ["# scripts/bench_lidar.py: raw LiDAR scans -> depth ground truth (sde_lidar_depth, hip/lidar.py), MI355X"]
    if not a.only_feeds:
        # in a child of its own as well: this process never opens the GPU
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--feed", "frame", "--runs", str(a.runs)], stdout=subprocess.PIPE, text=True, timeout=a.limit, cwd=ROOT)
        if p.returncode != 0:
            raise SystemExit(f"the per-frame measurement ended with status {p.returncode}")
        lines += ["", "1. per frame"] + json.loads(p.stdout.strip().splitlines()[-1])
    if not a.only_frame:
        lines += ["", "2. training step with the input side in the timed region"] + feeds(a)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

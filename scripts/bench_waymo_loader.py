"""MotionLearning on Waymo with the data loader in the loop: IMS_PER_BATCH 16, 1280 x 1920 JPEG frames, CropTopTo 1152, Resize to 192 x 320
(projects/MotionLearning/configs/resnet18_waymo.yaml over Base_waymo.yaml, get_project_cfg("MotionLearningWaymo", datasets=True)); GoogleResNetv2-18 +
GoogleMotionNet, forward + backward replayed as a captured graph, fused grad-norm clip + Adam, as scripts/bench_motion_train.py runs it.

Four ways of feeding the same trainer, each timed over --steps steps after --warmup (wall clock between two synchronisations, ms per step):

    static     one batch resident on the device                                            (the step alone)
    host       WaymoDepth loader, Resize / RandomImageAug on the host, fp32 batches through DevicePrefetcher
    device     ON_DEVICE: True  -- uint8 frames at source size (1152 x 1920) cross PCIe, DeviceImageAug resizes and jitters behind the upload
    taps       ON_DEVICE: "taps" -- only the rows and columns the resize reads (384 x 640) cross PCIe, with renumbered tap tables

and, for the two device routes, the frame bytes uploaded per step.  The tree is synthetic and built here, in a temporary directory: --frames full-size
JPEG frames and mask PNGs in two segments, read over and over through the infinite TrainingSampler.  The loader's workers decode the same JPEGs in
every variant; what differs is the resize (host / device) and the bytes per frame.

    python scripts/bench_waymo_loader.py [--steps N] [--warmup W] [--workers 16] [--frames 32] [--b 16] [--dtype bf16|fp32] [--only VARIANT ...]

Every variant runs in a child process of its own (its loader forks the workers before the child opens the GPU; a child that fails ends the run).
Prints one JSON line."""
import argparse
import json
import os
import pickle
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = ("static", "host", "device", "taps")
SRC_H, SRC_W, CROP_H, IMG_H, IMG_W = 1280, 1920, 1152, 192, 320


def make_tree(root, frames, seed=0):
    """Two segments of frames / 2 FRONT frames each: smooth colour fields with texture (JPEG decode cost close to a camera frame's), masks with a few boxes."""
    from PIL import Image
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:SRC_H, 0:SRC_W].astype(np.float32)
    infos = {}
    for si in range(2):
        seg = f"segment-{si:04d}"
        K = np.eye(4)
        K[0, 0] = K[1, 1] = 2055.0
        K[0, 2], K[1, 2] = SRC_W / 2, SRC_H / 2
        fr = {}
        for i in range(frames // 2):
            t = 1550000000000000 + 10 ** 9 * si + 100000 * i
            fr[t] = {"cams": {"FRONT": t + 7}}
            for sub in ("image", "segmentation"):
                os.makedirs(os.path.join(root, sub, seg, "FRONT"), exist_ok=True)
            ph = r.uniform(0, 6.28, 3)
            img = np.stack([127 + 90 * np.sin(x / (40 + 25 * c) + ph[c] + 0.02 * i) * np.cos(y / (55 + 15 * c)) for c in range(3)], -1)
            img = np.clip(img + r.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(root, "image", seg, "FRONT", f"{t + 7}.jpg"), quality=90)
            m = np.zeros((SRC_H, SRC_W), np.uint8)
            for k in range(4):
                y0, x0 = int(r.integers(200, SRC_H - 200)), int(r.integers(0, SRC_W - 300))
                m[y0:y0 + int(r.integers(60, 200)), x0:x0 + int(r.integers(80, 300))] = k + 1
            Image.fromarray(m).save(os.path.join(root, "segmentation", seg, "FRONT", f"{t + 7}.png"))
        infos[seg] = {"cams": {"FRONT": {"intrinsics": K, "extrinsics": np.eye(4)}}, "frames": fr}
    with open(os.path.join(root, "infos.pkl"), "wb") as f:
        pickle.dump(infos, f)


def make_cfg(root, a, on_device):
    from simpledepthestimation_amd.config import get_project_cfg
    cfg = get_project_cfg("MotionLearningWaymo", datasets=True)
    d = cfg.DATASETS.TRAIN
    d.DATA_ROOT, d.DEPTH_ROOT, d.MASK_ROOT, d.SPLIT, d.DOWNSAMPLE = os.path.join(root, "image"), os.path.join(root, "depth"), os.path.join(root, "segmentation"), \
        os.path.join(root, "infos.pkl"), 1
    steps = [dict(s) for s in d.PREPROCESS]
    for s in steps:
        if s["NAME"] in ("Resize", "RandomImageAug") and on_device:
            s["ON_DEVICE"] = on_device
    d.PREPROCESS = steps
    assert [(s.get("IMG_H"), s.get("IMG_W")) for s in steps if s["NAME"] == "Resize"] == [(IMG_H, IMG_W)] and steps[2]["IMG_H"] == CROP_H
    cfg.SOLVER.IMS_PER_BATCH, cfg.DATALOADER.NUM_WORKERS, cfg.DATALOADER.SAMPLER_TRAIN = a.b, a.workers, "TrainingSampler"
    cfg.MODEL.DEVICE, cfg.MODEL.COMPUTE_DTYPE = "cuda:0", a.dtype
    return cfg


def frame_bytes(batch):
    def size(v):
        if isinstance(v, (list, tuple)):
            return sum(size(x) for x in v)
        return int(v.numel() * v.element_size()) if torch.is_tensor(v) else int(np.asarray(v).nbytes)
    return sum(size(batch[k]) for k in ("img_u8", "ctx_img_u8") if k in batch)


def run_variant(name, root, a):
    from simpledepthestimation_amd.data import DevicePrefetcher, build_detection_train_loader
    from simpledepthestimation_amd.data.device_aug import DeviceImageAug
    from simpledepthestimation_amd.engine.trainer import motion_learning_trainer
    from simpledepthestimation_amd.modeling import build_model
    on_device = {"static": False, "host": False, "device": True, "taps": "taps"}[name]
    cfg = make_cfg(root, a, on_device)
    if name == "static":
        cfg.DATALOADER.NUM_WORKERS = 0
    # the workers are forked BEFORE this process touches the GPU (the first HIP call is build_model's): they never hold the device open
    loader = build_detection_train_loader(cfg)
    it = iter(loader)
    host_first = next(it)
    torch.manual_seed(0)
    tr = motion_learning_trainer(build_model(cfg).train(), cfg, use_graph=True)
    res, counted = {}, [frame_bytes(host_first)]

    def stream():
        b = host_first
        while True:
            b["flip"] = False                   # one captured graph: the flip draw stays in the workers' chain, its value is not the subject here
            yield b
            b = next(it)
    if name == "static":
        first = next(iter(DevicePrefetcher([dict(host_first, flip=False)], "cuda:0")))
        batches = (first for _ in range(a.warmup + a.steps))
    else:
        batches = iter(DevicePrefetcher(stream(), "cuda:0", device_aug=DeviceImageAug("cuda:0") if on_device else None))
    for _ in range(a.warmup):
        tr.step(next(batches))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = tr.step(next(batches))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.steps * 1e3
    res.update(ms_per_step=round(ms, 2), images_per_s=round(a.b / ms * 1e3, 1), loss=round(float(sum(float(v.detach()) for v in out.values())), 5))
    if on_device:
        res["frame_bytes_per_step"] = counted[0]
        res["frame_mb_per_step"] = round(counted[0] / 1e6, 2)
    del batches, it
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--b", type=int, default=16)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--only", nargs="*", choices=VARIANTS)
    ap.add_argument("--root", help="an existing tree (make_tree): run the one variant of --only in this process")
    ap.add_argument("--limit", type=float, default=240.0, help="seconds a variant's child process may take")
    a = ap.parse_args()
    a.workers = min(a.workers, 16)
    line = {"workload": "motion_learning_waymo_with_loader", "batch": a.b, "source": [SRC_H, SRC_W], "crop_h": CROP_H, "size": [IMG_H, IMG_W], "dtype": a.dtype,
            "workers": a.workers, "frames_on_disk": a.frames, "steps": a.steps, "warmup": a.warmup}
    if a.root:                                  # one variant, in this process, over a tree that exists (what the parent below starts)
        if not torch.cuda.is_available():
            raise SystemExit("bench_waymo_loader.py needs a GPU: a CPU run measures nothing")
        print(json.dumps(run_variant(a.only[0], a.root, a)))
        return
    # every variant in a fresh child process: its loader forks the workers before the child opens the GPU
    import subprocess
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        make_tree(root, a.frames)
        line["tree_s"] = round(time.perf_counter() - t0, 1)
        for name in (a.only or VARIANTS):
            cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--only", name, "--steps", str(a.steps), "--warmup", str(a.warmup),
                   "--workers", str(a.workers), "--b", str(a.b), "--dtype", a.dtype]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)
            if p.returncode != 0:               # a fault or an abort: nothing more is started on the device
                line[name] = {"failed": p.returncode}
                print(json.dumps(line))
                raise SystemExit(f"variant {name} ended with status {p.returncode}")
            line[name] = json.loads(p.stdout.strip().splitlines()[-1])
            print(f"# {name}: {line[name]}", file=sys.stderr, flush=True)
    print(json.dumps(line))


if __name__ == "__main__":
    main()

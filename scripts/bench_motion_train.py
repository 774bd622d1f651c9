"""One MotionLearning training step at the reference setting (projects/MotionLearning/configs/Base.yaml + resnet18.yaml): IMS_PER_BATCH 16, 128x416,
GoogleResNet-18 (randLN) + GoogleMotionNet in bf16, losses fp32, forward + backward replayed as a captured graph, then the optimizer.  Three variants of
the same trainer in one process, timed alternately:

    off        no gradient clipping                                     (Adam, eps 1e-7)
    fused      HipTrainer(clip_grad=10): sde_grad_norm + the coefficient inside sde_adam_step
    composed   torch.nn.utils.clip_grad_norm_ over the parameters' gradient views (views of the flat gradient), then the same Adam launch

    python scripts/bench_motion_train.py [--reps R] [--runs K] [--b B] [--height H] [--width W] [--dtype bf16|fp32] [--clip C] [--only VARIANT] [--no-graph]

Prints one JSON line: per variant ms per step (median over K runs of the mean of R warm steps between device events; min and max next to it) and images
per second; the flat gradient's size, the bytes the norm pass reads (4 * numel, once) and the time those bytes take at 4 TB/s.  The GPU time of the norm
launches themselves comes from a separate profiler run over `--only fused` (kernels grad_norm_partial_kernel / grad_norm_finalize_kernel)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

VARIANTS = ("off", "fused", "composed")


def build(dtype, dev="cuda:0"):
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.modeling import build_model
    cfg = get_cfg()
    cfg.merge_from_other_cfg({"MODEL": {"META_ARCHITECTURE": "MotionLearningModel", "DEVICE": dev, "COMPUTE_DTYPE": dtype,
                                        "DEPTH_NET": {"NAME": "GoogleResNet", "NORM": "randLN", "NOISE_STDDEV": 0.5, "RAMPUP_ITERS": 10000},
                                        "POSE_NET": {"NAME": "GoogleMotionNet", "USE_DEPTH": True, "GROUP_NORM": False, "MASK_MOTION": True, "LEARN_SCALE": True,
                                                     "SCALE_CONSTRAIN": "clip_ste", "BURN_IN_ITERS": 20000}},
                              "LOSS": {"NUM_SCALES": 1, "SSIM_WEIGHT": 3.0, "C1": "inf", "C2": 9e-6, "CLIP": 0.0, "DEPTH_L1_WEIGHT": 0.0, "SMOOTHNESS_WEIGHT": 1e-3,
                                       "SUPERVISED_WEIGHT": 0.0, "VAR_LOSS_WEIGHT": 0.0, "MOTION_SMOOTHNESS_WEIGHT": 1.0, "MOTION_SPARSITY_WEIGHT": 0.2,
                                       "ROT_CYCLE_WEIGHT": 1e-3, "TRANS_CYCLE_WEIGHT": 5e-2, "SCALE_NORMALIZE": False},
                              "SOLVER": {"IMS_PER_BATCH": 16, "DEPTH_LR": 2e-4, "POSE_LR": 2e-4}})
    cfg.MODEL.DEPTH_NET.ENCODER_NAME = "18"
    torch.manual_seed(0)
    return build_model(cfg).train(), cfg


def make_trainer(variant, a):
    from simpledepthestimation_amd.engine.trainer import motion_learning_trainer
    model, cfg = build(a.dtype)
    tr = motion_learning_trainer(model, cfg, use_graph=not a.no_graph, clip_grad=a.clip if variant == "fused" else None)
    if variant == "composed":
        params = [p for g in tr.groups for _, p in g.named_params]
        plain = tr._optimizer

        def composed():
            tr.composed_norm = torch.nn.utils.clip_grad_norm_(params, a.clip)
            plain()
        tr._optimizer = composed
    return tr


def timed(tr, batch, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = tr.step(batch)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--b", type=int, default=16)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=416)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--clip", type=float, default=10.0)
    ap.add_argument("--only", choices=VARIANTS)
    ap.add_argument("--no-graph", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_motion_train.py needs a GPU: a CPU run measures nothing")
    import motion_loss_init as MI
    v = MI.inputs(a.b, a.height, a.width)
    batch = {"img": v["frame1"].cuda(), "ctx_img": [v["frame2"].cuda()], "intrinsics": v["K"].cuda()}
    names = [a.only] if a.only else list(VARIANTS)
    trainers = {n: make_trainer(n, a) for n in names}
    for tr in trainers.values():               # the capture and a few warm steps of every variant before any timed window
        for _ in range(5):
            tr.step(batch)
    torch.cuda.synchronize()
    times, last = {n: [] for n in names}, {}
    for _ in range(a.runs):                    # the variants alternate inside every run
        for n in names:
            ms, out = timed(trainers[n], batch, a.reps)
            times[n].append(ms)
            last[n] = out
    numel = next(iter(trainers.values())).numel
    line = {"workload": "motion_learning_train_step", "batch": a.b, "size": [a.height, a.width], "dtype": a.dtype, "graph": not a.no_graph, "clip": a.clip,
            "reps": a.reps, "runs": a.runs, "grad_numel": numel, "norm_pass_bytes": 4 * numel, "norm_pass_us_at_4TBps": round(4 * numel / 4e12 * 1e6, 2)}
    for n in names:
        t = times[n]
        med = statistics.median(t)
        line[n] = {"ms_per_step": round(med, 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "images_per_s": round(a.b / med * 1e3, 1),
                   "loss": round(float(sum(float(x.detach()) for x in last[n].values())), 5)}
    if "fused" in trainers:
        line["fused"]["grad_norm"], line["fused"]["clip_coef"] = (round(float(x), 5) for x in trainers["fused"].clip_state)
    if "composed" in trainers:
        line["composed"]["grad_norm"] = round(float(trainers["composed"].composed_norm), 5)
    if not a.only:
        line["fused_minus_off_ms"] = round(line["fused"]["ms_per_step"] - line["off"]["ms_per_step"], 3)
        line["composed_minus_off_ms"] = round(line["composed"]["ms_per_step"] - line["off"]["ms_per_step"], 3)
    print(json.dumps(line))


if __name__ == "__main__":
    main()

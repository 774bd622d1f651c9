"""BtsModel (projects/Supervised/configs/bts_r50.yaml) training step: bf16, bs 8, 352x704, hipGraph replay.  Prints one JSON line.

    python scripts/bench_bts.py [--steps K] [--warmup W] [--bs B] [--dtype bf16|fp32] [--no-graph]
                                [--encoder resnet50_bts|resnet101_bts|resnext101_bts|densenet121_bts] [--gconv-composed] [--layers]
                                [--dense-composed] [--dense-ops]

--dense-composed runs the dense blocks of a DenseNet encoder through cat + channel_stats + BatchNorm (hip.dense.DENSE_DIRECT = False, the A/B baseline).
--dense-ops times, instead of the step, the norm1 of the last (widest) layer of each DenseNet-121 block stand-alone at the workload's shapes: the
concat-free forward and backward and the gradient gather of a middle piece, against cat + channel_stats + BatchNorm forward and backward.

--gconv-composed runs the grouped convolutions of a ResNeXt encoder as dense block-diagonal layers (hip.nn.GCONV_DIRECT = False, the A/B baseline).
--layers times, instead of the step, every distinct grouped 3x3 layer of the chosen encoder stand-alone at the workload's shapes: forward, data
gradient and weight gradient, on the grouped kernels and on the composed route (its GEMMs only: the dense weight's assembly and pack are not counted),
with the kernels' ideal traffic (x + y, dz + dx, x + dz) over time as a fraction of 6.3 TB/s.

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


def make(bs, H, W, dtype, graph, encoder="resnet50_bts"):
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.engine.trainer import supervised_trainer
    from simpledepthestimation_amd.modeling import build_model
    cfg = get_cfg()
    cfg.MODEL.META_ARCHITECTURE, cfg.MODEL.DEVICE, cfg.MODEL.DATASET, cfg.MODEL.COMPUTE_DTYPE = "SupDepthModel", "cuda:0", "kitti", dtype
    cfg.MODEL.DEPTH_NET.NAME, cfg.MODEL.DEPTH_NET.ENCODER_NAME, cfg.MODEL.DEPTH_NET.BTS_SIZE = "BtsModel", encoder, 512
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


def grouped_layers(encoder, H, W):
    """[(C, groups, stride, h, w, count)]: the distinct grouped 3x3 layers of the encoder with their input sizes for an H x W image."""
    from simpledepthestimation_amd.layers.hip_modules import HipGroupedConv2d
    from simpledepthestimation_amd.modeling.depth_net.BTSNet import BtsEncoder
    bm = BtsEncoder(encoder).base_model
    h, w = ((H - 1) // 2 + 1 - 1) // 2 + 1, ((W - 1) // 2 + 1 - 1) // 2 + 1          # stem convolution and max-pool, stride 2 each
    found = {}
    for layer in (bm.layer1, bm.layer2, bm.layer3, bm.layer4):
        for blk in layer:
            c = blk.conv2
            if isinstance(c, HipGroupedConv2d):
                key = (c.in_channels, c.groups, c.stride, h, w)
                found[key] = found.get(key, 0) + 1
            h, w = (h - 1) // c.stride + 1, (w - 1) // c.stride + 1
    return [k + (n,) for k, n in found.items()]


def time_layers(encoder, bs, H, W, dtype, reps=200):
    from simpledepthestimation_amd.hip import lib as L
    from simpledepthestimation_amd.hip import nn as HN
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    es = 2 if dtype == "bf16" else 4
    rows = []
    for C, G, stride, h, w, count in grouped_layers(encoder, H, W):
        x = torch.randn(bs, h, w, C, device="cuda").to(dt).requires_grad_(True)
        wt = (torch.randn(C, C // G, 3, 3, device="cuda") * 0.05).requires_grad_(True)
        oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
        gy = torch.randn(bs, oh, ow, C, device="cuda").to(dt)
        nx, ny = x.numel() * es, gy.numel() * es
        row = {"C": C, "groups": G, "stride": stride, "in": [bs, h, w], "layers": count}
        for direct in (True, False):
            HN.GCONV_DIRECT = direct
            try:
                for timed in (False, True):           # one untimed pass first (code-object load, allocator)
                    x.grad = wt.grad = None
                    L.PROFILE, L.PROFILE_REPEAT = ([], reps) if timed else (None, 1)
                    HN.grouped_conv3x3(x, wt, G, stride).backward(gy)
                    torch.cuda.synchronize()
                rec = {}
                for kind, _, _, e0, e1, _, rep in L.PROFILE:
                    rec[kind] = rec.get(kind, 0.0) + e0.elapsed_time(e1) / rep * 1e3
            finally:
                L.PROFILE, L.PROFILE_REPEAT, HN.GCONV_DIRECT = None, 1, True
            us = {"fwd": rec.get("igemm_fwd", 0.0), "dgrad": rec.get("igemm_dgrad", 0.0), "wgrad": rec.get("wgrad", 0.0) + rec.get("wgrad_reduce", 0.0)}
            tag = "kernels" if direct else "composed"
            row[tag + "_us"] = {k: round(v, 1) for k, v in us.items()}
            if direct:
                row["hbm_fraction"] = {k: round((nx + ny) / (us[k] * 1e-6) / 6.3e12, 3) for k in us if us[k] > 0}
        rows.append(row)
    return rows


def _timeit(fn, reps):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / reps * 1e3, 1)


def time_dense_ops(bs, H, W, dtype, reps=20):
    """Per block of DenseNet-121: microseconds of the last layer's norm1 + ReLU on both routes (forward; forward + backward), and of one gather."""
    import ctypes
    from simpledepthestimation_amd.hip import bts as HB
    from simpledepthestimation_amd.hip import dense as HD
    from simpledepthestimation_amd.hip import lib as L
    from simpledepthestimation_amd.hip import nn as HN
    from simpledepthestimation_amd.layers.hip_modules import HipBatchNorm2d
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    rows = []
    h, w = ((H - 1) // 2 + 1 - 1) // 2 + 1, ((W - 1) // 2 + 1 - 1) // 2 + 1
    for c0, n in ((64, 6), (128, 12), (256, 24), (512, 16)):
        widths = [c0] + [32] * (n - 1)
        cin = sum(widths)
        pieces = [torch.randn(bs, h, w, c, device="cuda").to(dt) for c in widths]
        gy = torch.randn(bs, h, w, cin, device="cuda").to(dt)
        norm = HipBatchNorm2d(cin).cuda().train()
        head = torch.randn(bs, h, w, cin - 32, device="cuda").to(dt).requires_grad_(True)      # the composed route's concatenation so far
        last = pieces[-1].clone().requires_grad_(True)
        blk = HD.DenseBlock(cin)                # the block as the last layer finds it: every piece filed, the table complete
        for p in pieces:
            HD.dense_piece(p, blk, HB.channel_stats(p))

        def run(direct, backward):
            HD.DENSE_DIRECT = direct
            try:
                if direct:                      # forward: parameters + apply; backward: reduce + apply (the gathers are timed below)
                    del blk.consumers[:]
                    y = HD.dense_bn_relu(blk, norm)
                else:                           # forward: cat + channel_stats + BatchNorm; backward: BatchNorm + the split of the concatenation
                    x = HB.cat([(head, cin - 32), (last, 32)])
                    y = norm(x, HB.channel_stats(x), relu=True)
                if backward:
                    y.backward(gy)
            finally:
                HD.DENSE_DIRECT = True

        # the gather of a middle piece: the dx tensors of the n - j layers behind it
        j = n // 2
        dxs = [torch.randn(bs, h, w, sum(widths[:k]), device="cuda").to(dt) for k in range(j + 1, n + 1)]
        out = torch.empty(bs, h, w, 32, device="cuda", dtype=dt)
        desc = HD._desc(dxs)

        def gather():
            L.check(L.lib().sde_dense_grad_gather(ctypes.byref(desc), bs * h * w, sum(widths[:j]), 32, HN.dtype_code(dt), None, L.ptr(out), L.stream()), "gather")

        row = {"block_input": c0, "layers": n, "Cin": cin, "map": [bs, h, w],
               "direct_fwd_us": _timeit(lambda: run(True, False), reps), "direct_fwd_bwd_us": _timeit(lambda: run(True, True), reps),
               "composed_fwd_us": _timeit(lambda: run(False, False), reps), "composed_fwd_bwd_us": _timeit(lambda: run(False, True), reps),
               "gather_us": _timeit(gather, reps), "gather_sources": len(dxs)}
        rows.append(row)
        h, w = h // 2, w // 2
    return rows


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
    ap.add_argument("--encoder", default="resnet50_bts")
    ap.add_argument("--gconv-composed", action="store_true")
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--dense-composed", action="store_true")
    ap.add_argument("--dense-ops", action="store_true")
    ap.add_argument("--reps", type=int, default=200, help="--layers: back-to-back launches per timed window")
    a = ap.parse_args()
    if a.layers:
        print(json.dumps({"workload": "bts_grouped_layers", "encoder": a.encoder, "dtype": a.dtype, "bs": a.bs, "size": [a.height, a.width],
                          "reps": a.reps,
                          "layers": time_layers(a.encoder, a.bs, a.height, a.width, a.dtype, a.reps)}))
        return
    if a.dense_ops:
        print(json.dumps({"workload": "bts_dense_ops", "dtype": a.dtype, "bs": a.bs, "size": [a.height, a.width],
                          "note": "eager calls between two events, launch path included",
                          "blocks": time_dense_ops(a.bs, a.height, a.width, a.dtype)}))
        return
    if a.gconv_composed:
        from simpledepthestimation_amd.hip import nn as HN
        HN.GCONV_DIRECT = False
    if a.dense_composed:
        from simpledepthestimation_amd.hip import dense as HD
        HD.DENSE_DIRECT = False
    model, tr, batch = make(a.bs, a.height, a.width, a.dtype, not a.no_graph, a.encoder)
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
    line = {"workload": {"resnet50_bts": "bts_r50"}.get(a.encoder, "bts_" + a.encoder[:-4]), "gconv": "composed" if a.gconv_composed else "kernels",
            "dense": "composed" if a.dense_composed else "kernels", "dtype": a.dtype, "bs": a.bs, "size": [a.height, a.width], "graph": not a.no_graph, "steps": a.steps,
            "ms_per_step": round(ms, 3), "images_per_s": round(a.bs * 1000.0 / ms, 1), "loss": loss, "finite": loss == loss}
    if not a.no_dilated:
        line["dilated_fwd"] = time_dilated(a.bs, a.height, a.width, a.dtype)
    print(json.dumps(line))


if __name__ == "__main__":
    main()

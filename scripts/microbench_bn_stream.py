#!/usr/bin/env python
"""Per-launch time of the fused BatchNorm finalize + apply launches (sde_bn_finalize_apply, sde_bn_bwd_from_part) at three ResNet-50 shapes of the
Supervised-R50 step (bf16, batch 12, 192 x 640): layer1 C = 256 with residual, layer3 C = 1024 with residual, layer4 C = 512.

Each launch is timed from captured graphs: `alone` is the replay of a graph that holds one launch (it carries the replay's own launch path), `chain` is
(replay of 41 back-to-back launches - replay of 1) / 40.  Bytes are rows x channels x 2 B per tensor read or written; the rate is bytes / chain time,
against the 6.3 TB/s DESIGN 5 calls achievable.  The buffers are the same for every launch, so the smaller layers stay cache-resident: an upper bound
on what the step sees.  A/B builds:  SDE_HIP_LIB=/path/to/other.so python scripts/microbench_bn_stream.py
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from simpledepthestimation_amd.hip import lib as L, nn as HN  # noqa: E402

DEV = "cuda:0"
# name, C, M, slab rows, residual
LAYERS = [("layer1 C=256 +res", 256, 92160, 192, True), ("layer3 C=1024 +res", 1024, 5760, 90, True), ("layer4 C=512", 512, 1440, 23, False)]
CHAIN = 40


def replay_us(launch, n, reps=30):
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        launch()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            for _ in range(n):
                launch()
    times = []
    for _ in range(reps + 5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(times[5:])


def main():
    print("library:", L.LIB_PATH)
    code = HN.dtype_code(torch.bfloat16)
    gen = torch.Generator().manual_seed(0)
    for name, C, M, rows, with_res in LAYERS:
        y = torch.randn(M, C, generator=gen).to(torch.bfloat16).to(DEV)
        res = torch.randn(M, C, generator=gen).to(torch.bfloat16).to(DEV)
        out = torch.empty_like(y)
        slab = torch.zeros(rows + 64, C, 2)
        slab[:rows, :, 0] = torch.randn(rows, C, generator=gen) * 0.3 * M / rows
        slab[:rows, :, 1] = (torch.rand(rows, C, generator=gen) + 1) * M / rows
        slab = slab.to(DEV)
        gamma, beta, bnp = torch.ones(C, device=DEV), torch.zeros(C, device=DEV), torch.empty(4, C, device=DEV)
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        dgamma, dbeta, coef = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(2, C, device=DEV)

        def fwd():
            L.check(L.lib().sde_bn_finalize_apply(L.ptr(slab), rows, C, M, L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), 0.1, 1e-5, L.ptr(bnp), L.ptr(y),
                                                  L.ptr(res if with_res else None), 1, code, L.ptr(out), L.stream()), "sde_bn_finalize_apply")

        def bwd():
            L.check(L.lib().sde_bn_bwd_from_part(L.ptr(slab), rows, L.ptr(res), L.ptr(y), L.ptr(bnp), M, C, code, L.ptr(coef), L.ptr(dgamma), L.ptr(dbeta), 0,
                                                 L.ptr(out), L.stream()), "sde_bn_bwd_from_part")

        for tag, fn, tensors in (("forward", fwd, 2 + with_res), ("backward", bwd, 3)):
            alone = replay_us(fn, 1)
            chain = (replay_us(fn, CHAIN + 1) - alone) / CHAIN
            nbytes = M * C * 2 * tensors
            print(f"{name:20s} {tag:8s} alone {alone:7.2f} us  chain {chain:7.2f} us/launch  {nbytes / 1e6:7.2f} MB  {nbytes / chain / 1e6:5.2f} TB/s "
                  f"= {nbytes / chain / 1e6 / 6.3 * 100:5.1f} % of 6.3 TB/s")


if __name__ == "__main__":
    main()

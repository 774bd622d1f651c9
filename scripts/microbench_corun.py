"""How much slower does a data-gradient GEMM run while a weight-gradient GEMM of the same layer is resident beside it?

The backward pass runs the data-gradient chain on one queue and the weight-gradient GEMMs on a second one (hip/nn.py: WGradReducer).  Both kernel
families size their workgroups by LDS, so what is resident on a compute unit beside the chain decides how many of the chain's workgroups fit.  Per layer:
  * "alone": REP back-to-back data-gradient launches on stream B between two events;
  * "co-run": the same, while stream A runs back-to-back weight-gradient launches of that layer (enough of them to outlast stream B; B starts after
    A's first launch is enqueued and waits for an event behind it, so A is running when B's first launch starts -- the `A ends after B` column says
    whether A really covered B);
for every LDS ring of the weight-gradient kernel (SDE_OPT_WGRAD_DMA_RING) and every grid size of the persistent GEMM (SDE_OPT_PGEMM_PER_CU) asked for.
min / median / max over ROUNDS interleaved rounds in one process: the spread of "alone" is the noise the co-run slowdown has to beat.

   python scripts/microbench_corun.py [rings, e.g. 0,1,2] [per-CU values, e.g. 4,2]"""
import ctypes, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from simpledepthestimation_amd.hip import nn as HN, lib as L

REP, ROUNDS = 20, 7
dev, dt, B = "cuda", torch.bfloat16, 12
LAYERS = [  # name, H, W, Cin, Cout, k (stride 1): shapes of profiles/r03l_gemm_microbench.txt
    ("l1.c3 64>256", 48, 160, 64, 256, 1), ("l2.c1 256>128", 48, 160, 256, 128, 1), ("l2.c3 128>512", 24, 80, 128, 512, 1),
    ("l3.c1 512>256", 24, 80, 512, 256, 1), ("l3.c2 3x3 256", 12, 40, 256, 256, 3), ("l4.c1 1024>512", 12, 40, 1024, 512, 1),
]


def stats(v):
    v = sorted(v)
    return v[0], v[len(v) // 2], v[-1]


def main():
    rings = [int(t) for t in sys.argv[1].split(",")] if len(sys.argv) > 1 else [0, 1, 2]
    per_cus = [int(t) for t in sys.argv[2].split(",")] if len(sys.argv) > 2 else [4, 2]
    lib = L.lib()
    g = torch.Generator().manual_seed(0)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    print(f"lib: {os.path.relpath(L.LIB_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))}")
    print(f"B={B}, 192x640, bf16; us per data-gradient launch, {REP} back-to-back per event pair, min / median / max of {ROUNDS} rounds")
    print("LDS bytes per workgroup: pgemm", HN.kernel_lds_bytes(HN.KERNEL_PGEMM, 3), " wgrad_dma ring",
          {r: HN.kernel_lds_bytes(HN.KERNEL_WGRAD_DMA, r) for r in rings})
    print(f"{'layer':16s} {'ring':>4s} {'perCU':>5s} {'fwd var':>8s} {'wg grid':>7s} | {'alone min':>9s} {'med':>6s} {'max':>6s} | {'co-run min':>10s} {'med':>6s} {'max':>6s} | "
          f"{'slowdown':>8s} | {'wgrad alone':>11s} {'co-run':>7s} | A ends after B")
    for name, H, W, Cin, Cout, k in LAYERS:
        pad = k // 2
        x0 = torch.randn(B, H, W, Cin, generator=g).to(dt).to(dev)
        dz = torch.randn(B, H, W, Cout, generator=g).to(dt).to(dev)
        w = (torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)).to(dev)
        wd = HN.pack_weight(w, dt, Cin, Cout, for_dgrad=True)
        dd = HN._desc(dz, None, HN.SRC_PLAIN, k, k, 1, k - 1 - pad, False, H, W, H, W)         # the data gradient: a stride-1 convolution of dz
        dw_desc = HN._desc(x0, None, HN.SRC_PLAIN, k, k, 1, pad, False, H, W, H, W)
        splits = lib.sde_conv_wgrad_splits(ctypes.byref(dw_desc), Cout)
        assert lib.sde_conv_wgrad_variant(ctypes.byref(dw_desc), Cout, Cout) == HN.WGRAD_DMA_KERNEL, name
        wg_grid = (Cout // 64) * ((k * k * Cin // 64 + 1) // 2) * splits
        slab = torch.empty(splits, Cout, k * k * Cin, device=dev)
        dx = torch.empty(B, H, W, Cin, device=dev, dtype=dt)
        variant = lib.sde_conv_fwd_variant(ctypes.byref(dd), Cin)
        wsb = lib.sde_conv_fwd_ws_bytes(ctypes.byref(dd), Cin)
        ws = torch.empty(max(wsb, 16) // 4, device=dev)

        def dgrad():
            L.check(lib.sde_conv_fwd_ws(ctypes.byref(dd), L.ptr(wd), None, 0, L.ptr(dx), Cin, Cin, None, L.ptr(ws) if wsb else None, wsb, L.stream()), "dgrad")

        def wgrad():
            L.check(lib.sde_conv_wgrad_partial(ctypes.byref(dw_desc), L.ptr(dz), Cout, Cout, L.ptr(slab), splits, L.stream()), "wgrad")

        def timed(stream, fn, n, after=None):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                if after is not None:
                    stream.wait_event(after)
                e0.record()
                for _ in range(n):
                    fn()
                e1.record()
            return e0, e1

        torch.cuda.synchronize()
        res = {}
        for rnd in range(ROUNDS + 1):             # round 0 warms up
            for ring in rings:
                for pc in per_cus:
                    HN.set_option(HN.OPT_WGRAD_DMA_RING, ring)
                    HN.set_option(HN.OPT_PGEMM_PER_CU, pc)
                    r = res.setdefault((ring, pc), dict(alone=[], co=[], wa=[], wc=[], cover=[]))
                    a0, a1 = timed(sb, dgrad, REP)
                    a1.synchronize()
                    alone = a0.elapsed_time(a1) * 1e3 / REP
                    w0, w1 = timed(sa, wgrad, REP)
                    w1.synchronize()
                    walone = w0.elapsed_time(w1) * 1e3 / REP
                    n_a = max(REP, int(math.ceil(3.0 * alone * REP / walone)))      # stream A outlasts stream B even if B slows down a lot
                    with torch.cuda.stream(sa):
                        wgrad()
                        first = torch.cuda.Event()
                        first.record()
                    c0, c1 = timed(sa, wgrad, n_a)
                    b0, b1 = timed(sb, dgrad, REP, after=first)
                    torch.cuda.synchronize()
                    if rnd:
                        r["alone"].append(alone); r["wa"].append(walone)
                        r["co"].append(b0.elapsed_time(b1) * 1e3 / REP); r["wc"].append(c0.elapsed_time(c1) * 1e3 / n_a)
                        r["cover"].append(b1.elapsed_time(c1) > 0)
        for (ring, pc), r in res.items():
            a, c = stats(r["alone"]), stats(r["co"])
            print(f"{name:16s} {ring:4d} {pc:5d} {variant:8d} {wg_grid:7d} | {a[0]:9.1f} {a[1]:6.1f} {a[2]:6.1f} | {c[0]:10.1f} {c[1]:6.1f} {c[2]:6.1f} | "
                  f"{c[1] / a[1]:8.2f} | {stats(r['wa'])[1]:11.1f} {stats(r['wc'])[1]:7.1f} | {sum(r['cover'])}/{len(r['cover'])}")
    HN.set_option(HN.OPT_WGRAD_DMA_RING, 0)
    HN.set_option(HN.OPT_PGEMM_PER_CU, 4)


if __name__ == "__main__":
    main()

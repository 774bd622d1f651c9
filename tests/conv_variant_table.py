"""The convolution dispatcher's instantiations, one small layer each, with the kernel every GEMM of the layer must take (helper, no tests).

A row names what sde_conv_fwd_variant has to return for the layer's forward GEMM and for its data-gradient GEMM, the split-K factor of each
(through sde_conv_fwd_ws_bytes = S M ldy 4) and what sde_conv_wgrad_variant returns, per dtype class ("16": bf16 and fp16, "32": fp32).  The
queries are host code: test_conv_variant_table.py checks the routing of every row without a GPU, test_gpu_conv_variants.py asserts it again
before it runs and compares.  Shapes are the smallest with a ragged M tile (M = 273, 546, 930 ... rows against 64- and 128-row tiles, 15 x 31 and
14 x 30 against the 8 x 16 halo tile), a ragged N tile (Cout 72 against 64) and every border.

Variant codes (csrc/conv.hip): 64064 / 128032 / 128016 register-staged tiles, 3128<BN> LDS-halo 3x3 kernel, 5<Cin><ldy> narrow-input halo kernel,
7<BM><BN> persistent LDS-DMA GEMM.  Weight gradient: 1 halo, 2 LDS-DMA, 3 register-staged.
"""
import contextlib
import ctypes
from collections import namedtuple

import torch

Row = namedtuple("Row", "name B H W C0 C1 Cout k stride pad reflect bias act upcat opts expect")
# expect: {"16": (fwd variant, dgrad variant, S fwd, S dgrad, wgrad variant), "32": (...)}; a missing class is not run
Z, R = False, True


def _row(name, B, H, W, C0, C1, Cout, k, stride, pad, reflect, bias, act, expect, upcat=False, **opts):
    return Row(name, B, H, W, C0, C1, Cout, k, stride, pad, reflect, bias, act, upcat, opts, expect)


S64, S12832, S12816, PG = 64064, 128032, 128016, 7064064
H64, H32, H16 = 3128064, 3128032, 3128016

ROWS = [
    # ---- register-staged 64x64 tile: one row per gather, with the one-tap path (Cin a multiple of the 16 / 32 elements a thread stages) and without
    _row("rs64_1x1_40_72", 1, 13, 21, 40, 0, 72, 1, 1, 0, Z, Z, 0, {"16": (S64, S64, 1, 1, 3), "32": (S64, S64, 1, 1, 3)}),
    _row("rs64_zero3_48_72_onetap", 1, 13, 21, 48, 0, 72, 3, 1, 1, Z, R, 0, {"16": (S64, S64, 1, 1, 3), "32": (S64, S64, 1, 2, 3)}),
    _row("rs64_zero3_193_72", 1, 13, 21, 193, 0, 72, 3, 1, 1, Z, R, 0, {"16": (S64, S64, 1, 1, 3), "32": (S64, S64, 1, 1, 3)}, splitk=0),      # (one pass over K; split: below)
    _row("rs64_zero3_9_72", 1, 13, 21, 9, 0, 72, 3, 1, 1, Z, R, 0, {"16": (S64, S12816, 1, 1, 3), "32": (S64, S12816, 1, 1, 3)}),
    _row("rs64_refl3_48_72_onetap_elu", 1, 13, 21, 48, 0, 72, 3, 1, 1, R, R, 1, {"16": (S64, S64, 1, 1, 3), "32": (S64, S64, 1, 2, 3)}),
    _row("rs64_refl3_193_72", 1, 13, 21, 193, 0, 72, 3, 1, 1, R, R, 0, {"16": (S64, S64, 1, 1, 3), "32": (S64, S64, 1, 1, 3)}, splitk=0),
    _row("rs64_upcat_16_32_72_onetap_elu", 1, 7, 11, 16, 32, 72, 3, 1, 1, R, R, 1, {"16": (S64, S64, 1, 1, 3), "32": (S64, S64, 1, 2, 3)}, upcat=True),
    _row("rs64_upcat_24_24_72", 1, 7, 11, 24, 24, 72, 3, 1, 1, R, R, 0, {"16": (S64, S64, 1, 1, 3), "32": (S64, S64, 1, 2, 3)}, upcat=True),
    # stride 2: the data gradient gathers the zero-inserted gradient image (Cout 80: one tap per stage; 72: a stage straddles taps)
    _row("rs64_s2_48_80_dgrad_onetap", 1, 13, 21, 48, 0, 80, 3, 2, 1, Z, Z, 0, {"16": (S64, S64, 1, 1, 3), "32": (S64, S64, 1, 2, 3)}),
    _row("rs64_s2_48_72_dgrad", 1, 13, 21, 48, 0, 72, 3, 2, 1, Z, R, 0, {"16": (S64, S64, 1, 1, 3), "32": (S64, S64, 1, 2, 3)}),
    # ---- register-staged 128x32 and 128x16 tiles; Cin 16 / 32: the halo kernel is refused by its narrow-input rule, not by the layer's size
    _row("rs128032_refl_32_24_elu", 2, 13, 21, 32, 0, 24, 3, 1, 1, R, R, 1, {"16": (S12832, S12832, 1, 1, 3), "32": (S12832, S12832, 1, 1, 3)}, halo_min=0),
    _row("rs128032_zero_16_24", 2, 13, 21, 16, 0, 24, 3, 1, 1, Z, Z, 0, {"16": (S12832, S12816, 1, 1, 3), "32": (S12832, S12816, 1, 1, 3)}, halo_min=0),
    _row("rs128016_refl_32_1_head", 2, 16, 32, 32, 0, 1, 3, 1, 1, R, R, 0, {"16": (S12816, S12832, 1, 1, 3), "32": (S12816, S12832, 1, 1, 3)}, halo_min=0),
    _row("rs128016_refl_16_16_elu", 2, 24, 48, 16, 0, 16, 3, 1, 1, R, R, 1, {"16": (S12816, S12816, 1, 1, 3), "32": (S12816, S12816, 1, 1, 3)}, halo_min=0),
    # ---- LDS-halo 3x3 kernel, N tiles 64 / 32 / 16 (forced: the default asks for 192 workgroups); 15 x 31 = one full and one partial 8 x 16 tile each way
    _row("halo64_zero_64_64", 2, 15, 31, 64, 0, 64, 3, 1, 1, Z, Z, 0, {"16": (H64, H64, 1, 1, 2)}, halo_min=0),
    _row("halo64_refl_96_64_elu", 2, 15, 31, 96, 0, 64, 3, 1, 1, R, R, 1, {"16": (H64, PG, 1, 1, 3)}, halo_min=0),
    _row("halo32_zero_96_32", 2, 15, 31, 96, 0, 32, 3, 1, 1, Z, R, 0, {"16": (H32, S64, 1, 1, 3)}, halo_min=0),
    _row("halo32_refl_64_32_elu", 2, 15, 31, 64, 0, 32, 3, 1, 1, R, R, 1, {"16": (H32, S64, 1, 1, 3)}, halo_min=0),
    _row("halo16_refl_64_1_head", 2, 15, 31, 64, 0, 1, 3, 1, 1, R, R, 0, {"16": (H16, S64, 1, 1, 3)}, halo_min=0),
    _row("halo16_zero_96_1", 2, 15, 31, 96, 0, 1, 3, 1, 1, Z, Z, 0, {"16": (H16, S64, 1, 1, 3)}, halo_min=0),
    _row("halo64_upcat_32_32_64_elu", 2, 7, 15, 32, 32, 64, 3, 1, 1, R, R, 1, {"16": (H64, H64, 1, 1, 3)}, upcat=True, halo_min=0),      # (padded gradient 16 x 32: full halo tiles)
    _row("halo32_upcat_32_64_32", 2, 7, 15, 32, 64, 32, 3, 1, 1, R, R, 0, {"16": (H32, S64, 1, 1, 3)}, upcat=True, halo_min=0),
    _row("halo16_upcat_64_0_1", 2, 7, 15, 64, 0, 1, 3, 1, 1, R, R, 0, {"16": (H16, S64, 1, 1, 3)}, upcat=True, halo_min=0),
    # ---- persistent LDS-DMA GEMM at its default (every tile, ring depth and source kind: test_gpu_pgemm.py) and the narrow-input halo kernel
    _row("pgemm_1x1_64_72", 2, 13, 21, 64, 0, 72, 1, 1, 0, Z, R, 1, {"16": (PG, S64, 1, 1, 3)}),
    _row("pgemm_3x3_64_64_not_halo", 2, 15, 31, 64, 0, 64, 3, 1, 1, Z, Z, 0, {"16": (PG, PG, 1, 1, 2)}),      # (default halo threshold: 8 workgroups are too few)
    _row("chalo_refl_16_16_elu", 2, 90, 100, 16, 0, 16, 3, 1, 1, R, R, 1, {"16": (5016016, 5016016, 1, 1, 1)}),
    # ---- split-K: 2, an intermediate factor and 8 ranges, forward and data gradient, on the persistent GEMM and (pgemm=0) the register-staged kernel
    _row("splitk_3x3_128_72_elu", 2, 6, 10, 128, 0, 72, 3, 1, 1, Z, R, 1, {"16": (PG, S64, 2, 1, 3), "32": (S64, S64, 4, 2, 3)}),
    _row("splitk_3x3_128_72_elu_staged", 2, 6, 10, 128, 0, 72, 3, 1, 1, Z, R, 1, {"16": (S64, S64, 2, 1, 3)}, pgemm=0),
    _row("splitk_3x3_256_256", 2, 6, 10, 256, 0, 256, 3, 1, 1, Z, Z, 0, {"16": (PG, PG, 4, 4, 2), "32": (S64, S64, 8, 8, 3)}),
    _row("splitk_3x3_256_256_staged", 2, 6, 10, 256, 0, 256, 3, 1, 1, Z, Z, 0, {"16": (S64, S64, 4, 4, 2)}, pgemm=0),
    _row("splitk_3x3_512_64", 1, 6, 10, 512, 0, 64, 3, 1, 1, Z, R, 0, {"16": (PG, PG, 8, 1, 2), "32": (S64, S64, 8, 2, 3)}),
    _row("splitk_3x3_512_64_staged", 1, 6, 10, 512, 0, 64, 3, 1, 1, Z, R, 0, {"16": (S64, S64, 8, 1, 2)}, pgemm=0),
    _row("splitk_zero3_193_72", 1, 13, 21, 193, 0, 72, 3, 1, 1, Z, R, 0, {"16": (S64, S64, 3, 1, 3), "32": (S64, S64, 7, 2, 3)}),      # K tail inside the last range
    _row("splitk_refl3_193_72", 1, 13, 21, 193, 0, 72, 3, 1, 1, R, R, 0, {"16": (S64, S64, 3, 1, 3), "32": (S64, S64, 7, 2, 3)}),
    _row("splitk_dgrad_3x3_72_128", 2, 6, 10, 72, 0, 128, 3, 1, 1, Z, Z, 0, {"16": (S64, PG, 1, 2, 3), "32": (S64, S64, 2, 4, 3)}),
    _row("splitk_dgrad_3x3_72_128_staged", 2, 6, 10, 72, 0, 128, 3, 1, 1, Z, Z, 0, {"16": (S64, S64, 1, 2, 3)}, pgemm=0),
    _row("splitk_dgrad_3x3_64_512", 1, 6, 10, 64, 0, 512, 3, 1, 1, Z, Z, 0, {"16": (PG, PG, 1, 8, 2), "32": (S64, S64, 2, 8, 3)}),
    _row("splitk_dgrad_3x3_64_512_staged", 1, 6, 10, 64, 0, 512, 3, 1, 1, Z, Z, 0, {"16": (S64, S64, 1, 8, 2)}, pgemm=0),
]

WRow = namedtuple("WRow", "name B H W Cin Cout k reflect expect")
# weight-gradient kernels through the C ABI (sde_conv_wgrad), each with an OIHW and a channels-last gradient: the streaming reduce takes
# channels-last or 1x1 gradients without channel padding, the transposing one the rest
WROWS = [
    WRow("wg_halo_refl_32_24", 2, 90, 100, 32, 24, 3, R, {"16": 1}),
    WRow("wg_dma_zero_64_64", 2, 13, 21, 64, 64, 3, Z, {"16": 2, "32": 3}),
    WRow("wg_dma_1x1_128_64", 2, 13, 21, 128, 64, 1, Z, {"16": 2, "32": 3}),
    WRow("wg_staged_refl_48_24", 2, 13, 21, 48, 24, 3, R, {"16": 3, "32": 3}),
    WRow("wg_staged_zero_193_72_padded_cin", 1, 13, 21, 193, 72, 3, Z, {"16": 3, "32": 3}),
]

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}


def dtype_class(dtype):
    return "32" if dtype == torch.float32 else "16"


def params(rows):
    """(row, dtype name) for every dtype a row runs in, and their ids."""
    out = [(r, n) for r in rows for n, dt in DTYPES.items() if dtype_class(dt) in r.expect]
    return out, [f"{r.name}-{n}" for r, n in out]


def pad_to(c, v):
    return (c + v - 1) // v * v


def geometry(row, dtype):
    """(V, input height / width of the convolution, output height / width, ldy, padded input channels) of a row."""
    V = 4 if dtype == torch.float32 else 8
    IH, IW = (2 * row.H, 2 * row.W) if row.upcat else (row.H, row.W)
    OH, OW = (IH + 2 * row.pad - row.k) // row.stride + 1, (IW + 2 * row.pad - row.k) // row.stride + 1
    return V, IH, IW, OH, OW, pad_to(row.Cout, V), pad_to(row.C0, V) + pad_to(row.C1, V)


def layer_descs(NN, row, x0, x1, dz):
    """The forward and data-gradient descriptors hip/nn.py builds for this layer (x0, x1, dz: NHWC tensors; only shape, dtype and address matter)."""
    V, IH, IW, OH, OW, ldy, Cv = geometry(row, x0.dtype)
    k = row.k
    fwd = NN._desc(x0, x1, NN.SRC_UPCAT if row.upcat else NN.SRC_PLAIN, k, k, row.stride, row.pad, row.reflect, IH, IW, OH, OW)
    if row.reflect:
        dg = NN._desc(dz, None, NN.SRC_PLAIN, k, k, 1, k - 1, False, OH, OW, IH + 2, IW + 2)
    elif row.stride == 1:
        dg = NN._desc(dz, None, NN.SRC_PLAIN, k, k, 1, k - 1 - row.pad, False, OH, OW, IH, IW)
    else:
        dg = NN._desc(dz, None, NN.SRC_ZEROINS, k, k, 1, k - 1 - row.pad, False, 2 * OH - 1, 2 * OW - 1, IH, IW)
    return fwd, dg


def routing(lib, NN, row, x0, x1, dz):
    """(fwd variant, dgrad variant, S fwd, S dgrad, wgrad variant) as the dispatcher reports them under the options in force."""
    V, IH, IW, OH, OW, ldy, Cv = geometry(row, x0.dtype)
    fwd, dg = layer_descs(NN, row, x0, x1, dz)

    def split(d, M, ld):
        b = lib.sde_conv_fwd_ws_bytes(ctypes.byref(d), ld)
        assert b % (M * ld * 4) == 0, f"workspace of {b} bytes is no multiple of M ldy 4 = {M * ld * 4}"
        return max(1, b // (M * ld * 4))
    B = x0.shape[0]
    return (lib.sde_conv_fwd_variant(ctypes.byref(fwd), ldy), lib.sde_conv_fwd_variant(ctypes.byref(dg), Cv),
            split(fwd, B * OH * OW, ldy), split(dg, B * dg.OH * dg.OW, Cv), lib.sde_conv_wgrad_variant(ctypes.byref(fwd), row.Cout, ldy))


@contextlib.contextmanager
def options(lib, NN, opts):
    """Dispatcher options of a row (pgemm = SDE_OPT_PGEMM, splitk = SDE_OPT_SPLITK, halo_min = sde_conv_set_halo_min_blocks), restored on exit."""
    old_pg = NN.set_option(NN.OPT_PGEMM, opts["pgemm"]) if "pgemm" in opts else None
    old_sk = NN.set_option(NN.OPT_SPLITK, opts["splitk"]) if "splitk" in opts else None
    old_halo = lib.sde_conv_set_halo_min_blocks(opts["halo_min"]) if "halo_min" in opts else None
    try:
        yield
    finally:
        if old_pg is not None:
            NN.set_option(NN.OPT_PGEMM, old_pg)
        if old_sk is not None:
            NN.set_option(NN.OPT_SPLITK, old_sk)
        if old_halo is not None:
            lib.sde_conv_set_halo_min_blocks(old_halo)

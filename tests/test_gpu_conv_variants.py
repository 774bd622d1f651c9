"""GPU: one pinned case per reachable instantiation of the convolution engine, every element against an fp64 reference.

Each row of tests/conv_variant_table.py is run through hip.nn.conv2d (forward, data gradient, weight and bias gradients, skip gradient) in bf16 and
fp16, and in fp32 where fp32 can reach the kernel.  BEFORE anything is compared the dispatcher is asked which kernel it takes for the forward and
the data-gradient GEMM, how many K ranges each is split into and which weight-gradient kernel runs: a case that a later change re-routes fails
there instead of silently testing something else.  Results are held to tests/conv_bounds.py: no element further from the fp64 reference than the
a-priori bound of the fp32 accumulation and the storage rounding, and padded output channels exactly zero.  The weight-gradient kernels are also
driven through sde_conv_wgrad directly, once per reduce kernel (streaming / transposing).
"""
import ctypes
import functools
import math

import pytest
import torch

import conv_bounds as CB
import conv_variant_table as T

pytestmark = pytest.mark.gpu
dev = "cuda"

PARAMS, IDS = T.params(T.ROWS)
WPARAMS, WIDS = T.params(T.WROWS)


@pytest.fixture(scope="module")
def engine():
    from simpledepthestimation_amd.hip import lib as L
    from simpledepthestimation_amd.hip import nn as NN
    return L, NN


def nhwc(x, dtype, V):
    B, C, H, W = x.shape
    out = torch.zeros(B, H, W, T.pad_to(C, V), dtype=dtype)
    out[..., :C] = x.permute(0, 2, 3, 1).to(dtype)
    return out.to(dev).contiguous()


def nchw(y, C):
    return y[..., :C].float().permute(0, 3, 1, 2).cpu()


@functools.lru_cache(maxsize=None)
def reference(shape_key, dt):
    """Operands (rounded to the storage dtype) and the fp64 bounds of a layer: computed once per (layer, dtype) -- the rows that differ only in
    dispatcher options share them -- and left unchanged."""
    B, H, W, C0, C1, Cout, k, stride, pad, reflect, bias, act, upcat = shape_key
    dtype = T.DTYPES[dt]
    g = torch.Generator().manual_seed(1000 * C0 + 10 * Cout + k + H)
    x0 = CB.rounded(torch.randn(B, C0, H, W, generator=g), dtype)
    x1 = CB.rounded(torch.randn(B, C1, 2 * H, 2 * W, generator=g), dtype) if C1 else None
    w = CB.rounded(torch.randn(Cout, C0 + C1, k, k, generator=g) / math.sqrt((C0 + C1) * k * k), dtype)
    b = torch.randn(Cout, generator=g) * 0.1 if bias else None
    case = CB.ConvCase(x0, w, b, dtype, stride=stride, pad=pad, reflect=reflect, act=act, x1=x1, upcat=upcat)
    gy = CB.rounded(torch.randn(case.y.ref.shape, generator=g), dtype)
    return x0, x1, w, b, gy, case, case.backward([gy])


@pytest.mark.parametrize("row,dt", PARAMS, ids=IDS)
def test_conv_variant(engine, row, dt):
    L, NN = engine
    lib = L.lib()
    dtype = T.DTYPES[dt]
    V, IH, IW, OH, OW, ldy, Cv = T.geometry(row, dtype)
    x0, x1, w, b, gy, case, bounds = reference(tuple(row[1:14]), dt)
    xd = nhwc(x0, dtype, V).requires_grad_(True)
    x1d = nhwc(x1, dtype, V).requires_grad_(True) if row.C1 else None
    wd = w.clone().to(dev).requires_grad_(True)
    bd = b.clone().to(dev).requires_grad_(True) if row.bias else None
    gyd = nhwc(gy, dtype, V)
    with T.options(lib, NN, row.opts):
        got = T.routing(lib, NN, row, xd, x1d, gyd)
        assert got == row.expect[T.dtype_class(dtype)], "(forward variant, data-gradient variant, S forward, S data gradient, weight-gradient variant)"
        y = NN.conv2d(xd, wd, bd, stride=row.stride, pad=row.pad, reflect=row.reflect, act=row.act, skip=x1d, upsample=row.upcat)
        y.backward(gyd)
        torch.cuda.synchronize()
    assert y.shape == (row.B, OH, OW, ldy)
    if ldy > row.Cout:
        assert (y[..., row.Cout:] == 0).all(), "padded output channels must be exact zeros"
    CB.assert_within(nchw(y.detach(), row.Cout), case.y, dtype, f"{row.name} y")
    CB.assert_within(nchw(xd.grad, row.C0), bounds["dX"], dtype, f"{row.name} dX")
    if xd.shape[3] > row.C0:
        assert (xd.grad[..., row.C0:] == 0).all(), "gradient of the input's padding channels must be exact zeros"
    if row.C1:
        CB.assert_within(nchw(x1d.grad, row.C1), bounds["dSkip"], dtype, f"{row.name} dSkip")
    CB.assert_within(wd.grad.cpu(), bounds["dW"], dtype, f"{row.name} dW")
    if row.bias:
        CB.assert_within(bd.grad.cpu(), bounds["dbias"], dtype, f"{row.name} dbias")


@pytest.mark.parametrize("layout", ["oihw", "ohwi"])
@pytest.mark.parametrize("row,dt", WPARAMS, ids=WIDS)
def test_wgrad_variant(engine, row, dt, layout):
    """sde_conv_wgrad on the kernel sde_conv_wgrad_variant names, into an OIHW and into a channels-last gradient: the streaming reduce takes
    channels-last (or 1x1) gradients without channel padding, the transposing one the rest."""
    L, NN = engine
    lib = L.lib()
    dtype = T.DTYPES[dt]
    V = 4 if dtype == torch.float32 else 8
    k, Cin, Cout = row.k, row.Cin, row.Cout
    lrow = T.Row(row.name, row.B, row.H, row.W, Cin, 0, Cout, k, 1, k // 2, row.reflect, False, 0, False, {}, {})
    x0, _, w, _, gy, case, bounds = reference(tuple(lrow[1:14]), dt)
    xd, gyd = nhwc(x0, dtype, V), nhwc(gy, dtype, V)
    Cin_pad, ldd = xd.shape[3], gyd.shape[3]
    d = NN._desc(xd, None, NN.SRC_PLAIN, k, k, 1, k // 2, row.reflect, row.H, row.W, row.H, row.W)
    assert lib.sde_conv_wgrad_variant(ctypes.byref(d), Cout, ldd) == row.expect[T.dtype_class(dtype)]
    streams = (layout == "ohwi" or k == 1) and Cin_pad == Cin          # (launch_wreduce's rule; a fresh torch allocation is 16-byte aligned)
    assert streams == (row.name != "wg_staged_zero_193_72_padded_cin" and (layout == "ohwi" or k == 1))
    splits = lib.sde_conv_wgrad_splits(ctypes.byref(d), Cout)
    slab = torch.empty(splits, Cout, k * k * Cin_pad, device=dev)
    dw = torch.full((Cout, k, k, Cin), 7.0, device=dev).permute(0, 3, 1, 2) if layout == "ohwi" else torch.full((Cout, Cin, k, k), 7.0, device=dev)
    assert NN.is_ohwi(dw) == (layout == "ohwi" and k > 1) and dw.data_ptr() % 16 == 0
    flags = 2 if layout == "ohwi" else 0                                 # SDE_WREDUCE_OHWI; no accumulation: every element is overwritten
    L.check(lib.sde_conv_wgrad(ctypes.byref(d), L.ptr(gyd), Cout, ldd, Cin, L.ptr(slab), splits, ctypes.c_void_p(dw.data_ptr()), flags, L.stream()), "sde_conv_wgrad")
    torch.cuda.synchronize()
    CB.assert_within(dw.cpu(), bounds["dW"], dtype, f"{row.name} dW ({layout}, {splits} slabs)")
    # accumulation into the same slot: twice the gradient on top of the first (one more fp32 rounding per element)
    L.check(lib.sde_conv_wgrad(ctypes.byref(d), L.ptr(gyd), Cout, ldd, Cin, L.ptr(slab), splits, ctypes.c_void_p(dw.data_ptr()), flags | 1, L.stream()), "sde_conv_wgrad")
    torch.cuda.synchronize()
    twice = CB.Bound(2 * bounds["dW"].ref, 2 * bounds["dW"].lim + CB.E32 * 2 * (bounds["dW"].ref.abs() + bounds["dW"].lim))
    CB.assert_within(dw.cpu(), twice, dtype, f"{row.name} dW accumulated ({layout})")

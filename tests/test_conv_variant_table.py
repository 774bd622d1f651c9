"""CPU: every row of tests/conv_variant_table.py routes where the table says (the dispatcher's queries are host code and never touch their operands).

A change to a dispatcher rule that re-routes a kernel-level case fails here, on the machine where the change is made, not only on the GPU."""
import ctypes

import pytest
import torch

import conv_variant_table as T

PARAMS, IDS = T.params(T.ROWS)
WPARAMS, WIDS = T.params(T.WROWS)


@pytest.fixture(scope="module")
def engine():
    from simpledepthestimation_amd.hip import lib as L
    from simpledepthestimation_amd.hip import nn as NN
    return L.lib(), NN


@pytest.mark.parametrize("row,dt", PARAMS, ids=IDS)
def test_row_routes_as_the_table_says(engine, row, dt):
    lib, NN = engine
    dtype = T.DTYPES[dt]
    V, IH, IW, OH, OW, ldy, Cv = T.geometry(row, dtype)
    x0 = torch.empty(row.B, row.H, row.W, T.pad_to(row.C0, V), dtype=dtype)
    x1 = torch.empty(row.B, 2 * row.H, 2 * row.W, T.pad_to(row.C1, V), dtype=dtype) if row.C1 else None
    dz = torch.empty(row.B, OH, OW, ldy, dtype=dtype)
    with T.options(lib, NN, row.opts):
        got = T.routing(lib, NN, row, x0, x1, dz)
    assert got == row.expect[T.dtype_class(dtype)], "(forward variant, data-gradient variant, S forward, S data gradient, weight-gradient variant)"


@pytest.mark.parametrize("row,dt", WPARAMS, ids=WIDS)
def test_weight_gradient_row_routes_as_the_table_says(engine, row, dt):
    lib, NN = engine
    dtype = T.DTYPES[dt]
    V = 4 if dtype == torch.float32 else 8
    x0 = torch.empty(row.B, row.H, row.W, T.pad_to(row.Cin, V), dtype=dtype)
    d = NN._desc(x0, None, NN.SRC_PLAIN, row.k, row.k, 1, row.k // 2, row.reflect, row.H, row.W, row.H, row.W)
    assert lib.sde_conv_wgrad_variant(ctypes.byref(d), row.Cout, T.pad_to(row.Cout, V)) == row.expect[T.dtype_class(dtype)]
    old = {key: NN.set_option(key, 0) for key in (NN.OPT_WGRAD_HALO, NN.OPT_WGRAD_DMA)}      # both special kernels off: the register-staged one
    try:
        assert lib.sde_conv_wgrad_variant(ctypes.byref(d), row.Cout, T.pad_to(row.Cout, V)) == NN.WGRAD_STAGED_KERNEL
    finally:
        for key, value in old.items():
            NN.set_option(key, value)
    assert lib.sde_conv_wgrad_variant(None, row.Cout, 8) == 0


def test_table_covers_every_forward_variant_and_split():
    """Every value sde_conv_fwd_variant can return at the dispatcher's defaults (the forced 128-row persistent tiles: test_gpu_pgemm.py), split
    factors 2, an intermediate one and 8 for both GEMMs, and the three weight-gradient kernels."""
    fwd, dg, sf, sd, wg = (set(e[i] for r in T.ROWS for e in r.expect.values()) for i in range(5))
    assert {T.S64, T.S12832, T.S12816, T.H64, T.H32, T.H16, T.PG, 5016016} <= fwd | dg
    assert {2, 4, 8} <= sf and {2, 4, 8} <= sd
    assert wg | set(v for r in T.WROWS for v in r.expect.values()) == {1, 2, 3}

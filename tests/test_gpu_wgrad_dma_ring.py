"""The slim LDS rings of the LDS-DMA weight-gradient kernel (csrc/wgrad_dma.hip, SDE_OPT_WGRAD_DMA_RING 1 = 32 pixels x 4 stages, 2 = 32 x 3)
against today's ring (0 = 64 pixels x 3 stages), through the module-level path tests/test_gpu_wgrad_dma.py uses.

A 32-pixel stage feeds every accumulator the same MFMA sequence in the same pixel order as a 64-pixel one (rows past the end of a pixel range are
zeros in both), the slabs go through the same fixed-order reduction, so the weight gradients must be BIT-equal: torch.equal, no tolerance.
Shapes: the smallest that can break a 32-pixel stage -- pixel ranges that are multiples of neither 32 nor 64, a last stage of fewer than 8 rows (one
DMA piece partly, the other three wholly out of range), a range shorter than the ring, an odd number of 64-column K blocks, stride 2 with odd
sizes, the 1x1 fast path, reflection padding, the up-sampled (+ concatenated) source, fp16, one pixel range and many.
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"

CASES = [
    # name, B, H, W (input), C0, Cout, k, stride, pad, dtype, reflect, C1 (-1: up-sampled source without a skip tensor), splits ("one" / "many" / None = whatever)
    ("3x3_64_64_ragged_oddK", 3, 23, 41, 64, 64, 3, 1, 1, torch.bfloat16, False, 0, None),          # M = 2829 = 88 * 32 + 13; 9 K blocks: the last tile's second half is empty
    ("3x3_128_64_last_stage_1_row", 1, 5, 13, 128, 64, 3, 1, 1, torch.bfloat16, False, 0, "one"),   # M = 65: the third 32-pixel stage holds one row
    ("3x3_512_512_tinyM", 2, 6, 20, 512, 512, 3, 1, 1, torch.bfloat16, False, 0, "one"),            # M = 240, 288 tiles: one range of 7.5 slim stages
    ("3x3_s2_64_128_odd", 2, 13, 21, 64, 128, 3, 2, 1, torch.bfloat16, False, 0, None),             # M = 2 * 7 * 11 = 154
    ("1x1_64_256_many_splits", 4, 48, 80, 64, 256, 1, 1, 0, torch.bfloat16, False, 0, "many"),      # the 1x1 fast path, 4 tiles: up to 60 pixel ranges
    ("refl_128_64_ragged", 3, 13, 41, 128, 64, 3, 1, 1, torch.bfloat16, True, 0, None),
    ("upcat_64_256_64", 2, 48, 80, 64, 64, 3, 1, 1, torch.bfloat16, True, 256, "many"),
    ("upcat_128_0_128", 2, 24, 40, 128, 128, 3, 1, 1, torch.bfloat16, True, -1, None),
    ("3x3_64_64_fp16", 2, 48, 80, 64, 64, 3, 1, 1, torch.float16, False, 0, "many"),
]
_RING0 = {}      # case name -> weight gradient with ring 0 (computed once, shared by the slim variants, never modified)


def _weight_grad(case, ring):
    from simpledepthestimation_amd.hip import nn as NN, lib as L
    name, B, H, W, C0, Cout, k, stride, pad, dt, reflect, C1, want_splits = case
    upcat = C1 != 0
    C1 = max(C1, 0)
    g = torch.Generator().manual_seed(len(name) * 7 + B)
    xh, xw = (H // 2, W // 2) if upcat else (H, W)
    xd = torch.randn(B, xh, xw, C0, generator=g).to(dt).to(dev)
    x1d = torch.randn(B, H, W, C1, generator=g).to(dt).to(dev) if C1 else None
    wd = (torch.randn(Cout, C0 + C1, k, k, generator=g) / math.sqrt((C0 + C1) * k * k)).to(dev).requires_grad_(True)
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    gy = torch.randn(B, OH, OW, Cout, generator=g).to(dt).to(dev)
    # the dispatcher's own word that this layer takes the LDS-DMA kernel, and how many pixel ranges it cuts
    d = NN._desc(xd, x1d, NN.SRC_UPCAT if upcat else NN.SRC_PLAIN, k, k, stride, pad, reflect, H, W, OH, OW)
    assert L.lib().sde_conv_wgrad_variant(ctypes.byref(d), Cout, Cout) == NN.WGRAD_DMA_KERNEL
    splits = L.lib().sde_conv_wgrad_splits(ctypes.byref(d), Cout)
    assert want_splits is None or (splits == 1) == (want_splits == "one"), splits
    old = NN.set_option(NN.OPT_WGRAD_DMA_RING, ring)
    try:
        y = NN.conv2d(xd, wd, None, stride=stride, pad=pad, reflect=reflect, skip=x1d, upsample=upcat)
        assert tuple(y.shape) == (B, OH, OW, Cout)
        y.backward(gy)
        torch.cuda.synchronize()
    finally:
        assert NN.set_option(NN.OPT_WGRAD_DMA_RING, old) == ring
    return wd.grad.detach().clone()


@pytest.mark.parametrize("ring", [1, 2])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_slim_ring_bit_equal(case, ring):
    if case[0] not in _RING0:
        _RING0[case[0]] = _weight_grad(case, 0)
    ref = _RING0[case[0]]
    got = _weight_grad(case, ring)
    assert torch.isfinite(ref).all() and ref.abs().sum() > 0
    assert torch.equal(got, ref), f"{case[0]} ring {ring}: max |diff| {(got - ref).abs().max().item():.3e}"


def test_ring_option_rejects_unknown():
    from simpledepthestimation_amd.hip import nn as NN, lib as L
    with pytest.raises(L.SdeHipError):
        NN.set_option(NN.OPT_WGRAD_DMA_RING, 3)
    assert NN.set_option(NN.OPT_WGRAD_DMA_RING, 0) == 0

"""GPU: the LDS-halo 3x3 kernel's pipelined main loop (csrc/conv.hip halo3_kernel) at the channel-block counts where it can go wrong.

The loop walks 64-channel blocks; inside a block the nine taps are unrolled with the tap, the weight register set (tap % 3) and the "is there a
next block" question fixed at compile time, the weight ring slot is (block + tap) & 1, and the last block is peeled.  So what matters is the
number of blocks and whether the last one is ragged:
  Cin 48, 64    one block: only the peeled block runs (48: ragged);
  Cin 96        two blocks, the second ragged: one trip through the loop, then the peeled block with the odd ring parity;
  Cin 160, 192  three blocks (160 ragged): the loop runs with both ring parities before the peeled block;
  Cin 256       four blocks.
Every case is 2 x 15 x 31 pixels -- one full and one partial 8x16 tile each way -- through the public ops with the halo kernel forced
(sde_conv_set_halo_min_blocks(0), as test_gpu_nn.py's force_halo) and the kernel asserted (sde_conv_fwd_variant == 3128<BN>) before anything is
compared.  Forward, data gradient and weight gradient are held per element to the fp64 bound of tests/conv_bounds.py; BatchNorm partial rows to
the column sums of the stored output; the two BatchNorm-backward epilogues to the separate bn_bwd_reduce route."""
import ctypes
import math

import pytest
import torch

import conv_bounds as CB

pytestmark = pytest.mark.gpu
dev = "cuda"
V = 8
B, H, W = 2, 15, 31
DTYPES = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "fp16"]


@pytest.fixture(scope="module")
def NN():
    from simpledepthestimation_amd.hip import nn
    return nn


@pytest.fixture
def force_halo(NN):
    from simpledepthestimation_amd.hip import lib as L
    old = L.lib().sde_conv_set_halo_min_blocks(0)
    yield
    L.lib().sde_conv_set_halo_min_blocks(old)


def nhwc(x, dtype):
    b, c, h, w = x.shape
    out = torch.zeros(b, h, w, (c + V - 1) // V * V, dtype=dtype)
    out[..., :c] = x.permute(0, 2, 3, 1).to(dtype)
    return out.to(dev).contiguous()


def nchw(y, C):
    return y[..., :C].float().permute(0, 3, 1, 2).cpu()


def relerr(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def fwd_variant(NN, x0, x1, upcat, reflect, ldy):
    from simpledepthestimation_amd.hip import lib as L
    _, h, w, _ = x0.shape
    h, w = (2 * h, 2 * w) if upcat else (h, w)
    d = NN._desc(x0, x1, NN.SRC_UPCAT if upcat else NN.SRC_PLAIN, 3, 3, 1, 1, reflect, h, w, h, w)
    return L.lib().sde_conv_fwd_variant(ctypes.byref(d), ldy)


def halo_variant(ldy):
    return 3128000 + (64 if ldy > 32 else 32 if ldy > 16 else 16)


def ldy_of(Cout):
    return (Cout + V - 1) // V * V


# (Cin, zero-padded Cout, reflection-padded Cout): every block count with both paddings; Cout 64, 72 (two N tiles, the second ragged) -> BN 64,
# 32 and 24 (ragged) -> BN 32, 1 (ldy 8) -> BN 16.  Zero-padded layers are the encoder's (no bias, no activation), reflection-padded ones the
# decoder's (bias + ELU).
PLAIN = [(48, 64, 24), (64, 72, 1), (96, 32, 64), (160, 24, 72), (192, 64, 32), (256, 1, 64)]
PLAIN_CASES = [(cin, co, False) for cin, co, _ in PLAIN] + [(cin, co, True) for cin, _, co in PLAIN]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("Cin,Cout,reflect", PLAIN_CASES, ids=[f"cin{c}_cout{o}_{'reflect' if r else 'zero'}" for c, o, r in PLAIN_CASES])
def test_halo3_block_counts(NN, force_halo, Cin, Cout, reflect, dtype):
    g = torch.Generator().manual_seed(Cin * 131 + Cout * 2 + int(reflect))
    x = torch.randn(B, Cin, H, W, generator=g).to(dtype).float()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)).to(dtype).float()
    b = torch.randn(Cout, generator=g) * 0.1 if reflect else None
    act = 1 if reflect else 0
    cb = CB.ConvCase(x, w, b, dtype, stride=1, pad=1, reflect=reflect, act=act)
    gy = torch.randn(cb.y.ref.shape, generator=g).to(dtype).float()
    lim = cb.backward([gy])
    xd = nhwc(x, dtype).requires_grad_(True)
    wd = w.clone().to(dev).requires_grad_(True)
    bd = b.clone().to(dev).requires_grad_(True) if b is not None else None
    assert fwd_variant(NN, xd, None, False, reflect, ldy_of(Cout)) == halo_variant(ldy_of(Cout))
    y = NN.conv2d(xd, wd, bd, stride=1, pad=1, reflect=reflect, act=act)
    CB.assert_within(nchw(y, Cout), cb.y, dtype, "y")
    assert (y[..., Cout:] == 0).all()
    y.backward(nhwc(gy, dtype))
    CB.assert_within(nchw(xd.grad, Cin), lim["dX"], dtype, "dX")
    CB.assert_within(wd.grad.cpu(), lim["dW"], dtype, "dW")        # (dtype: the relative-L2 line; the limit itself is the fp32 one)
    if b is not None:
        CB.assert_within(bd.grad.cpu(), lim["dbias"], dtype, "dbias")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C0,C1,Cout", [(32, 64, 32), (32, 64, 24), (64, 96, 64)])
def test_halo3_upsample_concat(NN, force_halo, C0, C1, Cout, dtype):
    """Nearest x2 up-sampling + skip concat in the halo loader: 32 + 64 channels put both sources into the first 64-channel block (and leave the
    second ragged), 64 + 96 change source exactly at a block boundary and end in a ragged third block."""
    g = torch.Generator().manual_seed(C0 * 7 + C1 + Cout)
    h, w = 7, 15
    x0 = torch.randn(B, C0, h, w, generator=g).to(dtype).float()
    x1 = torch.randn(B, C1, 2 * h, 2 * w, generator=g).to(dtype).float()
    wt = (torch.randn(Cout, C0 + C1, 3, 3, generator=g) / math.sqrt((C0 + C1) * 9)).to(dtype).float()
    bs = torch.randn(Cout, generator=g) * 0.1
    cb = CB.ConvCase(x0, wt, bs, dtype, stride=1, pad=1, reflect=True, act=1, x1=x1, upcat=True)
    gy = torch.randn(cb.y.ref.shape, generator=g).to(dtype).float()
    lim = cb.backward([gy])
    x0d, x1d = nhwc(x0, dtype).requires_grad_(True), nhwc(x1, dtype).requires_grad_(True)
    wd = wt.clone().to(dev).requires_grad_(True)
    assert fwd_variant(NN, x0d, x1d, True, True, ldy_of(Cout)) == halo_variant(ldy_of(Cout))
    y = NN.conv2d(x0d, wd, bs.to(dev), stride=1, pad=1, reflect=True, act=1, skip=x1d, upsample=True)
    CB.assert_within(nchw(y, Cout), cb.y, dtype, "y")
    y.backward(nhwc(gy, dtype))
    CB.assert_within(nchw(x0d.grad, C0), lim["dX"], dtype, "dx0")
    CB.assert_within(nchw(x1d.grad, C1), lim["dSkip"], dtype, "dx1")
    CB.assert_within(wd.grad.cpu(), lim["dW"], dtype, "dW")        # (dtype: the relative-L2 line; the limit itself is the fp32 one)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("Cin,Cout", [(64, 64), (96, 32), (160, 72), (192, 24)])
def test_halo3_batchnorm_partial_rows(NN, force_halo, Cin, Cout, dtype):
    """One (sum, sum of squares) row per 8x16 tile, taken from the values as stored: against fp64 column sums of the stored output over that tile's
    pixels inside the image.  Bound: an fp32 sum of n <= 128 terms in any order, (n + 3) 2^-24 sum |t| (conv_bounds' dot-product bound), with one
    more rounding for each square."""
    g = torch.Generator().manual_seed(Cin + Cout)
    x = (torch.randn(B, Cin, H, W, generator=g) + 0.3).to(dtype).float()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)).to(dtype).float()
    xd = nhwc(x, dtype)
    assert fwd_variant(NN, xd, None, False, False, ldy_of(Cout)) == halo_variant(ldy_of(Cout))
    y, stats = NN.conv2d(xd, w.to(dev), None, stride=1, pad=1, bn_stats=True)
    ty, tx = (H + 7) // 8, (W + 15) // 16
    rows = stats[:B * ty * tx].double().cpu()
    assert stats.shape[0] == B * ty * tx + NN.REDUCE_ROWS and stats.shape[1] == Cout
    ys = y[..., :Cout].double().cpu()
    for n in range(B):
        for i in range(ty):
            for j in range(tx):
                t = ys[n, 8 * i:8 * i + 8, 16 * j:16 * j + 16].reshape(-1, Cout)
                row = rows[(n * ty + i) * tx + j]
                k = t.shape[0] + 3
                assert ((row[:, 0] - t.sum(0)).abs() <= k * CB.E32 * t.abs().sum(0) + 1e-30).all(), (n, i, j, "sum")
                assert ((row[:, 1] - (t * t).sum(0)).abs() <= (k + 1) * CB.E32 * (t * t).sum(0) + 1e-30).all(), (n, i, j, "sum of squares")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C", [64, 128])
def test_halo3_batchnorm_backward_epilogue(NN, force_halo, C, dtype):
    """conv_a (1x1) -> BatchNorm + ReLU -> conv_b (3x3 on the halo kernel), backward: conv_b's data gradient with the BatchNorm-backward epilogue
    against the separate bn_bwd_reduce pass, compared as test_gpu_nn.py::test_bn_backward_reduce_in_the_dgrad_epilogue compares them (the same
    summands in another order for the statistics; the outputs and conv_b's weight gradient do not depend on the route)."""
    g = torch.Generator().manual_seed(1000 + C)
    Cin = 64
    x = (torch.randn(B, Cin, H, W, generator=g) + 0.2).to(dtype).float()
    wa = (torch.randn(C, Cin, 1, 1, generator=g) / math.sqrt(Cin)).to(dtype).float()
    wb = (torch.randn(C, C, 3, 3, generator=g) / math.sqrt(C * 9)).to(dtype).float()
    gamma = torch.rand(C, generator=g) + 0.5; beta = torch.randn(C, generator=g) * 0.3
    go = torch.randn(B, C, H, W, generator=g).to(dtype).float()
    res = []
    for fused in (False, True):
        kept, NN.BNBWD_FUSED = NN.BNBWD_FUSED, fused
        try:
            xd = nhwc(x, dtype).requires_grad_(True)
            wad, wbd, gd, bd = (t.clone().to(dev).requires_grad_(True) for t in (wa, wb, gamma, beta))
            hits = NN.BNBWD_HITS
            y, stats = NN.conv2d(xd, wad, None, stride=1, pad=0, bn_stats=True)
            a = NN.batch_norm_act(y, stats, gd, bd, torch.zeros(C, device=dev), torch.ones(C, device=dev), relu=True)
            assert fwd_variant(NN, a, None, False, False, C) == 3128064          # conv_b and its data gradient: same shapes, same kernel
            out = NN.conv2d(a, wbd, None, stride=1, pad=1)
            out.backward(nhwc(go, dtype))
            torch.cuda.synchronize()
            assert NN.BNBWD_HITS - hits == (1 if fused else 0), f"fused path {'not ' if fused else ''}taken"
            res.append([t.detach().float().cpu() for t in (out, xd.grad, wad.grad, wbd.grad, gd.grad, bd.grad)])
        finally:
            NN.BNBWD_FUSED = kept
    for nm, u, f in zip(("out", "dX", "dWa", "dWb", "dgamma", "dbeta"), res[0], res[1]):
        assert torch.isfinite(f).all(), f"{nm}: not finite"
        assert relerr(f, u) < (1e-6 if nm in ("out", "dWb") else 3e-3), f"{nm}: fused vs separate {relerr(f, u):.3e}"


@pytest.mark.parametrize("C", [64, 128])
def test_halo3_residual_batchnorm_backward_epilogue(NN, force_halo, C):
    """The residual form (gm = (g + skip gradient) * [block output > 0]) in the halo kernel's epilogue against the separate reduce pass, compared as
    test_gpu_nn.py::test_residual_batchnorm_backward_in_the_data_gradient compares them."""
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(2000 + C)
    x = (torch.randn(B, 64, H, W, generator=g) + 0.2).to(dt).float()
    r = (torch.randn(B, C, H, W, generator=g) * 0.5).to(dt).float()
    wa = (torch.randn(C, 64, 1, 1, generator=g) / 8).to(dt).float()
    w1 = (torch.randn(C, C, 3, 3, generator=g) / math.sqrt(C * 9)).to(dt).float()
    w3 = (torch.randn(C, C, 1, 1, generator=g) / math.sqrt(C)).to(dt).float()
    ga, ba, gb, bb = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    go = torch.randn(B, C, H, W, generator=g).to(dt).float()
    res = []
    for fused in (False, True):
        kept, NN.RESBN_FUSED = NN.RESBN_FUSED, fused
        try:
            xd, rd = nhwc(x, dt).requires_grad_(True), nhwc(r, dt).requires_grad_(True)
            wad, w1d, w3d, gad, bad, gbd, bbd = (t.clone().to(dev).requires_grad_(True) for t in (wa, w1, w3, ga, ba, gb, bb))
            hits = NN.RESBN_HITS
            ya, sa = NN.conv2d(xd, wad, None, stride=1, pad=0, bn_stats=True)
            ua, ub = NN.batch_norm_act(ya, sa, gad, bad, torch.zeros(C, device=dev), torch.ones(C, device=dev), residual=rd, relu=True, n_out=2)
            assert fwd_variant(NN, ua, None, False, False, C) == 3128064
            h = NN.conv2d(ua, w1d, None, stride=1, pad=1)
            y3, s3 = NN.conv2d(h, w3d, None, stride=1, pad=0, bn_stats=True)
            out = NN.batch_norm_act(y3, s3, gbd, bbd, torch.zeros(C, device=dev), torch.ones(C, device=dev), residual=ub, relu=True)
            out.backward(nhwc(go, dt))
            torch.cuda.synchronize()
            assert NN.RESBN_HITS - hits == (1 if fused else 0), f"residual form {'not ' if fused else ''}taken"
            res.append([t.detach().float().cpu() for t in (out, xd.grad, rd.grad, wad.grad, w1d.grad, w3d.grad, gad.grad, bad.grad, gbd.grad, bbd.grad)])
        finally:
            NN.RESBN_FUSED = kept
    for nm, u, f in zip(("out", "dX", "dR", "dWa", "dW1", "dW3", "dgamma_a", "dbeta_a", "dgamma_b", "dbeta_b"), res[0], res[1]):
        assert torch.isfinite(f).all(), f"{nm}: not finite"
        assert relerr(f, u) < (1e-6 if nm in ("out", "dW3", "dgamma_b", "dbeta_b", "dW1") else 3e-3), f"{nm}: fused vs separate {relerr(f, u):.3e}"

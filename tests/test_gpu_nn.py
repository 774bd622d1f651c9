"""GPU parity: convolution engine + surrounding layers (through the C ABI) vs plain torch-CPU fp32 ops.

fp32 mode is held to ~1e-5 (f32 MFMA is an exact fmaf chain; only summation order differs); bf16 mode is checked against
an fp32 reference evaluated on the bf16-rounded operands with a tolerance that reflects bf16 output rounding (2^-8 rel).
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import conv_bounds as CB
import norm_bounds as NB

pytestmark = pytest.mark.gpu
dev = "cuda"


@pytest.fixture(scope="module")
def NN():
    from simpledepthestimation_amd.hip import nn
    return nn


def nhwc(x, dtype, V):
    """NCHW fp32 cpu -> NHWC device tensor with channel padding."""
    B, C, H, W = x.shape
    Cp = (C + V - 1) // V * V
    out = torch.zeros(B, H, W, Cp, dtype=dtype)
    out[..., :C] = x.permute(0, 2, 3, 1).to(dtype)
    return out.to(dev).contiguous()


def nchw(y, C):
    return y[..., :C].float().permute(0, 3, 1, 2).cpu()


def relerr(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def check(a, b, dtype, name, f32_tol=2e-5, bf16_tol=1.5e-2, bound=None):
    """bound (conv_bounds.Bound, the convolution tests): in addition, no element further from the fp64 reference than its a-priori limit."""
    if bound is not None:
        CB.assert_within(a, bound, dtype, name, l2_tol=float("inf"))          # (the relative-L2 line is the one below)
    e = relerr(a, b)
    # fp16: the bf16 tolerance scaled by the ratio of the unit roundoffs, 2^-11 / 2^-8, and not below the fp32 one
    tol = f32_tol if dtype == torch.float32 else bf16_tol if dtype == torch.bfloat16 else max(f32_tol, bf16_tol * 2.0 ** -3)
    assert e < tol, f"{name}: relative L2 error {e:.3e} > {tol}"
    mx = (a.double() - b.double()).abs().max().item()
    scale = b.abs().max().item() + 1e-30
    assert mx / scale < tol * 50, f"{name}: max abs error {mx:.3e} (scale {scale:.3e})"


CONV_CASES = [
    # name, B, H, W, Cin, Cout, k, stride, pad, reflect, bias, act
    ("3x3_s1_64_64", 2, 24, 40, 64, 64, 3, 1, 1, False, False, 0),
    ("3x3_s2_64_128", 2, 24, 40, 64, 128, 3, 2, 1, False, False, 0),
    ("1x1_s1_256_64", 2, 12, 20, 256, 64, 1, 1, 0, False, False, 0),
    ("1x1_s2_64_256", 2, 24, 40, 64, 256, 1, 2, 0, False, False, 0),
    ("7x7_s2_stem", 2, 32, 64, 3, 64, 7, 2, 3, False, False, 0),
    ("refl_32_16_elu", 2, 16, 24, 32, 16, 3, 1, 1, True, True, 1),
    ("refl_16_1_head", 2, 16, 24, 16, 1, 3, 1, 1, True, True, 0),
    # the four disparity heads (single output channel, N = 1 GEMMs): every Cin of the decoder, several thousand pixels, odd sizes, and the
    # zero-padded form
    ("refl_32_1_head", 2, 48, 64, 32, 1, 3, 1, 1, True, True, 0),
    ("refl_64_1_head", 1, 13, 21, 64, 1, 3, 1, 1, True, True, 0),
    ("refl_128_1_head", 2, 8, 12, 128, 1, 3, 1, 1, True, True, 0),
    ("zero_16_1_head", 2, 16, 24, 16, 1, 3, 1, 1, False, True, 0),
    ("3x3_256_512_tinyM", 2, 6, 10, 256, 512, 3, 1, 1, False, False, 0),
    ("k5_s2_pose", 2, 24, 40, 16, 32, 5, 2, 2, False, True, 0),
    ("k7_s2_pose_in9", 2, 32, 64, 9, 16, 7, 2, 3, False, True, 0),
    ("3x3_bigM_64_128", 2, 96, 160, 64, 128, 3, 1, 1, False, False, 0),
    ("3x3_s2_odd", 1, 13, 21, 32, 32, 3, 2, 1, False, True, 0),
    # PackNet01 shapes (layers01.py): huge K after the 3-D convolution (weight-gradient transpose in channel chunks), 5x5 / 7x7 stride 1,
    # concatenated inputs with an odd channel count (193 = 128 + 64 + 1 inverse-depth channel)
    ("3x3_2048_64_bigK", 1, 6, 10, 2048, 64, 3, 1, 1, False, True, 0),
    ("5x5_1024_64_pack", 1, 8, 12, 1024, 64, 5, 1, 2, False, True, 0),
    ("7x7_s1_64_64", 1, 12, 20, 64, 64, 7, 1, 3, False, True, 0),
    ("3x3_193_128_cat", 1, 8, 12, 193, 128, 3, 1, 1, False, True, 0),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "fp16"])
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_fwd_bwd(NN, case, dtype):
    name, B, H, W, Cin, Cout, k, stride, pad, reflect, has_bias, act = case
    g = torch.Generator().manual_seed(hash(name) % 1000)
    V = 4 if dtype == torch.float32 else 8
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    b = torch.randn(Cout, generator=g) * 0.1 if has_bias else None
    if dtype != torch.float32:   # reference sees the same rounded operands
        x = x.to(dtype).float(); w = w.to(dtype).float()
    xr = x.clone().requires_grad_(True); wr = w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if has_bias else None
    xin = F.pad(xr, (1, 1, 1, 1), mode="reflect") if reflect else xr
    yr = F.conv2d(xin, wr, br, stride, 0 if reflect else pad)
    if act == 1:
        yr = F.elu(yr)
    gy = torch.randn(yr.shape, generator=g)
    if dtype != torch.float32:
        gy = gy.to(dtype).float()
    yr.backward(gy)
    cb = CB.ConvCase(x, w, b, dtype, stride=stride, pad=pad, reflect=reflect, act=act)      # fp64 reference with per-element limits
    lim = cb.backward([gy])

    xd = nhwc(x, dtype, V).requires_grad_(True)
    wd = w.clone().to(dev).requires_grad_(True)
    bd = b.clone().to(dev).requires_grad_(True) if has_bias else None
    y = NN.conv2d(xd, wd, bd, stride=stride, pad=pad, reflect=reflect, act=act)
    assert y.shape[:3] == (B, yr.shape[2], yr.shape[3])
    if y.shape[3] > Cout:
        assert (y[..., Cout:] == 0).all(), "padded output channels must be exact zeros"
    check(nchw(y, Cout), yr.detach(), dtype, "y", bound=cb.y)
    y.backward(nhwc(gy, dtype, V))
    check(wd.grad.cpu(), wr.grad, dtype, "dW", bound=lim["dW"])
    check(nchw(xd.grad, Cin), xr.grad, dtype, "dX", bound=lim["dX"])
    if has_bias:
        check(bd.grad.cpu(), br.grad, dtype, "dbias", bound=lim["dbias"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "fp16"])
@pytest.mark.parametrize("C0,C1,Cout", [(32, 64, 32), (16, 0, 16), (256, 1024, 256), (64, 64, 128)])
def test_conv_upsample_concat(NN, dtype, C0, C1, Cout):
    """depth_decoder.py:L102-105: upconv(i,1)(cat(upsample(x), skip)) with reflection pad, bias, ELU -- gathered on the fly."""
    g = torch.Generator().manual_seed(C0 + C1)
    V = 4 if dtype == torch.float32 else 8
    B, h, w = 2, 6, 10
    x0 = torch.randn(B, C0, h, w, generator=g)
    x1 = torch.randn(B, C1, 2 * h, 2 * w, generator=g) if C1 else None
    wt = torch.randn(Cout, C0 + C1, 3, 3, generator=g) / math.sqrt((C0 + C1) * 9)
    bs = torch.randn(Cout, generator=g) * 0.1
    if dtype != torch.float32:
        x0 = x0.to(dtype).float(); wt = wt.to(dtype).float()
        x1 = x1.to(dtype).float() if C1 else None
    x0r = x0.clone().requires_grad_(True); x1r = x1.clone().requires_grad_(True) if C1 else None
    wr = wt.clone().requires_grad_(True); br = bs.clone().requires_grad_(True)
    up = F.interpolate(x0r, scale_factor=2, mode="nearest")
    cat = torch.cat([up, x1r], 1) if C1 else up
    yr = F.elu(F.conv2d(F.pad(cat, (1, 1, 1, 1), mode="reflect"), wr, br))
    gy = torch.randn(yr.shape, generator=g)
    if dtype != torch.float32:
        gy = gy.to(dtype).float()
    yr.backward(gy)
    cb = CB.ConvCase(x0, wt, bs, dtype, stride=1, pad=1, reflect=True, act=1, x1=x1, upcat=True)
    lim = cb.backward([gy])
    x0d = nhwc(x0, dtype, V).requires_grad_(True)
    x1d = nhwc(x1, dtype, V).requires_grad_(True) if C1 else None
    wd = wt.clone().to(dev).requires_grad_(True); bd = bs.clone().to(dev).requires_grad_(True)
    y = NN.conv2d(x0d, wd, bd, stride=1, pad=1, reflect=True, act=1, skip=x1d, upsample=True)
    check(nchw(y, Cout), yr.detach(), dtype, "y", bound=cb.y)
    y.backward(nhwc(gy, dtype, V))
    check(wd.grad.cpu(), wr.grad, dtype, "dW", bound=lim["dW"])
    check(bd.grad.cpu(), br.grad, dtype, "dbias", bound=lim["dbias"])
    check(nchw(x0d.grad, C0), x0r.grad, dtype, "dx0 (through nearest-upsample)", bound=lim["dX"])
    if C1:
        check(nchw(x1d.grad, C1), x1r.grad, dtype, "dx1 (skip)", bound=lim["dSkip"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "fp16"])
@pytest.mark.parametrize("C,with_res,relu", [(64, False, True), (128, True, True), (256, False, False)])
def test_conv_batchnorm(NN, dtype, C, with_res, relu):
    """conv (stats in the GEMM epilogue) -> training-mode BatchNorm [+ residual] [+ ReLU], forward and backward."""
    g = torch.Generator().manual_seed(C)
    V = 4 if dtype == torch.float32 else 8
    B, H, W, Cin = 3, 14, 22, 32
    x = torch.randn(B, Cin, H, W, generator=g) + 0.3
    w = torch.randn(C, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    gamma = torch.rand(C, generator=g) + 0.5; beta = torch.randn(C, generator=g) * 0.2
    res = torch.randn(B, C, H, W, generator=g) if with_res else None
    if dtype != torch.float32:
        x = x.to(dtype).float(); w = w.to(dtype).float()
        res = res.to(dtype).float() if with_res else None
    xr, wr, gr, br = (t.clone().requires_grad_(True) for t in (x, w, gamma, beta))
    rr = res.clone().requires_grad_(True) if with_res else None
    rm, rv = torch.zeros(C), torch.ones(C)
    yc = F.conv2d(xr, wr, None, 1, 1)
    if dtype != torch.float32:   # the GPU path stores the conv output in the 16-bit type before normalising
        yc = yc + (yc.detach().to(dtype).float() - yc.detach())
    o = F.batch_norm(yc, rm, rv, gr, br, True, 0.1, 1e-5)
    if with_res:
        o = o + rr
    if relu:
        o = F.relu(o)
    go = torch.randn(o.shape, generator=g)
    if dtype != torch.float32:
        go = go.to(dtype).float()
    o.backward(go)
    xd = nhwc(x, dtype, V).requires_grad_(True)
    wd, gd, bd = (t.clone().to(dev).requires_grad_(True) for t in (w, gamma, beta))
    rd = nhwc(res, dtype, V).requires_grad_(True) if with_res else None
    rmd, rvd = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    y, stats = NN.conv2d(xd, wd, None, stride=1, pad=1, bn_stats=True)
    out = NN.batch_norm_act(y, stats, gd, bd, rmd, rvd, residual=rd, relu=relu)
    # per element: the fp64 BatchNorm of the convolution output AS STORED, on the slab the epilogue left (norm_bounds.BNForward)
    M = B * H * W
    fwd = NB.BNForward(stats[:stats.shape[0] - NN.REDUCE_ROWS].cpu(), M, gamma, beta, 1e-5)
    lim = fwd.out(y.detach().float().cpu().view(M, C), rd.detach().float().cpu().view(M, C) if with_res else None, relu, dtype)
    to_nchw = lambda t: t.view(B, H, W, C).permute(0, 3, 1, 2)
    check(nchw(out, C), o.detach(), dtype, "bn out", bound=CB.Bound(to_nchw(lim.ref), to_nchw(lim.lim)))
    brm, brv = fwd.running(torch.zeros(C), torch.ones(C))
    check(rmd.cpu(), rm, dtype, "running_mean", 1e-5, 1e-2, bound=brm)
    check(rvd.cpu(), rv, dtype, "running_var", 1e-5, 1e-2, bound=brv)
    out.backward(nhwc(go, dtype, V))
    check(gd.grad.cpu(), gr.grad, dtype, "dgamma", 5e-5, 3e-2)
    check(bd.grad.cpu(), br.grad, dtype, "dbeta", 5e-5, 3e-2)
    check(nchw(xd.grad, Cin), xr.grad, dtype, "dX", 5e-5, 3e-2)
    check(wd.grad.cpu(), wr.grad, dtype, "dW", 5e-5, 3e-2)
    if with_res:
        check(nchw(rd.grad, C), rr.grad, dtype, "dres")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "fp16"])
@pytest.mark.parametrize("n_out,with_res,relu", [(3, True, True), (2, False, True), (2, False, False), (3, True, False)])
def test_batchnorm_several_consumers(NN, dtype, n_out, with_res, relu):
    """The block output feeds up to three consumers (next conv1, residual / down-sampling path, decoder skip): batch_norm_act(n_out) hands
    each its own alias and backward sums the separately arriving gradients inside the BN-backward kernels (no autograd add kernels).
    Some consumers may not contribute (None gradient)."""
    g = torch.Generator().manual_seed(7 * n_out + int(relu))
    V = 4 if dtype == torch.float32 else 8
    B, H, W, Cin, C = 2, 10, 14, 16, 64
    x = torch.randn(B, Cin, H, W, generator=g) + 0.2
    w = torch.randn(C, Cin, 1, 1, generator=g) / math.sqrt(Cin)
    gamma = torch.rand(C, generator=g) + 0.5; beta = torch.randn(C, generator=g) * 0.2
    res = torch.randn(B, C, H, W, generator=g) if with_res else None
    cw = [torch.randn(B, C, H, W, generator=g) for _ in range(n_out)]          # consumer k: weighted sum of the output, scaled by (k + 1)
    if dtype != torch.float32:
        x, w = x.to(dtype).float(), w.to(dtype).float()
        res = res.to(dtype).float() if with_res else None
    xr, wr, gr, br = (t.clone().requires_grad_(True) for t in (x, w, gamma, beta))
    rr = res.clone().requires_grad_(True) if with_res else None
    yc = F.conv2d(xr, wr)
    if dtype != torch.float32:
        yc = yc + (yc.detach().to(dtype).float() - yc.detach())
    o = F.batch_norm(yc, torch.zeros(C), torch.ones(C), gr, br, True, 0.1, 1e-5)
    o = o + rr if with_res else o
    o = F.relu(o) if relu else o
    used = list(range(n_out)) if n_out == 2 else [0, 2]                          # with three aliases the middle one stays unused
    loss = sum(((k + 1) * (o * cw[k]).sum()) for k in used)
    loss.backward()
    xd = nhwc(x, dtype, V).requires_grad_(True)
    wd, gd, bd = (t.clone().to(dev).requires_grad_(True) for t in (w, gamma, beta))
    rd = nhwc(res, dtype, V).requires_grad_(True) if with_res else None
    y, stats = NN.conv2d(xd, wd, None, bn_stats=True)
    outs = NN.batch_norm_act(y, stats, gd, bd, torch.zeros(C, device=dev), torch.ones(C, device=dev), residual=rd, relu=relu, n_out=n_out)
    assert len(outs) == n_out and all(t.data_ptr() == outs[0].data_ptr() for t in outs)
    lossd = sum(((k + 1) * (outs[k].float() * nhwc(cw[k], torch.float32, 4)[..., :C].to(dev)).sum()) for k in used)
    lossd.backward()
    check(gd.grad.cpu(), gr.grad, dtype, "dgamma", 5e-5, 3e-2)
    check(bd.grad.cpu(), br.grad, dtype, "dbeta", 5e-5, 3e-2)
    check(nchw(xd.grad, Cin), xr.grad, dtype, "dX", 5e-5, 3e-2)
    check(wd.grad.cpu(), wr.grad, dtype, "dW", 5e-5, 3e-2)
    if with_res:
        check(nchw(rd.grad, C), rr.grad, dtype, "dres", 5e-5, 2e-2)


def gn_bound(x, gamma, beta, act, dtype, groups=16, eps=1e-5):
    """The per-element limit of GroupNorm's output (norm_bounds.GNForward) for an NCHW input holding storage values, as an NCHW Bound."""
    B, C, H, W = x.shape
    b = NB.GNForward(x.permute(0, 2, 3, 1).reshape(B, H * W, C), None, gamma, beta, groups, eps, act, dtype).out
    return CB.Bound(b.ref.view(B, H, W, C).permute(0, 3, 1, 2), b.lim.view(B, H, W, C).permute(0, 3, 1, 2))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "fp16"])
def test_maxpool(NN, dtype):
    g = torch.Generator().manual_seed(1)
    V = 4 if dtype == torch.float32 else 8
    for (B, C, H, W) in [(2, 64, 16, 24), (1, 16, 13, 21)]:
        x = torch.randn(B, C, H, W, generator=g)
        if dtype != torch.float32:
            x = x.to(dtype).float()
        xr = x.clone().requires_grad_(True)
        yr = F.max_pool2d(xr, 3, 2, 1)
        gy = torch.randn(yr.shape, generator=g)
        yr.backward(gy)
        xd = nhwc(x, dtype, V).requires_grad_(True)
        y = NN.max_pool_3x3_s2(xd)
        assert torch.equal(nchw(y, C), yr.detach())
        y.backward(nhwc(gy, dtype, V))
        check(nchw(xd.grad, C), xr.grad.to(dtype).float(), dtype, "maxpool dx", 1e-6, 1e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "fp16"])
@pytest.mark.parametrize("flip", [False, True])
def test_depth_head(NN, dtype, flip):
    g = torch.Generator().manual_seed(2)
    V = 4 if dtype == torch.float32 else 8
    B, H, W = 2, 12, 20
    y = torch.randn(B, 1, H, W, generator=g) * 3
    y[0, 0, 0, 0] = 25.0   # softplus threshold branch
    if dtype != torch.float32:
        y = y.to(dtype).float()
    yr = y.clone().requires_grad_(True)
    sd = 1 / 80 + (1 / 0.1 - 1 / 80) * F.softplus(yr)
    dr = 1 / sd
    if flip:
        dr = torch.flip(dr, [3])
    gd = torch.randn(dr.shape, generator=g)
    dr.backward(gd)
    yd = nhwc(y, dtype, V).requires_grad_(True)
    d = NN.depth_head(yd, 0.1, 80.0, flip)
    assert d.dtype == torch.float32 and d.shape == (B, 1, H, W)
    check(d.cpu(), dr.detach(), torch.float32, "depth", 1e-5)
    d.backward(gd.to(dev))
    assert (yd.grad[..., 1:] == 0).all()
    check(nchw(yd.grad, 1), yr.grad, dtype, "d logit", 2e-5, 1e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "fp16"])
@pytest.mark.parametrize("C,H,W", [(16, 24, 40), (32, 12, 20), (256, 3, 5), (256, 2, 5)])
def test_group_norm_relu(NN, dtype, C, H, W):
    g = torch.Generator().manual_seed(C + H)
    V = 4 if dtype == torch.float32 else 8
    B = 3
    x = torch.randn(B, C, H, W, generator=g) * 2 + 0.5
    gamma = torch.rand(C, generator=g) + 0.5; beta = torch.randn(C, generator=g) * 0.3
    if dtype != torch.float32:
        x = x.to(dtype).float()
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    o = F.relu(F.group_norm(xr, 16, gr, br, 1e-5))
    go = torch.randn(o.shape, generator=g)
    o.backward(go)
    xd = nhwc(x, dtype, V).requires_grad_(True)
    gd, bd = (t.clone().to(dev).requires_grad_(True) for t in (gamma, beta))
    out = NN.group_norm_relu(xd, gd, bd, 16, 1e-5)
    check(nchw(out, C), o.detach(), dtype, "gn out", bound=gn_bound(x, gamma, beta, NB.ACT_RELU, dtype))
    out.backward(nhwc(go, dtype, V))
    check(nchw(xd.grad, C), xr.grad, dtype, "gn dx", 5e-5, 3e-2)
    check(gd.grad.cpu(), gr.grad, dtype, "gn dgamma", 5e-5, 3e-2)
    check(bd.grad.cpu(), br.grad, dtype, "gn dbeta", 5e-5, 3e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("C,H,W", [(64, 12, 20), (512, 6, 10)])
def test_group_norm_elu(NN, dtype, C, H, W):
    """PackNet's Conv2D tail: GroupNorm(16) + ELU (layers01.py:L33-40)."""
    g = torch.Generator().manual_seed(C + H + 1)
    V = 4 if dtype == torch.float32 else 8
    B = 2
    x = torch.randn(B, C, H, W, generator=g) * 2 + 0.3
    gamma = torch.rand(C, generator=g) + 0.5; beta = torch.randn(C, generator=g) * 0.3
    if dtype != torch.float32:
        x = x.to(dtype).float()
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    o = F.elu(F.group_norm(xr, 16, gr, br, 1e-5))
    go = torch.randn(o.shape, generator=g)
    o.backward(go)
    xd = nhwc(x, dtype, V).requires_grad_(True)
    gd, bd = (t.clone().to(dev).requires_grad_(True) for t in (gamma, beta))
    out = NN.group_norm_relu(xd, gd, bd, 16, 1e-5, "elu")
    check(nchw(out, C), o.detach(), dtype, "gn-elu out", bound=gn_bound(x, gamma, beta, NB.ACT_ELU, dtype))
    out.backward(nhwc(go, dtype, V))
    check(nchw(xd.grad, C), xr.grad, dtype, "gn-elu dx", 5e-5, 3e-2)
    check(gd.grad.cpu(), gr.grad, dtype, "gn-elu dgamma", 5e-5, 3e-2)
    check(bd.grad.cpu(), br.grad, dtype, "gn-elu dbeta", 5e-5, 3e-2)


@functools.lru_cache(maxsize=None)
def conv3d_reference(dtype, B, D, H, W):
    """Operands (rounded to the storage type), the CPU fp32 result and the per-element bounds from fp64 (conv_bounds.Conv3dPackCase): computed once per
    case, never modified."""
    g = torch.Generator().manual_seed(D + H)
    x = torch.randn(B, D, H, W, generator=g)
    w = torch.randn(8, 1, 3, 3, 3, generator=g) * 0.3
    bias = torch.randn(8, generator=g) * 0.2
    x = CB.rounded(x, dtype)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, bias))
    o = F.conv3d(xr.unsqueeze(1), wr, br, padding=1).reshape(B, 8 * D, H, W)
    go = CB.rounded(torch.randn(o.shape, generator=g), dtype)
    o.backward(go)
    case = CB.Conv3dPackCase(x, w, bias, dtype)
    return dict(x=x, w=w, bias=bias, go=go, o=o.detach(), dx=xr.grad, dw=wr.grad, db=br.grad, case=case, bw=case.backward(go))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,D,H,W", [(2, 16, 5, 7), (1, 64, 9, 12), (2, 256, 3, 4),
                                     (2, 64, 40, 36), (1, 192, 47, 50), (3, 128, 26, 33)])     # more than 64 channel groups per wave boundary / several waves per pixel row
def test_conv3d_pack(NN, dtype, B, D, H, W):
    """layers01.py:L223-298: x.unsqueeze(1) -> Conv3d(1, 8, 3, padding=1) -> view(b, 8*D, h, w), forward and all three gradients, in the three
    activation dtypes the kernels are instantiated for (PackNet trains in fp16)."""
    ref = conv3d_reference(dtype, B, D, H, W)
    case, bw = ref["case"], ref["bw"]
    V = 4 if dtype == torch.float32 else 8
    xd = nhwc(ref["x"], dtype, V).requires_grad_(True)
    wd, bd = (t.clone().to(dev).requires_grad_(True) for t in (ref["w"], ref["bias"]))
    out = NN.conv3d_pack(xd, wd, bd)
    assert out.shape == (B, H, W, 8 * D) and out.dtype == dtype
    tag = CB.DT_NAME[dtype]
    check(nchw(out, 8 * D), ref["o"], dtype, f"{tag} conv3d out", bound=case.y)
    out.backward(nhwc(ref["go"], dtype, V))
    check(nchw(xd.grad, D), ref["dx"], dtype, f"{tag} conv3d dx", bound=bw["dX"])
    # gradients are accumulated and stored in fp32 from the same rounded operands, whatever the activation dtype
    check(wd.grad.cpu(), ref["dw"], torch.float32, f"{tag} conv3d dw", 2e-5, 2e-5, bound=bw["dW"])
    check(bd.grad.cpu(), ref["db"], torch.float32, f"{tag} conv3d dbias", 2e-5, 2e-5, bound=bw["dbias"])


@pytest.mark.parametrize("layout", ["oihw", "ohwi"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_weight_packer_equals_per_layer_pack(NN, dtype, layout):
    """sde_pack_weights_batched (LDS-tiled, every layer in one launch) == sde_pack_weight per layer and operand, bit for bit.
    "ohwi": channels-last master weights, as HipTrainer keeps them (16-bit operands without channel padding take the vectorised path)."""
    from simpledepthestimation_amd.layers.hip_modules import HipConv2d
    V = 4 if dtype == torch.float32 else 8
    shapes = [(3, 64, 7), (64, 64, 3), (193, 128, 3), (256, 64, 5), (64, 256, 1), (16, 1, 3), (520, 40, 3), (2048, 24, 1)]
    torch.manual_seed(5)
    net = torch.nn.ModuleList([HipConv2d(ci, co, k, padding=k // 2) for ci, co, k in shapes]).to(dev)
    if layout == "ohwi":
        for m in net:
            m.weight.data = m.weight.data.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
            assert NN.is_ohwi(m.weight) or m.kernel_size == 1          # (a 1x1 weight is the same memory either way)
    for m, (ci, co, k) in zip(net, shapes):
        x = torch.zeros(1, 8, 8, (ci + V - 1) // V * V, device=dev, dtype=dtype)
        m(x)                                   # records the padded operand shapes
    packer = NN.WeightPacker(net)
    packer.run()
    for m, (ci, co, k) in zip(net, shapes):
        dt, cin_pad, ldy = m._pack_shapes
        wp, wd = m._packed
        assert torch.equal(wp, NN.pack_weight(m.weight, dt, cin_pad, ldy, for_dgrad=False)), f"forward operand {ci}->{co} k{k}"
        assert torch.equal(wd, NN.pack_weight(m.weight, dt, cin_pad, ldy, for_dgrad=True)), f"dgrad operand {ci}->{co} k{k}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", [(2, 6, 20, 256, 512, 3, True), (1, 12, 40, 2048, 256, 1, False), (2, 6, 20, 2048, 256, 3, False)],
                         ids=["3x3_256_512_bias_elu", "1x1_2048_256_stats", "3x3_2048_256_stats"])
def test_split_k_equals_single_pass(NN, dtype, shape):
    """sde_conv_fwd_ws (split-K: partial tiles + fixed-order finish kernel) against sde_conv_fwd (one pass over K) on the same operands:
    outputs, padded channels, and the BatchNorm partial slabs (summed over tiles)."""
    import ctypes
    from simpledepthestimation_amd.hip import lib as L
    B, H, W, Cin, Cout, k, with_bias = shape
    g = torch.Generator().manual_seed(Cin + Cout)
    V = 4 if dtype == torch.float32 else 8
    x = nhwc(torch.randn(B, Cin, H, W, generator=g), dtype, V)
    w = (torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)).to(dev)
    bias = (torch.randn(Cout, generator=g) * 0.1).to(dev) if with_bias else None
    act = NN.ACT_ELU if with_bias else NN.ACT_NONE
    ldy = (Cout + V - 1) // V * V
    wp = NN.pack_weight(w, dtype, x.shape[-1], ldy)
    d = NN._desc(x, None, NN.SRC_PLAIN, k, k, 1, k // 2, False, H, W, H, W)
    lib = L.lib()
    ws_bytes = lib.sde_conv_fwd_ws_bytes(ctypes.byref(d), ldy)
    assert ws_bytes > 0, "shape was chosen to run split-K"
    tiles = lib.sde_conv_fwd_tiles_m(ctypes.byref(d), ldy)
    outs = []
    for use_ws in (False, True):
        y = torch.empty(B, H, W, ldy, device=dev, dtype=dtype)
        stats = None if with_bias else torch.zeros(tiles + NN.REDUCE_ROWS, Cout, 2, device=dev)
        ws = torch.empty(ws_bytes // 4, device=dev) if use_ws else None
        if use_ws:
            L.check(lib.sde_conv_fwd_ws(ctypes.byref(d), L.ptr(wp), L.ptr(bias), act, L.ptr(y), Cout, ldy, L.ptr(stats), L.ptr(ws), ws_bytes, L.stream()), "ws")
        else:
            L.check(lib.sde_conv_fwd(ctypes.byref(d), L.ptr(wp), L.ptr(bias), act, L.ptr(y), Cout, ldy, L.ptr(stats), L.stream()), "plain")
        outs.append((y.float().cpu(), None if stats is None else stats[:tiles].sum(0).cpu()))
    check(outs[1][0], outs[0][0], dtype, "split-K output", 2e-5, 1e-2)
    assert (outs[1][0][..., Cout:] == 0).all()
    if outs[0][1] is not None:
        check(outs[1][1], outs[0][1], dtype, "split-K BN partial sums", 1e-4, 1e-2)


def test_prep_input(NN):
    g = torch.Generator().manual_seed(3)
    img = torch.rand(2, 3, 10, 14, generator=g)
    mean = torch.tensor([0.485, 0.456, 0.406]); std = torch.tensor([0.229, 0.224, 0.225])
    ref = (img - mean.view(1, 3, 1, 1)) / std.view(1, 3, 1, 1)
    for dtype, V in [(torch.float32, 4), (torch.bfloat16, 8), (torch.float16, 8)]:
        for flip in (False, True):
            out = NN.prep_input(img.to(dev), mean.to(dev), std.to(dev), dtype, flip)
            assert out.shape == (2, 10, 14, V) and (out[..., 3:] == 0).all()
            r = torch.flip(ref, [3]) if flip else ref
            check(nchw(out, 3), r, dtype, "prep_input", 1e-6, 5e-3)
    nine = torch.rand(2, 9, 6, 8, generator=g)
    out = NN.prep_input(nine.to(dev), None, None, torch.float32)
    assert out.shape == (2, 6, 8, 12)
    assert torch.equal(nchw(out, 9), nine)


@pytest.mark.parametrize("decoupled", [False, True])
def test_adam_step(NN, decoupled):
    g = torch.Generator().manual_seed(4)
    n1, n2 = 1000, 777
    p = torch.randn(n1 + n2, generator=g); gr = torch.randn(n1 + n2, generator=g)
    pa, pb = p[:n1].clone().requires_grad_(True), p[n1:].clone().requires_grad_(True)
    groups = [{"params": [pa], "lr": 2e-4, "weight_decay": 1e-2 if decoupled else 0.0}, {"params": [pb], "lr": 1e-4, "weight_decay": 0.0}]
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(groups, eps=1e-6)
    pd, m, v = p.clone().to(dev), torch.zeros(n1 + n2, device=dev), torch.zeros(n1 + n2, device=dev)
    seg_end = [n1, n1 + n2]
    seg_lr = [2e-4, 1e-4]; seg_wd = [1e-2 if decoupled else 0.0, 0.0]
    for t in range(1, 4):
        gt = gr * (1.0 + 0.1 * t)
        pa.grad, pb.grad = gt[:n1].clone(), gt[n1:].clone()
        opt.step()
        bc = torch.tensor([1 - 0.9 ** t, 1 - 0.999 ** t], device=dev)
        NN.adam_step(pd, gt.to(dev), m, v, seg_end, seg_lr, seg_wd, bc, eps=1e-6, decoupled_wd=decoupled)
    ref = torch.cat([pa.detach(), pb.detach()])
    assert (pd.cpu() - ref).abs().max().item() < 1e-6


def test_adam_step_with_loss_scaling_keeps_torch_step_count_across_a_skipped_step(NN):
    """torch.optim.AdamW driven the way GradScaler.step drives it (detectron2/engine/train_loop.py:L294-341): on an overflow optimizer.step()
    is not called at all, so Adam's `step` -- and with it the bias corrections -- does not advance.  The fused path keeps the count of APPLIED
    steps on the device (scale_state[3]); p, m, v after steps {ok, overflow, ok, ok} must equal torch's after three applied steps."""
    g = torch.Generator().manual_seed(14)
    n1, n2 = 1000, 777
    p = torch.randn(n1 + n2, generator=g); gr = torch.randn(n1 + n2, generator=g)
    pa, pb = p[:n1].clone().requires_grad_(True), p[n1:].clone().requires_grad_(True)
    opt = torch.optim.AdamW([{"params": [pa], "lr": 2e-4, "weight_decay": 1e-2}, {"params": [pb], "lr": 1e-4, "weight_decay": 0.0}], eps=1e-6)
    pd, m, v = p.clone().to(dev), torch.zeros(n1 + n2, device=dev), torch.zeros(n1 + n2, device=dev)
    state = torch.tensor([1024.0, 0.0, 0.0, 0.0], device=dev)
    seg_end, seg_lr, seg_wd = [n1, n1 + n2], [2e-4, 1e-4], [1e-2, 0.0]
    scales = []
    for t, overflow in enumerate([False, True, False, False], start=1):
        gt = gr * (1.0 + 0.1 * t)
        scale = float(state[0])
        gdev = (gt * scale).to(dev)                      # what backward of the scaled loss leaves in the flat gradient
        if overflow:
            gdev[5] = float("inf")
        else:
            pa.grad, pb.grad = gt[:n1].clone(), gt[n1:].clone()
            opt.step()                                   # GradScaler.step: only without found_inf
        NN.grad_check(gdev, state)
        # a deliberately WRONG host-side bias correction: with scale_state the kernel must use its own count
        NN.adam_step(pd, gdev, m, v, seg_end, seg_lr, seg_wd, (0.5, 0.5), eps=1e-6, decoupled_wd=True, scale_state=state)
        NN.loss_scale_update(state, 2.0, 0.5, 1000)
        scales.append(float(state[0]))
    assert scales == [1024.0, 512.0, 512.0, 512.0] and float(state[3]) == 3.0 and float(state[1]) == 0.0
    ref = torch.cat([pa.detach(), pb.detach()])
    assert (pd.cpu() - ref).abs().max().item() < 1e-6
    st = opt.state[pa]
    assert float(st["step"]) == 3.0
    assert (m[:n1].cpu() - st["exp_avg"]).abs().max().item() < 1e-6 and (v[:n1].cpu() - st["exp_avg_sq"]).abs().max().item() < 1e-6


BNBWD_CASES = [
    # name, B, H, W, C (BatchNorm'd channels = input of the second convolution), Cout2, k2, expected kernel
    ("1x1_per_tile", 2, 24, 40, 64, 256, 1),            # persistent GEMM, one statistics row per tile
    ("1x1_ragged_M", 1, 7, 9, 128, 128, 1),             # M = 63 < one tile
    ("1x1_per_workgroup", 12, 48, 160, 64, 64, 1),      # 1440 tiles on 768 persistent workgroups: partials kept in registers over a workgroup's tiles
    ("1x1_wide", 3, 12, 20, 512, 128, 1),               # eight N tiles
    ("3x3_halo", 4, 48, 160, 64, 64, 3),                # LDS-halo 3x3 kernel (240 workgroups)
    ("3x3_halo_ragged", 12, 20, 36, 128, 128, 3),       # 8x16 tiles overhang the image
    ("3x3_small", 1, 8, 16, 64, 64, 3),                 # too few tiles for the halo kernel: persistent GEMM with filter taps
]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", BNBWD_CASES, ids=[c[0] for c in BNBWD_CASES])
def test_bn_backward_reduce_in_the_dgrad_epilogue(NN, case, dt):
    """conv_a -> BatchNorm + ReLU (no residual, one consumer) -> conv_b, backward: the data gradient of conv_b masks its output with relu'(bn(y)) and
    leaves BatchNorm's (sum gm, sum gm * xhat) partials in its epilogue (sde_conv_dgrad_bnbwd + sde_bn_bwd_from_part) against the separate
    bn_bwd_reduce pass over the same tensors (same summands, another order), and -- on the small cases -- against torch-CPU fp32 autograd on the
    16-bit-rounded operands."""
    name, B, H, W, C, Cout2, k2 = case
    if dt == torch.float16 and name not in ("1x1_per_tile", "3x3_halo"):
        pytest.skip("fp16 instantiation: one case per kernel")
    g = torch.Generator().manual_seed(B * 1000 + C + k2)
    Cin = 64
    x = (torch.randn(B, Cin, H, W, generator=g) + 0.2).to(dt).float()
    wa = (torch.randn(C, Cin, 1, 1, generator=g) / math.sqrt(Cin)).to(dt).float()
    wb = (torch.randn(Cout2, C, k2, k2, generator=g) / math.sqrt(C * k2 * k2)).to(dt).float()
    gamma = torch.rand(C, generator=g) + 0.5; beta = torch.randn(C, generator=g) * 0.3
    go = torch.randn(B, Cout2, H, W, generator=g).to(dt).float()
    res = []
    for fused in (False, True):
        NN.BNBWD_FUSED = fused
        try:
            xd = nhwc(x, dt, 8).requires_grad_(True)
            wad, wbd, gd, bd = (t.clone().to(dev).requires_grad_(True) for t in (wa, wb, gamma, beta))
            hits = NN.BNBWD_HITS
            y, stats = NN.conv2d(xd, wad, None, stride=1, pad=0, bn_stats=True)
            a = NN.batch_norm_act(y, stats, gd, bd, torch.zeros(C, device=dev), torch.ones(C, device=dev), relu=True)
            out = NN.conv2d(a, wbd, None, stride=1, pad=k2 // 2)
            out.backward(nhwc(go, dt, 8))
            torch.cuda.synchronize()
            assert NN.BNBWD_HITS - hits == (1 if fused else 0), f"{name}: fused path {'not ' if fused else ''}taken"
            res.append([t.detach().float().cpu() for t in (out, xd.grad, wad.grad, wbd.grad, gd.grad, bd.grad)])
        finally:
            NN.BNBWD_FUSED = True
    for nm, u, f in zip(("out", "dX", "dWa", "dWb", "dgamma", "dbeta"), res[0], res[1]):
        assert relerr(f, u) < (1e-6 if nm in ("out", "dWb") else 3e-3), f"{name} {nm}: fused vs separate {relerr(f, u):.3e}"
    if B * H * W <= 4000:
        xr, war, wbr, gr, br = (t.clone().requires_grad_(True) for t in (x, wa, wb, gamma, beta))
        yc = F.conv2d(xr, war)
        yc = yc + (yc.detach().to(dt).float() - yc.detach())          # the GPU path stores the convolution output in 16 bits before normalising
        ar = F.relu(F.batch_norm(yc, torch.zeros(C), torch.ones(C), gr, br, True, 0.1, 1e-5))
        F.conv2d(ar, wbr, None, 1, k2 // 2).backward(go)
        check(nchw(res[1][1].to(dev), Cin), xr.grad, torch.bfloat16, "dX vs cpu", bf16_tol=3e-2)
        check(res[1][2], war.grad, torch.bfloat16, "dWa vs cpu", bf16_tol=3e-2)
        check(res[1][4], gr.grad, torch.bfloat16, "dgamma vs cpu", bf16_tol=3e-2)
        check(res[1][5], br.grad, torch.bfloat16, "dbeta vs cpu", bf16_tol=3e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "fp16"])
def test_space_to_depth_and_depth_to_space(NN, dtype):
    """layers01.py:L138-160 `packing` and nn.PixelShuffle(2) on NHWC as one permutation kernel each (csrc/packnet.hip), each other's backward: vs the
    reference's view / permute chain and F.pixel_shuffle on NCHW, exactly (pure data movement)."""
    g = torch.Generator().manual_seed(40)
    B, C, H, W = 2, 16, 6, 10
    x = torch.randn(B, C, H, W, generator=g).to(dtype).float()
    # the reference's packing (layers01.py:L138-160): view(b,c,oh,r,ow,r) -> permute(0,1,3,5,2,4) -> view(b, c*r*r, oh, ow)
    ref = x.view(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 3, 5, 2, 4).contiguous().view(B, C * 4, H // 2, W // 2)
    xd = nhwc(x, dtype, 1).requires_grad_(True)
    y = NN.space_to_depth(xd)
    assert y.shape == (B, H // 2, W // 2, 4 * C) and torch.equal(nchw(y, 4 * C), ref)
    gy = torch.randn(y.shape, generator=g).to(dtype).to(dev)
    y.backward(gy)
    assert torch.equal(xd.grad, NN.depth_to_space(gy))                                   # the backward IS the inverse permutation
    z = NN.depth_to_space(y.detach())
    assert torch.equal(z, xd.detach())
    ps = F.pixel_shuffle(ref, 2)
    assert torch.equal(nchw(NN.depth_to_space(nhwc(ref, dtype, 1)), C), ps)
    with pytest.raises(Exception):
        NN.space_to_depth(torch.zeros(1, 5, 6, 16, device=dev, dtype=dtype))            # odd height


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "fp16"])
@pytest.mark.parametrize("add,with_inv,with_p1", [(False, True, True), (False, False, True), (True, True, True), (True, False, True), (False, True, False)])
def test_concat_with_upsampled_inverse_depth(NN, dtype, add, with_inv, with_p1):
    """PackNet01.py:L150-199: cat([unpacked, skip(, nearest_x2(inv depth))], 1) / [unpacked + skip(, ...)] in one pass, zero-filled to the 16-byte group;
    backward = slices and the 2x2 sums of the inverse-depth channel."""
    g = torch.Generator().manual_seed(41)
    V = 4 if dtype == torch.float32 else 8
    B, H, W, C0 = 2, 8, 12, 16
    C1 = C0 if add else 24
    p0 = torch.randn(B, C0, H, W, generator=g).to(dtype).float()
    p1 = torch.randn(B, C1, H, W, generator=g).to(dtype).float() if with_p1 else None
    inv = torch.rand(B, H // 2, W // 2, generator=g) if with_inv else None
    p0r = p0.clone().requires_grad_(True); p1r = p1.clone().requires_grad_(True) if with_p1 else None
    invr = inv.clone().requires_grad_(True) if with_inv else None
    parts = [p0r + p1r] if add else ([p0r, p1r] if with_p1 else [p0r])
    if with_inv:
        parts.append(F.interpolate(invr.unsqueeze(1), scale_factor=2, mode="nearest").to(dtype).float())
    ref = torch.cat(parts, 1)
    if add and dtype != torch.float32:
        ref = ref + (ref.detach().to(dtype).float() - ref.detach())
    p0d = nhwc(p0, dtype, V).requires_grad_(True); p1d = nhwc(p1, dtype, V).requires_grad_(True) if with_p1 else None
    invd = inv.clone().to(dev).requires_grad_(True) if with_inv else None
    out = NN.concat(p0d, p1d, invd, add=add)
    Cu = ref.shape[1]
    assert out.shape[3] == (Cu + V - 1) // V * V and (out[..., Cu:] == 0).all()
    check(nchw(out, Cu), ref.detach(), dtype, "concat", 1e-6, 8e-3)
    go = torch.randn(B, out.shape[3], H, W, generator=g).to(dtype).float()
    ref.backward(go[:, :Cu])
    out.backward(go.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev))
    check(nchw(p0d.grad, C0), p0r.grad, dtype, "d p0", 1e-6, 1e-6)
    if with_p1:
        check(nchw(p1d.grad, C1), p1r.grad, dtype, "d p1", 1e-6, 1e-6)
    if with_inv:
        check(invd.grad.cpu(), invr.grad, dtype, "d inv", 1e-6, 1e-6)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "fp16"])
@pytest.mark.parametrize("flip", [False, True])
def test_inv_depth_head(NN, dtype, flip):
    """layers01.py:L105-133 (sigmoid / min_depth) + PackNet01.py:L120-123,L199 (disp_to_depth, flip back) in one kernel, both outputs with gradients."""
    g = torch.Generator().manual_seed(42)
    B, H, W, ld = 2, 6, 10, (4 if dtype == torch.float32 else 8)
    y = torch.zeros(B, H, W, ld)
    y[..., 0] = (torch.randn(B, H, W, generator=g) * 2).to(dtype).float()
    yr = y[..., 0].clone().requires_grad_(True)
    inv_r = torch.sigmoid(yr) / 0.5
    dep_r = 1.0 / (1.0 / 80.0 + (1.0 / 0.1 - 1.0 / 80.0) * inv_r.unsqueeze(1))
    if flip:
        dep_r = dep_r.flip(3)
    yd = y.to(dtype).to(dev).requires_grad_(True)
    inv, dep = NN.inv_depth_head(yd, 0.5, 0.1, 80.0, flip)
    assert inv.shape == (B, H, W) and dep.shape == (B, 1, H, W) and inv.dtype == torch.float32
    check(inv.cpu(), inv_r.detach(), torch.float32, "inv", 1e-6)
    check(dep.cpu(), dep_r.detach(), torch.float32, "depth", 2e-6)
    gi = torch.randn(B, H, W, generator=g); gd = torch.randn(B, 1, H, W, generator=g)
    (inv_r * gi).sum().add((dep_r * gd).sum()).backward()
    (inv * gi.to(dev)).sum().add((dep * gd.to(dev)).sum()).backward()
    check(yd.grad[..., 0].float().cpu(), yr.grad, dtype, "d logit", 2e-5, 8e-3)
    assert (yd.grad[..., 1:] == 0).all()
    # one of the two outputs unused (the finest level's inverse depth has no consumer)
    yd2 = y.to(dtype).to(dev).requires_grad_(True)
    _, dep2 = NN.inv_depth_head(yd2, 0.5, 0.1, 80.0, flip)
    (dep2 * gd.to(dev)).sum().backward()
    yr2 = y[..., 0].clone().requires_grad_(True)
    d2 = 1.0 / (1.0 / 80.0 + (1.0 / 0.1 - 1.0 / 80.0) * (torch.sigmoid(yr2) / 0.5).unsqueeze(1))
    ((d2.flip(3) if flip else d2) * gd).sum().backward()
    check(yd2.grad[..., 0].float().cpu(), yr2.grad, dtype, "d logit (depth only)", 2e-5, 8e-3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [64, 256])
def test_group_norm_elu_with_residual(NN, dtype, C):
    """layers01.py:L74-76 ResidualConv: ELU(GroupNorm(x_out + shortcut)) with the sum formed inside the GroupNorm kernels (fp32), gradient to both inputs."""
    g = torch.Generator().manual_seed(43 + C)
    B, H, W = 2, 9, 14
    x = torch.randn(B, C, H, W, generator=g).to(dtype).float(); r = (torch.randn(B, C, H, W, generator=g) * 0.7).to(dtype).float()
    gamma = torch.rand(C, generator=g) + 0.5; beta = torch.randn(C, generator=g) * 0.2
    xr, rr, gr, br = (t.clone().requires_grad_(True) for t in (x, r, gamma, beta))
    ref = F.elu(F.group_norm(xr + rr, 16, gr, br, 1e-5))
    go = torch.randn(ref.shape, generator=g).to(dtype).float()
    ref.backward(go)
    V = 4 if dtype == torch.float32 else 8
    xd = nhwc(x, dtype, V).requires_grad_(True); rd = nhwc(r, dtype, V).requires_grad_(True)
    gd, bd = gamma.clone().to(dev).requires_grad_(True), beta.clone().to(dev).requires_grad_(True)
    out = NN.group_norm_relu(xd, gd, bd, 16, 1e-5, "elu", residual=rd)
    check(nchw(out, C), ref.detach(), dtype, "gn(x + r)")
    out.backward(nhwc(go, dtype, V))
    check(nchw(xd.grad, C), xr.grad, dtype, "dx", 5e-5, 3e-2)
    assert torch.equal(xd.grad, rd.grad)
    check(gd.grad.cpu(), gr.grad, dtype, "dgamma", 5e-5, 3e-2)
    check(bd.grad.cpu(), br.grad, dtype, "dbeta", 5e-5, 3e-2)


def test_full_size_conv_properties(NN):
    """BASELINE size (B=12, 48x160, 64->64 3x3, bf16): linearity in the input and agreement of a strided sub-sample with fp32 CPU."""
    g = torch.Generator().manual_seed(5)
    B, H, W, C = 12, 48, 160, 64
    x1 = torch.randn(B, H, W, C, generator=g).bfloat16().to(dev); x2 = torch.randn(B, H, W, C, generator=g).bfloat16().to(dev)
    w = (torch.randn(C, C, 3, 3, generator=g) / 24).bfloat16().float().to(dev)
    y1 = NN.conv2d(x1, w, None, stride=1, pad=1).float(); y2 = NN.conv2d(x2, w, None, stride=1, pad=1).float()
    y12 = NN.conv2d((x1.float() + x2.float()).bfloat16(), w, None, stride=1, pad=1).float()
    assert relerr(y12.cpu(), (y1 + y2).cpu()) < 2e-2
    ref = F.conv2d(x1[:2].float().permute(0, 3, 1, 2).cpu(), w.cpu(), None, 1, 1)
    check(nchw(y1[:2].to(torch.bfloat16), C), ref, torch.bfloat16, "sub-sample vs fp32 cpu")


HALO_CASES = [
    # name, B, H, W, Cin, Cout, reflect, bias, act; "halo_*" run on the LDS-halo kernel (asserted), "staged_*" do not: halo_applicable refuses inputs narrower
    # than 48 channels, so these two run on the register-staged 128x16 tile (also rows of tests/conv_variant_table.py, under that variant)
    ("halo_64_64_zero", 2, 16, 32, 64, 64, False, False, 0),
    ("halo_128_128_zero", 2, 16, 32, 128, 128, False, False, 0),
    ("halo_96_32_refl_elu", 2, 24, 48, 96, 32, True, True, 1),        # channel tail inside the second 64-channel block
    ("staged_16_16_refl_elu", 2, 24, 48, 16, 16, True, True, 1),
    ("staged_32_1_refl_head", 2, 16, 32, 32, 1, True, True, 0),
    ("halo_ragged_64_64", 2, 20, 44, 64, 64, False, True, 0),         # 20x44 is not a multiple of the 8x16 tile
    ("halo_256_256_zero", 1, 16, 32, 256, 256, False, False, 0),      # 4 channel blocks, 2 N tiles
]


@pytest.fixture
def force_halo(NN):
    from simpledepthestimation_amd.hip import lib as L
    old = L.lib().sde_conv_set_halo_min_blocks(0)
    yield
    L.lib().sde_conv_set_halo_min_blocks(old)


def fwd_variant(NN, x0, x1, upcat, reflect, ldy):
    """sde_conv_fwd_variant of the 3x3 stride-1 layer hip.nn.conv2d builds from these NHWC inputs."""
    import ctypes
    from simpledepthestimation_amd.hip import lib as L
    B, H, W, _ = x0.shape
    H, W = (2 * H, 2 * W) if upcat else (H, W)
    d = NN._desc(x0, x1, NN.SRC_UPCAT if upcat else NN.SRC_PLAIN, 3, 3, 1, 1, reflect, H, W, H, W)
    return L.lib().sde_conv_fwd_variant(ctypes.byref(d), ldy)


def halo_variant(ldy):
    return 3128000 + (64 if ldy > 32 else 32 if ldy > 16 else 16)


def halo_kernel_case(NN, case, dtype):
    name, B, H, W, Cin, Cout, reflect, has_bias, act = case
    V = 8
    g = torch.Generator().manual_seed(len(name.replace("staged", "halo")) * 7)       # (the seeds the cases had under their first names)
    x = torch.randn(B, Cin, H, W, generator=g).to(dtype).float()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)).to(dtype).float()
    b = torch.randn(Cout, generator=g) * 0.1 if has_bias else None
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if has_bias else None
    xin = F.pad(xr, (1, 1, 1, 1), mode="reflect") if reflect else xr
    yr = F.conv2d(xin, wr, br, 1, 0 if reflect else 1)
    if act == 1:
        yr = F.elu(yr)
    gy = torch.randn(yr.shape, generator=g).to(dtype).float()
    yr.backward(gy)
    cb = CB.ConvCase(x, w, b, dtype, stride=1, pad=1, reflect=reflect, act=act)
    lim = cb.backward([gy])
    xd = nhwc(x, dtype, V).requires_grad_(True)
    wd = w.clone().to(dev).requires_grad_(True)
    bd = b.clone().to(dev).requires_grad_(True) if has_bias else None
    # which kernel runs is asserted first: a dispatcher rule that re-routes a case must not leave it testing something else
    assert fwd_variant(NN, xd, None, False, reflect, (Cout + V - 1) // V * V) == (halo_variant(Cout) if name.startswith("halo") else 128016), name
    y = NN.conv2d(xd, wd, bd, stride=1, pad=1, reflect=reflect, act=act)
    check(nchw(y, Cout), yr.detach(), dtype, "y", bound=cb.y)
    if y.shape[3] > Cout:
        assert (y[..., Cout:] == 0).all()
    y.backward(nhwc(gy, dtype, V))
    check(nchw(xd.grad, Cin), xr.grad, dtype, "dX", bound=lim["dX"])
    check(wd.grad.cpu(), wr.grad, dtype, "dW", bound=lim["dW"])


@pytest.mark.parametrize("case", HALO_CASES, ids=[c[0] for c in HALO_CASES])
def test_conv_halo_kernel(NN, force_halo, case):
    """The LDS-halo 3x3 kernel (forward and data-gradient, incl. the padded 'full' gradient of reflection layers) vs fp32 CPU."""
    halo_kernel_case(NN, case, torch.bfloat16)


@pytest.mark.parametrize("case", HALO_CASES, ids=[c[0] for c in HALO_CASES])
def test_conv_halo_kernel_fp16(NN, force_halo, case):
    halo_kernel_case(NN, case, torch.float16)


def halo_upsample_concat_case(NN, C0, C1, Cout, dtype):
    V = 8
    g = torch.Generator().manual_seed(C0 * 3 + C1)
    B, h, w = 2, 8, 16
    x0 = torch.randn(B, C0, h, w, generator=g).to(dtype).float()
    x1 = torch.randn(B, C1, 2 * h, 2 * w, generator=g).to(dtype).float() if C1 else None
    wt = (torch.randn(Cout, C0 + C1, 3, 3, generator=g) / math.sqrt((C0 + C1) * 9)).to(dtype).float()
    bs = torch.randn(Cout, generator=g) * 0.1
    x0r = x0.clone().requires_grad_(True); x1r = x1.clone().requires_grad_(True) if C1 else None
    wr = wt.clone().requires_grad_(True)
    up = F.interpolate(x0r, scale_factor=2, mode="nearest")
    cat = torch.cat([up, x1r], 1) if C1 else up
    yr = F.elu(F.conv2d(F.pad(cat, (1, 1, 1, 1), mode="reflect"), wr, bs))
    gy = torch.randn(yr.shape, generator=g).to(dtype).float()
    yr.backward(gy)
    cb = CB.ConvCase(x0, wt, bs, dtype, stride=1, pad=1, reflect=True, act=1, x1=x1, upcat=True)
    lim = cb.backward([gy])
    x0d = nhwc(x0, dtype, V).requires_grad_(True)
    x1d = nhwc(x1, dtype, V).requires_grad_(True) if C1 else None
    wd = wt.clone().to(dev).requires_grad_(True)
    # (16 input channels are too narrow for the halo kernel: that case runs on the register-staged 128x16 tile)
    assert fwd_variant(NN, x0d, x1d, True, True, Cout) == (halo_variant(Cout) if C0 + C1 >= 48 else 128016)
    y = NN.conv2d(x0d, wd, bs.to(dev), stride=1, pad=1, reflect=True, act=1, skip=x1d, upsample=True)
    check(nchw(y, Cout), yr.detach(), dtype, "y", bound=cb.y)
    y.backward(nhwc(gy, dtype, V))
    check(nchw(x0d.grad, C0), x0r.grad, dtype, "dx0", bound=lim["dX"])
    if C1:
        check(nchw(x1d.grad, C1), x1r.grad, dtype, "dx1", bound=lim["dSkip"])


@pytest.mark.parametrize("C0,C1,Cout", [(32, 64, 32), (16, 0, 16), (64, 256, 64)])
def test_conv_halo_upsample_concat(NN, force_halo, C0, C1, Cout):
    halo_upsample_concat_case(NN, C0, C1, Cout, torch.bfloat16)


@pytest.mark.parametrize("C0,C1,Cout", [(32, 64, 32), (16, 0, 16), (64, 256, 64)])
def test_conv_halo_upsample_concat_fp16(NN, force_halo, C0, C1, Cout):
    halo_upsample_concat_case(NN, C0, C1, Cout, torch.float16)


def halo_batchnorm_stats_case(NN, Cin, variant):
    g = torch.Generator().manual_seed(9)
    B, H, W, C = 2, 20, 44, 64
    x = (torch.randn(B, Cin, H, W, generator=g) + 0.3).bfloat16().float()
    w = (torch.randn(C, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)).bfloat16().float()
    gamma = torch.rand(C, generator=g) + 0.5; beta = torch.randn(C, generator=g) * 0.2
    yc = F.conv2d(x, w, None, 1, 1)
    yc = yc.bfloat16().float()
    o = F.relu(F.batch_norm(yc, torch.zeros(C), torch.ones(C), gamma, beta, True, 0.1, 1e-5))
    xd = nhwc(x, torch.bfloat16, 8)
    assert fwd_variant(NN, xd, None, False, False, C) == variant
    y, stats = NN.conv2d(xd, w.to(dev), None, stride=1, pad=1, bn_stats=True)
    out = NN.batch_norm_act(y, stats, gamma.to(dev), beta.to(dev), torch.zeros(C, device=dev), torch.ones(C, device=dev))
    check(nchw(out, C), o, torch.bfloat16, "bn(halo conv)")


def test_conv_halo_batchnorm_stats(NN, force_halo):
    """BatchNorm statistics from the convolution's epilogue over ragged tiles.  (32 input channels are too narrow for the halo kernel -- halo_applicable --
    so this case has always run on the register-staged 64x64 tile; the next test is the halo kernel's.)"""
    halo_batchnorm_stats_case(NN, 32, 64064)


def test_conv_halo_batchnorm_stats_on_the_halo_kernel(NN, force_halo):
    """BatchNorm statistics produced by the halo kernel's epilogue (ragged tiles must not pollute them)."""
    halo_batchnorm_stats_case(NN, 64, 3128064)


@pytest.mark.parametrize("C,R,with_res,relu,dtype", [(256, 192, False, True, torch.bfloat16), (512, 96, True, True, torch.bfloat16), (2048, 23, False, False, torch.bfloat16),
                                                    (64, 256, True, True, torch.float16), (1024, 1, False, True, torch.bfloat16)])
def test_bn_finalize_apply_fused_equals_separate(NN, C, R, with_res, relu, dtype):
    """sde_bn_finalize_apply (one launch; every workgroup re-reduces the slab columns of its 64 channels) against sde_bn_finalize + sde_bn_apply:
    the same statistics (fp64 sums in a different order: 1e-6), running statistics, and outputs equal up to that."""
    g = torch.Generator().manual_seed(C + R)
    M = 37 * R + 11                                        # ragged: not a multiple of the 32-row pass
    y = (torch.randn(M, C, generator=g) * 1.5 + 0.2).to(dtype)
    res = torch.randn(M, C, generator=g).to(dtype) if with_res else None
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    yf = y.float()
    bounds = [round(i * M / R) for i in range(R + 1)]
    stats = torch.zeros(R + NN.REDUCE_ROWS, C, 2)
    for i in range(R):
        blk = yf[bounds[i]:bounds[i + 1]]
        stats[i, :, 0], stats[i, :, 1] = blk.sum(0), (blk * blk).sum(0)
    outs = {}
    for fused in (True, False):
        old, NN.FUSE_BN_FINALIZE = NN.FUSE_BN_FINALIZE, fused
        try:
            rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
            yd = y.to(dev).view(1, 1, M, C)
            rd = res.to(dev).view(1, 1, M, C) if with_res else None
            with torch.no_grad():
                out = NN.batch_norm_act(yd, stats.to(dev), gamma.to(dev), beta.to(dev), rm, rv, residual=rd, relu=relu)
            torch.cuda.synchronize()
            outs[fused] = (out.float().cpu().view(M, C), rm.cpu(), rv.cpu())
        finally:
            NN.FUSE_BN_FINALIZE = old
    (o1, rm1, rv1), (o0, rm0, rv0) = outs[True], outs[False]
    assert torch.allclose(rm1, rm0, rtol=1e-6, atol=1e-7) and torch.allclose(rv1, rv0, rtol=1e-6, atol=1e-7)
    ulp = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10
    bad = ((o1 - o0).abs() > ulp * torch.maximum(o1.abs(), o0.abs()) + 1e-6).sum().item()
    assert bad == 0, f"{bad} of {o1.numel()} outputs differ by more than one ulp"
    assert (o1 != o0).float().mean().item() < 1e-3          # and almost all are bit-identical
    ref = torch.nn.functional.batch_norm(yf, None, None, gamma, beta, True, 0.1, 1e-5)
    if with_res:
        ref = ref + res.float()
    if relu:
        ref = torch.relu(ref)
    assert ((o1 - ref).norm() / ref.norm()).item() < (6e-3 if dtype == torch.bfloat16 else 1e-3)


@pytest.mark.parametrize("C,M,with_res,relu,n_grads", [(256, 5760, False, True, 1), (512, 1440, True, True, 2), (1024, 1445, True, False, 3), (64, 3000, False, True, 1),
                                                         (256, 23040, True, True, 2), (64, 92163, False, True, 1), (2048, 1441, True, True, 1)])      # the last three: 1024-thread reduce
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_bn_bwd_finalize_apply_fused_equals_separate(NN, C, M, with_res, relu, n_grads, dt):
    """sde_bn_bwd with its finalize + apply passes in one launch (short partial slabs; big layers: 1024-thread reduce workgroups keep the slab
    short) against the three-launch form (sde_bn_set_fuse(0)):
    dy equal up to one bf16 ulp on a handful of elements, parameter gradients to 1e-6 (fp64 column sums in a different order)."""
    from simpledepthestimation_amd.hip import lib as L
    g = torch.Generator().manual_seed(C + M)
    y = (torch.randn(M, C, generator=g) * 1.3 + 0.1).to(dt)
    res = torch.randn(M, C, generator=g).to(dt) if with_res else None
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    yf = y.float()
    stats = torch.zeros(1 + NN.REDUCE_ROWS, C, 2)
    stats[0, :, 0], stats[0, :, 1] = yf.sum(0), (yf * yf).sum(0)
    grads = [torch.randn(M, C, generator=g).to(dt) for _ in range(n_grads)]
    outs = {}
    for fuse in (1, 0):
        old = L.lib().sde_bn_set_fuse(fuse)
        try:
            yd = y.to(dev).view(1, 1, M, C).requires_grad_(True)
            rd = res.to(dev).view(1, 1, M, C).requires_grad_(True) if with_res else None
            gd, bd = gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True)
            o = NN.batch_norm_act(yd, stats.to(dev), gd, bd, torch.zeros(C, device=dev), torch.ones(C, device=dev), residual=rd, relu=relu, n_out=n_grads)
            o = o if isinstance(o, tuple) else (o,)
            torch.autograd.backward(list(o), [gr.to(dev).view(1, 1, M, C) for gr in grads])
            torch.cuda.synchronize()
            outs[fuse] = (yd.grad.float().cpu().view(M, C), gd.grad.cpu(), bd.grad.cpu(), rd.grad.float().cpu().view(M, C) if with_res else None)
        finally:
            L.lib().sde_bn_set_fuse(old)
    (dy1, dg1, db1, dr1), (dy0, dg0, db0, dr0) = outs[1], outs[0]
    # short slabs: the same fp32 partials, summed in fp64 in another order; 1024-thread reduce: the partials themselves are folded in another fp32 order
    wide = M * C // 8192 > 256
    tol = 2e-5 if wide else 1e-6
    assert torch.allclose(dg1, dg0, rtol=tol, atol=tol * float(dg0.abs().max())) and torch.allclose(db1, db0, rtol=tol, atol=tol * float(db0.abs().max()))
    bad = ((dy1 - dy0).abs() > 2.0 ** -7 * torch.maximum(dy1.abs(), dy0.abs()) + 1e-6).sum().item()
    assert bad == 0, f"{bad} of {dy1.numel()} elements of dy differ by more than one bf16 ulp (fp16: the same bound, eight of its ulps)"
    assert (dy1 != dy0).float().mean().item() < (2e-2 if wide else 1e-3)
    if with_res:
        assert torch.equal(dr1, dr0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "fp16"])
@pytest.mark.parametrize("act,has_bias", [(1, True), (0, False), (0, True)])
def test_conv_output_with_two_consumers(NN, dtype, act, has_bias):
    """conv2d(..., n_out=2): two aliases of the (ELU) output -- a decoder level feeds its disparity head and the next level; backward gets the
    two gradients separately and sums them inside the activation-backward kernel (sde_act_bwd_bias_sum)."""
    g = torch.Generator().manual_seed(11 + act)
    V = 4 if dtype == torch.float32 else 8
    B, H, W, Cin, Cout = 2, 12, 20, 32, 64
    x = torch.randn(B, Cin, H, W, generator=g); w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    b = torch.randn(Cout, generator=g) * 0.1 if has_bias else None
    if dtype != torch.float32:
        x = x.to(dtype).float(); w = w.to(dtype).float()
    g0, g1 = torch.randn(B, Cout, H, W, generator=g), torch.randn(B, Cout, H, W, generator=g)
    if dtype != torch.float32:
        g0, g1 = g0.to(dtype).float(), g1.to(dtype).float()
    xr = x.clone().requires_grad_(True); wr = w.clone().requires_grad_(True); br = b.clone().requires_grad_(True) if has_bias else None
    yr = F.conv2d(F.pad(xr, (1, 1, 1, 1), mode="reflect"), wr, br)
    if act == 1:
        yr = F.elu(yr)
    yr.backward(g0 + g1)
    cb = CB.ConvCase(x, w, b, dtype, stride=1, pad=1, reflect=True, act=act)
    lim = cb.backward([g0, g1])          # the two gradients are summed (and the sum stored in the activation dtype) by the activation-backward kernel
    xd = nhwc(x, dtype, V).requires_grad_(True); wd = w.clone().to(dev).requires_grad_(True)
    bd = b.clone().to(dev).requires_grad_(True) if has_bias else None
    ya, yb = NN.conv2d(xd, wd, bd, stride=1, pad=1, reflect=True, act=act, n_out=2)
    assert ya.data_ptr() == yb.data_ptr()
    check(nchw(ya.detach(), Cout), yr.detach(), dtype, "y", bound=cb.y)
    torch.autograd.backward([ya, yb], [nhwc(g0, dtype, V), nhwc(g1, dtype, V)])
    check(wd.grad.cpu(), wr.grad, dtype, "dW", bound=lim["dW"])
    check(nchw(xd.grad, Cin), xr.grad, dtype, "dX", bound=lim["dX"])
    if has_bias:
        check(bd.grad.cpu(), br.grad, dtype, "dbias", bound=lim["dbias"])
    # one consumer only: the other alias's gradient is None
    xd2 = nhwc(x, dtype, V).requires_grad_(True)
    ya, yb = NN.conv2d(xd2, wd, bd, stride=1, pad=1, reflect=True, act=act, n_out=2)
    wd.grad = None
    ya.backward(nhwc(g0 + g1, dtype, V))
    check(nchw(xd2.grad, Cin), xr.grad, dtype, "dX one consumer")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "fp16"])
def test_maxpool_two_consumers(NN, dtype):
    g = torch.Generator().manual_seed(3)
    V = 4 if dtype == torch.float32 else 8
    B, C, H, W = 2, 64, 16, 24
    x = torch.randn(B, C, H, W, generator=g)
    if dtype != torch.float32:
        x = x.to(dtype).float()
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 3, 2, 1)
    g0, g1 = torch.randn(yr.shape, generator=g), torch.randn(yr.shape, generator=g)
    if dtype != torch.float32:
        g0, g1 = g0.to(dtype).float(), g1.to(dtype).float()
    yr.backward(g0 + g1)
    xd = nhwc(x, dtype, V).requires_grad_(True)
    ya, yb = NN.max_pool_3x3_s2(xd, n_out=2)
    assert torch.equal(nchw(ya, C), yr.detach()) and ya.data_ptr() == yb.data_ptr()
    torch.autograd.backward([ya, yb], [nhwc(g0, dtype, V), nhwc(g1, dtype, V)])
    check(nchw(xd.grad, C), xr.grad, dtype, "maxpool dx (two consumers)", 1e-6, 2e-2)


@pytest.mark.parametrize("reserve", [32, 64])
def test_persistent_kernels_with_a_cu_reserve(NN, reserve):
    """SDE_OPT_CU_RESERVE: the persistent GEMM / halo kernels sized for fewer compute units (what a data-parallel run leaves to RCCL) -- conv + BatchNorm
    statistics + both gradients at a shape with more tiles than workgroups, against the same calls without a reserve."""
    g = torch.Generator().manual_seed(reserve)
    B, H, W, Cin, C = 12, 48, 160, 64, 64
    x = (torch.randn(B, H, W, Cin, generator=g) * 0.5).bfloat16().to(dev)
    w = (torch.randn(C, Cin, 1, 1, generator=g) / 8).to(dev)
    w3 = (torch.randn(16, 16, 3, 3, generator=g) / 12).to(dev)
    x16 = (torch.randn(4, 96, 320, 16, generator=g) * 0.5).bfloat16().to(dev)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(dev), (torch.randn(C, generator=g) * 0.1).to(dev)

    def run():
        xd, wd, gd, bd = x.clone().requires_grad_(True), w.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        y, stats = NN.conv2d(xd, wd, None, stride=1, pad=0, bn_stats=True)                       # pgemm 1x1: 1440 tiles
        out = NN.batch_norm_act(y, stats, gd, bd, torch.zeros(C, device=dev), torch.ones(C, device=dev), relu=True)
        xs, ws = x16.clone().requires_grad_(True), w3.clone().requires_grad_(True)
        ys = NN.conv2d(xs, ws, None, stride=1, pad=1, reflect=True)                              # chalo / whalo: the small-channel halo kernels
        (out.float().square().mean() + ys.float().square().mean()).backward()
        torch.cuda.synchronize()
        return [t.detach().float().cpu() for t in (out, ys, xd.grad, wd.grad, gd.grad, bd.grad, xs.grad, ws.grad)]
    ref = run()
    old = NN.set_option(NN.OPT_CU_RESERVE, reserve)
    try:
        got = run()
    finally:
        NN.set_option(NN.OPT_CU_RESERVE, old)
    for name, a, b in zip(("out", "y_small", "dx", "dw", "dgamma", "dbeta", "dx_small", "dw_small"), got, ref):
        tol = 2e-2 * float(b.abs().max()) + 1e-6           # bf16 storage; the order of the fp32 partial sums follows the grid
        assert float((a - b).abs().max()) <= tol, (name, float((a - b).abs().max()), tol)
    with pytest.raises(Exception):
        NN.set_option(NN.OPT_CU_RESERVE, 12)


@pytest.mark.parametrize("case", [("k64_single_stage", 2, 24, 40, 256, 64, 1), ("k128", 2, 12, 20, 512, 128, 1), ("3x3", 4, 24, 40, 128, 128, 3), ("3x3_halo64", 4, 48, 80, 64, 64, 3),
                                  ("many_tiles", 12, 48, 160, 256, 64, 1), ("ragged_rows", 1, 7, 9, 256, 64, 1)], ids=lambda c: c[0])
def test_residual_batchnorm_backward_in_the_data_gradient(NN, case):
    """Residual form of the fused BatchNorm backward (sde_conv_dgrad_bnbwd_res): block input u = relu(bn_a(y_a) + r) feeds the next block's first convolution
    and its skip path; that convolution's data gradient forms gm = (g + skip gradient) * relu'(u) and bn_a's partial sums.  Against the separate reduce pass."""
    name, B, H, W, C, C2, k = case
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(B * 100 + C + k)
    x = (torch.randn(B, 64, H, W, generator=g) + 0.2).to(dt).float()
    r = (torch.randn(B, C, H, W, generator=g) * 0.5).to(dt).float()
    wa = (torch.randn(C, 64, 1, 1, generator=g) / 8).to(dt).float()
    w1 = (torch.randn(C2, C, k, k, generator=g) / math.sqrt(C * k * k)).to(dt).float()
    w3 = (torch.randn(C, C2, 1, 1, generator=g) / math.sqrt(C2)).to(dt).float()
    ga, ba, gb, bb = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    go = torch.randn(B, C, H, W, generator=g).to(dt).float()
    res = []
    for fused in (False, True):
        kept, NN.RESBN_FUSED = NN.RESBN_FUSED, fused
        try:
            xd, rd = nhwc(x, dt, 8).requires_grad_(True), nhwc(r, dt, 8).requires_grad_(True)
            wad, w1d, w3d, gad, bad, gbd, bbd = (t.clone().to(dev).requires_grad_(True) for t in (wa, w1, w3, ga, ba, gb, bb))
            hits = NN.RESBN_HITS
            ya, sa = NN.conv2d(xd, wad, None, stride=1, pad=0, bn_stats=True)
            ua, ub = NN.batch_norm_act(ya, sa, gad, bad, torch.zeros(C, device=dev), torch.ones(C, device=dev), residual=rd, relu=True, n_out=2)
            h = NN.conv2d(ua, w1d, None, stride=1, pad=k // 2)
            y3, s3 = NN.conv2d(h, w3d, None, stride=1, pad=0, bn_stats=True)
            out = NN.batch_norm_act(y3, s3, gbd, bbd, torch.zeros(C, device=dev), torch.ones(C, device=dev), residual=ub, relu=True)
            out.backward(nhwc(go, dt, 8))
            torch.cuda.synchronize()
            took = NN.RESBN_HITS - hits          # (3x3: only where the dispatcher runs this layer on the persistent GEMM; the results must agree either way)
            assert took == (1 if fused else 0) or (name.startswith("3x3") and took == 0), f"{name}: residual form {'not ' if fused else ''}taken"
            res.append([t.detach().float().cpu() for t in (out, xd.grad, rd.grad, wad.grad, w1d.grad, w3d.grad, gad.grad, bad.grad, gbd.grad, bbd.grad)])
        finally:
            NN.RESBN_FUSED = kept
    for nm, u, f in zip(("out", "dX", "dR", "dWa", "dW1", "dW3", "dgamma_a", "dbeta_a", "dgamma_b", "dbeta_b"), res[0], res[1]):
        assert torch.isfinite(f).all(), f"{name} {nm}: not finite"
        assert relerr(f, u) < (1e-6 if nm in ("out", "dW3", "dgamma_b", "dbeta_b", "dW1") else 3e-3), f"{name} {nm}: fused vs separate {relerr(f, u):.3e}"

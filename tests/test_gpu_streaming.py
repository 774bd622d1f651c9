"""GPU: the streaming kernels around the convolutions (csrc/bts.hip, packnet.hip; max-pool, the depth head and prep_input of nn.hip), element by
element against the fp64 references and limits of tests/stream_bounds.py, in fp32, bf16 and fp16.

The data-movement kernels and max-pool are called through the C ABI with their results carved out of a sentinel-filled buffer (stream_bounds.guarded):
afterwards no element of the result may still be the sentinel -- padding channels included -- and the 256 bytes before and after it must be untouched.
The heads and the autograd wrappers go through hip/bts.py and hip/nn.py; where both routes exist they must agree bit for bit.
tests/test_stream_bounds.py shows on the CPU that these same assertions reject single planted faults."""
import ctypes
import types

import pytest
import torch

import stream_bounds as SB

pytestmark = pytest.mark.gpu
dev = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "fp16"]
bydtype = pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
INF = float("inf")
MIN_D, MAX_D = 0.1, 80.0


@pytest.fixture(scope="module")
def K():
    from simpledepthestimation_amd.hip import bts, lib, nn
    return types.SimpleNamespace(L=lib, HN=nn, HB=bts)


def up(t, dtype):
    return t.to(dtype).to(dev).contiguous()


def call(K, name, *args):
    K.L.check(getattr(K.L.lib(), name)(*args, K.L.stream()), name)


def result(guard, name):
    """The guarded result on the CPU, after the guard-band check."""
    buf, out = guard
    torch.cuda.synchronize()
    SB.assert_guards(buf, out, name)
    return out.cpu() if out.dtype == torch.uint8 else out.float().cpu()


def same_bits(a, b, name):
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), \
        f"{name}: the wrapper and the C ABI call differ"


# ---------------------------------------------------------------------------------------------------------------------------------------
# nearest x2 up-sampling
# ---------------------------------------------------------------------------------------------------------------------------------------
@bydtype
@pytest.mark.parametrize("shape", [(2, 3, 5, 8), (1, 1, 1, 8), (2, 7, 4, 40)], ids=lambda s: "x".join(map(str, s)))
def test_upsample2(K, dtype, shape):
    B, H, W, C = shape
    code = K.HN.dtype_code(dtype)
    x = SB.draw(shape, dtype, 2)
    xd = up(x, dtype)
    y = SB.guarded((B, 2 * H, 2 * W, C), dtype, dev)
    call(K, "sde_upsample2_fwd", K.L.ptr(xd), B, H, W, C, code, K.L.ptr(y[1]))
    SB.assert_equal(result(y, "upsample2"), SB.upsample2(x), dtype, "upsample2")
    dout = SB.draw((B, 2 * H, 2 * W, C), dtype, 3)          # the four members of a cell differ
    dd = up(dout, dtype)
    dx = SB.guarded(shape, dtype, dev)
    call(K, "sde_upsample2_bwd", K.L.ptr(dd), B, H, W, C, code, K.L.ptr(dx[1]))
    SB.assert_within(result(dx, "upsample2 dx"), SB.upsample2_bwd(dout, dtype), dtype, "upsample2 dx", l2_tol=INF)
    xg = xd.clone().requires_grad_(True)
    yw = K.HB.upsample2(xg)
    yw.backward(dd)
    same_bits(yw.detach(), y[1], "upsample2")
    same_bits(xg.grad, dx[1], "upsample2 dx")


def test_upsample2_second_grid_stride_trip():
    """1 x 132 x 256 x 256 in bf16: 4 325 376 output groups, above the 16384 x 256 lanes of one trip.  Small integers: the backward's four-term sums
    (4 x, |x| <= 15) are exact in bf16, so both directions are compared for equality with torch indexing of the same tensor."""
    from simpledepthestimation_amd.hip import bts as HB
    B, H, W, C = 1, 132, 256, 256
    assert B * 4 * H * W * (C // 8) > 16384 * 256
    x = torch.randint(-15, 16, (B, H, W, C), device=dev, generator=torch.Generator(dev).manual_seed(5)).to(torch.bfloat16).requires_grad_(True)
    y = HB.upsample2(x)
    iy, ix = torch.arange(2 * H, device=dev) // 2, torch.arange(2 * W, device=dev) // 2
    assert torch.equal(y.detach(), x.detach()[:, iy][:, :, ix])
    y.backward(y.detach())                  # constant per cell
    assert torch.equal(x.grad, x.detach() * 4)


# ---------------------------------------------------------------------------------------------------------------------------------------
# multi-piece concatenation
# ---------------------------------------------------------------------------------------------------------------------------------------
def piece_table(K, tensors, meta):
    arr = (K.HB.CatPiece * K.HB.CAT_MAX)()
    for k, (t, (c, ld, m)) in enumerate(zip(tensors, meta)):
        arr[k].p, arr[k].C, arr[k].ld, arr[k].f32map = t.data_ptr(), c, ld, int(m)
    return arr


@bydtype
@pytest.mark.parametrize("kind", list("abcdef"))
def test_cat(K, dtype, kind):
    pieces = SB.cat_case(kind, dtype)
    code = K.HN.dtype_code(dtype)
    B, H, W = pieces[0][0].shape[:3]
    P = B * H * W
    meta = [(c, (1 if m else t.shape[3]), m) for t, c, m in pieces]
    tens = [t.to(dev).contiguous() if m else up(t, dtype) for t, _, m in pieces]
    ref = SB.cat(pieces, dtype)
    Ct = ref.shape[3]
    out = SB.guarded(ref.shape, dtype, dev)
    arr = piece_table(K, tens, meta)
    call(K, "sde_cat_fwd", ctypes.cast(arr, ctypes.c_void_p), len(pieces), P, Ct, code, K.L.ptr(out[1]))
    SB.assert_equal(result(out, f"cat ({kind})"), ref, dtype, f"cat ({kind})")
    # backward: every piece's gradient into its own guarded buffer; padding channels zero, map gradients exact
    dout = SB.draw(ref.shape, dtype, 7)
    dd = up(dout, dtype)
    grads = [SB.guarded((B, 1, H, W), torch.float32, dev) if m else SB.guarded((B, H, W, ld), dtype, dev) for _, ld, m in meta]
    garr = piece_table(K, [g[1] for g in grads], meta)
    call(K, "sde_cat_bwd", K.L.ptr(dd), P, Ct, code, ctypes.cast(garr, ctypes.c_void_p), len(pieces))
    refs = SB.cat_bwd(dout, meta)
    for k, (g, r) in enumerate(zip(grads, refs)):
        got = result(g, f"cat ({kind}) grad {k}")
        SB.assert_equal(got, r, dtype, f"cat ({kind}) grad {k}")
        c, ld, m = meta[k]
        assert m or ld == c or float(got[..., c:].abs().max()) == 0.0
    # the autograd wrapper
    leaves = [t.clone().requires_grad_(True) for t in tens]
    yw = K.HB.cat([(t, c) for t, (c, _, _) in zip(leaves, meta)])
    yw.backward(dd)
    same_bits(yw.detach(), out[1], f"cat ({kind})")
    for k, (t, g) in enumerate(zip(leaves, grads)):
        same_bits(t.grad, g[1], f"cat ({kind}) grad {k}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# channel statistics, ReLU
# ---------------------------------------------------------------------------------------------------------------------------------------
@bydtype
@pytest.mark.parametrize("M,C", SB.STATS_SHAPES)
def test_channel_stats(K, dtype, M, C):
    """A tile of one row, a partial last tile, C / V below, equal to and not a multiple of the 32 groups of a workgroup, two workgroups in y."""
    x = SB.rounded(SB.draw((M, C), dtype, M) + 0.5, dtype)
    xd = up(x, dtype)
    tiles = K.L.lib().sde_channel_stats_tiles(M)
    assert tiles == -(-M // SB.STATS_ROWS)
    part = SB.guarded((tiles, C, 2), torch.float32, dev)
    call(K, "sde_channel_stats", K.L.ptr(xd), M, C, K.HN.dtype_code(dtype), K.L.ptr(part[1]))
    SB.assert_within(result(part, "channel_stats"), SB.channel_stats(x), dtype, "channel_stats", l2_tol=INF)
    same_bits(K.HB.channel_stats(xd)[:tiles].contiguous(), part[1], "channel_stats")       # (the rows behind belong to the next stage)


@bydtype
@pytest.mark.parametrize("MC", [(1, 0), (15, 24)], ids=["one_group", "3x5x24"])
def test_relu(K, dtype, MC):
    """+0, -0, the smallest subnormal of either sign; backward through sde_act_bwd_bias: dz is dy or 0."""
    V = SB.VEC[dtype]
    M, C = MC[0], MC[1] or V
    n = M * C
    code = K.HN.dtype_code(dtype)
    sub = 2.0 * SB.TINY[dtype]
    x = SB.draw((M, C), dtype, n)
    x.view(-1)[:4] = torch.tensor([0.0, -0.0, sub, -sub])
    assert torch.equal(SB.rounded(x, dtype), x)
    xd = up(x, dtype)
    y = SB.guarded((M, C), dtype, dev)
    call(K, "sde_relu_fwd", K.L.ptr(xd), n, code, K.L.ptr(y[1]))
    yr = SB.relu(x)
    SB.assert_equal(result(y, "relu"), yr, dtype, "relu")
    dy = SB.draw((M, C), dtype, n + 1)
    dyd = up(dy, dtype)
    dz = SB.guarded((M, C), dtype, dev)
    call(K, "sde_act_bwd_bias", K.L.ptr(dyd), K.L.ptr(y[1]), K.HN.ACT_RELU, M, C, code, K.L.ptr(dz[1]), None, None, 0, 0)
    SB.assert_equal(result(dz, "relu dz"), SB.relu_bwd(dy, yr), dtype, "relu dz")
    xg = xd.clone().requires_grad_(True)
    yw = K.HB.relu(xg)
    yw.backward(dyd)
    same_bits(yw.detach(), y[1], "relu")
    same_bits(xg.grad, dz[1], "relu dz")


# ---------------------------------------------------------------------------------------------------------------------------------------
# space-to-batch of the dilated convolutions
# ---------------------------------------------------------------------------------------------------------------------------------------
@bydtype
@pytest.mark.parametrize("C", [8, 40])
@pytest.mark.parametrize("d", [1, 2, 3, 8])
def test_dilate_split_merge(K, dtype, d, C):
    """d = 8 exceeds H and W: most phase images are zero fill only."""
    B, H, W = 2, 5, 7
    code = K.HN.dtype_code(dtype)
    x = SB.draw((B, H, W, C), dtype, d + C)
    xd = up(x, dtype)
    ref = SB.dilate_split(x, d)
    sub = SB.guarded(ref.shape, dtype, dev)
    call(K, "sde_dilate_split", K.L.ptr(xd), B, H, W, C, d, code, K.L.ptr(sub[1]))
    SB.assert_equal(result(sub, "split"), ref, dtype, "split")
    back = SB.guarded((B, H, W, C), dtype, dev)
    call(K, "sde_dilate_merge", K.L.ptr(sub[1]), B, H, W, C, d, code, K.L.ptr(back[1]))
    SB.assert_equal(result(back, "merge(split)"), x, dtype, "merge(split)")
    s2 = SB.draw(ref.shape, dtype, 9)               # data also where split writes zeros: merge must not read it
    m2 = SB.guarded((B, H, W, C), dtype, dev)
    s2d = up(s2, dtype)
    call(K, "sde_dilate_merge", K.L.ptr(s2d), B, H, W, C, d, code, K.L.ptr(m2[1]))
    SB.assert_equal(result(m2, "merge"), SB.dilate_merge(s2, B, H, W, d), dtype, "merge")


# ---------------------------------------------------------------------------------------------------------------------------------------
# max-pool
# ---------------------------------------------------------------------------------------------------------------------------------------
@bydtype
@pytest.mark.parametrize("shape", SB.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool(K, dtype, shape):
    """Inputs of five values: most windows tie.  The saved byte is the first maximum in row-major window order, as ATen's index."""
    B, H, W, C = shape
    code = K.HN.dtype_code(dtype)
    x = SB.pool_input(shape, dtype)
    xd = up(x, dtype)
    yr, ir = SB.maxpool(x)
    y, idx = SB.guarded(yr.shape, dtype, dev), SB.guarded(ir.shape, torch.uint8, dev)
    call(K, "sde_maxpool_fwd", K.L.ptr(xd), B, H, W, C, code, K.L.ptr(y[1]), K.L.ptr(idx[1]))
    SB.assert_equal(result(y, "maxpool y"), yr, dtype, "maxpool y")
    SB.assert_equal(result(idx, "maxpool arg-max"), ir, dtype, "maxpool arg-max")
    g0, g1 = SB.draw(yr.shape, dtype, 12), SB.draw(yr.shape, dtype, 13)
    g0d, g1d = up(g0, dtype), up(g1, dtype)
    dxs = []
    for second, sd in ((g1, g1d), (None, None)):
        dx = SB.guarded(shape, dtype, dev)
        call(K, "sde_maxpool_bwd_sum", K.L.ptr(g0d), K.L.ptr(sd), K.L.ptr(idx[1]), B, H, W, C, code, K.L.ptr(dx[1]))
        name = "maxpool dx" + (" (two consumers)" if second is not None else "")
        SB.assert_within(result(dx, name), SB.maxpool_bwd(g0, second, ir, H, W, dtype), dtype, name, l2_tol=INF)
        dxs.append(dx[1])
    one = SB.guarded(shape, dtype, dev)         # the one-consumer entry point
    call(K, "sde_maxpool_bwd", K.L.ptr(g0d), K.L.ptr(idx[1]), B, H, W, C, code, K.L.ptr(one[1]))
    result(one, "maxpool dx")
    same_bits(one[1], dxs[1], "maxpool dx")
    xg = xd.clone().requires_grad_(True)
    ya, yb = K.HN.max_pool_3x3_s2(xg, n_out=2)
    torch.autograd.backward([ya, yb], [g0d, g1d])
    same_bits(ya.detach(), y[1], "maxpool y")
    same_bits(xg.grad, dxs[0], "maxpool dx (two consumers)")
    xg = xd.clone().requires_grad_(True)
    K.HN.max_pool_3x3_s2(xg).backward(g0d)
    same_bits(xg.grad, dxs[1], "maxpool dx")


# ---------------------------------------------------------------------------------------------------------------------------------------
# PackNet's data movement
# ---------------------------------------------------------------------------------------------------------------------------------------
@bydtype
@pytest.mark.parametrize("add,with_inv,with_p1", SB.CONCAT_MODES)
@pytest.mark.parametrize("hw", [(2, 8, 12), (1, 2, 2)], ids=["2x8x12", "1x2x2"])
def test_packnet_concat(K, dtype, hw, add, with_inv, with_p1):
    B, H, W = hw
    C0 = 8
    code = K.HN.dtype_code(dtype)
    for C1 in ([C0] if add else [8, 24] if with_p1 else [0]):
        p0 = SB.draw((B, H, W, C0), dtype, 1)
        p1 = SB.draw((B, H, W, C1), dtype, 2) if with_p1 else None
        inv = torch.rand(B, H // 2, W // 2, generator=torch.Generator().manual_seed(3)) if with_inv else None
        p0d, p1d, invd = up(p0, dtype), (up(p1, dtype) if with_p1 else None), (inv.to(dev) if with_inv else None)
        b = SB.concat(p0, p1, inv, add, dtype)
        Ct = b.ref.shape[3]
        out = SB.guarded(b.ref.shape, dtype, dev)
        call(K, "sde_concat_fwd", K.L.ptr(p0d), K.L.ptr(p1d), K.L.ptr(invd), int(add), B, H, W, C0, C1, Ct, code, K.L.ptr(out[1]))
        got = result(out, "concat")
        if add:
            SB.assert_within(got, b, dtype, "concat (add)", l2_tol=INF)
        else:
            SB.assert_equal(got, b.ref.float(), dtype, "concat")
        dout = SB.draw(b.ref.shape, dtype, 4)
        dd = up(dout, dtype)
        r0, r1, rinv = SB.concat_bwd(dout, C0, C1, add, with_inv, dtype)
        d0 = SB.guarded((B, H, W, C0), dtype, dev)
        d1 = SB.guarded((B, H, W, C1), dtype, dev) if r1 is not None else None
        dinv = SB.guarded((B, H // 2, W // 2), torch.float32, dev) if with_inv else None
        call(K, "sde_concat_bwd", K.L.ptr(dd), int(add), B, H, W, C0, C1, Ct, code, K.L.ptr(d0[1]), K.L.ptr(d1[1] if d1 else None), K.L.ptr(dinv[1] if dinv else None))
        SB.assert_equal(result(d0, "concat d0"), r0, dtype, "concat d0")
        if d1 is not None:
            SB.assert_equal(result(d1, "concat d1"), r1, dtype, "concat d1")
        if with_inv:
            SB.assert_within(result(dinv, "concat d inv"), rinv, dtype, "concat d inv", l2_tol=INF)
        # the autograd wrapper
        l0, l1 = p0d.clone().requires_grad_(True), (p1d.clone().requires_grad_(True) if with_p1 else None)
        li = invd.clone().requires_grad_(True) if with_inv else None
        yw = K.HN.concat(l0, l1, li, add=add)
        yw.backward(dd)
        same_bits(yw.detach(), out[1], "concat")
        same_bits(l0.grad, d0[1], "concat d0")
        if with_p1:
            same_bits(l1.grad, d0[1] if add else d1[1], "concat d1")
        if with_inv:
            same_bits(li.grad, dinv[1], "concat d inv")


@pytest.mark.parametrize("HW", [(128, 256), (512, 512)], ids=["128x256", "512x512"])
def test_packnet_concat_large(HW):
    """bf16, concat mode with the inverse-depth group, C0 = C1 = 32: 72 output channels = 9 groups per pixel.  128 x 256 is 2 359 296 output ELEMENTS
    (294 912 groups: one trip); 512 x 512 is 2 359 296 GROUPS, above the 8192 x 256 lanes of one trip.  Small integers: the inverse depth's
    four-term sums are exact; everything is compared for equality with torch indexing of the same tensors."""
    from simpledepthestimation_amd.hip import nn as HN
    H, W = HW
    C0 = C1 = 32
    g = torch.Generator(dev).manual_seed(6)
    p0 = torch.randint(-15, 16, (1, H, W, C0), device=dev, generator=g).to(torch.bfloat16).requires_grad_(True)
    p1 = torch.randint(-15, 16, (1, H, W, C1), device=dev, generator=g).to(torch.bfloat16).requires_grad_(True)
    inv = torch.randint(0, 16, (1, H // 2, W // 2), device=dev, generator=g).float().requires_grad_(True)
    out = HN.concat(p0, p1, inv)
    assert out.shape == (1, H, W, 72) and (H * W * 9 > 8192 * 256) == (H == 512)
    iy, ix = torch.arange(H, device=dev) // 2, torch.arange(W, device=dev) // 2
    ref = torch.cat([p0.detach(), p1.detach(), inv.detach()[:, iy][:, :, ix].unsqueeze(3).to(torch.bfloat16), torch.zeros(1, H, W, 7, device=dev, dtype=torch.bfloat16)], 3)
    assert torch.equal(out.detach(), ref)
    out.backward(ref)                   # the gradient of the inverse-depth channel is constant per 2 x 2 cell
    assert torch.equal(p0.grad, p0.detach()) and torch.equal(p1.grad, p1.detach())
    assert torch.equal(inv.grad, inv.detach() * 4)


@bydtype
@pytest.mark.parametrize("shape", [(2, 6, 10, 16), (1, 2, 2, 8)], ids=["2x6x10x16", "1x2x2x8"])
def test_space_to_depth_and_depth_to_space(K, dtype, shape):
    B, H, W, C = shape
    code = K.HN.dtype_code(dtype)
    x = SB.draw(shape, dtype, 5)
    xd = up(x, dtype)
    y = SB.guarded((B, H // 2, W // 2, 4 * C), dtype, dev)
    call(K, "sde_space_to_depth", K.L.ptr(xd), B, H, W, C, code, K.L.ptr(y[1]))
    SB.assert_equal(result(y, "space_to_depth"), SB.space_to_depth(x), dtype, "space_to_depth")
    z = SB.guarded(shape, dtype, dev)
    call(K, "sde_depth_to_space", K.L.ptr(y[1]), B, H // 2, W // 2, 4 * C, code, K.L.ptr(z[1]))
    SB.assert_equal(result(z, "depth_to_space"), x, dtype, "depth_to_space")


# ---------------------------------------------------------------------------------------------------------------------------------------
# input preparation
# ---------------------------------------------------------------------------------------------------------------------------------------
@bydtype
@pytest.mark.parametrize("C", [1, 3, 9])
@pytest.mark.parametrize("flip", [False, True], ids=["", "flip"])
@pytest.mark.parametrize("norm", [False, True], ids=["raw", "meanstd"])
def test_prep_input(K, dtype, C, flip, norm):
    g = torch.Generator().manual_seed(C)
    code = K.HN.dtype_code(dtype)
    for (B, H, W) in [(2, 5, 7), (2, 3, 1)]:
        img = torch.rand(B, C, H, W, generator=g)
        mean, std = (torch.rand(C, generator=g), torch.rand(C, generator=g) * 0.2 + 0.2) if norm else (None, None)
        b = SB.prep_input(img, mean, std, dtype, flip)
        out = SB.guarded(b.ref.shape, dtype, dev)
        imgd, md, sd = img.to(dev), (mean.to(dev) if norm else None), (std.to(dev) if norm else None)
        call(K, "sde_prep_input", K.L.ptr(imgd), K.L.ptr(md), K.L.ptr(sd), B, C, H, W, b.ref.shape[3], int(flip), code, K.L.ptr(out[1]))
        got = result(out, "prep_input")
        if norm:
            SB.assert_within(got, b, dtype, "prep_input", l2_tol=INF)
        else:
            SB.assert_equal(got, b.ref.float(), dtype, "prep_input (raw)")
        assert float(got[..., C:].abs().max() if got.shape[3] > C else 0) == 0.0
        same_bits(K.HN.prep_input(imgd, md, sd, dtype, flip), out[1], "prep_input")


# ---------------------------------------------------------------------------------------------------------------------------------------
# heads
# ---------------------------------------------------------------------------------------------------------------------------------------
HEAD_CASES = [((2, 5, 7), False, 1), ((2, 5, 7), True, 1), ((2, 5, 7), False, 2), ((2, 5, 7), True, 2), ((2, 3, 1), True, 1), ((2, 3, 1), False, 1)]
head_cases = pytest.mark.parametrize("shape,flip,groups", HEAD_CASES, ids=[f"{'x'.join(map(str, s))}{'_flip' if f else ''}_ld{g}V" for s, f, g in HEAD_CASES])


def head_operands(dtype, shape, groups):
    """(stored logits v [B,H,W], the NHWC tensor holding them in channel 0 and other data elsewhere, the incoming gradients of a [B,1,H,W] and a [B,H,W]
    output, and those two on the device: a pointer handed to the C ABI needs its tensor alive)"""
    B, H, W = shape
    v = SB.head_logits(dtype, shape, 31)
    y = SB.draw((B, H, W, groups * SB.VEC[dtype]), dtype, 33)
    y[..., 0] = v
    g = torch.Generator().manual_seed(32)
    dd, di = torch.randn(B, 1, H, W, generator=g), torch.randn(B, H, W, generator=g)
    return v, up(y, dtype), dd, di, dd.to(dev), di.to(dev)


def check_logit_grad(grad, bound, dtype, name):
    """Channel 0 inside its limit; every other channel of every group zero."""
    SB.assert_within(grad[..., 0].float().cpu(), bound, dtype, name, l2_tol=INF)
    assert float(grad[..., 1:].float().abs().max()) == 0.0, f"{name}: the padding channels of the logit gradient are not zero"


@bydtype
@head_cases
def test_depth_head(K, dtype, shape, flip, groups):
    B, H, W = shape
    v, yd, dd, _, ddd, _ = head_operands(dtype, shape, groups)
    yd.requires_grad_(True)
    d = K.HN.depth_head(yd, MIN_D, MAX_D, flip)
    assert d.dtype == torch.float32 and tuple(d.shape) == (B, 1, H, W)
    SB.assert_within(d.detach().cpu(), SB.depth_head(v, MIN_D, MAX_D, flip), dtype, "depth_head", l2_tol=INF)
    d.backward(ddd)
    check_logit_grad(yd.grad, SB.depth_head_bwd(v, dd, MIN_D, MAX_D, flip, dtype), dtype, "depth_head d logit")
    # the same backward into a buffer that holds stale non-zero data
    dy = SB.guarded(tuple(yd.shape), dtype, dev)
    call(K, "sde_depth_head_bwd", K.L.ptr(yd.detach()), K.L.ptr(ddd), B, H, W, yd.shape[3], MIN_D, MAX_D, int(flip), K.HN.dtype_code(dtype), K.L.ptr(dy[1]))
    result(dy, "depth_head d logit")
    same_bits(yd.grad, dy[1], "depth_head d logit")


@bydtype
def test_depth_head_fused_bias_gradient(K, dtype):
    """A one-output-channel HipConv2d in front: depth_head's backward also sums its stored logit gradients into the bias gradient (HEAD_BIAS_HITS).
    The terms are the gradients the kernel stored, so the limit is that of one fp32 sum of B H W terms."""
    from simpledepthestimation_amd.layers.hip_modules import HipConv2d
    HN = K.HN
    g = torch.Generator().manual_seed(34)
    B, H, W, Cin = 2, 5, 7, 16
    x = up(SB.draw((B, H, W, Cin), dtype, 35), dtype)
    conv = HipConv2d(Cin, 1, 3, 1, 1, bias=True, reflect=True).to(dev)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(1, Cin, 3, 3, generator=g) * 0.3)
        conv.bias.fill_(0.25)
    w, b = conv.weight, conv.bias
    w.grad, b.grad = torch.zeros_like(w), torch.zeros_like(b)          # pre-allocated slots, as under HipTrainer
    dd = torch.randn(B, 1, H, W, generator=g)
    hits = HN.HEAD_BIAS_HITS
    y = conv(x)
    d = HN.depth_head(y, MIN_D, MAX_D)
    d.backward(dd.to(dev))
    torch.cuda.synchronize()
    assert HN.HEAD_BIAS_HITS == hits + 1
    v = y.detach()[..., 0].float().cpu()            # the logits as the convolution stored them
    SB.assert_within(d.detach().cpu(), SB.depth_head(v, MIN_D, MAX_D, False), dtype, "depth_head behind a convolution", l2_tol=INF)
    leaf = y.detach().clone().requires_grad_(True)   # the same kernel without the bias sum: the gradients it stores
    HN.depth_head(leaf, MIN_D, MAX_D).backward(dd.to(dev))
    check_logit_grad(leaf.grad, SB.depth_head_bwd(v, dd, MIN_D, MAX_D, False, dtype), dtype, "depth_head d logit behind a convolution")
    terms = leaf.grad[..., 0].float().cpu().reshape(-1, 1)
    assert terms.shape[0] == B * H * W
    SB.assert_within(b.grad.cpu(), SB.sum_bound(terms, torch.float32), dtype, "depth_head d bias", l2_tol=INF)


@bydtype
@head_cases
def test_inv_depth_head(K, dtype, shape, flip, groups):
    B, H, W = shape
    v, yd, dd, di, ddd, did = head_operands(dtype, shape, groups)
    bi, bd = SB.inv_depth_head(v, 0.5, MIN_D, MAX_D, flip)
    for use_inv, use_dep in ((True, True), (False, True), (True, False)):
        leaf = yd.clone().requires_grad_(True)
        inv, dep = K.HN.inv_depth_head(leaf, 0.5, MIN_D, MAX_D, flip)
        assert tuple(inv.shape) == (B, H, W) and tuple(dep.shape) == (B, 1, H, W) and inv.dtype == dep.dtype == torch.float32
        SB.assert_within(inv.detach().cpu(), bi, dtype, "inv_depth_head inv", l2_tol=INF)
        SB.assert_within(dep.detach().cpu(), bd, dtype, "inv_depth_head depth", l2_tol=INF)
        torch.autograd.backward([t for t, u in ((inv, use_inv), (dep, use_dep)) if u], [t for t, u in ((did, use_inv), (ddd, use_dep)) if u])
        bound = SB.inv_depth_head_bwd(v, di if use_inv else None, dd if use_dep else None, 0.5, MIN_D, MAX_D, flip, dtype)
        check_logit_grad(leaf.grad, bound, dtype, "inv_depth_head d logit" + ("" if use_inv and use_dep else " (one output)"))
        if use_inv and use_dep:
            dy = SB.guarded(tuple(yd.shape), dtype, dev)
            call(K, "sde_inv_depth_head_bwd", K.L.ptr(yd), K.L.ptr(did), K.L.ptr(ddd), B, H, W, yd.shape[3], 0.5, MIN_D, MAX_D, int(flip),
                 K.HN.dtype_code(dtype), K.L.ptr(dy[1]))
            result(dy, "inv_depth_head d logit")
            same_bits(leaf.grad, dy[1], "inv_depth_head d logit")


@bydtype
@head_cases
def test_sigmoid_head(K, dtype, shape, flip, groups):
    B, H, W = shape
    v, yd, dd, _, ddd, _ = head_operands(dtype, shape, groups)
    focal = torch.tensor([700.0, 720.5])
    for scale, fo, div in ((80.0, focal, 715.0873), (1.0, None, 1.0)):
        leaf = yd.clone().requires_grad_(True)
        fd = fo.to(dev) if fo is not None else None
        out = K.HB.sigmoid_head(leaf, scale, fd, div, flip)
        assert tuple(out.shape) == (B, 1, H, W) and out.dtype == torch.float32
        name = "sigmoid_head" + (" (focal)" if fo is not None else "")
        SB.assert_within(out.detach().cpu(), SB.sigmoid_head(v, scale, fo, div, flip), dtype, name, l2_tol=INF)
        out.backward(ddd)
        check_logit_grad(leaf.grad, SB.sigmoid_head_bwd(v, dd, scale, fo, div, flip, dtype), dtype, name + " d logit")
        dy = SB.guarded(tuple(yd.shape), dtype, dev)
        call(K, "sde_sigmoid_head_bwd", K.L.ptr(yd), K.L.ptr(ddd), B, H, W, yd.shape[3], scale, K.L.ptr(fd), div, int(flip), K.HN.dtype_code(dtype), K.L.ptr(dy[1]))
        result(dy, name + " d logit")
        same_bits(leaf.grad, dy[1], name + " d logit")

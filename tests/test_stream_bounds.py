"""CPU self-test of tests/stream_bounds.py: every streaming kernel restated in fp32 in its own operation order stays inside the helper's assertion,
and single planted faults -- the ones a whole-tensor relative L2 lets through -- are rejected by the same assertion functions the GPU tests call.

The emulations follow the kernels' index arithmetic (flat index -> source, as csrc/bts.hip, packnet.hip and nn.hip compute it), not the helper's
torch expressions, so the two are independent statements of each operator."""
import functools

import pytest
import torch
import torch.nn.functional as F

import stream_bounds as SB

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "fp16"]
bydtype = pytest.mark.parametrize("dtype", DTYPES, ids=IDS)


def st(t, dtype):
    """(T)v: the value after the store in the activation type"""
    return t.to(dtype).float()


draw = SB.draw


def rejects(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


def push_past_limit(got, bound, dtype, idx):
    """got with the element at idx moved, in steps of one unit in the last place of the storage type, until it is the first step beyond its limit."""
    got = got.clone().double()
    ulp = float(SB.ulp_of(bound.ref[idx].reshape(1), dtype))
    room = float(bound.lim[idx]) - (float(got[idx]) - float(bound.ref[idx]))
    steps = int(room // ulp) + 1
    got[idx] = got[idx] + steps * ulp
    within = got.clone()
    within[idx] = within[idx] - ulp                     # one step less: still inside
    return got, within


def one_ulp_fault(got, bound, dtype, name, idx):
    SB.assert_within(got, bound, dtype, name, l2_tol=float("inf"))
    bad, edge = push_past_limit(got, bound, dtype, idx)
    SB.assert_within(edge, bound, dtype, name + " (last step inside)", l2_tol=float("inf"))
    rejects(SB.assert_within, bad, bound, dtype, name + " (one ulp beyond)", l2_tol=float("inf"))


# ---------------------------------------------------------------------------------------------------------------------------------------
# emulations
# ---------------------------------------------------------------------------------------------------------------------------------------
def emu_up2_fwd(x):
    B, H, W, C = x.shape
    y, xx = torch.arange(2 * H) >> 1, torch.arange(2 * W) >> 1
    return x[:, y][:, :, xx]


def emu_up2_bwd(dout, dtype):
    acc = torch.zeros_like(dout[:, ::2, ::2])
    for k in range(4):
        acc = acc + dout[:, (k >> 1)::2, (k & 1)::2]
    return st(acc, dtype)


def emu_dilate(t, B, H, W, d, merge):
    """dilate_kernel's flat index arithmetic (one channel group = the whole channel axis here)."""
    C = t.shape[3]
    Hs, Ws = -(-H // d), -(-W // d)
    flat = t.reshape(-1, C)
    if merge:
        pix = torch.arange(B * H * W)
        w, h, b = pix % W, (pix // W) % H, pix // (W * H)
        sb = (b * d + h % d) * d + w % d
        return flat[(sb * Hs + h // d) * Ws + w // d].reshape(B, H, W, C)
    pix = torch.arange(B * d * d * Hs * Ws)
    j, ii, sb = pix % Ws, (pix // Ws) % Hs, pix // (Ws * Hs)
    pw, ph, b = sb % d, (sb // d) % d, sb // (d * d)
    h, w = ii * d + ph, j * d + pw
    ok = (h < H) & (w < W)
    src = ((b * H + h.clamp(max=H - 1)) * W + w.clamp(max=W - 1))
    return torch.where(ok.unsqueeze(1), flat[src], torch.zeros(1, C)).reshape(B * d * d, Hs, Ws, C)


def emu_cat_fwd(pieces, dtype):
    """cat_fwd_kernel, channel by channel: the piece that holds channel c, a map through one conversion, zero past the last piece."""
    B, H, W = pieces[0][0].shape[:3]
    off = [0]
    for _, c, _ in pieces:
        off.append(off[-1] + c)
    Ct = SB.pad_to(off[-1], SB.VEC[dtype])
    out = torch.zeros(B, H, W, Ct)
    for c in range(Ct):
        k = 0
        while k < len(pieces) and off[k + 1] <= c:
            k += 1
        if k < len(pieces):
            t, _, m = pieces[k]
            out[..., c] = st(t[:, 0], dtype) if m else t[..., c - off[k]]
    return out


def emu_cat_bwd(dout, meta):
    B, H, W, _ = dout.shape
    grads, off = [], 0
    for c, ld, m in meta:
        if m:
            grads.append(dout[..., off].clone().reshape(B, 1, H, W))
        else:
            g = torch.empty(B, H, W, ld)
            for e in range(ld):
                g[..., e] = dout[..., off + e] if e < c else 0.0
            grads.append(g)
        off += c
    return grads


def emu_s2d(x):
    B, H, W, C = x.shape
    out = torch.empty(B, H // 2, W // 2, 4 * C)
    for k in range(4):
        for c in range(C):
            out[..., c * 4 + k] = x[:, (k >> 1)::2, (k & 1)::2, c]
    return out


def emu_d2s(x):
    B, H, W, C4 = x.shape
    out = torch.empty(B, 2 * H, 2 * W, C4 // 4)
    for k in range(4):
        for c in range(C4 // 4):
            out[:, (k >> 1)::2, (k & 1)::2, c] = x[..., c * 4 + k]
    return out


def emu_concat_fwd(p0, p1, inv, add, dtype):
    B, H, W, C0 = p0.shape
    V = SB.VEC[dtype]
    C1 = 0 if (add or p1 is None) else p1.shape[3]
    Ct = SB.pad_to(C0 + C1 + (1 if inv is not None else 0), V)
    out = torch.zeros(B, H, W, Ct)
    out[..., :C0] = st(p0 + p1, dtype) if add else p0
    if C1:
        out[..., C0:C0 + C1] = p1
    if inv is not None:
        y, x = torch.arange(H) >> 1, torch.arange(W) >> 1
        out[..., C0 + C1] = st(inv[:, y][:, :, x], dtype)
    return out


def emu_concat_bwd_inv(dout, ch):
    r0, r1 = dout[:, 0::2, :, ch], dout[:, 1::2, :, ch]
    return (r0[:, :, 0::2] + r0[:, :, 1::2]) + (r1[:, :, 0::2] + r1[:, :, 1::2])


def emu_maxpool_fwd(x, later_tie=False):
    """maxpool_fwd_kernel; later_tie: `>=` instead of `>` (the planted fault)."""
    B, H, W, C = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.full((B, 2 * OH + 1, 2 * OW + 1, C), float("-inf"))
    xp[:, 1:1 + H, 1:1 + W] = x
    best = torch.full((B, OH, OW, C), float("-inf"))
    bi = torch.zeros(B, OH, OW, C, dtype=torch.uint8)
    for k in range(9):
        kh, kw = divmod(k, 3)
        v = xp[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2]
        take = (v >= best) & (v > float("-inf")) if later_tie else v > best
        best = torch.where(take, v, best)
        bi = torch.where(take, torch.full_like(bi, k), bi)
    return best, bi


def emu_maxpool_bwd(g0, g1, idx, H, W, dtype, drop=None):
    """maxpool_bwd_kernel: the windows that reach an element in kh, kw order, d = dout + dout1 first.  drop = (ih, iw, kh, kw): skipped."""
    B, OH, OW, C = g0.shape
    d = g0 + g1 if g1 is not None else g0
    dx = torch.zeros(B, 2 * OH + 1, 2 * OW + 1, C)
    for k in range(9):
        kh, kw = divmod(k, 3)
        add = torch.where(idx == k, d, torch.zeros_like(d))
        if drop is not None and (drop[2], drop[3]) == (kh, kw):
            add[:, (drop[0] + 1 - kh) // 2, (drop[1] + 1 - kw) // 2] = 0.0
        dx[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] += add
    return st(dx[:, 1:1 + H, 1:1 + W], dtype)


def emu_prep_input(img, mean, std, dtype, flip):
    B, C, H, W = img.shape
    out = torch.zeros(B, H, W, SB.pad_to(C, SB.VEC[dtype]))
    xs = torch.arange(W - 1, -1, -1) if flip else torch.arange(W)
    for c in range(C):
        v = img[:, c][:, :, xs]
        if mean is not None:
            v = (v - mean[c]) / std[c]
        out[..., c] = st(v, dtype)
    return out


def emu_channel_stats(x):
    """channel_stats_kernel: eight row lanes add every eighth row, one thread adds the eight lane sums."""
    M, C = x.shape
    tiles = -(-M // SB.STATS_ROWS)
    part = torch.zeros(tiles, C, 2)
    for t in range(tiles):
        rows = x[t * SB.STATS_ROWS:(t + 1) * SB.STATS_ROWS]
        a = torch.zeros(C, 2)
        for lane in range(8):
            s = torch.zeros(C, 2)
            for r in range(lane, rows.shape[0], 8):
                s[:, 0] = s[:, 0] + rows[r]
                s[:, 1] = s[:, 1] + rows[r] * rows[r]
            a = a + s
        part[t] = a
    return part


def sigm(v):
    return 1.0 / (1.0 + torch.exp(-v))


def emu_depth_head(v, mn, mx, flip):
    lo, hi = torch.tensor(SB.f32_recip(mx)), torch.tensor(SB.f32_recip(mn))
    sp = torch.where(v > 20.0, v, torch.log1p(torch.exp(v)))
    d = 1.0 / (lo + (hi - lo) * sp)
    return (d.flip(2) if flip else d).unsqueeze(1)


def emu_depth_head_bwd(v, dd, mn, mx, flip, dtype):
    lo, hi = torch.tensor(SB.f32_recip(mx)), torch.tensor(SB.f32_recip(mn))
    sp = torch.where(v > 20.0, v, torch.log1p(torch.exp(v)))
    sd = lo + (hi - lo) * sp
    dsp = torch.where(v > 20.0, torch.ones_like(v), sigm(v))
    g = (dd[:, 0].flip(2) if flip else dd[:, 0]) * (-1.0 / (sd * sd)) * (hi - lo) * dsp
    return st(g, dtype)


def emu_inv_depth_head(v, md, mn, mx, flip):
    lo, hi = torch.tensor(SB.f32_recip(mx)), torch.tensor(SB.f32_recip(mn))
    d = sigm(v) / md
    dep = 1.0 / (lo + (hi - lo) * d)
    return d, (dep.flip(2) if flip else dep).unsqueeze(1)


def emu_inv_depth_head_bwd(v, di, dd, md, mn, mx, flip, dtype):
    lo, hi = torch.tensor(SB.f32_recip(mx)), torch.tensor(SB.f32_recip(mn))
    sg = sigm(v)
    d = sg / md
    g = di.clone() if di is not None else torch.zeros_like(v)
    if dd is not None:
        sd = lo + (hi - lo) * d
        g = g + (dd[:, 0].flip(2) if flip else dd[:, 0]) * (-(hi - lo) / (sd * sd))
    return st(g * (sg * (1.0 - sg) / md), dtype)


def emu_sigmoid_head(v, scale, focal, div, flip):
    o = sigm(v) * scale
    if focal is not None:
        o = (o * focal.view(-1, 1, 1)) / div
    return (o.flip(2) if flip else o).unsqueeze(1)


def emu_sigmoid_head_bwd(v, dout, scale, focal, div, flip, dtype):
    s = sigm(v)
    g = dout[:, 0].flip(2) if flip else dout[:, 0]
    if focal is not None:
        g = (g / div) * focal.view(-1, 1, 1)
    return st(g * scale * s * (1.0 - s), dtype)


# ---------------------------------------------------------------------------------------------------------------------------------------
# data movement: the emulation passes, a planted fault does not
# ---------------------------------------------------------------------------------------------------------------------------------------
@bydtype
def test_guard_bands_see_unwritten_elements_and_stray_writes(dtype):
    buf, out = SB.guarded((2, 3, 5, 8), dtype)
    rejects(SB.assert_guards, buf, out, "nothing written")
    out.copy_(draw((2, 3, 5, 8), dtype, 1).to(dtype))
    SB.assert_guards(buf, out, "written")
    keep = buf.clone()
    end = SB.GUARD + out.numel() * out.element_size()
    buf[end - out.element_size():end] = SB.SENTINEL
    rejects(SB.assert_guards, buf, out, "the last padding channel skipped")
    buf.copy_(keep)
    buf[SB.GUARD - 1] = 0
    rejects(SB.assert_guards, buf, out, "one byte before")
    buf.copy_(keep)
    buf[end] = 0
    rejects(SB.assert_guards, buf, out, "one group past the end")
    buf.copy_(keep)
    SB.assert_guards(buf, out, "restored")


@bydtype
@pytest.mark.parametrize("shape", [(2, 3, 5, 8), (1, 1, 1, 8), (2, 7, 4, 40)])
def test_upsample2(dtype, shape):
    x = draw(shape, dtype, 2)
    y = emu_up2_fwd(x)
    SB.assert_equal(y, SB.upsample2(x), dtype, "upsample2")
    dout = draw(y.shape, dtype, 3)
    b = SB.upsample2_bwd(dout, dtype)
    idx = tuple(s - 1 for s in shape)
    one_ulp_fault(emu_up2_bwd(dout, dtype), b, dtype, "upsample2 dx", idx)
    # one cell member read twice instead of its neighbour (the gradient's four cell members differ)
    twice = dout.clone()
    twice[:, 1::2, 1::2] = dout[:, 1::2, 0::2]
    rejects(SB.assert_within, emu_up2_bwd(twice, dtype), b, dtype, "upsample2 dx with one member read twice", l2_tol=float("inf"))


@bydtype
@pytest.mark.parametrize("C", [8, 40])
@pytest.mark.parametrize("d", [1, 2, 3, 8])
def test_dilate_split_merge(dtype, d, C):
    B, H, W = 2, 5, 7
    x = draw((B, H, W, C), dtype, d + C)
    sub = emu_dilate(x, B, H, W, d, merge=False)
    SB.assert_equal(sub, SB.dilate_split(x, d), dtype, "split")
    SB.assert_equal(emu_dilate(sub, B, H, W, d, merge=True), x, dtype, "merge(split)")
    s2 = draw(sub.shape, dtype, 9)
    SB.assert_equal(emu_dilate(s2, B, H, W, d, merge=True), SB.dilate_merge(s2, B, H, W, d), dtype, "merge")
    if d > 1:       # phase images transposed (ph <-> pw)
        Hs, Ws = sub.shape[1:3]
        wrong = sub.reshape(B, d, d, Hs, Ws, C).transpose(1, 2).reshape(sub.shape)
        rejects(SB.assert_equal, wrong, SB.dilate_split(x, d), dtype, "split with the phases transposed")


@bydtype
@pytest.mark.parametrize("kind", list("abcdef"))
def test_cat(dtype, kind):
    pieces = SB.cat_case(kind, dtype)
    ref = SB.cat(pieces, dtype)
    SB.assert_equal(emu_cat_fwd(pieces, dtype), ref, dtype, f"cat ({kind})")
    used = sum(c for _, c, _ in pieces)
    assert ref.shape[3] == SB.pad_to(used, SB.VEC[dtype]) and bool((ref[..., used:] == 0).all())
    if kind == "d":
        assert len(pieces) == SB.CAT_MAX and ref.shape[3] > used                                    # a zero tail
    if kind == "f":
        assert ref.shape[3] == SB.VEC[dtype]                                                        # one group only
    acts = [k for k, p in enumerate(pieces) if not p[2]]
    if len(acts) > 1:       # two (activation) pieces swapped
        sw = list(pieces)
        sw[acts[0]], sw[acts[1]] = sw[acts[1]], sw[acts[0]]
        rejects(SB.assert_equal, emu_cat_fwd(sw, dtype), ref, dtype, f"cat ({kind}) with two pieces swapped")
    # a map that skipped its rounding (copied as fp32 bits would be): visible in the 16-bit types
    if dtype != torch.float32 and any(m for _, _, m in pieces):
        raw = ref.clone()
        k = next(i for i, p in enumerate(pieces) if p[2])
        off = sum(c for _, c, _ in pieces[:k])
        raw[..., off] = pieces[k][0][:, 0]
        rejects(SB.assert_equal, raw, ref, dtype, "cat with an unrounded map")
    # backward
    dout = draw(ref.shape, dtype, 7)
    meta = [(c, (1 if m else t.shape[3]), m) for t, c, m in pieces]
    grads, refs = emu_cat_bwd(dout, meta), SB.cat_bwd(dout, meta)
    for k, (g, r) in enumerate(zip(grads, refs)):
        SB.assert_equal(g, r, dtype, f"cat ({kind}) grad {k}")
        if not meta[k][2] and meta[k][1] > meta[k][0]:          # one padding channel left non-zero
            bad = g.clone()
            bad[1, 2, 4, meta[k][1] - 1] = dout[1, 2, 4, 0] + 1.0
            rejects(SB.assert_equal, bad, r, dtype, f"cat ({kind}) grad {k} with a stale padding channel")


@bydtype
def test_relu(dtype):
    V = SB.VEC[dtype]
    sub = 2.0 * SB.TINY[dtype]
    for n in (V, 3 * 5 * 24):
        x = draw((n,), dtype, n)
        x[:4] = torch.tensor([0.0, -0.0, sub, -sub])
        assert torch.equal(SB.rounded(x, dtype), x) and float(x[2]) > 0
        y = torch.where(x > 0, x, torch.zeros(()))
        SB.assert_equal(y, SB.relu(x), dtype, "relu")
        assert float(SB.relu(x)[2]) == sub and float(SB.relu(x)[3]) == 0.0
        dy = draw((n,), dtype, n + 1)
        SB.assert_equal(torch.where(y > 0, dy, torch.zeros(())), SB.relu_bwd(dy, y), dtype, "relu dz")
        flushed = torch.where(x.abs() < 1.5 * sub, torch.zeros(()), y)      # a kernel that flushes the subnormal
        rejects(SB.assert_equal, flushed, SB.relu(x), dtype, "relu with the subnormal flushed")


@bydtype
@pytest.mark.parametrize("add,with_inv,with_p1", SB.CONCAT_MODES)
@pytest.mark.parametrize("hw", [(2, 8, 12), (1, 2, 2)])
def test_packnet_concat(dtype, hw, add, with_inv, with_p1):
    B, H, W = hw
    C0 = 8
    for C1 in ([C0] if add else [8, 24] if with_p1 else [0]):
        p0 = draw((B, H, W, C0), dtype, 1)
        p1 = draw((B, H, W, C1), dtype, 2) if with_p1 else None
        inv = torch.rand(B, H // 2, W // 2, generator=torch.Generator().manual_seed(3)) if with_inv else None
        b = SB.concat(p0, p1, inv, add, dtype)
        out = emu_concat_fwd(p0, p1, inv, add, dtype)
        if add:
            SB.assert_within(out, b, dtype, "concat (add)", l2_tol=float("inf"))
            one_ulp_fault(out, b, dtype, "concat (add)", (B - 1, H - 1, W - 1, C0 - 1))
        else:
            assert float(b.lim.max()) == 0.0
            SB.assert_equal(out, b.ref, dtype, "concat")
        dout = draw(out.shape, dtype, 4)
        d0, d1, dinv = SB.concat_bwd(dout, C0, C1, add, with_inv, dtype)
        SB.assert_equal(dout[..., :C0].clone(), d0, dtype, "d0")
        if with_inv:
            one_ulp_fault(emu_concat_bwd_inv(dout, C0 + (0 if add else C1)), dinv, torch.float32, "d inv", (B - 1, H // 2 - 1, W // 2 - 1))
            if C0 + (0 if add else C1) + 1 < out.shape[3]:      # the channel next to the inverse depth holds a gradient too: reading it instead shows
                rejects(SB.assert_within, emu_concat_bwd_inv(dout, C0 + (0 if add else C1) + 1), dinv, torch.float32, "d inv of the wrong channel", l2_tol=float("inf"))


@bydtype
def test_space_to_depth_and_back(dtype):
    x = draw((2, 6, 10, 16), dtype, 5)
    y = emu_s2d(x)
    SB.assert_equal(y, SB.space_to_depth(x), dtype, "space_to_depth")
    SB.assert_equal(emu_d2s(y), x, dtype, "depth_to_space(space_to_depth)")
    SB.assert_equal(SB.depth_to_space(y), x, dtype, "reference round trip")
    nchw = F.pixel_unshuffle(x.permute(0, 3, 1, 2), 2)              # the same channel order as the reference network's packing
    SB.assert_equal(SB.space_to_depth(x), nchw.permute(0, 2, 3, 1), dtype, "space_to_depth against pixel_unshuffle")
    rejects(SB.assert_equal, emu_s2d(x.transpose(1, 2)).transpose(1, 2), SB.space_to_depth(x), dtype, "dy and dx exchanged")


@bydtype
@pytest.mark.parametrize("C", [1, 3, 9])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("norm", [False, True])
def test_prep_input(dtype, C, flip, norm):
    g = torch.Generator().manual_seed(C)
    for (B, H, W) in [(2, 5, 7), (2, 3, 1)]:
        img = torch.rand(B, C, H, W, generator=g)
        mean, std = (torch.rand(C, generator=g), torch.rand(C, generator=g) * 0.2 + 0.2) if norm else (None, None)
        b = SB.prep_input(img, mean, std, dtype, flip)
        out = emu_prep_input(img, mean, std, dtype, flip)
        if norm:
            one_ulp_fault(out, b, dtype, "prep_input", (B - 1, H - 1, W - 1, C - 1))
        else:
            assert float(b.lim.max()) == 0.0
            SB.assert_equal(out, b.ref, dtype, "prep_input")
        assert b.ref.shape[3] == SB.pad_to(C, SB.VEC[dtype]) and bool((b.ref[..., C:] == 0).all())
        if W > 1:       # one row flipped when flip is off (and the other way round)
            bad = out.clone()
            bad[0, 1] = bad[0, 1].flip(0)
            rejects(SB.assert_within, bad, b, dtype, "prep_input with one row mirrored", l2_tol=float("inf"))


# ---------------------------------------------------------------------------------------------------------------------------------------
# max-pool
# ---------------------------------------------------------------------------------------------------------------------------------------
@bydtype
@pytest.mark.parametrize("shape", SB.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool(dtype, shape):
    B, H, W, C = shape
    x = SB.pool_input(shape, dtype)
    y, idx = SB.maxpool(x)
    ye, ie = emu_maxpool_fwd(x)
    SB.assert_equal(ye, y, dtype, "maxpool y")
    SB.assert_equal(ie, idx, dtype, "maxpool arg-max")
    g0, g1 = draw(y.shape, dtype, 12), draw(y.shape, dtype, 13)
    for second in (g1, None):
        b = SB.maxpool_bwd(g0, second, idx, H, W, dtype)
        dx = emu_maxpool_bwd(g0, second, idx, H, W, dtype)
        hit = (b.ref != 0).nonzero()
        one_ulp_fault(dx, b, dtype, "maxpool dx", tuple(int(v) for v in hit[len(hit) // 2]))
        # the gradients of all elements add up to the gradients of all windows: nothing dropped, nothing doubled
        assert abs(float(b.ref.sum()) - float(g0.double().sum() + (second.double().sum() if second is not None else 0))) < 1e-9
    if H == 1:
        assert bool((idx == 4).all())       # the centre tap is the only one inside the map
        return
    # a tie resolved to the LATER window: the values agree, the saved byte and the gradient do not
    yl, il = emu_maxpool_fwd(x, later_tie=True)
    assert torch.equal(yl, y) and not torch.equal(il, idx)
    rejects(SB.assert_equal, il, idx, dtype, "arg-max with ties resolved to the later tap")
    b = SB.maxpool_bwd(g0, g1, idx, H, W, dtype)
    rejects(SB.assert_within, emu_maxpool_bwd(g0, g1, il, H, W, dtype), b, dtype, "dx scattered by the later tap", l2_tol=float("inf"))
    # one border window dropped in backward: the last window's contribution to one border element
    drop = next((ih, iw, kh, kw) for ih in (H - 1,) for iw in range(W - 1, -1, -1) for kh in range(3) for kw in range(3)
                if (ih + 1 - kh) % 2 == 0 and (iw + 1 - kw) % 2 == 0 and (ih + 1 - kh) // 2 < y.shape[1] and (iw + 1 - kw) // 2 < y.shape[2]
                and bool(((idx[:, (ih + 1 - kh) // 2, (iw + 1 - kw) // 2] == kh * 3 + kw) & (g0[:, (ih + 1 - kh) // 2, (iw + 1 - kw) // 2] + g1[:, (ih + 1 - kh) // 2, (iw + 1 - kw) // 2] != 0)).any()))
    rejects(SB.assert_within, emu_maxpool_bwd(g0, g1, idx, H, W, dtype, drop=drop), b, dtype, "dx with one border window dropped", l2_tol=float("inf"))


def test_the_whole_tensor_check_accepts_what_the_element_bound_rejects():
    """The issue's example: the bf16 max-pool gradient at 2 x 64 x 16 x 24; one element wrong by 1 passes relative L2 < 1e-2 and max-abs < 0.5 of the largest value."""
    dtype = torch.bfloat16
    x = draw((2, 16, 24, 64), dtype, 21)
    _, idx = SB.maxpool(x)
    g0 = draw(idx.shape, dtype, 22)
    b = SB.maxpool_bwd(g0, None, idx, 16, 24, dtype)
    dx = emu_maxpool_bwd(g0, None, idx, 16, 24, dtype)
    bad = dx.clone()
    bad[1, 7, 11, 5] += 1.0
    e = float((bad.double() - b.ref).norm() / b.ref.norm())
    assert e < 1e-2 and float((bad.double() - b.ref).abs().max() / b.ref.abs().max()) < 50 * 1e-2      # test_gpu_nn.check() lets it through
    SB.assert_within(dx, b, dtype, "maxpool dx", l2_tol=float("inf"))
    rejects(SB.assert_within, bad, b, dtype, "maxpool dx with one wrong element", l2_tol=float("inf"))


# ---------------------------------------------------------------------------------------------------------------------------------------
# channel statistics
# ---------------------------------------------------------------------------------------------------------------------------------------
@bydtype
@pytest.mark.parametrize("M,C", SB.STATS_SHAPES)
def test_channel_stats(dtype, M, C):
    x = draw((M, C), dtype, M) + SB.rounded(torch.tensor(0.5), dtype)
    x = SB.rounded(x, dtype)
    b = SB.channel_stats(x)
    part = emu_channel_stats(x)
    assert b.ref.shape == (-(-M // 256), C, 2)
    SB.assert_within(part, b, torch.float32, "channel_stats", l2_tol=float("inf"))
    one_ulp_fault(part, b, torch.float32, "channel_stats", (b.ref.shape[0] - 1, C - 1, 1))
    if b.ref.shape[0] > 1:      # one tile's partial attributed to the next tile
        rejects(SB.assert_within, part.roll(1, 0), b, torch.float32, "channel_stats with the tiles shifted", l2_tol=float("inf"))
        # one row of the last, partial tile missed
        short = emu_channel_stats(x[:M - 1])
        rejects(SB.assert_within, short, b, torch.float32, "channel_stats without the last row", l2_tol=float("inf"))


# ---------------------------------------------------------------------------------------------------------------------------------------
# heads
# ---------------------------------------------------------------------------------------------------------------------------------------
HEAD_SHAPES = SB.HEAD_SHAPES


@functools.lru_cache(maxsize=None)
def head_case(dtype, shape, flip):
    v = SB.head_logits(dtype, shape, 31)
    g = torch.Generator().manual_seed(32)
    B, H, W = shape
    return v, torch.randn(B, 1, H, W, generator=g), torch.randn(B, H, W, generator=g)


def mirrored_row(t):
    """one row of a planar map flipped along x"""
    bad = t.clone()
    bad[0, ..., 1, :] = bad[0, ..., 1, :].flip(-1)
    return bad


@bydtype
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_depth_head(dtype, shape, flip):
    v, dd, _ = head_case(dtype, shape, flip)
    b = SB.depth_head(v, 0.1, 80.0, flip)
    d = emu_depth_head(v, 0.1, 80.0, flip)
    one_ulp_fault(d, b, torch.float32, "depth", (0, 0, 0, 0))
    bb = SB.depth_head_bwd(v, dd, 0.1, 80.0, flip, dtype)
    dy = emu_depth_head_bwd(v, dd, 0.1, 80.0, flip, dtype)
    one_ulp_fault(dy, bb, dtype, "d logit", (shape[0] - 1, shape[1] - 1, shape[2] - 1))
    terms = dy.reshape(-1, 1)
    sb = SB.sum_bound(terms, torch.float32)
    s = torch.zeros(())
    for t in dy.reshape(-1):
        s = s + t
    one_ulp_fault(s.reshape(1), sb, torch.float32, "d bias", (0,))
    if shape[2] > 1:
        rejects(SB.assert_within, mirrored_row(d), b, torch.float32, "depth with one row mirrored", l2_tol=float("inf"))
        rejects(SB.assert_within, mirrored_row(dy), bb, dtype, "d logit with one row mirrored", l2_tol=float("inf"))
    # the softplus branch taken one storage step early (at 20 instead of above it) is inside: softplus(20) - 20 = 2e-9; taken at 0 it is not
    early = emu_depth_head(torch.where(v == 0, torch.full_like(v, 1e-30), v), 0.1, 80.0, flip)
    SB.assert_within(early, b, torch.float32, "depth", l2_tol=float("inf"))
    wrong = d.clone().reshape(-1)
    j = int((_flat(v, flip) == 0).nonzero()[0])
    wrong[j] = 1.0 / SB.f32_recip(80.0)                 # softplus(0) taken as 0
    rejects(SB.assert_within, wrong.reshape(d.shape), b, torch.float32, "depth with softplus(0) = 0", l2_tol=float("inf"))


def _flat(v, flip):
    return (v.flip(2) if flip else v).reshape(-1)


@bydtype
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_inv_depth_head(dtype, shape, flip):
    v, dd, di = head_case(dtype, shape, flip)
    bi, bd = SB.inv_depth_head(v, 0.5, 0.1, 80.0, flip)
    inv, dep = emu_inv_depth_head(v, 0.5, 0.1, 80.0, flip)
    one_ulp_fault(inv, bi, torch.float32, "inv", (0, 0, 0))
    one_ulp_fault(dep, bd, torch.float32, "depth", (0, 0, 0, 0))
    last = (shape[0] - 1, shape[1] - 1, shape[2] - 1)
    for a, c in ((di, dd), (None, dd), (di, None)):
        bb = SB.inv_depth_head_bwd(v, a, c, 0.5, 0.1, 80.0, flip, dtype)
        dy = emu_inv_depth_head_bwd(v, a, c, 0.5, 0.1, 80.0, flip, dtype)
        one_ulp_fault(dy, bb, dtype, "d logit", last)
        if shape[2] > 1 and c is not None:
            rejects(SB.assert_within, emu_inv_depth_head_bwd(v, a, mirrored_row(c), 0.5, 0.1, 80.0, flip, dtype), bb, dtype, "d logit from a mirrored row", l2_tol=float("inf"))


@bydtype
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_sigmoid_head(dtype, shape, flip):
    v, dd, _ = head_case(dtype, shape, flip)
    focal = torch.tensor([700.0, 720.5])
    last = (shape[0] - 1, shape[1] - 1, shape[2] - 1)
    for sc, fo, div in ((80.0, focal, 715.0873), (1.0, None, 1.0)):
        b = SB.sigmoid_head(v, sc, fo, div, flip)
        o = emu_sigmoid_head(v, torch.tensor(SB.f32(sc)), fo, torch.tensor(SB.f32(div)), flip)
        one_ulp_fault(o, b, torch.float32, "sigmoid head", (0, 0, 0, 0))
        bb = SB.sigmoid_head_bwd(v, dd, sc, fo, div, flip, dtype)
        dy = emu_sigmoid_head_bwd(v, dd, torch.tensor(SB.f32(sc)), fo, torch.tensor(SB.f32(div)), flip, dtype)
        one_ulp_fault(dy, bb, dtype, "d logit", last)
        if fo is not None:      # the focal lengths of the two samples exchanged
            rejects(SB.assert_within, emu_sigmoid_head(v, torch.tensor(SB.f32(sc)), fo.flip(0), torch.tensor(SB.f32(div)), flip), b, torch.float32, "focal of the other sample",
                    l2_tol=float("inf"))


@bydtype
def test_the_sigmoid_gradient_needs_its_absolute_term(dtype):
    """At v = 20 the fp32 sigmoid is 1 and 1 - s is 0: the kernel's gradient is 0 where the reference is 2e-9 of the incoming gradient.  A limit
    relative to the reference (c 2^-24 |ref|) would reject the honest kernel; the 4 u s term of 1 - s is what holds."""
    v = SB.rounded(torch.full((1, 1, 1), 20.0), dtype)
    dout = torch.ones(1, 1, 1, 1)
    b = SB.sigmoid_head_bwd(v, dout, 1.0, None, 1.0, False, dtype)
    dy = emu_sigmoid_head_bwd(v, dout, torch.tensor(1.0), None, torch.tensor(1.0), False, dtype)
    assert float(dy) == 0.0 and float(b.ref) > 2e-9 and float(b.lim) < 4.1 * SB.E32 + SB.TINY[dtype] + 1e-12
    SB.assert_within(dy, b, dtype, "d logit at 20", l2_tol=float("inf"))

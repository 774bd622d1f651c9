"""Element-level references for the streaming kernels around the convolutions (helper, no tests; imported like conv_bounds.py).

conv_bounds.py opens with the argument: a relative L2 over a tensor cannot see one wrong element.  For the bf16 max-pool gradient at 2 x 64 x 16 x 24
(norm about 110) one wrong element of size 1 is a relative L2 of 0.009, below the 1e-2 the whole-tensor check allows; a tie resolved to the later
window, a dropped border window or one flipped row pass it the same way.  The kernels here either MOVE elements -- then the reference is exact and the
assertion is torch.equal -- or add a handful of stored values in fp32, or evaluate a short closed form; each gets the fp64 result on the operands as
the kernel reads them (already rounded to the storage type: rounded()) and, where the result is not exact, a per-element limit counted from the
kernel's source.  No constant is fitted to a run.  All tensors are laid out as the kernels see them: NHWC [B, H, W, C] with the padding channels
present, planar maps [B, 1, H, W] / [B, H, W] in fp32.  u = 2^-24 (E32) below.

Exact (assert_equal):
  upsample2 forward (bts.hip up2_fwd_kernel), dilate split / merge (dilate_kernel), space_to_depth / depth_to_space and concat without `add` and
  its slice backward (packnet.hip), relu forward and its backward through act_bwd_bias_kernel (nn.hip: `o > 0 ? d : 0`, so dz is dy or 0), max-pool
  values and the saved arg-max byte (maxpool_fwd_kernel: `v > best || v != v` over kh, kw ascending = the FIRST maximum in row-major window order,
  what ATen's max_pool2d returns as its index), prep_input without mean / std (one conversion to the storage type), and cat (cat_fwd_kernel /
  cat_bwd_kernel): an activation piece is copied; a planar fp32 map goes through `(T)v` once (round to nearest even) on the way in and `(float)src[0]`
  (exact widening) on the way back; channels past the last piece, and a gradient piece's channels past its real count, are written as zero.

fp32 sums of n stored terms, rounded once (sum_bound): the running fp32 sum of n terms in any order has error <= (n - 1) u sum|terms| to first order
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 4.4), then one rounding to the stored type:

    |computed - ref| <= u_out |ref| + (n - 1) 2^-24 sum|terms| + tiny

  upsample2 backward            up2_bwd_kernel: acc = 0; acc += four cell members; (T)acc.  n = 4.
  concat forward, add mode      concat_fwd_kernel: (T)((float)a + (float)b).  n = 2 on the first C0 channels; the other groups are copies (limit 0).
  inverse-depth gradient        concat_bwd_inv_kernel: (r0[0] + r0[Ct]) + (r1[0] + r1[Ct]), fp32 output.  n = 4.
  max-pool backward             maxpool_bwd_kernel: per window d = dout + dout1 (second consumer), then g += d for every window whose saved byte names this
                                element -- at most 2 x 2 windows reach an element (kh and kw are fixed by the parity of ih, iw up to the pair {0, 2}), so
                                n <= 8.  Which windows contribute is read from the reference indices; n is counted per element.
  depth_head's bias gradient    depth_head_bwd_kernel sums `(float)(T)g`, the STORED logit gradients, per thread, per workgroup (sde_block_sum) and
                                in head_bias_finalize_kernel: one fp32 sum of n = B H W terms in some order.  The terms are the gradients the kernel
                                stored (its dy output, checked on its own), so this assertion sees the sum alone.

channel_stats (channel_stats_kernel): part[tile][c][0 | 1] = sum of x, x^2 over the tile's rows (a tile = SDE_STATS_ROWS = 256 rows): eight row lanes
  each add every eighth row in fp32, then one thread adds the eight lane sums.  For the plain sums that is n = rows additions of exact terms:
  (rows - 1) u sum|x|; the squares are rounded before they are added (`f * f`, one more u each): rows u sum x^2.  Both are inside the one limit

    (rows_in_tile + 1) 2^-24 sum|x|        (sum x^2 for the squares)

  The slab is fp32: no further rounding.  Rows of the wrapper's buffer past `tiles` belong to the next stage and are not compared.

prep_input with mean and std (prep_input_kernel): `(v - mean[c]) / std[c]` on fp32 operands: the difference is rounded (u), the quotient is rounded
  (u; hipcc divides fp32 correctly rounded unless told otherwise, and a 1 ulp division would be 2 u): error <= 3 u |ref|, then the store.

Heads.  The reference is the closed form in fp64 at the stored logit v; the limit counts the kernel's roundings.  The HIP math API reference (the
single-precision table of the HIP documentation, the source conv_bounds.py quotes for expm1f) gives expf and log1pf a maximum error of 1 ulp, i.e. a
relative 2 u; +, *, / round once (u).  A sum or product of POSITIVE quantities carries the largest relative error of its terms (sum) or their sum
(product) plus its own u.  Counting first-order terms and adding 1 u for everything of second order:

  s = sigm(v) = 1 / (1 + expf(-v))           expf 2, the sum 2 + 1 = 3, the reciprocal 4:                                 rel(s) <= 4 u
  1 - s                                      exact for s >= 1/2 (Sterbenz), rounded below: abs error <= 4 u s + u (1 - s).  THIS is the one place a head
                                             cancels: at v = 20 the fp32 s is 1 and 1 - s is 0 where the true 1 - s is 2e-9, so a limit relative to the
                                             reference alone cannot hold for the sigmoid gradients; the absolute term 4 u s carries it.
  sp = v > 20 ? v : log1pf(expf(v))          expf 2, through log1p (condition number x / ((1 + x) log1p x) <= 1) 2, log1pf 2: rel(sp) <= 4 u; the branch
                                             replaces softplus by v: absolute error log1p(e^-v) <= e^-20 there (added as it is).

  depth_head forward (nn.hip)      sd = min_disp + (max_disp - min_disp) * sp: the difference 1, the product 4 + 1 + 1 = 6, the sum 7;
                                   depth = 1 / sd: 8.                                                                                c = 8 + 1
  depth_head backward              g = ddepth * (-1 / (sd * sd)) * (max_disp - min_disp) * dsp, dsp = v > 20 ? 1 : 1 / (1 + expf(-v)):
                                   sd 7, sd^2 15, the reciprocal 16, * ddepth 17, * the difference (1) 19, * dsp (4) 24 (+ e^-v relative where the
                                   branch sets dsp = 1); the result is stored in the activation type: stored().                      c = 24 + 1
  inv_depth_head forward (packnet.hip)   inv = s / md_head: 5.                                                                      c = 5 + 1
                                   depth = 1 / (lo + (hi - lo) * inv): the difference 1, the product 5 + 1 + 1 = 7, the sum 8, the reciprocal 9.
                                                                                                                                     c = 9 + 1
  inv_depth_head backward          g = d_inv + t2, t2 = d_depth * (-(hi - lo) / (sd * sd)): sd 8, sd^2 17, the quotient 17 + 1 + 1 = 19, * d_depth 20;
                                   the two terms may cancel, so the sum is bounded absolutely: err(g) <= 20 u |t2| + u |g| (no rounding when one of
                                   them is absent).  f = (s * (1 - s)) / md_head: err(s (1 - s)) <= s (4 u s + u (1 - s)) + 4 u s (1 - s) + u s (1 - s),
                                   the quotient one more: err(f) <= (4 u s^2 + 7 u s (1 - s)) / md_head.  dy = g * f:
                                   err <= |g| err(f) + err(g) f + 2 u |g f|, then stored().
  sigmoid_head forward (bts.hip)   s * scale 5, (v * focal) / focal_div 7.                                                           c = 7 + 1
  sigmoid_head backward            A = ((dout / focal_div) * focal) * scale * s: 2 + 1 + 4 + 1 = 8; dy = A * (1 - s):
                                   err <= |A| (4 u s + u (1 - s)) + 8 u |A| (1 - s) + u |A| (1 - s) + u |dy|, then stored().

  lo = 1 / max_depth and hi = 1 / min_depth are formed in fp32 on the host; the references take the same fp32 values (f32()).
  The local-planar-guidance head is not here: its plane denominator can cancel, and it keeps its whole-tensor assertions.

SDE_BOUNDS_LOG: every assertion, the exact ones included (0 or inf), goes through conv_bounds' record.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import conv_bounds as CB
from conv_bounds import E32, TINY, U_OUT, Bound, assert_within, rounded, stored      # noqa: F401  (re-exported to the tests)

STATS_ROWS = 256      # SDE_STATS_ROWS
CAT_MAX = 6           # SDE_CAT_MAX
VEC = {torch.float32: 4, torch.bfloat16: 8, torch.float16: 8}       # elements in a 16-byte group


def f32(v):
    """A Python number as the fp32 value a kernel argument holds (exactly, as a Python float)."""
    return float(np.float32(v))


def f32_recip(v):
    """1.0f / v as the host code forms it."""
    return float(np.float32(1.0) / np.float32(v))


def pad_to(c, v):
    return (c + v - 1) // v * v


def assert_equal(got, ref, dtype, name):
    """torch.equal, with the first differing element in the message."""
    assert tuple(got.shape) == tuple(ref.shape), f"{name}: shape {tuple(got.shape)} != reference {tuple(ref.shape)}"
    got, ref = got.detach().cpu(), ref.detach().cpu()
    if got.dtype != ref.dtype:
        got, ref = got.double(), ref.double()
    same = torch.equal(got, ref)
    CB._record(dtype, name, 0.0 if same else float("inf"))
    if not same:
        bad = ~(got == ref)
        i = int(bad.flatten().to(torch.uint8).argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), got.shape))
        raise AssertionError(f"{name}: {int(bad.sum())} of {got.numel()} elements differ; first at {idx}: got {got[idx].item()!r}, reference {ref[idx].item()!r}")


def sum_bound(terms, dtype, n=None):
    """terms [k, ...]: the stored values one fp32 accumulator adds (zeros where a slot is empty); n: additions counted (default k; a tensor for a
    per-element count)."""
    t = terms.double()
    n = t.shape[0] if n is None else n
    ref = t.sum(0)
    nm1 = (n - 1.0).clamp(min=0) if torch.is_tensor(n) else max(n - 1, 0)
    return Bound(ref, U_OUT[dtype] * ref.abs() + nm1 * E32 * t.abs().sum(0) + TINY[dtype])


# ---------------------------------------------------------------------------------------------------------------------------------------
# guard bands: what a kernel writes outside its result, and what it leaves unwritten inside
# ---------------------------------------------------------------------------------------------------------------------------------------
GUARD = 256           # bytes before and after the result (a multiple of 16: the result keeps the allocation's 16-byte alignment)
SENTINEL = 0xFF       # every byte: a NaN in all three storage types and in the fp32 maps, 255 as an arg-max byte -- no kernel here produces either


def guarded(shape, dtype, device="cpu"):
    """(buffer, result): `result` is an uninitialised-looking tensor of `shape` carved out of a sentinel-filled byte buffer, GUARD bytes in."""
    n = math.prod(shape) * torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((GUARD + pad_to(n, 16) + GUARD,), SENTINEL, dtype=torch.uint8, device=device)
    out = buf[GUARD:GUARD + n].view(dtype).view(shape)
    assert out.data_ptr() % 16 == 0
    return buf, out


def assert_guards(buf, out, name):
    """Every element of the result was written (no element is still the sentinel pattern) and nothing outside it was."""
    es = out.element_size()
    n = out.numel() * es
    b = buf.cpu()
    inside = b[GUARD:GUARD + n].view(-1, es)
    left = (inside == SENTINEL).all(1)
    assert not bool(left.any()), f"{name}: {int(left.sum())} of {out.numel()} elements were never written; first at flat index {int(left.to(torch.uint8).argmax())}"
    for what, g in (("before", b[:GUARD]), ("after", b[GUARD + n:])):
        hit = g != SENTINEL
        assert not bool(hit.any()), f"{name}: the kernel wrote {int(hit.sum())} bytes {what} its result; first at byte {int(hit.to(torch.uint8).argmax())} of that guard"


# ---------------------------------------------------------------------------------------------------------------------------------------
# data movement
# ---------------------------------------------------------------------------------------------------------------------------------------
def upsample2(x):
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2)


def upsample2_bwd(dout, dtype):
    B, H2, W2, C = dout.shape
    cells = dout.reshape(B, H2 // 2, 2, W2 // 2, 2, C).permute(2, 4, 0, 1, 3, 5).reshape(4, B, H2 // 2, W2 // 2, C)
    return sum_bound(cells, dtype)


def dilate_split(x, d):
    """sub[(b d + ph) d + pw, i, j, :] = x[b, i d + ph, j d + pw, :], zero beyond the map."""
    B, H, W, C = x.shape
    Hs, Ws = -(-H // d), -(-W // d)
    out = torch.zeros(B, d, d, Hs, Ws, C, dtype=x.dtype)
    for ph in range(d):
        for pw in range(d):
            s = x[:, ph::d, pw::d]
            out[:, ph, pw, :s.shape[1], :s.shape[2]] = s
    return out.reshape(B * d * d, Hs, Ws, C)


def dilate_merge(sub, B, H, W, d):
    Hs, Ws, C = sub.shape[1:]
    s = sub.reshape(B, d, d, Hs, Ws, C)
    out = torch.zeros(B, H, W, C, dtype=sub.dtype)
    for ph in range(min(d, H)):
        for pw in range(min(d, W)):
            t = out[:, ph::d, pw::d]
            t.copy_(s[:, ph, pw, :t.shape[1], :t.shape[2]])
    return out


def space_to_depth(x):
    """out[b, y, x, c 4 + dy 2 + dx] = in[b, 2y + dy, 2x + dx, c]"""
    B, H, W, C = x.shape
    return x.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, 4 * C)


def depth_to_space(x):
    B, H, W, C4 = x.shape
    return x.reshape(B, H, W, C4 // 4, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * H, 2 * W, C4 // 4)


def cat(pieces, dtype):
    """pieces: [(tensor, real channels, is_map)]: an activation [B, H, W, ld] holding storage values, or a planar fp32 map [B, 1, H, W]."""
    B, H, W = pieces[0][0].shape[:3]
    cols = []
    for t, c, m in pieces:
        cols.append(rounded(t.reshape(B, H, W, 1), dtype) if m else t[..., :c].float())
    used = sum(c for _, c, _ in pieces)
    cols.append(torch.zeros(B, H, W, pad_to(used, VEC[dtype]) - used))
    return torch.cat(cols, 3)


def cat_bwd(dout, meta):
    """meta: [(real channels, ld, is_map)] -> the gradient of every piece: [B, H, W, ld] with zero padding channels, or [B, 1, H, W] fp32."""
    B, H, W, _ = dout.shape
    out, off = [], 0
    for c, ld, m in meta:
        if m:
            out.append(dout[..., off].float().reshape(B, 1, H, W))
        else:
            g = torch.zeros(B, H, W, ld)
            g[..., :c] = dout[..., off:off + c].float()
            out.append(g)
        off += c
    return out


def relu(x):
    return torch.where(x > 0, x, torch.zeros_like(x))


def relu_bwd(dy, y):
    return torch.where(y > 0, dy, torch.zeros_like(dy))


def concat(p0, p1, inv, add, dtype):
    """[p0 (+ p1 | , p1)] ++ [nearest_x2(inv)] ++ zero fill.  -> Bound: limit 0 wherever the kernel copies."""
    B, H, W, C0 = p0.shape
    if add:
        first = sum_bound(torch.stack([p0, p1]), dtype)
        refs, lims = [first.ref], [first.lim]
    else:
        refs, lims = [p0.double()], [torch.zeros(p0.shape, dtype=torch.float64)]
        if p1 is not None:
            refs.append(p1.double())
            lims.append(torch.zeros(p1.shape, dtype=torch.float64))
    used = sum(r.shape[3] for r in refs)
    if inv is not None:
        refs.append(rounded(inv, dtype).double().repeat_interleave(2, 1).repeat_interleave(2, 2).unsqueeze(3))
        used += 1
    ref = torch.cat(refs, 3)
    ref = torch.cat([ref, torch.zeros(B, H, W, pad_to(used, VEC[dtype]) - used, dtype=torch.float64)], 3)
    lim = torch.zeros_like(ref)
    if add:
        lim[..., :C0] = lims[0]
    return Bound(ref, lim)


def concat_bwd(dout, C0, C1, add, has_inv, dtype):
    """-> (d0, d1 | None, Bound of d_inv | None)"""
    d0 = dout[..., :C0]
    d1 = dout[..., C0:C0 + C1] if (C1 and not add) else None
    dinv = None
    if has_inv:
        ch = C0 + (0 if add else C1)
        g = dout[..., ch]
        B, H, W = g.shape
        dinv = sum_bound(g.reshape(B, H // 2, 2, W // 2, 2).permute(2, 4, 0, 1, 3).reshape(4, B, H // 2, W // 2), torch.float32)
    return d0, d1, dinv


def prep_input(img, mean, std, dtype, flip):
    """img [B, C, H, W] fp32 -> Bound on [B, H, W, Cpad]; without mean / std the limit is 0 (one conversion: the reference is rounded(img))."""
    B, C, H, W = img.shape
    src = img.flip(3) if flip else img
    Cp = pad_to(C, VEC[dtype])
    ref = torch.zeros(B, H, W, Cp, dtype=torch.float64)
    lim = torch.zeros_like(ref)
    if mean is None:
        ref[..., :C] = rounded(src, dtype).double().permute(0, 2, 3, 1)
    else:
        r = ((src.double() - mean.double().view(1, C, 1, 1)) / std.double().view(1, C, 1, 1)).permute(0, 2, 3, 1)
        b = stored(r, 3.0 * E32 * r.abs(), dtype)
        ref[..., :C], lim[..., :C] = b.ref, b.lim
    return Bound(ref, lim)


# ---------------------------------------------------------------------------------------------------------------------------------------
# max-pool 3x3, stride 2, padding 1
# ---------------------------------------------------------------------------------------------------------------------------------------
def maxpool(x):
    """x [B, H, W, C] -> (values [B, OH, OW, C], arg-max byte kh * 3 + kw [B, OH, OW, C] uint8) from F.max_pool2d(return_indices=True)."""
    B, H, W, C = x.shape
    y, flat = F.max_pool2d(x.float().permute(0, 3, 1, 2).contiguous(), 3, 2, 1, return_indices=True)
    OH, OW = y.shape[2:]
    ih, iw = flat // W, flat % W
    kh = ih - (2 * torch.arange(OH).view(1, 1, OH, 1) - 1)
    kw = iw - (2 * torch.arange(OW).view(1, 1, 1, OW) - 1)
    assert int(kh.min()) >= 0 and int(kh.max()) <= 2 and int(kw.min()) >= 0 and int(kw.max()) <= 2
    return y.permute(0, 2, 3, 1).contiguous(), (kh * 3 + kw).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def maxpool_bwd(g0, g1, idx, H, W, dtype):
    """g0, g1 (None: one consumer) [B, OH, OW, C], idx the reference's arg-max bytes -> Bound on dx [B, H, W, C]."""
    B, OH, OW, C = g0.shape
    gs = [g0.double()] + ([g1.double()] if g1 is not None else [])
    # window (oh, ow), tap (kh, kw) -> element (2 oh - 1 + kh, 2 ow - 1 + kw): a padded grid of 2 OH + 1 rows starting at row -1
    terms = torch.zeros(9 * len(gs), B, 2 * OH + 1, 2 * OW + 1, C, dtype=torch.float64)
    count = torch.zeros(B, 2 * OH + 1, 2 * OW + 1, C, dtype=torch.float64)
    for k in range(9):
        kh, kw = divmod(k, 3)
        hit = (idx == k).double()
        for j, g in enumerate(gs):
            terms[k * len(gs) + j, :, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] = g * hit
        count[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] += hit * len(gs)
    terms, count = terms[:, :, 1:1 + H, 1:1 + W], count[:, 1:1 + H, 1:1 + W]
    assert float(count.max()) <= 8
    return sum_bound(terms, dtype, n=count)


# ---------------------------------------------------------------------------------------------------------------------------------------
# channel statistics
# ---------------------------------------------------------------------------------------------------------------------------------------
def channel_stats(x):
    """x [M, C] -> Bound on part[tiles][C][2]."""
    M, C = x.shape
    tiles = -(-M // STATS_ROWS)
    xd = x.double()
    ref = torch.zeros(tiles, C, 2, dtype=torch.float64)
    lim = torch.zeros_like(ref)
    for t in range(tiles):
        rows = xd[t * STATS_ROWS:(t + 1) * STATS_ROWS]
        n = rows.shape[0]
        ref[t, :, 0], ref[t, :, 1] = rows.sum(0), (rows * rows).sum(0)
        lim[t, :, 0], lim[t, :, 1] = (n + 1) * E32 * rows.abs().sum(0), (n + 1) * E32 * (rows * rows).sum(0)
    return Bound(ref, lim)


# ---------------------------------------------------------------------------------------------------------------------------------------
# heads: v [B, H, W] stored logits (channel 0), gradients in fp32
# ---------------------------------------------------------------------------------------------------------------------------------------
def _flip(t, flip):
    return t.flip(-1) if flip else t


def _planar(b):
    return Bound(b.ref.unsqueeze(1), b.lim.unsqueeze(1))


def _softplus(v):
    """(softplus, absolute error of the kernel's branch `v > 20 ? v : ...`, the same relative to sigmoid(v) for its derivative)"""
    tail = torch.log1p(torch.exp(-v.abs()))            # softplus(v) = max(v, 0) + log1p(e^-|v|), without overflow
    far = v > 20.0
    return v.clamp(min=0) + tail, torch.where(far, tail, torch.zeros_like(v)), torch.where(far, torch.exp(-v), torch.zeros_like(v))


def depth_head(v, min_depth, max_depth, flip):
    """depth [B, 1, H, W] = 1 / (min_disp + (max_disp - min_disp) softplus(v)), mirrored along x when flip."""
    v = v.double()
    lo, hi = f32_recip(max_depth), f32_recip(min_depth)
    sp, sp_abs, _ = _softplus(v)
    sd = lo + (hi - lo) * sp
    ref = 1.0 / sd
    # the branch moves sd by (hi - lo) sp_abs, the depth by that over sd, relatively
    lim = (9.0 * E32 + (hi - lo) * sp_abs / sd) * ref
    return _planar(Bound(_flip(ref, flip), _flip(lim, flip)))


def depth_head_bwd(v, ddepth, min_depth, max_depth, flip, dtype):
    """ddepth [B, 1, H, W] -> Bound on the stored logit gradient [B, H, W]."""
    v = v.double()
    lo, hi = f32_recip(max_depth), f32_recip(min_depth)
    sp, sp_abs, dsp_rel = _softplus(v)
    sd = lo + (hi - lo) * sp
    g = _flip(ddepth.double()[:, 0], flip) * (-1.0 / (sd * sd)) * (hi - lo) * torch.sigmoid(v)
    rel = 25.0 * E32 + 2.0 * (hi - lo) * sp_abs / sd + dsp_rel
    return stored(g, rel * g.abs(), dtype)


def inv_depth_head(v, md_head, min_depth, max_depth, flip):
    """-> (Bound of inv [B, H, W], Bound of depth [B, 1, H, W])"""
    v = v.double()
    lo, hi = f32_recip(max_depth), f32_recip(min_depth)
    inv = torch.sigmoid(v) / f32(md_head)
    dep = 1.0 / (lo + (hi - lo) * inv)
    return Bound(inv, 6.0 * E32 * inv), _planar(Bound(_flip(dep, flip), _flip(10.0 * E32 * dep, flip)))


def inv_depth_head_bwd(v, d_inv, d_depth, md_head, min_depth, max_depth, flip, dtype):
    """d_inv [B, H, W] | None, d_depth [B, 1, H, W] | None -> Bound on the stored logit gradient [B, H, W]."""
    v = v.double()
    lo, hi, md = f32_recip(max_depth), f32_recip(min_depth), f32(md_head)
    s, oms = torch.sigmoid(v), torch.sigmoid(-v)
    sd = lo + (hi - lo) * (s / md)
    t1 = d_inv.double() if d_inv is not None else torch.zeros_like(v)
    t2 = _flip(d_depth.double()[:, 0], flip) * (-(hi - lo) / (sd * sd)) if d_depth is not None else torch.zeros_like(v)
    g = t1 + t2
    g_err = 20.0 * E32 * t2.abs() + (E32 * g.abs() if (d_inv is not None and d_depth is not None) else 0.0)
    f = s * oms / md
    f_err = (4.0 * E32 * s * s + 7.0 * E32 * s * oms) / md
    ref = g * f
    return stored(ref, g.abs() * f_err + g_err * f + 2.0 * E32 * ref.abs(), dtype)


def sigmoid_head(v, scale, focal, focal_div, flip):
    """-> Bound of [B, 1, H, W]: sigmoid(v) scale [focal[b] / focal_div], mirrored along x when flip."""
    v = v.double()
    ref = torch.sigmoid(v) * f32(scale)
    if focal is not None:
        ref = ref * focal.double().view(-1, 1, 1) / f32(focal_div)
    return _planar(Bound(_flip(ref, flip), _flip(8.0 * E32 * ref, flip)))


def sigmoid_head_bwd(v, dout, scale, focal, focal_div, flip, dtype):
    v = v.double()
    s, oms = torch.sigmoid(v), torch.sigmoid(-v)
    g = _flip(dout.double()[:, 0], flip)
    if focal is not None:
        g = g / f32(focal_div) * focal.double().view(-1, 1, 1)
    A = (g * f32(scale) * s).abs()
    ref = g * f32(scale) * s * oms
    return stored(ref, A * (4.0 * E32 * s + E32 * oms) + 9.0 * E32 * A * oms + E32 * ref.abs(), dtype)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases, shared by the CPU self-test and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------------
def draw(shape, dtype, seed, scale=1.0):
    """Normal draws holding storage values (fp32 CPU)."""
    return rounded(torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale, dtype)


def cat_case(kind, dtype, seed=0):
    """[(tensor, real channels, is_map)] at 2 x 3 x 5 pixels.  The padding channels of an activation piece hold data: they must not leak.
      a  two aligned pieces, 16 + 24                      b  real 21 of ld 24, then 16: misaligned offset, per-element paths both ways
      c  activation + fp32 map + activation               d  SDE_CAT_MAX pieces, maps second and last, a total that needs a zero tail
      e  one piece with C < ld                            f  real 3 of ld 8 + a map = 4 channels: one group (all of it in fp32, V = 4)"""
    B, H, W = 2, 3, 5
    V = VEC[dtype]

    def act(real, ld, s):
        return draw((B, H, W, ld), dtype, seed * 100 + s), real, False

    def fmap(s):
        return torch.randn(B, 1, H, W, generator=torch.Generator().manual_seed(seed * 100 + s)) * 3.0, 1, True
    return {"a": [act(16, 16, 1), act(24, 24, 2)],
            "b": [act(21, 24, 1), act(16, 16, 2)],
            "c": [act(16, 16, 1), fmap(2), act(16, 16, 3)],
            "d": [act(8, 8, 1), fmap(2), act(13, 16, 3), act(8, 8, 4), act(2 * V, 2 * V, 5), fmap(6)],
            "e": [act(5, 8, 1)],
            "f": [act(3, 8, 1), fmap(2)]}[kind]


CONCAT_MODES = [(False, True, True), (False, False, True), (True, True, True), (True, False, True), (False, True, False)]      # add, with_inv, with_p1
POOL_SHAPES = [(1, 1, 1, 8), (2, 2, 3, 8), (1, 13, 21, 16), (2, 16, 24, 64)]
STATS_SHAPES = [(1, 8), (255, 8), (256, 40), (257, 264), (700, 512)]
HEAD_SHAPES = [(2, 5, 7), (2, 3, 1)]


def pool_input(shape, dtype, seed=11):
    """Five values only: most windows tie, some across all nine taps."""
    vals = rounded(torch.tensor([-1.5, -0.25, 0.0, 0.75, 2.0]), dtype)
    return vals[torch.randint(0, 5, shape, generator=torch.Generator().manual_seed(seed))]


def head_logits(dtype, shape, seed):
    """Stored logits [B, H, W] for the head tests: 0, +-20, 20 + one storage ulp (the softplus branch), +-60 (fp32, bf16) or the largest finite fp16
    value, the rest normal draws of both signs."""
    g = torch.Generator().manual_seed(seed)
    v = rounded(torch.randn(shape, generator=g) * 3.0, dtype)
    ulp20 = 16.0 * 2.0 * U_OUT[dtype]                   # spacing of the storage type in [16, 32)
    special = [0.0, 20.0, -20.0, 20.0 + ulp20] + ([65504.0, -65504.0] if dtype == torch.float16 else [60.0, -60.0])
    flat = v.reshape(-1)
    n = min(len(special), flat.numel())
    flat[:n] = torch.tensor(special[:n])
    assert torch.equal(rounded(v, dtype), v)
    return v


def ulp_of(ref, dtype):
    """One unit in the last place of the storage type at |ref| (a power of two; the subnormal spacing near zero)."""
    r = ref.abs().double().clamp(min=2.0 * TINY[dtype] / (2.0 * U_OUT[dtype]))
    return 2.0 ** torch.floor(torch.log2(r)) * 2.0 * U_OUT[dtype]

"""Element-level references for the normalisation kernels (helper, no tests; imported like stream_bounds.py): BatchNorm and GroupNorm of csrc/nn.hip
and the random layer norm of csrc/google.hip.

stream_bounds.py explains why a whole-tensor relative L2 cannot see one wrong element.  It cannot see a wrong coefficient either: a BatchNorm `dy` that
drops its `xhat * mean(dz * xhat)` term moves the L2 of the data gradient by a few per cent, inside the 3e-2 the bf16 gradients are allowed.  Here every
result gets the fp64 value on the operands AS THE KERNEL READS THEM -- activations already rounded to the storage type, the partial-sum slab as the fp32
values uploaded, fp32 parameters as they are -- and a per-element limit counted from the kernel source.  No constant is fitted to a run.  Tensors are
laid out as the kernels see them: activations [M, C] or [B, HW, C] (NHWC, padding channels present).  u = 2^-24 (E32), e = 2^-53 (E64); `rd` is one
rounding.  hipcc contracts a * b + c into one fma where it likes: that removes a rounding, so counting every written operation is an upper limit for
either code.  Second-order terms are kept by evaluating every first-order term at the PERTURBED magnitude (|x| + err(x)) instead of |x|.

Building blocks
  fold of a slab      The finalize kernels add the slab's column in fp64, in their own order: |sum - exact| <= R e sum|rows|, and the same again for the
                      fp64 reference's own sum: 2 R e sum|rows| (delta).  A slab of more than 4096 rows first goes through rows_reduce_kernel
                      (pre_reduce): chunks of ceil(R / 32) rows are added in fp32 (16 row lanes, then 16 lane sums; additions of an exact 0 are
                      exact), any order: (chunk - 1) u sum|rows| more.
  mean, var           mean = s1 / n (one fp64 division): err(mean) <= delta1 / n + e |mean|.  var = s2 / n - mean^2, clamped at 0 (1-Lipschitz):
                      err(var) <= delta2 / n + 2 |mean| err(mean) + err(mean)^2 + 2^-52 (s2 / n + mean^2).  The last term is the fp64 cancellation: the
                      quotient, the square and the difference round once each, relative to at most s2 / n + mean^2.  It is negligible against eps
                      (at mean 100 it is 2e-12) but it is why a constant channel's variance is only ~0 and may clamp.
  rstd                (float)(1 / sqrt(var + eps)) is decreasing in var, so its error is at most the larger of its distances to the values at
                      max(var - err(var), 0) and at var + err(var) (the first, by convexity, unless the clamp at 0 cuts it short: a constant channel
                      sits AT the clamp and can only move up); + 4 e for sqrt, sum, division in fp64, + u for the conversion.
  normalise           xhat = (v - m) * r from fp32 operands: two roundings, err <= 2 u |xhat|; with operand errors
                      err(xhat) <= r (err(v) + err(m)) + |v - m| err(r) + 2 u |xhat|.
  stored()            the rounding to the storage type, conv_bounds.stored.

BatchNorm forward (bn_finalize_kernel / bn_finalize_apply_kernel, then bn_apply_kernel)
  bnp = [mean, rstd, scale, shift].  Column sums and the variance are fp64, so only these roundings count: the conversions (float)mean, (float)rstd;
  scale = gamma * rstd (u); shift = beta - mean * scale (the product u, the difference u).
      err(mean_f)  <= err(mean) + u |mean|
      err(scale)   <= |gamma| err(rstd) + u |gamma rstd|
      err(shift)   <= |scale| err(mean_f) + |mean| err(scale) + u |mean scale| + u (|beta| + |mean scale|)          ABSOLUTE: beta and mean * scale cancel
  out = max(fma(y, scale, shift) [+ res], 0): with t = y scale + shift in fp64
      err(t)       <= |y| err(scale) + err(shift) + u |t|               NOT relative to the reference alone: shift cancels against y * scale when the
                                                                        mean is large (mean 50, sd 0.01: |t| ~ 1, |y scale| ~ 5000)
      + res: one more rounding, u |t + res|; max(., 0) is 1-Lipschitz; then stored().
  Running statistics (torch's momentum convention, unbiased variance var n / (n - 1); var itself when n = 1):
      new = (1 - momentum) * old + momentum * (float)stat: 1 - momentum, the two products and the sum round once each -- three with the fma hipcc forms
      from the second product, four without; four are counted: err <= momentum err(stat_f) + 3 u |(1 - momentum) old| + 2 u |momentum stat|.
  Eval mode (bn_eval_params_kernel): rstd = 1.0f / sqrtf(rvar + eps).  The sum rounds (u), sqrtf is within 1 ulp = 2 u in the single-precision table of
      the HIP math API reference (the table conv_bounds.py quotes for expm1f), through the square root the sum's u halves, the division rounds (u):
      rel(rstd) <= u / 2 + 2 u + u < 4 u; scale 5 u; shift = beta - rmean * scale: 6 u |rmean scale| + u (|beta| + |rmean scale|).  mean is a copy.

ReLU masks (bn_load_dz)
  Mode 1 reads the stored output (`out > 0`); mode 2 re-derives `fma(y, scale, shift) > 0` from the fp32 bnp it is given.  The reference mask is the
  sign of the fp64 t (+ res in mode 1).  An element is UNDECIDED when
      |t| is within the output's own limit of zero (the computed value may have either sign), or
      t > 0 but t rounds to zero in the storage type: fp16 underflow below 2^-25.  There mode 1 sees a stored 0 and masks, mode 2 sees the fp32 value
      and passes: the two modes legitimately differ, and either result is accepted.
  An undecided element of gm may be 0 or the sum: its limit is |dz| (+ the sum's own limit).  The reduced sums below are built from the gm the kernel
  STORED, so an undecided element contributes exactly what the kernel wrote and its contribution needs no separate bound.  assert_decided() holds
  every tensor to at most 1 undecided element in 1000, on the reference alone.  Planted exact zeros are decided: a channel with gamma = 0, beta = 0 has
  t = 0 in fp64 and in fp32 alike (mask 0 in both modes, not `t > 0`), and so has y == mean with beta = 0 ... as long as scale and shift are the
  operands: t is evaluated on the fp32 bnp the backward kernel reads, where fma(y, 0, 0) = 0 exactly.

BatchNorm backward (bn_bwd_reduce_kernel, bn_bwd_finalize_kernel + bn_bwd_apply_kernel | bn_bwd_finalize_apply_kernel)
  gm = rd_T(mask * (d0 [+ d1 [+ d2]])): an fp32 sum of 1 to 3 stored terms, rounded once: stream_bounds.sum_bound on the masked terms.
  dbeta = sum gm, dgamma = sum gm * xhat, coef = [sum gm / n, sum gm xhat / n], from the gm the kernel stored (checked on its own; the precedent is the
  depth head's bias gradient in stream_bounds.py).  Per workgroup the terms are added in fp32: per thread over its grid-stride trips, then
  block_group_reduce (256 threads: the 256 / cch threads of a column in thread order; 1024 threads: the four quarters first), or LDS float atomics in
  the fallback (any order).  All of them are fp32 sums of n_part terms in SOME order, n_part = the rows one workgroup adds into one column:
      fast path  ceil(M cch / (blocks NT)) * (NT / cch)          fallback  ceil(M / blocks)
  -> (n_part - 1) u sum|terms| over the whole column; the terms gm * xhat carry 3 u each (xhat 2, the product 1).  The fold across workgroups is the
  fp64 slab fold above (with pre_reduce above 4096 rows).  (float) rounds the result (u); `accumulate` adds it to the slot in fp32 (u |new|).
  dy = scale * (dz - k1 - xhat * k2), k = coef: the three terms cancel, so the limit is absolute, from |dz|, |k1| and |xhat k2|:
      err(inner) <= err(k1) + |xhat| err(k2) + |k2| 2 u |xhat| + u |xhat k2| + u (|dz| + |k1|) + u (|dz| + |k1| + |xhat k2|)
      err(dy)    <= |scale| err(inner) + u |dy|, then stored().
  In the fused launch coef stays in LDS (the coef buffer is not written); the limit is the same.

GroupNorm (gn_stats_kernel, gn_finalize_kernel, gn_apply_kernel; gn_bwd_stats_kernel, gn_bwd_finalize_kernel, gn_bwd_apply_kernel)
  The operand is v = x, or rd(x + res) in fp32 in the residual form: err(v) <= u |v|.
  part[b][chunk][c] = (sum v, sum v^2) over the chunk's ceil(HW / SDE_GN_CHUNKS) pixels, in fp32, in one of the kernel's orders (16-byte groups with a
  binary tree; one slot per thread; LDS atomics -- the fixed-channel-per-thread order needs C < the 16-byte group, which the host refuses): all of
  them are sums of n = pixels-in-chunk terms in some order, so as channel_stats: (n + 1) u sum|v| and (n + 1) u sum v^2, + err(v) on every term in the
  residual form (u sum|v|, 2 u sum v^2).  The partials are compared directly, chunk by chunk; chunks past the last pixel hold zeros.
  gnp[b][g] = (mean, rstd): the fp64 finalize above over cpg * chunks partials, n = HW cpg.
  out = act((v - mean) * rstd * gamma + beta), no fma written: normalise (above), * gamma (u), + beta (u).  ReLU is 1-Lipschitz; ELU is 1-Lipschitz and
  calls expm1f, 1 ulp = 2 u of the result (the same table).  Then stored().
  Backward takes the activation derivative from the STORED output, as the reference's in-place activations do, so there is no undecided element: the
  stored output is an operand.  de = d (none), out > 0 ? d : 0 (ReLU, exact), out > 0 ? d : d * (out + 1) (ELU: the sum u, the product u).
  The bwd partials (sum de, sum de xhat) are fp32 chunk sums like the forward ones (n - 1) u, the terms carry err(de) and 3 u + err(v) through xhat;
  coef[b][g] = (sum_c gamma_c S1 / n, sum_c gamma_c S2 / n) and dgamma, dbeta are fp64 folds, rounded to float (u) (+ accumulate u).
  dx = rstd * (gamma * de - c1 - xhat * c2): absolute, as BatchNorm's dy with A = gamma * de (u).

Random layer norm (google.hip rln_*; fp32 and bf16)
  Statistics are of d = rd(x[b, p, c] - x[b, 0, c]) (u |d|): part[b][chunk][c] = (sum d, sum d^2), chunks = clamp(HW / 64, 1, 32), n = pixels in the chunk
  added by the TY row lanes and folded (fold_rows): n u sum|d| and (n + 2) u sum d^2.
  mean = x[b, 0, c] + s1 / n; var = (s2 - s1^2 / n) / (n - 1) clamped at 0: err(var) <= (delta2 + 2 |s1| delta1 / n + delta1^2 / n) / (n - 1) + 4 e (s2 + s1^2 / n) / (n - 1).
  The noise factors are f = rd(1 + fmodf(rd(z s), 2 s)): the reference takes the same fp32 product z s, fmod is exact, 2 s is exact; one rounding (u).
  train = 0 and stddev = 0 give factor 1 exactly.
  m = (float)mean * fm: err <= fm err(mean) + 3 u |mean fm|.  r = (float)(1 / sqrt((double)((float)var * fv) + eps)): the argument carries
  fv err(var) + 3 u var fv; through the convex rstd as above.  rlnp[b][c] = (m, r), zero for c >= Cr.
  out = max(gamma * ((v - m) * r) + beta [+ res], 0): normalise, * gamma, + beta, + res (u each); channels >= Cr are written as zero (limit 0).
  Backward: gv = mask * (d0 [+ d1 [+ d2]]) in fp32, NOT rounded before it is used (gm_out = rd_T(gv) is stored for the residual only): mask from the
  stored output (an operand: decided).  dx = gv * k, k = rd(gamma * r) for c < Cr, else 0: err <= |k| err(gv) + 2 u |gv k|, then stored().  The
  statistics carry no gradient, as in the original.  dbeta = sum gv, dgamma = sum gv xhat: fp32 chunk sums (n - 1) u + the terms' own errors, an fp64 fold
  over (b, chunk), (float) (+ accumulate).

SDE_BOUNDS_LOG: every assertion goes through conv_bounds' record.
"""
import math

import torch

import conv_bounds as CB
from conv_bounds import E32, TINY, U_OUT, Bound, _record, assert_within, rounded, stored      # noqa: F401  (re-exported to the tests)
from stream_bounds import (GUARD, SENTINEL, VEC, assert_equal, assert_guards, draw, f32, guarded, pad_to, sum_bound, ulp_of)      # noqa: F401

E64 = 2.0 ** -53
GN_CHUNKS = 64        # SDE_GN_CHUNKS
RLN_CHUNKS = 32       # SDE_RLN_CHUNKS
REDUCE_ROWS = 32      # SDE_REDUCE_ROWS
PRE_REDUCE_ABOVE = 4096
BNFA_MAX_ROWS = 256
ACT_NONE, ACT_RELU, ACT_ELU = 0, 1, 2
UNDECIDED_MAX = 1e-3
D = torch.float64


def f32t(t):
    """A tensor as the fp32 values a kernel reads, in fp64."""
    return t.float().double()


# ---------------------------------------------------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------------------------------------------------
def pre_reduce_chunk(rows):
    """Rows per fp32 chunk of rows_reduce_kernel, or 0 when the slab is read as it is."""
    return -(-rows // REDUCE_ROWS) if rows > PRE_REDUCE_ABOVE else 0


def fold_slab(part):
    """part [R, ...] fp32 -> (column sums fp64, delta): what the fp64 fold of the finalize kernels (behind pre_reduce when R > 4096) may differ by."""
    p = part.double()
    R = p.shape[0]
    mag = p.abs().sum(0)
    delta = 2.0 * R * E64 * mag
    chunk = pre_reduce_chunk(R)
    if chunk:
        delta = delta + (chunk - 1) * E32 * mag
    return p.sum(0), delta


def mean_var(s1, d1, s2, d2, n):
    """-> mean, err(mean), var (clamped), err(var)"""
    mean = s1 / n
    em = d1 / n + E64 * mean.abs()
    raw = s2 / n - mean * mean
    ev = d2 / n + 2.0 * mean.abs() * em + em * em + 2.0 ** -52 * (s2.abs() / n + mean * mean)
    return mean, em, raw.clamp(min=0), ev


def rstd_of(var, ev, eps):
    """(float)(1 / sqrt(var + eps)) -> rstd (fp64), err"""
    r = 1.0 / torch.sqrt(var + eps)
    hi = 1.0 / torch.sqrt((var - ev).clamp(min=0) + eps)
    lo = 1.0 / torch.sqrt(var + ev + eps)
    return r, torch.maximum(hi - r, r - lo) + (4.0 * E64 + E32) * hi


def normalise(v, ev, m, em, r, er):
    """xhat = (v - m) * r in fp32 -> xhat, err"""
    xh = (v - m) * r
    dv = ev + em
    exh = r.abs() * dv + (v - m).abs() * er + dv * er
    return xh, exh + 2.0 * E32 * (xh.abs() + exh)


def scale_shift(xh, exh, gamma, beta):
    """xhat * gamma + beta, two roundings -> o, err"""
    p = xh * gamma
    ep = gamma.abs() * exh + E32 * (p.abs() + gamma.abs() * exh)
    o = p + beta
    return o, ep + E32 * (p.abs() + ep + beta.abs())


def act_fwd(o, eo, act):
    if act == ACT_RELU:
        return o.clamp(min=0), eo
    if act == ACT_ELU:
        a = torch.where(o > 0, o, torch.expm1(o))
        return a, eo + 2.0 * E32 * (a.abs() + eo)
    return o, eo


def cancel3(outer, eouter, A, eA, k1, ek1, xh, exh, k2, ek2):
    """outer * (A - k1 - xh * k2) in fp32 -> ref, err (absolute: the three terms cancel)"""
    prod = xh * k2
    eprod = xh.abs() * ek2 + k2.abs() * exh + exh * ek2
    eprod = eprod + E32 * (prod.abs() + eprod)
    inner = A - k1 - prod
    first = A.abs() + eA + k1.abs() + ek1
    einner = eA + ek1 + eprod + E32 * first + E32 * (first + prod.abs() + eprod)
    ref = outer * inner
    err = outer.abs() * einner + eouter * (inner.abs() + einner)
    return ref, err + E32 * (ref.abs() + err)


def to_float(ref, err, prior=None):
    """(float)value [added to the fp32 slot `prior`] -> Bound"""
    lim = err + E32 * (ref.abs() + err)
    if prior is not None:
        ref = ref + prior.double()
        lim = lim + E32 * (ref.abs() + lim)
    return Bound(ref, lim + TINY[torch.float32])


def assert_decided(undecided, name):
    share = float(undecided.double().mean()) if undecided.numel() else 0.0
    assert share <= UNDECIDED_MAX, f"{name}: {share:.2e} of the elements have an undecided ReLU mask (> {UNDECIDED_MAX}): choose other inputs"
    return share


# ---------------------------------------------------------------------------------------------------------------------------------------
# BatchNorm forward
# ---------------------------------------------------------------------------------------------------------------------------------------
class BNForward:
    """part [R, C, 2] fp32 slab, n rows of activations, gamma / beta [C] fp32, eps / momentum as the kernel arguments (f32()).
    .bnp Bound [4, C]; running(old_mean, old_var) -> (Bound, Bound); out(y, res, relu, dtype) -> Bound [M, C]."""

    def __init__(self, part, n, gamma, beta, eps, momentum=0.1):
        s, d = fold_slab(part)
        self.n, self.mom = float(n), f32(momentum)
        g, b = f32t(gamma), f32t(beta)
        self.mean, em, self.var, self.ev = mean_var(s[:, 0], d[:, 0], s[:, 1], d[:, 1], self.n)
        self.emf = em + E32 * (self.mean.abs() + em)
        self.rstd, self.er = rstd_of(self.var, self.ev, f32(eps))
        self.scale = g * self.rstd
        self.es = g.abs() * self.er + E32 * g.abs() * (self.rstd + self.er)
        ms = (self.mean.abs() + self.emf) * (self.scale.abs() + self.es)
        self.shift = b - self.mean * self.scale
        self.esh = self.scale.abs() * self.emf + self.mean.abs() * self.es + self.emf * self.es + E32 * ms + E32 * (b.abs() + ms * (1.0 + E32))
        self.bnp = Bound(torch.stack([self.mean, self.rstd, self.scale, self.shift]),
                         torch.stack([self.emf, self.er, self.es, self.esh]) + TINY[torch.float32])

    def running(self, old_mean, old_var):
        n, mom = self.n, self.mom
        one_m = f32(1.0 - mom)                                     # the reference keeps the kernel's rounded 1 - momentum out of the limit's way:
        unb = self.var * n / (n - 1.0) if n > 1 else self.var       # its rounding is counted below against the exact value
        eu = (self.ev * n / (n - 1.0) if n > 1 else self.ev) + 3.0 * E64 * unb
        euf = eu + E32 * (unb + eu)
        out = []
        for old, stat, es in ((f32t(old_mean), self.mean, self.emf), (f32t(old_var), unb, euf)):
            ref = (1.0 - mom) * old + mom * stat
            a, b = (one_m * old).abs(), (mom * stat).abs() + mom * es
            out.append(Bound(ref, mom * es + 3.0 * E32 * a + 2.0 * E32 * b + 4.0 * E32 * E32 * (a + b) + TINY[torch.float32]))
        return out

    def pre(self, y, res):
        """fp64 t (+ res) and its error before the store"""
        return _bn_pre(y.double(), self.scale, self.es, self.shift, self.esh, res)

    def out(self, y, res, relu, dtype):
        t, et = self.pre(y, res)
        return stored(t.clamp(min=0) if relu else t, et, dtype)


def _bn_pre(y, sc, es, sh, esh, res):
    t = y * sc + sh
    et = y.abs() * es + esh
    et = et + E32 * (t.abs() + et)
    if res is not None:
        t = t + res.double()
        et = et + E32 * (t.abs() + et)
    return t, et


def bn_apply(y, bnp, res, relu, dtype):
    """bn_apply_kernel on fp32 bnp operands -> Bound"""
    b = f32t(bnp)
    z = torch.zeros_like(b[0])
    t, et = _bn_pre(y.double(), b[2], z, b[3], z, res)
    return stored(t.clamp(min=0) if relu else t, et, dtype)


def bn_eval_params(gamma, beta, rmean, rvar, eps):
    g, b, m, v = (f32t(t) for t in (gamma, beta, rmean, rvar))
    r = 1.0 / torch.sqrt(v + f32(eps))
    sc = g * r
    ms = (m * sc).abs()
    return Bound(torch.stack([m, r, sc, b - m * sc]),
                 torch.stack([torch.zeros_like(m), 4.0 * E32 * r, 5.0 * E32 * sc.abs(), 6.0 * E32 * ms + E32 * (b.abs() + ms * (1.0 + 6.0 * E32))]) + TINY[torch.float32])


# ---------------------------------------------------------------------------------------------------------------------------------------
# BatchNorm backward
# ---------------------------------------------------------------------------------------------------------------------------------------
def bn_mask(y, bnp, res, relu_mode, dtype):
    """-> (mask fp64 [M, C], undecided bool [M, C]) from the fp64 t on the fp32 bnp the backward kernel reads (mode 1: + res, the stored output's t)."""
    if not relu_mode:
        return torch.ones(y.shape, dtype=D), torch.zeros(y.shape, dtype=torch.bool)
    b = f32t(bnp)
    z = torch.zeros_like(b[0])
    t, et = _bn_pre(y.double(), b[2], z, b[3], z, res if relu_mode == 1 else None)
    if relu_mode == 1:
        lim = stored(t, et, dtype).lim
        und = (t.abs() <= lim) & (t != 0) | ((t > 0) & (rounded(t.float(), dtype) == 0))
    else:
        und = (t != 0) & (t.abs() < 2.0 ** -126)            # fma rounds the exact value once: the sign is kept down to the subnormal range
    return (t > 0).double(), und


def bn_gm(grads, mask, undecided, dtype):
    """gm = rd_T(mask * sum of the gradients) -> Bound; an undecided element may be 0 or the sum."""
    terms = torch.stack([g.double() for g in grads])
    b = sum_bound(terms * mask, dtype)
    full = sum_bound(terms, dtype)
    return Bound(b.ref, torch.where(undecided, full.ref.abs() + full.lim, b.lim))


def bn_reduce_route(M, C, dtype, nblk0, fuse=1):
    """-> (route name, workgroups, n_part) of sde_bn_bwd's reduce pass; nblk0 = sde_reduce_num_blocks(M, C); fuse = the sde_bn_set_fuse state."""
    V = VEC[dtype]
    cch = C // V
    fast = cch <= 256 and 256 % cch == 0
    is16 = dtype != torch.float32
    if fuse == 1 and is16 and C % 64 == 0 and nblk0 > BNFA_MAX_ROWS and fast:
        nblk = (nblk0 + 3) // 4
        return "wide1024", nblk, -(-M * cch // (nblk * 1024)) * (1024 // cch)
    if fast:
        return "fast256", nblk0, -(-M * cch // (nblk0 * 256)) * (256 // cch)
    return "atomics", nblk0, -(-M // nblk0)


def bn_finalize_fused(rows, C, dtype, fuse=1):
    """The rule of sde_bn_bwd / sde_bn_bwd_from_part (and, with sde_bn_finalize_apply_ok, of the forward wrapper)."""
    return bool(fuse) and dtype != torch.float32 and C % 64 == 0 and 1 <= rows <= BNFA_MAX_ROWS


def bn_xhat(y, bnp):
    b = f32t(bnp)
    z = torch.zeros_like(b[0])
    return normalise(y.double(), 0.0, b[0], z, b[1], z)


def bn_sums(gm, y, bnp, n_part, rows, prior=None, part=None):
    """gm: the masked gradient as the kernel stored it (or d0 itself).  n_part: rows one workgroup adds into one column; rows: slab rows (for
    pre_reduce).  part: a host-built slab [R, C, 2] instead (sde_bn_bwd_from_part) -- then the sums are of the slab.
    -> {"dbeta", "dgamma", "coef"}: Bound, and k, ek (fp64 [2, C]) for bn_dy."""
    M = y.shape[0]
    if part is not None:
        s, d = fold_slab(part)
        s1, s2, e1, e2 = s[:, 0], s[:, 1], d[:, 0], d[:, 1]
    else:
        g = gm.double()
        xh, exh = bn_xhat(y, bnp)
        t2 = g * xh
        et2 = g.abs() * exh + E32 * (t2.abs() + g.abs() * exh)
        s1, s2 = g.sum(0), t2.sum(0)
        m1, m2 = g.abs().sum(0), (t2.abs() + et2).sum(0)
        chunk = pre_reduce_chunk(rows)
        extra = (chunk - 1) * E32 if chunk else 0.0
        fold = 2.0 * (rows + M) * E64
        e1 = ((n_part - 1) * E32 + extra + fold) * m1
        e2 = ((n_part - 1) * E32 + extra + fold) * m2 + et2.sum(0)
    pg, pb = (prior if prior is not None else (None, None))
    k = torch.stack([s1 / M, s2 / M])
    ek = torch.stack([e1 / M, e2 / M]) + E64 * k.abs()
    coef = to_float(k, ek)
    return {"dbeta": to_float(s1, e1, pb), "dgamma": to_float(s2, e2, pg), "coef": coef, "k": k, "ek": coef.lim}


def bn_dy(dz, y, bnp, k, ek, dtype):
    """dy = scale * (dz - k1 - xhat * k2) -> Bound"""
    b = f32t(bnp)
    xh, exh = bn_xhat(y, bnp)
    z = torch.zeros_like(b[0])
    ref, err = cancel3(b[2], z, dz.double(), 0.0, k[0], ek[0], xh, exh, k[1], ek[1])
    return stored(ref, err, dtype)


# ---------------------------------------------------------------------------------------------------------------------------------------
# GroupNorm
# ---------------------------------------------------------------------------------------------------------------------------------------
def gn_path(C, dtype):
    """The statistics order gn_stats_kernel / gn_bwd_stats_kernel pick from C (the rule in the source)."""
    V = VEC[dtype]
    if C % V == 0 and 256 % (C // V) == 0:
        return "vector"
    if 256 % C == 0:
        return "channel"
    if C % 256 == 0 and C <= 2048:
        return "slots"
    return "atomics"


def chunk_ranges(HW, chunks):
    per = -(-HW // chunks)
    return [(min(HW, q * per), min(HW, (q + 1) * per)) for q in range(chunks)]


def _chunk_sums(t, HW, chunks):
    """t [B, HW, C] fp64 -> [B, chunks, C] sums, [B, chunks, C] sums of |t|, pixels per chunk [chunks]"""
    B, _, C = t.shape
    s, a = torch.zeros(B, chunks, C, dtype=D), torch.zeros(B, chunks, C, dtype=D)
    n = torch.zeros(chunks, dtype=D)
    for q, (p0, p1) in enumerate(chunk_ranges(HW, chunks)):
        if p1 > p0:
            s[:, q], a[:, q], n[q] = t[:, p0:p1].sum(1), t[:, p0:p1].abs().sum(1), p1 - p0
    return s, a, n.view(1, chunks, 1)


def gn_operand(x, res):
    v = x.double()
    if res is None:
        return v, torch.zeros_like(v)
    v = v + res.double()
    return v, E32 * v.abs()


class GNForward:
    """x, res [B, HW, C] storage values, gamma / beta fp32 [C].  .part Bound [B, GN_CHUNKS, C, 2]; .gnp Bound [B, G, 2]; .out Bound [B, HW, C]."""

    def __init__(self, x, res, gamma, beta, G, eps, act, dtype):
        B, HW, C = x.shape
        cpg = C // G
        v, ev = gn_operand(x, res)
        s1, a1, n = _chunk_sums(v, HW, GN_CHUNKS)
        s2, a2, _ = _chunk_sums(v * v, HW, GN_CHUNKS)
        r1 = 1.0 if res is not None else 0.0
        l1, l2 = (n + 1 + r1) * E32 * a1, (n + 1 + 2 * r1 + 2 * r1 * E32) * E32 * a2
        self.part = Bound(torch.stack([s1, s2], 3), torch.stack([l1, l2], 3))
        cnt = float(HW * cpg)
        fold = 2.0 * GN_CHUNKS * cpg * E64

        def grp(t):
            return t.sum(1).view(B, G, cpg).sum(2)
        S1, S2 = grp(s1), grp(s2)
        D1, D2 = grp(l1) + fold * grp(a1), grp(l2) + fold * grp(a2)
        mean, em, var, evar = mean_var(S1, D1, S2, D2, cnt)
        emf = em + E32 * (mean.abs() + em)
        rstd, er = rstd_of(var, evar, f32(eps))
        self.gnp = Bound(torch.stack([mean, rstd], 2), torch.stack([emf, er], 2) + TINY[torch.float32])

        def per_c(t):
            return t.repeat_interleave(cpg, 1).view(B, 1, C)
        xh, exh = normalise(v, ev, per_c(mean), per_c(emf), per_c(rstd), per_c(er))
        o, eo = scale_shift(xh, exh, f32t(gamma).view(1, 1, C), f32t(beta).view(1, 1, C))
        a, ea = act_fwd(o, eo, act)
        self.out = stored(a, ea, dtype)


def gn_backward(dout, out, x, res, gnp, gamma, G, act, dtype, prior=None):
    """out: the stored output, gnp: fp32 [B, G, 2] as the forward kernel left them (operands).  -> {"coef", "dgamma", "dbeta", "dx"}: Bound"""
    B, HW, C = x.shape
    cpg = C // G
    g = f32t(gamma).view(1, 1, C)
    d, o = dout.double(), out.double()
    if act == ACT_RELU:
        de, ede = torch.where(o > 0, d, torch.zeros_like(d)), torch.zeros_like(d)
    elif act == ACT_ELU:
        de = torch.where(o > 0, d, d * (o + 1.0))
        ede = torch.where(o > 0, torch.zeros_like(d), 2.0 * E32 * de.abs() * (1.0 + E32))
    else:
        de, ede = d, torch.zeros_like(d)
    v, ev = gn_operand(x, res)
    st = f32t(gnp)

    def per_c(t):
        return t.repeat_interleave(cpg, 1).view(B, 1, C)
    m, r = per_c(st[..., 0]), per_c(st[..., 1])
    z = torch.zeros_like(m)
    xh, exh = normalise(v, ev, m, z, r, z)
    t2 = de * xh
    et2 = de.abs() * exh + ede * (xh.abs() + exh)
    et2 = et2 + E32 * (t2.abs() + et2)
    s1, a1, n = _chunk_sums(de, HW, GN_CHUNKS)
    s2, a2, _ = _chunk_sums(t2, HW, GN_CHUNKS)
    q1, _, _ = _chunk_sums(ede, HW, GN_CHUNKS)
    q2, _, _ = _chunk_sums(et2, HW, GN_CHUNKS)
    nm1 = (n - 1).clamp(min=0)
    l1, l2 = nm1 * E32 * (a1 + q1) + q1, nm1 * E32 * (a2 + q2) + q2
    # per channel over (b, chunk)
    fold_c = 2.0 * B * GN_CHUNKS * E64
    pg, pb = (prior if prior is not None else (None, None))
    dbeta = to_float(s1.sum((0, 1)), l1.sum((0, 1)) + fold_c * a1.sum((0, 1)), pb)
    dgamma = to_float(s2.sum((0, 1)), l2.sum((0, 1)) + fold_c * a2.sum((0, 1)), pg)
    # per (b, g): gamma-weighted
    cnt = float(HW * cpg)
    gc = g.view(1, C)
    fold_g = 3.0 * GN_CHUNKS * cpg * E64

    def grp(t):
        return (t.sum(1) * gc).view(B, G, cpg).sum(2)

    def grp_abs(t):
        return (t.sum(1) * gc.abs()).view(B, G, cpg).sum(2)
    c1, c2 = grp(s1) / cnt, grp(s2) / cnt
    e1 = (grp_abs(l1) + fold_g * grp_abs(a1)) / cnt + E64 * c1.abs()
    e2 = (grp_abs(l2) + fold_g * grp_abs(a2)) / cnt + E64 * c2.abs()
    coef = to_float(torch.stack([c1, c2], 2), torch.stack([e1, e2], 2))
    A = g * de
    eA = g.abs() * ede + E32 * (A.abs() + g.abs() * ede)
    ref, err = cancel3(r, z, A, eA, per_c(c1), per_c(coef.lim[..., 0]), xh, exh, per_c(c2), per_c(coef.lim[..., 1]))
    return {"coef": coef, "dgamma": dgamma, "dbeta": dbeta, "dx": stored(ref, err, dtype)}


# ---------------------------------------------------------------------------------------------------------------------------------------
# random layer norm
# ---------------------------------------------------------------------------------------------------------------------------------------
def rln_chunks(HW):
    return max(1, min(RLN_CHUNKS, HW // 64))


def rln_layout(C, dtype):
    """(cch, TX, TY, channel groups per thread) of google.hip's Layout"""
    cch = C // VEC[dtype]
    TX = min(cch, 256)
    return cch, TX, 256 // TX, -(-cch // 256)


def rln_factors(z, s, train, B, Cr):
    """fm, fv [B, Cr] fp64: rd(1 + fmod(rd(z s), 2 s)) as the kernel forms them; 1 when not training or s == 0."""
    if not train or f32(s) == 0.0:
        one = torch.ones(B, Cr, dtype=D)
        return one, one, 0.0
    sf = torch.tensor(s, dtype=torch.float32)
    zs = (z.float() * sf).double()                       # the same fp32 product
    f = 1.0 + torch.fmod(zs, 2.0 * f32(s))
    return f[0], f[1], E32


class RLNForward:
    """y, res [B, HW, C] storage values; gamma, beta [Cr]; z [2, B, Cr] fp32; s the stddev value.
    .part Bound [B, nch, C, 2] (all C channels: the statistics kernel does not know Cr); .rlnp Bound [B, C, 2]; .out Bound [B, HW, C]."""

    def __init__(self, y, res, gamma, beta, z, s, train, eps, relu, dtype):
        B, HW, C = y.shape
        Cr = gamma.numel()
        nch = rln_chunks(HW)
        v = y.double()
        k = v[:, :1]
        d = v - k
        s1, a1, n = _chunk_sums(d, HW, nch)
        s2, a2, _ = _chunk_sums(d * d, HW, nch)
        l1, l2 = n * E32 * a1, (n + 2 + 2 * E32) * E32 * a2
        self.part = Bound(torch.stack([s1, s2], 3), torch.stack([l1, l2], 3))
        fold = 2.0 * nch * E64
        S1, S2 = s1.sum(1), s2.sum(1)
        D1, D2 = l1.sum(1) + fold * a1.sum(1), l2.sum(1) + fold * a2.sum(1)
        cnt = float(HW)
        mean = k[:, 0] + S1 / cnt
        em = D1 / cnt + 2.0 * E64 * (k[:, 0].abs() + S1.abs() / cnt)
        sq = S1 * S1 / cnt
        var = ((S2 - sq) / (cnt - 1.0)).clamp(min=0)
        evar = (D2 + 2.0 * S1.abs() * D1 / cnt + D1 * D1 / cnt) / (cnt - 1.0) + 4.0 * E64 * (S2 + sq) / (cnt - 1.0)
        fm, fv, uf = rln_factors(z, s, train, B, Cr)
        mean, em, var, evar = mean[:, :Cr], em[:, :Cr], var[:, :Cr], evar[:, :Cr]
        m = mean * fm
        e_m = fm.abs() * em + 3.0 * E32 * (mean.abs() + em) * fm.abs()
        vv = var * fv
        evv = fv.abs() * evar + 3.0 * E32 * (var + evar) * fv.abs()
        assert float((vv - evv).min()) + f32(eps) > 0, "rln: the noisy variance may reach -eps: choose other inputs"
        r = 1.0 / torch.sqrt(vv + f32(eps))
        hi = 1.0 / torch.sqrt(vv - evv + f32(eps))
        lo = 1.0 / torch.sqrt(vv + evv + f32(eps))
        er = torch.maximum(hi - r, r - lo) + (4.0 * E64 + E32) * hi
        ref = torch.zeros(B, C, 2, dtype=D)
        lim = torch.zeros(B, C, 2, dtype=D)
        ref[:, :Cr, 0], ref[:, :Cr, 1], lim[:, :Cr, 0], lim[:, :Cr, 1] = m, r, e_m + TINY[torch.float32], er + TINY[torch.float32]
        self.rlnp = Bound(ref, lim)
        xh, exh = normalise(v[..., :Cr], 0.0, m.unsqueeze(1), e_m.unsqueeze(1), r.unsqueeze(1), er.unsqueeze(1))
        o, eo = scale_shift(xh, exh, f32t(gamma).view(1, 1, Cr), f32t(beta).view(1, 1, Cr))
        if res is not None:
            o = o + res.double()[..., :Cr]
            eo = eo + E32 * (o.abs() + eo)
        self.pre, self.epre = o, eo
        if relu:
            o = o.clamp(min=0)
        b = stored(o, eo, dtype)
        oref, olim = torch.zeros(B, HW, C, dtype=D), torch.zeros(B, HW, C, dtype=D)
        oref[..., :Cr], olim[..., :Cr] = b.ref, b.lim
        self.out = Bound(oref, olim)


def rln_backward(grads, out, y, rlnp, gamma, relu, dtype, prior=None):
    """out: the stored output (mask operand); rlnp fp32 [B, C, 2] as the forward kernel left it.  -> {"gm", "dx", "dgamma", "dbeta"}: Bound"""
    B, HW, C = y.shape
    Cr = gamma.numel()
    nch = rln_chunks(HW)
    terms = torch.stack([t.double() for t in grads])
    mask = (out.double() > 0).double() if relu else torch.ones(B, HW, C, dtype=D)
    terms = terms * mask
    gv = terms.sum(0)
    egv = (len(grads) - 1) * E32 * terms.abs().sum(0)
    st = f32t(rlnp)
    m, r = st[..., 0].unsqueeze(1), st[..., 1].unsqueeze(1)
    kk = torch.zeros(1, 1, C, dtype=D)
    g = f32t(gamma).view(1, 1, Cr)
    gr = g * r[..., :Cr]
    ek = torch.zeros(B, 1, C, dtype=D)
    kk = torch.zeros(B, 1, C, dtype=D)
    kk[..., :Cr], ek[..., :Cr] = gr, E32 * gr.abs()
    dx = gv * kk
    edx = kk.abs() * egv + ek * (gv.abs() + egv)
    edx = edx + E32 * (dx.abs() + edx)
    z = torch.zeros_like(m)
    xh, exh = normalise(y.double(), 0.0, m, z, r, z)
    t2 = gv * xh
    et2 = gv.abs() * exh + egv * (xh.abs() + exh)
    et2 = et2 + E32 * (t2.abs() + et2)
    s1, a1, n = _chunk_sums(gv, HW, nch)
    s2, a2, _ = _chunk_sums(t2, HW, nch)
    q1, _, _ = _chunk_sums(egv, HW, nch)
    q2, _, _ = _chunk_sums(et2, HW, nch)
    nm1 = (n - 1).clamp(min=0)
    fold = 2.0 * B * nch * E64
    l1 = (nm1 * E32 * (a1 + q1) + q1 + fold * a1).sum((0, 1))[:Cr]
    l2 = (nm1 * E32 * (a2 + q2) + q2 + fold * a2).sum((0, 1))[:Cr]
    pg, pb = (prior if prior is not None else (None, None))
    return {"gm": sum_bound(terms, dtype), "dx": stored(dx, edx, dtype),
            "dbeta": to_float(s1.sum((0, 1))[:Cr], l1, pb), "dgamma": to_float(s2.sum((0, 1))[:Cr], l2, pg)}


# ---------------------------------------------------------------------------------------------------------------------------------------
# the slab a convolution's epilogue hands to BatchNorm
# ---------------------------------------------------------------------------------------------------------------------------------------
def conv_slab_totals(y):
    """Column totals (sum y, sum y^2) of the slab conv2d(..., bn_stats=True) returns, against the STORED output y [M, C] -> Bound [C, 2].
    The epilogues add the values AS STORED, not the fp32 accumulator: conv.hip writes the rounded value back to the LDS tile "for the statistics pass"
    and pgemm.hip / the halo kernel unpack the packed 16-bit tile they are about to store ("of the rounded values"); in fp32 the two are the same.
    So the terms are exact and the seam is a sum: a slab row holds the fp32 sum of one tile's rows, or of all tiles a persistent workgroup walked
    (stats_acc), in interleaved row sets -- at most M terms in one partial, in some order -- and the rows are folded in fp64 by the caller.  As
    channel_stats with n = M (the tile size differs by kernel; M is valid for all of them):  (M + 1) u sum|y|,  (M + 1) u sum y^2."""
    yd = y.double()
    M = yd.shape[0]
    ref = torch.stack([yd.sum(0), (yd * yd).sum(0)], 1)
    lim = (M + 1) * E32 * torch.stack([yd.abs().sum(0), (yd * yd).sum(0)], 1)
    return Bound(ref, lim * (1.0 + 2.0 ** -20))            # (the fp64 folds of the slab and of this reference: M 2^-52, far inside the margin)


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs shared by the CPU self-test and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------------
def bn_input(M, C, dtype, seed):
    """y [M, C] storage values, gamma, beta [C] fp32.  Channel 0: constant 100.25 (variance ~0: may clamp); channel 1: mean 50, sd 0.01; channel 2:
    gamma = 0, beta = 0 (planted exact zeros: decided); the rest normal draws with a per-channel offset."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(M, C, generator=g) * 1.5 + torch.randn(C, generator=g) * 0.5
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    y[:, 0] = 100.25
    if C > 1:
        y[:, 1] = 50.0 + 0.01 * torch.randn(M, generator=g)
    if C > 2:
        gamma[2], beta[2] = 0.0, 0.0
    return rounded(y, dtype), gamma, beta


def host_slab(y, rows):
    """[rows, C, 2] fp32 partial sums of y [M, C] over `rows` contiguous row ranges (empty ranges give zero rows), summed in fp32 on the host."""
    M, C = y.shape
    edges = [round(i * M / rows) for i in range(rows + 1)]
    part = torch.zeros(rows, C, 2)
    yf = y.float()
    for i in range(rows):
        blk = yf[edges[i]:edges[i + 1]]
        if blk.shape[0]:
            part[i, :, 0], part[i, :, 1] = blk.sum(0), (blk * blk).sum(0)
    return part


def emu_bnp(part, n, gamma, beta, eps):
    """bn_finalize_kernel in its own arithmetic: fp64 fold and variance, then fp32.  -> [4, C] fp32"""
    s = part.double().sum(0)
    mean = s[:, 0] / n
    var = (s[:, 1] / n - mean * mean).clamp(min=0)
    rstd = (1.0 / torch.sqrt(var + f32(eps))).float()
    sc = gamma.float() * rstd
    return torch.stack([mean.float(), rstd, sc, beta.float() - mean.float() * sc]), var


def emu_fma(a, b, c):
    """fmaf on fp32 tensors: the product of two floats is exact in fp64; the sum rounds to fp64 and then to fp32 (a double rounding that can differ
    from fmaf in the last bit of rare cases: an emulation, inside the limits like the kernel)."""
    return (a.double() * b.double() + c.double()).float()


def bn_bwd_operands(C, M, dtype, n_grads, relu_mode, seed):
    """-> y [M, C], bnp [4, C] fp32 (the finalize kernel's arithmetic on a one-row slab), res (mode 1 only), the gradients, gamma, beta.  On top of bn_input's
    channels, channel 3 is a planted y == mean with beta = 0: values 0, +1, -1, ... that sum to exactly 0, so mean = 0, shift = 0 and t = 0 at the zeros."""
    y, gamma, beta = bn_input(M, C, dtype, seed)
    if C > 3:
        col = torch.zeros(M)
        k = (M - 1) // 2
        col[M - 2 * k:] = torch.tensor([1.0, -1.0]).repeat(k)
        y[:, 3], beta[3] = col, 0.0
    bnp, _ = emu_bnp(host_slab(y, 1), M, gamma, beta, 1e-5)
    res = draw((M, C), dtype, seed + 1) if relu_mode == 1 else None
    return y, bnp, res, [draw((M, C), dtype, seed + 2 + k) for k in range(n_grads)], gamma, beta


# C, M, storage types, gradients, relu mode, accumulate, the route the case is there for
BN_BWD_CASES = [
    (64, 1, "all", 1, 0, 0, "fast256"), (64, 37, "all", 2, 1, 1, "fast256"), (64, 3000, "all", 3, 2, 0, "fast256"),
    (64, 37, "all", 1, 2, 1, "fast256"), (64, 37, "all", 3, 1, 0, "fast256"),
    (24, 300, "f32", 2, 1, 1, "atomics"), (48, 300, "16", 3, 2, 0, "atomics"), (48, 41, "16", 1, 0, 1, "atomics"), (4096, 5, "bf16", 2, 1, 0, "atomics"),
    (64, 32900, "16", 2, 2, 1, "wide1024"),
]
BN_FROM_PART_ROWS = [1, 256, 257, 4097]


def dtypes_of(kind):
    return {"all": [torch.float32, torch.bfloat16, torch.float16], "16": [torch.bfloat16, torch.float16], "f32": [torch.float32],
            "bf16": [torch.bfloat16], "rln": [torch.float32, torch.bfloat16]}[kind]


def gn_operands(B, HW, C, dtype, with_res, seed):
    g = torch.Generator().manual_seed(seed)
    x = rounded(torch.randn(B, HW, C, generator=g) * 2.0 + 0.5, dtype)
    res = rounded(torch.randn(B, HW, C, generator=g), dtype) if with_res else None
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    dout = rounded(torch.randn(B, HW, C, generator=g), dtype)
    return x, res, gamma, beta, dout


# C, G, HW, activation, residual (the vector path only), the path the case is there for (by C and the storage type; None: whatever gn_path says)
GN_CASES = [
    (64, 16, 63, ACT_RELU, False, "vector"), (64, 64, 65, ACT_ELU, True, "vector"), (64, 16, 1, ACT_NONE, True, "vector"), (64, 16, 10, ACT_ELU, False, "vector"),
    (512, 16, 64, ACT_ELU, True, "vector"), (512, 512, 10, ACT_RELU, False, "vector"), (64, 16, 960, ACT_RELU, True, "vector"),
    (48, 16, 65, ACT_RELU, False, "atomics"), (48, 48, 10, ACT_ELU, False, "atomics"), (96, 16, 960, ACT_ELU, False, "atomics"), (96, 16, 1, ACT_NONE, False, "atomics"),
    (768, 16, 63, ACT_ELU, False, "slots"), (768, 768, 64, ACT_RELU, False, "slots"), (768, 16, 1, ACT_NONE, False, "slots"),
]


def rln_operands(B, HW, C, Cr, dtype, with_res, n_grads, seed):
    """The padding channels (>= Cr) of y, res and the gradients hold data: it must not leak into the results."""
    g = torch.Generator().manual_seed(seed)
    y = rounded(torch.randn(B, HW, C, generator=g) * 1.5 + torch.randn(B, 1, C, generator=g), dtype)
    res = rounded(torch.randn(B, HW, C, generator=g), dtype) if with_res else None
    gamma, beta = torch.rand(Cr, generator=g) + 0.5, torch.randn(Cr, generator=g) * 0.3
    z = torch.randn(2, B, Cr, generator=g) * 2.0
    grads = [rounded(torch.randn(B, HW, C, generator=g), dtype) for _ in range(n_grads)]
    return y, res, gamma, beta, z, grads


RLN_STDDEV = 0.1
RLN_EPS = 1e-3
# C, Cr, HW, train, stddev, residual, relu, gradients
RLN_CASES = [
    (64, 61, 2, 1, RLN_STDDEV, False, False, 1), (64, 61, 63, 1, RLN_STDDEV, True, True, 2), (64, 61, 64, 0, RLN_STDDEV, False, True, 3),
    (64, 61, 200, 1, 0.0, True, False, 1), (64, 64, 5000, 1, RLN_STDDEV, True, True, 3),
    (192, 192, 200, 1, RLN_STDDEV, False, True, 2), (192, 190, 63, 0, RLN_STDDEV, True, True, 1),
    (2048, 2048, 64, 1, RLN_STDDEV, True, True, 2), (2048, 2041, 2, 1, RLN_STDDEV, False, False, 1),
]

"""Element-level references for the loss kernels of csrc/photometric.hip (helper, no tests; imported like stream_bounds.py).

conv_bounds.py opens with the argument: a relative L2 over a tensor cannot see one wrong element.  The loss kernels are 1 300 lines of hand-derived VJPs
(SSIM through a reflected 3x3 box filter, L1, min-reprojection and auto-mask selection, bilinear sampling, projection, smoothness, SILog) whose tests
were whole-tensor checks.  A fixed tolerance is the wrong tool for them: `E[x^2] - mu^2` cancels in smooth windows, so the honest limit of an SSIM
value depends on the window, and the same holds for `dn_dmx*dn - n*dd_dmx` and `-(dX*X + dY*Y)` in the gradients.  So the limit is COMPUTED per element:

(a) V, a value-with-error arithmetic over fp64 tensors.  V.val is the exact-arithmetic (fp64) value of an expression, V.err a bound on |the fp32
    value a kernel computes - val|.  Every operation propagates the operand errors (products and quotients with their second-order terms) and adds its
    own rounding r: |fl(x) - x| <= r |x| <= r (|val| + propagated), plus 2^-150 for a subnormal result.  r = u = 2^-24 for + - * and fmaf; division and
    sqrt are correctly rounded (hipcc default, as stream_bounds.py notes): u; v_rcp_f32, expf and logf are 1 ulp = 2 u (the HIP math table figures
    conv_bounds.py and stream_bounds.py quote).  `x * y + z` is ONE rounding only where the kernel writes fmaf (the projection chain); under
    `#pragma clang fp contract(fast)` either count is admissible and the looser -- two roundings -- is taken.  An n-term fp32 sum in any order:
    gamma_(n-1) sum (|term| + its error) (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 4.4).  A literal such as 1.0f / 9.0f
    carries |1/9 - fp32(1/9)| as its error (V.c), a kernel argument that already is an fp32 value none (V.k).  No constant is fitted to a run.
    F32 is the same interface over fp32 tensors: every operation rounds.  The kernels' operation sequences below are written ONCE against that interface;
    run with V they give the limit, run with F32 they are the fp32 emulation tests/test_photo_bounds.py holds against the limit (and plants faults in).

(b) The VALUE of a reference never comes from those sequences: forward values are the oracle's formulas (oracle/losses.py, oracle/geometry.py) in
    fp64, gradients are fp64 autograd through them; V.err alone is used, as the limit.  tests/test_photo_bounds.py asserts that V.val -- the hand-derived
    VJP in exact arithmetic -- agrees with autograd to 1e-10 relative: the kernel's formula is the derivative and the restatement is right.

(c) Operands as the kernel reads them.  sde_photo_bwd reads the stored `sampled` and `sel`; the tests hand it the fp64 sample rounded to fp32 and the
    reference's arg-min, so the backward is tested in isolation: its reference is d/d(depth, pose) of <dL/dS, S(depth, pose)> with dL/dS taken at the
    stored S (two autograd stages), the sign of `sampled - A` is exact and no arg-min tie enters.  The projection is recomputed in the kernel; its
    discrete decisions -- the tap cell floor(ix), floor(iy), passx / passy, the zero-padding flags -- are bit-exact by this project's contract
    (tests/test_gpu_photometric.py) and are taken from the fp32 chain (F32 run of project(), asserted equal to oracle.geometry's on the CPU); the
    continuous quantities come from the fp64 chain with V's error.

(d) Undecided elements (as conv_bounds.DeconvCase.undecided for the step function), computed from the reference alone:
      forward sel          the two smallest maps lie within the sum of their limits (or a map within its limit of its clip threshold): either code is
                           accepted.  Cap 2 % of the pixels.
      photometric d_depth  the fp64 X or Y lies within its error of 0, W-1 / H-1 or an integer, or a window's SSIM distance within its error of the
                           clamp at 0 or 1: left out (the fp64 autograd took another branch than the fp32 chain may).  Cap 1 %.  The per-workgroup pose
                           partials need every pixel: for the pixels left out their reference is autograd through the sample function with the fp32
                           chain's decisions (photo_ref_sample(dec=)); a clamp the reference cannot decide leaves the window's coefficients at their
                           value or 0, and the difference enters the limit.
      smoothness d_depth   a neighbour difference v within its error of 0, not being exactly 0 in both precisions (equal depths): left out, cap 1 %;
                           its possible jump 2 wt / N is carried into the error of every sum that contains it (s_part, and through S every d_depth).

SDE_BOUNDS_LOG: every assertion goes through conv_bounds' record; `share` lines record the part left out per case.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

import conv_bounds as CB
from conv_bounds import E32, Bound, assert_within, _record      # noqa: F401  (re-exported to the tests)
from stream_bounds import GUARD, guarded, assert_guards, assert_equal, f32      # noqa: F401
from oracle import geometry as G, losses as OL

U = E32
D53 = 2.0 ** -53
SUB = 2.0 ** -150
F64 = torch.float64
FT = (14, 30)          # pixels a forward workgroup owns (FT_H - 2, FT_W - 2)
BT = (12, 28)          # pixels a backward workgroup owns (BT_H - 4, BT_W - 4)
SM_CHUNKS = 32
EPS = f32(1e-6)        # kEps, and the 1e-6f of the smoothness clamps


def _t(v):
    return v if torch.is_tensor(v) else torch.tensor(float(v), dtype=F64)


# ---------------------------------------------------------------------------------------------------------------------------------------
# (a) the two arithmetics
# ---------------------------------------------------------------------------------------------------------------------------------------
class V:
    """val: fp64 tensor; err: bound on |fp32 computation - val| (fp64, >= 0)."""
    __slots__ = ("val", "err")
    exact = False

    def __init__(self, val, err=None):
        self.val = _t(val).to(F64)
        self.err = torch.zeros_like(self.val) if err is None else _t(err).to(F64)

    @classmethod
    def inp(cls, t):
        """a stored fp32 operand: exact"""
        return cls(t.detach().double())

    @classmethod
    def k(cls, x):
        """a kernel argument or an integer: the fp32 value itself"""
        return cls(f32(x))

    @classmethod
    def c(cls, x):
        """a literal the kernel holds in fp32 where the reference holds the real number"""
        return cls(float(x), abs(float(x) - f32(x)))

    @classmethod
    def lift(cls, o):
        return o if isinstance(o, cls) else cls.c(o)

    @staticmethod
    def _rnd(val, prop, r):
        return V(val, prop * (1.0 + r) + r * val.abs() + (SUB if r else 0.0))

    def add(self, o, r=U):
        o = V.lift(o)
        return V._rnd(self.val + o.val, self.err + o.err, r)

    def sub(self, o, r=U):
        o = V.lift(o)
        return V._rnd(self.val - o.val, self.err + o.err, r)

    def _mulprop(self, o):
        return self.val.abs() * o.err + o.val.abs() * self.err + self.err * o.err

    def mul(self, o, r=U):
        o = V.lift(o)
        return V._rnd(self.val * o.val, self._mulprop(o), r)

    def fma(self, b, c):
        """fmaf(self, b, c): one rounding"""
        b, c = V.lift(b), V.lift(c)
        return V._rnd(self.val * b.val + c.val, self._mulprop(b) + c.err, U)

    def div(self, o, r=U):
        o = V.lift(o)
        q = self.val / o.val
        room = o.val.abs() - o.err                           # |computed denominator| >= room
        prop = torch.where(room > 0, (self.err + q.abs() * o.err) / room.clamp(min=1e-300), torch.full_like(q, float("inf")))
        prop = torch.where((self.err == 0) & (o.err == 0), torch.zeros_like(prop), prop)
        return V._rnd(q, prop, r)

    def rcp(self):
        """v_rcp_f32: 1 ulp"""
        return V.k(1.0).div(self, r=2.0 * U)

    def exp(self):
        v = torch.exp(self.val)
        return V._rnd(v, v * torch.expm1(self.err), 2.0 * U)

    def log(self):
        rel = (self.err / self.val.abs()).clamp(max=1.0 - 1e-12)
        return V._rnd(torch.log(self.val), -torch.log1p(-rel), 2.0 * U)

    def sqrt(self, r=U):
        v = torch.sqrt(self.val)
        return V._rnd(v, v - torch.sqrt((self.val - self.err).clamp(min=0.0)), r)      # concave: the lower side moves further

    def rnd(self, r=U):
        """one more rounding (a conversion to fp32)"""
        return V._rnd(self.val, self.err, r)

    def abs(self):
        return V(self.val.abs(), self.err)

    def scale(self, k):
        """times an exact factor that costs no rounding: a power of two, 0, +-1 (number or tensor)"""
        k = _t(k).to(F64)
        return V(self.val * k, self.err * k.abs())

    def minimum(self, o):
        o = V.lift(o)
        return V(torch.minimum(self.val, o.val), torch.maximum(self.err, o.err) + 0.0 * self.val)      # 1-Lipschitz in both

    def maximum(self, o):
        o = V.lift(o)
        return V(torch.maximum(self.val, o.val), torch.maximum(self.err, o.err) + 0.0 * self.val)

    def map(self, fn):
        """data movement (slicing, padding with zeros, reflection, gather): the same on both parts"""
        return V(fn(self.val), fn(self.err))

    def widen(self, extra):
        return V(self.val, self.err + extra)

    @staticmethod
    def where(cond, a, b):
        a, b = V.lift(a), V.lift(b)
        return V(torch.where(cond, a.val, b.val), torch.where(cond, a.err, b.err))

    def sumdim(self, dim, n=None, r=U):
        """fp32 sum of n terms along dim in any order (n: number or tensor of the result's shape; default the dimension's length)"""
        n = _t(self.val.shape[dim] if n is None else n).to(F64)
        nm1 = (n - 1.0).clamp(min=0.0)
        gam = nm1 * r / (1.0 - nm1 * r)
        return V(self.val.sum(dim), self.err.sum(dim) + gam * (self.val.abs() + self.err).sum(dim) + SUB)

    @classmethod
    def sum(cls, terms, n=None):
        return cls.stack(terms).sumdim(0, n)

    @classmethod
    def stack(cls, terms, dim=0):
        terms = [cls.lift(t) for t in terms]
        vs = torch.broadcast_tensors(*[t.val for t in terms])
        es = torch.broadcast_tensors(*[t.err + 0.0 * t.val for t in terms] + [vs[0]])[:-1]
        return cls(torch.stack(vs, dim), torch.stack(es, dim))

    def segsum(self, idx, nseg, n):
        """out[s] = sum of the elements with idx == s (1-D), n[s] of them"""
        z = torch.zeros(nseg, dtype=F64)
        nm1 = (n.double() - 1.0).clamp(min=0.0)
        gam = nm1 * U / (1.0 - nm1 * U)
        return V(z.index_add(0, idx, self.val), z.index_add(0, idx, self.err) + gam * z.index_add(0, idx, self.val.abs() + self.err) + SUB)

    def __getitem__(self, i):
        return self.map(lambda t: t[i])

    def __neg__(self):
        return V(-self.val, self.err)

    __add__ = add
    __radd__ = add
    __sub__ = sub
    __mul__ = mul
    __rmul__ = mul
    __truediv__ = div

    def __rsub__(self, o):
        return V.lift(o).sub(self)

    def __rtruediv__(self, o):
        return V.lift(o).div(self)


class F32:
    """The same interface in fp32: every operation rounds once (torch CPU), sums run in the order written."""
    __slots__ = ("val",)
    exact = True

    def __init__(self, val):
        self.val = _t(val).to(torch.float32)

    inp = classmethod(lambda cls, t: cls(t.detach().float()))
    k = classmethod(lambda cls, x: cls(float(x)))
    c = classmethod(lambda cls, x: cls(float(x)))
    lift = classmethod(lambda cls, o: o if isinstance(o, cls) else cls(float(o)))

    def add(self, o): return F32(self.val + F32.lift(o).val)
    def sub(self, o): return F32(self.val - F32.lift(o).val)
    def mul(self, o): return F32(self.val * F32.lift(o).val)
    def div(self, o): return F32(self.val / F32.lift(o).val)
    def fma(self, b, c): return F32((self.val.double() * F32.lift(b).val.double() + F32.lift(c).val.double()).float())      # oracle.geometry.fma32
    def rcp(self): return F32(1.0 / self.val)
    def exp(self): return F32(torch.exp(self.val))
    def log(self): return F32(torch.log(self.val))
    def sqrt(self): return F32(torch.from_numpy(np.sqrt(self.val.numpy())))      # (numpy rounds correctly; torch's vectorised CPU sqrt is off by up to 0.52 ulp)
    def abs(self): return F32(self.val.abs())
    def scale(self, k): return F32(self.val * _t(k).to(torch.float32))
    def minimum(self, o): return F32(torch.minimum(self.val, F32.lift(o).val))
    def maximum(self, o): return F32(torch.maximum(self.val, F32.lift(o).val))
    def map(self, fn): return F32(fn(self.val))
    def widen(self, extra): return self
    def sumdim(self, dim, n=None): return F32(self.val.sum(dim))

    @staticmethod
    def where(cond, a, b):
        return F32(torch.where(cond, F32.lift(a).val, F32.lift(b).val))

    @classmethod
    def sum(cls, terms, n=None):
        terms = [cls.lift(t) for t in terms]
        s = terms[0].val
        for t in terms[1:]:
            s = s + t.val
        return cls(s)

    @classmethod
    def stack(cls, terms, dim=0):
        return cls(torch.stack(torch.broadcast_tensors(*[cls.lift(t).val for t in terms]), dim))

    def segsum(self, idx, nseg, n):
        return F32(torch.zeros(nseg).index_add(0, idx, self.val))

    def __getitem__(self, i): return F32(self.val[i])
    def __neg__(self): return F32(-self.val)
    __add__ = add
    __radd__ = add
    __sub__ = sub
    __mul__ = mul
    __rmul__ = mul
    __truediv__ = div
    def __rsub__(self, o): return F32.lift(o).sub(self)
    def __rtruediv__(self, o): return F32.lift(o).div(self)


def bound(ref, v, skip=None):
    """Bound: the reference VALUE `ref` with V's error as the limit (infinite where `skip`)."""
    lim = torch.nan_to_num(v.err + 0.0 * v.val, nan=float("inf"))      # (inf - inf where a worst-case denominator reaches zero: no limit)
    if skip is not None:
        lim = torch.where(skip, torch.full_like(lim, float("inf")), lim)
    return Bound(ref.detach().double(), lim)


def check(got, b, name, left_out=False):
    """assert_within on the per-element limit alone (fp32 results).  left_out: the bound may leave elements out (an infinite limit: the undecided ones,
    counted against their cap); every other bound must hold a finite limit for every element."""
    assert left_out or bool(torch.isfinite(b.lim).all()), f"{name}: {int((~torch.isfinite(b.lim)).sum())} elements have no finite limit"
    got = got.detach().cpu().double().reshape(b.ref.shape)
    got = torch.where(torch.isinf(b.lim), b.ref, got)
    return assert_within(got, b, torch.float32, name, l2_tol=float("inf"))


def power(b):
    """How much a bound can see, from the reference alone: among the elements with a non-zero reference and a finite limit, the share whose limit exceeds
    the value itself (a dropped or sign-flipped element passes there) and the share whose limit exceeds a tenth of it."""
    m = torch.isfinite(b.lim) & (b.ref != 0)
    r = b.lim[m] / b.ref[m].abs()
    return float((r > 1.0).double().mean()), float((r > 0.1).double().mean()), float(r.median())


def check_sel(got, fwd, name):
    """the stored selection code: the reference's wherever the reference decides it; elsewhere one of the candidates the reference cannot tell apart (min:
    the arg-min or the runner-up, each as its index or 254; mean: the undecided clip bits free, the others fixed)"""
    got, ref = got.detach().cpu().to(torch.uint8), fwd["sel"]
    ok = (got.unsqueeze(0) == fwd["sel_alt"]).any(0) | ((((got.long() ^ ref.long()) & ~fwd["sel_free"]) == 0) & (fwd["sel_free"] > 0))
    assert bool(((fwd["sel_alt"] != ref) | (fwd["sel_free"] > 0).unsqueeze(0)).any(0).le(fwd["und_sel"]).all()), "alternatives only on undecided pixels"
    _record(torch.float32, name, 0.0 if bool(ok.all()) else float("inf"))
    assert bool(ok.all()), f"{name}: {int((~ok).sum())} pixels hold a code the reference excludes; first at {tuple(int(v) for v in (~ok).nonzero()[0])}"


def record_note(text):
    path = os.environ.get("SDE_BOUNDS_LOG")
    if path:
        with open(path, "a") as f:
            f.write(text + "\n")


def record_share(name, share, cap):
    record_note(f"share {name} {share:.5f} (cap {cap})")
    assert share <= cap, f"{name}: {share:.4%} of the elements are undecided, more than the cap of {cap:.0%}"


def vjp_agrees(v, ref, name, skip=None, tol=1e-10):
    """(b): the hand-derived formula in exact arithmetic is the autograd result."""
    d = (v.val - ref.detach().double()).abs()
    if skip is not None:
        d = torch.where(skip, torch.zeros_like(d), d)
    scale = float(ref.detach().abs().max()) + 1e-300
    assert float(d.max()) <= tol * scale, f"{name}: formula and autograd differ by {float(d.max()):.3e} at a scale of {scale:.3e}"


# ---------------------------------------------------------------------------------------------------------------------------------------
# shared pieces: the reflected 3x3 box sums, the workgroup tile sums
# ---------------------------------------------------------------------------------------------------------------------------------------
def _reflect1(t):
    s = t.shape
    return F.pad(t.reshape(1, -1, s[-2], s[-1]), (1, 1, 1, 1), mode="reflect").reshape(*s[:-2], s[-2] + 2, s[-1] + 2)


def _zero1(t):
    return F.pad(t, (1, 1, 1, 1))


def box9(A, t):
    """sum over the 3 x 3 window of ReflectionPad2d(1), rows then columns as the kernels' loops run"""
    H, W = t.val.shape[-2:]
    p = t.map(_reflect1)
    return A.sum([p[..., dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])


def tile_sum(A, t, th, tw, halo=0):
    """t [B, h, w] -> [B * gdy * gdx] per-workgroup sums, block index (b * gdy + by) * gdx + bx.  A workgroup has (tw + 2 halo) x (th + 2 halo) threads, x
    fastest; the threads outside the owned th x tw pixels add 0.  F32 follows sde_block_sum: sde_wave_sum's DPP steps pair lanes, quads, half rows, rows and
    the four rows -- a balanced binary tree over the 64 lanes -- then the waves are added in order."""
    B, h, w = t.val.shape
    gy, gx = -(-h // th), -(-w // tw)
    p = t.map(lambda v: F.pad(v, (0, gx * tw - w, 0, gy * th - h)).reshape(B, gy, th, gx, tw).permute(0, 1, 3, 2, 4))      # [B, gy, gx, th, tw]
    if A.exact:
        v = F.pad(p.val, (halo, halo, halo, halo)).reshape(B, gy, gx, -1, 64)
        while v.shape[-1] > 1:
            v = v[..., 0::2] + v[..., 1::2]
        return A.sum([A(v[..., i, 0]) for i in range(v.shape[-2])]).map(lambda q: q.reshape(-1))
    rows = (torch.tensor([min(th, h - i * th) for i in range(gy)]).view(gy, 1) * torch.tensor([min(tw, w - i * tw) for i in range(gx)]).view(1, gx))
    return p.map(lambda v: v.reshape(B, gy, gx, th * tw)).sumdim(3, n=rows.double().expand(B, gy, gx)).map(lambda v: v.reshape(-1))


def ref_tile_sum(t, th, tw):
    return tile_sum(V, V(t.detach()), th, tw).val


# ---------------------------------------------------------------------------------------------------------------------------------------
# SSIM distance (ssim_from_moments, ssim_map_kernel, ssim_bwd_gather_kernel)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _win(t):
    """[9, ..., H, W]: the nine taps of every reflected window"""
    H, W = t.shape[-2:]
    p = _reflect1(t)
    return torch.stack([p[..., dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])


def central(A, a, b):
    """E[a b] - E[a] E[b] over the reflected 3 x 3 window as the kernels form it: (sum a b) * inv9 - (sum a * inv9) * (sum b * inv9).
    With V the two terms are NOT treated as independent (their operand errors cancel exactly as the operands do): the error is
      R  the roundings of the fp32 evaluation, bounded on the magnitudes |a| + err, |b| + err (sums and products of non-negative numbers: the bound is
         monotone in them), plus the last subtraction's u max(term);
      P  the change of the exact central moment (1/9) sum (a_i - ma)(b_i - mb) under |da_i| <= ea_i, |db_i| <= eb_i:
         (1/9) sum [(ea_i + mean ea) |b_i - mb| + (eb_i + mean eb) |a_i - ma| + (ea_i + mean ea)(eb_i + mean eb)]   (all orders)."""
    inv9 = A.c(1.0 / 9.0)
    if A.exact:
        return box9(A, a * b) * inv9 - (box9(A, a) * inv9) * (box9(A, b) * inv9)
    am, bm = V(a.val.abs() + a.err), V(b.val.abs() + b.err)
    t1, t2 = box9(V, am * bm) * inv9, (box9(V, am) * inv9) * (box9(V, bm) * inv9)
    R = t1.err + t2.err + U * (t1.val + t1.err) + SUB
    wa, wb, ea, eb = _win(a.val), _win(b.val), _win(a.err + 0.0 * a.val), _win(b.err + 0.0 * b.val)
    ma, mb = wa.mean(0), wb.mean(0)
    ea, eb = ea + ea.mean(0), eb + eb.mean(0)
    P = (ea * (wb - mb).abs() + eb * (wa - ma).abs() + ea * eb).mean(0)
    return V((wa * wb).mean(0) - ma * mb, R + P)


def _ssim_chain(A, x, y, C1, C2):
    inv9 = A.c(1.0 / 9.0)
    mx, my = box9(A, x) * inv9, box9(A, y) * inv9
    mxy, mxx, myy = mx * my, mx * mx, my * my
    vx, vy, vxy = central(A, x, x), central(A, y, y), central(A, x, y)
    n = (mxy.scale(2.0) + C1) * (vxy.scale(2.0) + C2)
    d = (mxx + myy + C1) * (vx + vy + C2)
    return (1.0 - n * d.rcp()).scale(0.5).maximum(0.0).minimum(1.0)


def ssim_fwd(A, x, y, C1, C2):
    """ssim_from_moments on the nine-tap sums.  x, y: A-values [..., H, W] -> the distance map.
    With V and operands that carry an error (the samples the forward kernel has just formed) the numerator and the denominator are not independent either:
    SSIM of nearly equal windows moves little when both move.  So the error is split as fl f(x~) - f(x) = [fl f(x~) - f(x~)] + [f(x~) - f(x)]:
      the roundings of the evaluation, from the chain on the exact operands (the change of that bound between x and x~ is of order u * err: dropped, like
      every second-order term of a rounding), and
      the mean-value bound sum_i sup |df / dx_i| err_i over the nine taps, with the gradient -- the coefficients of ssim_coef, the clamp left out since
      it is 1-Lipschitz -- enclosed over the error box by V itself (|val| + err of the coefficient expression evaluated on the operands WITH their errors)."""
    C1, C2 = (C1 if isinstance(C1, A) else A.k(C1)), (C2 if isinstance(C2, A) else A.k(C2))
    if A.exact or not (bool((x.err > 0).any()) or bool((y.err > 0).any())):
        return _ssim_chain(A, x, y, C1, C2)
    out = _ssim_chain(V, V(x.val), V(y.val), C1, C2)
    cAx, cAy, cB, cC, _ = ssim_coef(V, x, y, V.c(-0.5 / 9.0), C1, C2, True, clamp=False)
    wx, wy = x.map(_win), y.map(_win)
    sens = lambda cA, a, b: (cA + a.scale(2.0) * cB) + b * cC      # noqa: E731
    sx, sy = sens(cAx, wx, wy), sens(cAy, wy, wx)
    P = ((sx.val.abs() + sx.err) * wx.err + (sy.val.abs() + sy.err) * wy.err).sum(0)
    return out.widen(P)


def ssim_coef(A, x, y, f, C1, C2, both, clamp=True):
    """The per-window coefficients of ssim_map_kernel / photo_bwd_body.  f: d out / d SSIM folded with the 1/9 of the box filter, per window.
    -> (cAx, cAy | None, cB, cC, undecided windows): zero where the clamp does not pass the gradient.  The second moments enter through central(): the
    same fp32 operations, and with V an error in which a window's operand errors cancel as the operands do (what ssim_fwd's gradient enclosure needs)."""
    inv9 = A.c(1.0 / 9.0)
    mx, my = box9(A, x) * inv9, box9(A, y) * inv9
    n1, n2 = (mx.scale(2.0) * my) + C1, central(A, x, y).scale(2.0) + C2          # exy - mx my, (exx - mx mx) + (eyy - my my): the same operations
    d1, d2 = (mx * mx + my * my) + C1, (central(A, x, x) + central(A, y, y)) + C2
    n, dn = n1 * n2, d1 * d2
    rdn = dn.rcp()
    l = (1.0 - n * rdn).scale(0.5)
    ok = ((l.val >= 0) & (l.val <= 1)) if clamp else torch.ones_like(l.val, dtype=torch.bool)
    und = torch.zeros_like(ok) if A.exact else ((l.val.abs() <= l.err) | ((l.val - 1.0).abs() <= l.err))
    r2 = rdn * rdn
    dd = (d2 - d1).scale(2.0)
    cAx = f * ((my.scale(2.0) * (n2 - n1)) * dn - (n * dd) * mx) * r2
    cAy = f * ((mx.scale(2.0) * (n2 - n1)) * dn - (n * dd) * my) * r2 if both else None
    cB = f * ((-n) * d1) * r2
    cC = f * n1.scale(2.0) * rdn
    # (a window whose clamp the reference cannot decide has the coefficient or 0: the difference is carried as error into every sum that contains it)
    z = lambda c: None if c is None else A.where(ok, c, 0.0).widen(0.0 if (A.exact or not clamp) else und.double() * (c.val.abs() + c.err))      # noqa: E731
    return z(cAx), z(cAy), z(cB), z(cC), und


def refl_mult(n, fault=None):
    """m[i, e]: how often pixel i occurs in the reflected window centred at i + e - 1 (0 where that window does not exist)"""
    m = torch.ones(n, 3, dtype=F64)
    i = torch.arange(n)
    m[:, 0] = torch.where(i == 1, 2.0, 1.0) * (i - 1 >= 0)
    m[:, 2] = torch.where(i == n - 2, 2.0, 1.0) * (i + 1 < n)
    if fault == "refl_mult":
        m[n - 2, 2] = 1.0
    return m


def ssim_gather(A, cA, cB, cC, xv, ov, fault=None):
    """every pixel gathers the up to nine windows that contain it: sum m (cA + 2 x cB + o cC) -- the gradient to x (o: the other image)"""
    H, W = xv.val.shape[-2:]
    my_, mx_ = refl_mult(H, fault), refl_mult(W)
    pA, pB, pC = cA.map(_zero1), cB.map(_zero1), cC.map(_zero1)
    terms = []
    for ey in range(3):
        for ex in range(3):
            s = (Ellipsis, slice(ey, ey + H), slice(ex, ex + W))
            m = my_[:, ey].view(H, 1) * mx_[:, ex].view(1, W)
            if fault == "refl_corners" and ey != 1:      # the row multiplicity 1 instead of 2 at the four pixels (1 | H-2, 1 | W-2) only
                m = m.clone()
                r = 1 if ey == 0 else H - 2
                m[r, 1], m[r, W - 2] = m[r, 1] / 2.0, m[r, W - 2] / 2.0
            if fault == "seam_halo" and ex == 2:
                m = m.clone()
                m[:, 27] = 0.0
            terms.append(((pA[s] + xv.scale(2.0) * pB[s]) + ov * pC[s]).scale(m))
    return A.sum(terms)


def ssim_bwd(A, x, y, gout, C1, C2):
    """sde_ssim_bwd -> (dx, dy, undecided pixels)"""
    xa, ya = A.inp(x), A.inp(y)
    f = A.inp(gout).scale(-0.5) * A.c(1.0 / 9.0)
    cAx, cAy, cB, cC, und = ssim_coef(A, xa, ya, f, A.k(C1), A.k(C2), True)
    und = F.max_pool2d(und.double().reshape(1, -1, *und.shape[-2:]), 3, 1, 1).reshape(und.shape) > 0
    return ssim_gather(A, cAx, cB, cC, xa, ya), ssim_gather(A, cAy, cB, cC, ya, xa), und


def ssim_case(x, y, gout, C1=1e-4, C2=9e-4):
    """{"map", "dx", "dy"} -> Bound, "share": the part of the gradient elements left out"""
    C1, C2 = f32(C1), f32(C2)
    xr, yr = x.double().requires_grad_(True), y.double().requires_grad_(True)
    ref = OL.ssim_distance(xr, yr, C1, C2)
    ref.backward(gout.double())
    vm = ssim_fwd(V, V.inp(x), V.inp(y), C1, C2)
    vdx, vdy, und = ssim_bwd(V, x, y, gout, C1, C2)
    return {"map": bound(ref, vm), "dx": bound(xr.grad, vdx, und), "dy": bound(yr.grad, vdy, und), "share": float(und.double().mean()),
            "v": (vm, vdx, vdy), "und": und, "ref": (ref.detach(), xr.grad, yr.grad)}


def ssim_inputs(B, C, h, w):
    """the inputs of test_gpu_photometric.test_ssim_module_stand_alone"""
    g = torch.Generator().manual_seed(B * 100 + h)
    x = torch.rand(B, C, h, w, generator=g)
    y = (x + 0.15 * torch.randn(B, C, h, w, generator=g)).clamp(0, 1)
    return x, y, torch.rand(B, C, h, w, generator=g)


SSIM_SHAPES = [(2, 3, 48, 160), (1, 3, 37, 53), (2, 1, 2, 2), (1, 2, 5, 130)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# SILog (silog_multi_fwd_kernel, silog_multi_finalize_kernel, silog_multi_bwd_kernel with one scale)
# ---------------------------------------------------------------------------------------------------------------------------------------
def silog_blocks(B, h, w):
    n = B * h * w
    return min(max((n + 1023) // 1024, 1), 1024)


def silog_nearest(gt, h, w):
    """gt [B, 1, H, W] -> [B, 1, h, w] by the kernel's index arithmetic (fp32 product, floor, clamp) = oracle.geometry.resize_nearest"""
    H, W = gt.shape[-2:]
    ys = (torch.arange(h, dtype=torch.float32) * torch.tensor(H / h, dtype=torch.float32)).floor().long()
    xs = (torch.arange(w, dtype=torch.float32) * torch.tensor(W / w, dtype=torch.float32)).floor().long()
    ys, xs = ys.clamp(max=H - 1), xs.clamp(max=W - 1)
    return gt[:, :, ys][:, :, :, xs]


def silog_fwd(A, est, gtn, fault=None):
    """est, gtn [B, 1, h, w] -> (mask, part [nb, 3] as three A-values: count, sum d, sum d^2)"""
    e, g = est.reshape(-1), gtn.reshape(-1)
    mask = (g >= 1.0) if fault == "silog_mask" else (g > 1.0)
    one = torch.ones_like(e)
    d = A.where(mask, A.inp(torch.where(mask, e, one)).log() - A.inp(torch.where(mask, g, one)).log(), 0.0)
    nb = silog_blocks(*est.shape[0:1], *est.shape[2:])
    blk = (torch.arange(e.numel()) // 256) % nb
    cnt = torch.zeros(nb, dtype=F64).index_add(0, blk, mask.double())
    return mask, cnt, d.segsum(blk, nb, cnt), (d * d).segsum(blk, nb, cnt)


def silog_finalize_v(cnt, s1, s2, vf):
    """fp64 sums of the fp32 partials, fp64 arithmetic, one conversion to fp32 each -> V of (mean d, mean d^2, loss)"""
    c = V(cnt.sum())
    S1, S2 = s1.sumdim(0, r=D53), s2.sumdim(0, r=D53)
    m1, m2 = S1.div(c, r=D53), S2.div(c, r=D53)
    loss = m2.sub(m1.mul(m1, r=D53).mul(V.k(vf), r=D53), r=D53).sqrt(r=D53).mul(V.k(10.0), r=D53)
    return m1.rnd(), m2.rnd(), loss.rnd()


def silog_finalize_emu(cnt, s1, s2, vf):
    c, S1, S2 = cnt.double().sum(), s1.double().sum(), s2.double().sum()
    m1, m2 = S1 / c, S2 / c
    return torch.stack([c, m1, m2, torch.sqrt(m2 - float(f32(vf)) * m1 * m1) * 10.0]).float()


def silog_bwd(A, est, gtn, stats, gout, gscale, vf, fault=None):
    """stats: (count, mean d, loss) as A-values (what the kernel reads back) -> d_est [B, 1, h, w]"""
    cnt, m1, loss = stats
    mask = (gtn >= 1.0) if fault == "silog_mask" else (gtn > 1.0)
    one = torch.ones_like(est)
    e = A.inp(torch.where(mask, est, one))
    d = e.log() - A.inp(torch.where(mask, gtn, one)).log()
    g = A.k(gout) * A.k(gscale)
    kk = A.k(100.0) / (loss * cnt)
    return A.where(mask, ((g * kk) * (d - A.k(vf) * m1)) / e, 0.0)


def silog_case(est, gt, gout=0.7, gscale=1.0, vf=0.85):
    """est [B, 1, h, w], gt [B, 1, H, W] -> bounds of part, stats, d_est (d_est with the reference's stats, rounded to fp32, as operand)"""
    B, _, h, w = est.shape
    gtn = silog_nearest(gt, h, w)
    assert torch.equal(gtn, G.resize_nearest(gt, (h, w)))
    vf = f32(vf)
    er = est.double().requires_grad_(True)
    lref = OL.silog(er, gtn.double(), vf)
    (lref * f32(gout) * f32(gscale)).backward()
    mask, cnt, s1, s2 = silog_fwd(V, est, gtn)
    dref = torch.where(mask, (torch.log(est.double()) - torch.log(gtn.double().clamp(min=0.5))).reshape(-1), torch.zeros(1, dtype=F64))
    nb = cnt.numel()
    blk = (torch.arange(dref.numel()) // 256) % nb
    z = torch.zeros(nb, dtype=F64)
    m1, m2, loss = silog_finalize_v(cnt, s1, s2, vf)
    c = cnt.sum()
    m1r, m2r = dref.sum() / c, (dref * dref).sum() / c
    stats_ref = torch.stack([c, m1r, m2r, lref.detach()])
    stats_in = stats_ref.float()                         # what the isolated backward reads
    sv = (V(c), V(m1r, (stats_in[1].double() - m1r).abs()), V(lref.detach(), (stats_in[3].double() - lref.detach()).abs()))
    vd = silog_bwd(V, est, gtn, sv, gout, gscale, vf)
    return {"gtn": gtn, "mask": mask, "cnt": cnt, "s1": bound(z.index_add(0, blk, dref), s1), "s2": bound(z.index_add(0, blk, dref * dref), s2),
            "stats": Bound(stats_ref, torch.stack([torch.zeros((), dtype=F64), m1.err, m2.err, loss.err])), "stats_in": stats_in,
            "d_est": bound(er.grad, vd), "v": vd, "vstats": (m1, m2, loss)}


def silog_inputs(seed=3):
    """5 x 7 estimates against 12 x 20 ground truth (non-integer ratios 2.4 and 2.857 in fp32), B = 2, ground truth holding exactly 1.0
    (mask off: the comparison is `> 1`) next to values just above it"""
    g = torch.Generator().manual_seed(seed)
    est = torch.rand(2, 1, 5, 7, generator=g) * 60 + 0.3
    gt = torch.where(torch.rand(2, 1, 12, 20, generator=g) < 0.7, torch.rand(2, 1, 12, 20, generator=g) * 79 + 1, torch.zeros(1))
    gt[:, :, ::2, ::3] = 1.0
    gt[:, :, 1::4, 1::6] = 1.0 + 2.0 ** -23
    return est, gt


# ---------------------------------------------------------------------------------------------------------------------------------------
# edge-aware smoothness (smooth_mean_body, smooth_fwd_body, smooth_bwd_body, reduce_partials_kernel)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _padr(t, dim):
    """an anchored-term map [B, h, w-1] / [B, h-1, w] -> ([B, h, w] with the term at its anchor, [B, h, w] with it at the neighbour)"""
    if dim == 2:
        return F.pad(t, (0, 1)), F.pad(t, (1, 0))
    return F.pad(t, (0, 0, 0, 1)), F.pad(t, (0, 0, 1, 0))


def smooth_fwd(A, depth, img, fault=None):
    """depth [B, 1, h, w], img [B, 3, h, w] -> dict of A-values: mean_part [B, 32], dn [B, h, w], loss_part, s_part [nblk], loss; und [B, h, w]"""
    B, _, h, w = depth.shape
    hw = h * w
    assert B * h * w < 2 ** 24
    Dp = depth[:, 0]
    inv = 1.0 / A.inp(Dp).maximum(A.k(EPS))
    per = -(-hw // SM_CHUNKS)
    chunks = inv.map(lambda v: F.pad(v.reshape(B, hw), (0, SM_CHUNKS * per - hw)).reshape(B, SM_CHUNKS, per))
    nch = torch.tensor([max(0, min(per, hw - c * per)) for c in range(SM_CHUNKS)], dtype=F64).expand(B, SM_CHUNKS)
    mean_part = chunks.sumdim(2, n=nch)
    m = mean_part.sumdim(1) / A.k(hw)
    mc = m.maximum(A.k(EPS)).map(lambda v: v.reshape(B, 1, 1))
    nx = 1.0 / A.k(B * h * (w - 1))
    nyn = 1.0 / A.k(B * (h if fault == "smooth_nyn" else h - 1) * w)
    n = inv / mc
    I = A.inp(img)
    gterms, lterms = [], []
    und = torch.zeros(B, h, w, dtype=torch.bool)
    for dim, nrm in ((2, nx), (1, nyn)):
        L = h if dim == 1 else w
        a, b = [slice(None)] * 3, [slice(None)] * 3
        a[dim], b[dim] = slice(0, L - 1), slice(1, L)
        a, b = tuple(a), tuple(b)
        ia, ib = (slice(None),) + a, (slice(None),) + b
        ia, ib = (ia[0], slice(None)) + ia[2:], (ib[0], slice(None)) + ib[2:]
        dI = (I[ia] - I[ib]).abs()                                  # [B, 3, ...]
        e = A.sum([dI[:, 0], dI[:, 1], dI[:, 2]])
        wt = (-(e / 3.0)).exp()
        v = (n[a] - n[b]) * wt
        flat = Dp[a] == Dp[b]                                      # equal depths: n0 - n1 is exactly 0 in fp32 and in fp64
        v = A.where(flat, 0.0, v)
        sg = torch.sign(v.val.double())
        t = wt.scale(sg) * nrm
        if not A.exact:
            u_ = (v.val.abs() <= v.err) & ~flat
            t = t.widen(u_.double() * 2.0 * wt.val * nrm.val)
            ua, ub = _padr(u_, dim)
            und |= ua | ub
        ta, tb = t.map(lambda q: _padr(q, dim)[0]), t.map(lambda q: _padr(q, dim)[1])
        if fault == "smooth_left" and dim == 2:
            tb = tb.scale((torch.arange(w) != 64).double())
        gterms += [ta, -tb]
        lterms.append((v.abs() * nrm).map(lambda q: _padr(q, dim)[0]))
    dn = A.sum(gterms)
    lossp = A.sum(lterms)
    sv = dn * inv
    loss_part, s_part = tile_sum(A, lossp, 4, 64), tile_sum(A, sv, 4, 64)
    return {"mean_part": mean_part, "dn": dn, "loss_part": loss_part, "s_part": s_part, "loss": loss_part.sumdim(0), "und": und, "inv": inv}


def smooth_bwd(A, depth, dn, mean_part, s_part, gout, gscale):
    """the kernel's reading of its forward's buffers -> d_depth [B, 1, h, w]"""
    B, _, h, w = depth.shape
    hw = h * w
    S = s_part.map(lambda v: v.reshape(B, -1)).sumdim(1).map(lambda v: v.reshape(B, 1, 1))
    m = (mean_part.sumdim(1) / A.k(hw)).map(lambda v: v.reshape(B, 1, 1))
    dv = A.inp(depth[:, 0])
    dinv = dn / m - S / ((A.k(hw) * m) * m)
    live = depth[:, 0] > EPS
    dd = A.where(live, (-dinv) / A.where(live, dv * dv, 1.0), 0.0)
    return ((A.k(gout) * A.k(gscale)) * dd).map(lambda v: v.unsqueeze(1))


def _smooth_from_nrm(nrm, image):
    """oracle.losses.smoothness from the normalised inverse depth on (smoothness_loss.py:L60-80)"""
    dgx, dgy = nrm[:, :, :, :-1] - nrm[:, :, :, 1:], nrm[:, :, :-1, :] - nrm[:, :, 1:, :]
    wx = torch.exp(-(image[:, :, :, :-1] - image[:, :, :, 1:]).abs().mean(1, True))
    wy = torch.exp(-(image[:, :, :-1, :] - image[:, :, 1:, :]).abs().mean(1, True))
    return (dgx * wx).abs(), (dgy * wy).abs()


def smooth_case(depth, img, gout=0.7, gscale=1.0):
    B, _, h, w = depth.shape
    dr = depth.double().requires_grad_(True)
    inv = 1.0 / dr.clamp(min=EPS)
    nrm = (inv / inv.mean(2, True).mean(3, True).clamp(min=EPS))
    nl = nrm.detach().requires_grad_(True)
    ax, ay = _smooth_from_nrm(nl, img.double())
    lref = ax.mean() + ay.mean()
    assert abs(float(lref.detach()) - float(OL.smoothness(depth.double(), img.double()))) <= 1e-12 * float(lref.detach())
    dn_ref, = torch.autograd.grad(lref, nl)
    lossp = F.pad(ax, (0, 1)) / ax.numel() + F.pad(ay, (0, 0, 0, 1)) / ay.numel()
    OL.smoothness(dr, img.double()).backward()
    dref = dr.grad * f32(gout) * f32(gscale)
    fw = smooth_fwd(V, depth, img)
    vd = smooth_bwd(V, depth, fw["dn"], fw["mean_part"], fw["s_part"], gout, gscale)
    hw = h * w
    per = -(-hw // SM_CHUNKS)
    invd = inv.detach()[:, 0]
    mp_ref = F.pad(invd.reshape(B, hw), (0, SM_CHUNKS * per - hw)).reshape(B, SM_CHUNKS, per).sum(2)
    und = fw["und"]
    return {"mean_part": bound(mp_ref, fw["mean_part"]), "dn": bound(dn_ref[:, 0], fw["dn"], und),
            "loss_part": bound(ref_tile_sum(lossp[:, 0], 4, 64), fw["loss_part"]), "s_part": bound(ref_tile_sum(dn_ref[:, 0] * invd, 4, 64), fw["s_part"]),
            "loss": bound(lref, fw["loss"]), "d_depth": bound(dref, vd, und.unsqueeze(1)), "share": float(und.double().mean()), "v": (fw, vd), "und": und}


SMOOTH_SHAPES = [(2, 2, 2), (1, 5, 65), (2, 9, 130)]


def smooth_inputs(B, h, w, seed=7):
    """a flat-depth patch (v == 0 exactly) and one depth below the 1e-6 clamp"""
    g = torch.Generator().manual_seed(seed + h)
    img = torch.rand(B, 3, h, w, generator=g)
    depth = torch.rand(B, 1, h, w, generator=g) * 40 + 0.5
    depth[0, 0, :2, :2] = 7.25
    if h * w > 4:
        depth[0, 0, -2:, -3:] = 3.5
        depth[-1, 0, h // 2, w // 2] = 5e-7
    return depth, img


# ---------------------------------------------------------------------------------------------------------------------------------------
# photometric term (photo_fwd_body, photo_bwd_body, reduce_partials_kernel, pose_grad_finalize_multi_kernel)
# ---------------------------------------------------------------------------------------------------------------------------------------
class PhotoCase:
    """One scale's operands, fp32 CPU tensors as the kernels read them."""

    def __init__(self, A, ctx, depth, K, poses, *, sx=1.0, sy=1.0, automask=True, reduce_mean=False, ssim_w=0.85, C1=1e-4, C2=9e-4, thr=None,
                 gout=0.7, gscale=1.0):
        self.A, self.ctx, self.depth, self.K, self.poses = A, list(ctx), depth, K, list(poses)
        self.B, _, self.h, self.w = A.shape
        self.nctx = len(self.ctx)
        self.sx, self.sy, self.automask, self.reduce_mean = f32(sx), f32(sy), bool(automask), bool(reduce_mean)
        self.ssim_w, self.C1, self.C2, self.gout, self.gscale = f32(ssim_w), f32(C1), f32(C2), f32(gout), f32(gscale)
        self.thr = None if thr is None else thr.float()
        self.nmaps = 2 * self.nctx if automask else self.nctx

    def mi(self, j):
        return 2 * j if self.automask else j


def photo_case(B, h, w, seed, nctx=2, **kw):
    """test_gpu_photometric._photo_case, for up to four contexts"""
    from oracle.gen_golden import kitti_K, smooth_images
    g = torch.Generator().manual_seed(seed)
    imgs = smooth_images(g, B, h, w, 1 + nctx)
    D = torch.rand(B, 1, h, w, generator=g) * 30 + 2
    D = F.avg_pool2d(F.pad(D, (2, 2, 2, 2), mode="replicate"), 5, 1)
    base = torch.tensor([[0.05, -0.01, 0.3, 0.002, -0.004, 0.001], [-0.03, 0.02, -0.25, -0.001, 0.003, 0.002], [0.1, 0.0, -0.1, 0.0, 0.01, 0.0]])
    vec = base[torch.arange(B) % 3] * (1.0 + 0.05 * (torch.arange(B) // 3).float().view(B, 1))
    sc = kw.get("sx", 1.0)
    Kfull = kitti_K(B, int(round(h / sc)), int(round(w / sc)))
    poses = [G.pose_vec2mat(vec * s) for s in (1.0, -1.0, 0.5, -0.5)[:nctx]]
    return PhotoCase(imgs[0], imgs[1:], D, Kfull, poses, **kw)


def make_cam(A, K, P, sx, sy):
    """projection.h make_cam: k (scaled intrinsics), ki (its inverse), kr = K R (mul, mul, add: no fma), kt = K t (mul, fma, fma); entries [B, 1, 1]"""
    e = lambda M, r, c: A.inp(M[:, r, c].reshape(-1, 1, 1))      # noqa: E731
    k = [e(K, i // 3, i % 3) for i in range(9)]
    k[0], k[4], k[2], k[5] = k[0] * A.k(sx), k[4] * A.k(sy), k[2] * A.k(sx), k[5] * A.k(sy)
    ki = list(k)
    ki[0], ki[4], ki[2], ki[5] = 1.0 / k[0], 1.0 / k[4], (-k[2]) / k[0], (-k[5]) / k[4]
    kr = [(k[3 * i] * e(P, 0, j) + k[3 * i + 1] * e(P, 1, j)) + k[3 * i + 2] * e(P, 2, j) for i in range(3) for j in range(3)]
    kt = [k[3 * i + 2].fma(e(P, 2, 3), k[3 * i + 1].fma(e(P, 1, 3), k[3 * i] * e(P, 0, 3))) for i in range(3)]
    return {"k": k, "ki": ki, "kr": kr, "kt": kt}


def project(A, cam, depth, dec=None, eps=None):
    """projection.h project + make_taps on every pixel.  dec: the discrete decisions (x0, y0, passx, passy) of the fp32 chain (required with V).
    cam["kt"] may hold per-pixel values [B, h, w] (motion_loss.hip: set_kt).  eps: kEps as an A-value (default: the fp32 number itself, for references
    that use that number; motion_bounds passes V.c(1e-6) since its reference holds the real 1e-6)."""
    B, _, h, w = depth.shape
    d = A.inp(depth[:, 0])
    fx, fy = A.inp(torch.arange(w).float().view(1, 1, w)), A.inp(torch.arange(h).float().view(1, h, 1))
    g0, g1 = fx * d, fy * d
    ki, kr, kt = cam["ki"], cam["kr"], cam["kt"]
    p = [ki[3 * i + 2].fma(d, ki[3 * i + 1].fma(g1, ki[3 * i] * g0)) for i in range(3)]
    q = [kr[3 * i + 2].fma(p[2], kr[3 * i + 1].fma(p[1], kr[3 * i] * p[0])) + kt[i] for i in range(3)]
    den = q[2] + (A.k(EPS) if eps is None else eps)
    X, Y = q[0] / den, q[1] / den
    out = {"p": p, "q": q, "X": X, "Y": Y, "den": den, "fx": fx, "fy": fy}
    for name, c, n in (("x", X, w), ("y", Y, h)):
        cs = c.maximum(0.0).minimum(A.k(n - 1))
        gn = (cs.scale(2.0) / A.k(n - 1)) - 1.0                 # the normalised grid coordinate (store_grid)
        i = (gn + 1.0) * A.k((n - 1) / 2.0)
        out["g" + name] = gn
        if dec is None:
            i0 = torch.floor(i.val)
            ps = torch.isfinite(c.val) & (c.val >= 0) & (c.val <= n - 1)
        else:
            i0, ps = dec[name + "0"].double(), dec["pass" + name]
        wgt = i - A.inp(i0)
        out.update({name + "0": i0.long(), "pass" + name: ps, "w" + name: wgt, "e" + name: 1.0 - wgt, "i" + name: i})
    return out


def undecided_coord(pr, h, w):
    """the fp64 X or Y within its error of 0, W-1 / H-1 or an integer"""
    u = torch.zeros_like(pr["X"].val, dtype=torch.bool)
    for c, i, n in ((pr["X"], pr["ix"], w), (pr["Y"], pr["iy"], h)):
        u |= (c.val.abs() <= c.err) | ((c.val - (n - 1)).abs() <= c.err)
        inside = (c.val > 0) & (c.val < n - 1)
        u |= inside & ((i.val - torch.round(i.val)).abs() <= i.err)
    return u


def tap_values(A, img, pr):
    """the four taps (nw, ne, sw, se) of every channel [B, 3, h, w], zero outside the image"""
    B, C, h, w = img.shape
    x0, y0 = pr["x0"], pr["y0"]
    flat = img.reshape(B, C, h * w)
    out = []
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        yy, xx = y0 + dy, x0 + dx
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        idx = (yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)).view(B, 1, -1).expand(B, C, -1)
        out.append(A.inp(flat.gather(2, idx).view(B, C, h, w) * ok.unsqueeze(1)))
    return out


def bilinear(A, taps, pr):
    u = lambda t: t.map(lambda v: v.unsqueeze(1))      # noqa: E731
    wx, ex, ny, sy = u(pr["wx"]), u(pr["ex"]), u(pr["wy"]), u(pr["ey"])
    nw, ne, sw, se = taps
    return ((nw * (sy * ex) + ne * (sy * wx)) + sw * (ny * ex)) + se * (ny * wx)


def tap_gradient(A, d, wgt):
    """d[0] (1 - w) + d[1] w as the kernel forms it (the weight 1 - w is rounded on its own).  With V the two weights are one quantity: the error of w
    enters through d[1] - d[0], which is exact (tap values are operands), and only the roundings come from the chain."""
    w = wgt.map(lambda v: v.unsqueeze(1))
    if A.exact:
        return d[0] * (1.0 - w) + d[1] * w
    w0 = V(w.val)
    return (d[0] * (1.0 - w0) + d[1] * w0).widen((d[1].val - d[0].val).abs() * (w.err + 0.0 * w.val))


def fp32_decisions(case):
    """per context: the fp32 chain's discrete decisions, = the kernel's by the bit-exactness contract"""
    out = []
    for j in range(case.nctx):
        pr = project(F32, make_cam(F32, case.K, case.poses[j], case.sx, case.sy), case.depth)
        out.append({k: pr[k] for k in ("x0", "y0", "passx", "passy")})
    return out


def photo_fwd(A, case, dec=None, fault=None):
    """-> dict: sampled [nctx] of [B, 3, h, w], maps [nmaps] of [B, h, w], sel [B, h, w] uint8, v (reduced map), partial, loss; V only: und_sel"""
    c = case
    B, h, w = c.B, c.h, c.w
    Aa = A.inp(c.A)
    sampled, prs = [], []
    for j in range(c.nctx):
        pr = project(A, make_cam(A, c.K, c.poses[j], c.sx, c.sy), c.depth, None if dec is None else dec[j])
        sampled.append(bilinear(A, tap_values(A, c.ctx[j], pr), pr))
        prs.append(pr)
    C1, C2, third = A.k(c.C1), A.k(c.C2), A.c(1.0 / 3.0)
    maps, clipped, uclip = [], [], []
    for m in range(2 * c.nctx):
        j, ident = m >> 1, m & 1
        if ident and not c.automask:
            continue
        x = A.inp(c.ctx[j]) if ident else sampled[j]
        if fault == "map_channel" and not ident and j == 1:
            x = A.stack([x[:, 0], x[:, 1], sampled[0][:, 2]], 1)
        ad = (x - Aa).abs()
        l = A.sum([ad[:, 0], ad[:, 1], ad[:, 2]]) * third
        pm = l
        if c.ssim_w > 0:
            s = ssim_fwd(A, x, Aa, C1, C2)
            pm = (A.sum([s[:, 0], s[:, 1], s[:, 2]]) * third) * A.k(c.ssim_w) + l * (1.0 - A.k(c.ssim_w))
        mi = len(maps)
        cl, uc = torch.zeros(B, h, w, dtype=torch.bool), torch.zeros(B, h, w, dtype=torch.bool)
        if c.thr is not None:
            t = float(c.thr[mi])
            cl = pm.val > t
            if not A.exact:
                uc = (pm.val - t).abs() <= pm.err
            pm = pm.minimum(A.k(t))
        maps.append(pm)
        clipped.append(cl)
        uclip.append(uc)
    best, bi = maps[0], torch.zeros(B, h, w, dtype=torch.long)
    for mi in range(1, len(maps)):
        lt = maps[mi].val < best.val
        best, bi = A.where(lt, maps[mi], best), torch.where(lt, torch.full_like(bi, mi), bi)
    clip_bits = sum(cl.long() << mi for mi, cl in enumerate(clipped))
    if c.reduce_mean:
        v = A.sum(maps) * A.c(1.0 / c.nmaps)
        sel = clip_bits if c.thr is not None else torch.full_like(bi, 255)
    else:
        v = best
        sel = torch.where(((clip_bits >> bi) & 1) > 0, torch.full_like(bi, 254), bi)
    out = {"sampled": sampled, "maps": maps, "sel": sel.to(torch.uint8), "v": v, "proj": prs}
    out["partial"] = tile_sum(A, v, *FT, halo=1)
    out["loss"] = out["partial"].sumdim(0) * (A.k(1.0) / A.k(B * h * w))
    if not A.exact:
        # the codes the reference cannot tell apart: `sel_alt` [K, B, h, w] lists every admissible code of the min reduce (the arg-min or, at a tie, the
        # runner-up; each as its index or 254 where its clip is undecided), `sel_free` the bits of the mean reduce's mask that may take either value
        cl, uc = torch.stack(clipped), torch.stack(uclip)
        und = uc.any(0)
        out["sel_free"] = sum(u_.long() << mi for mi, u_ in enumerate(uclip))
        cands = [sel]
        if not c.reduce_mean:
            st = torch.stack([m.val for m in maps]), torch.stack([m.err + 0.0 * m.val for m in maps])
            two = st[0].topk(min(2, len(maps)), 0, largest=False)
            e2 = st[1].gather(0, two.indices)
            tie = ((two.values[1] - two.values[0]) <= (e2[0] + e2[1])) if len(maps) > 1 else torch.zeros(B, h, w, dtype=torch.bool)
            und = tie.clone()
            code = lambda i, c_: torch.where(c_, torch.full_like(i, 254), i)      # noqa: E731
            for rank in range(two.indices.shape[0]):
                i = two.indices[rank]
                valid = tie if rank else torch.ones_like(tie)
                ci, ui = cl.gather(0, i.unsqueeze(0))[0], uc.gather(0, i.unsqueeze(0))[0]
                und |= valid & ui
                cands += [torch.where(valid, code(i, ci), sel), torch.where(valid & ui, code(i, ~ci), sel)]
        out["sel_alt"] = torch.stack(cands).to(torch.uint8)
        out["und_sel"] = und
    return out


def _sample_in_cell(img, ix, iy, x0, y0):
    """oracle.geometry.grid_sample_bilinear_zeros_ac with the tap cell given instead of floored from ix, iy"""
    B, C, H, W = img.shape
    wx, ny = ix - x0.double(), iy - y0.double()
    ex, sy = 1.0 - wx, 1.0 - ny
    flat = img.reshape(B, C, H * W)

    def tap(yy, xx):
        ok = ((xx >= 0) & (xx < W) & (yy >= 0) & (yy < H))
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).view(B, 1, -1).expand(B, C, -1)
        return flat.gather(2, idx).view(B, C, *ix.shape[1:]) * ok.unsqueeze(1).to(img.dtype)
    return (tap(y0, x0) * (sy * ex).unsqueeze(1) + tap(y0, x0 + 1) * (sy * wx).unsqueeze(1) + tap(y0 + 1, x0) * (ny * ex).unsqueeze(1)
            + tap(y0 + 1, x0 + 1) * (ny * wx).unsqueeze(1))


def photo_ref_sample(case, depth, poses, dec=None):
    """oracle.geometry.warp_coords / view_synthesis restated for fp64 (differentiable): the samples [nctx] of [B, 3, h, w].  dec: the fp32 chain's discrete
    decisions per context (tap cell; whether the clamp passes the gradient) in place of the ones fp64 would take -- the same function wherever the
    two agree, and the branch the kernel takes (bit-exact by contract) where the fp64 coordinate lies within its error of a boundary."""
    c = case
    B, h, w = c.B, c.h, c.w
    K = c.K.double().clone()
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = K[:, 0, 0] * c.sx, K[:, 1, 1] * c.sy, K[:, 0, 2] * c.sx, K[:, 1, 2] * c.sy
    Ki = G.inv_intrinsics(K)
    xs = torch.arange(w, dtype=F64).view(1, 1, w).expand(B, h, w)
    ys = torch.arange(h, dtype=F64).view(1, h, 1).expand(B, h, w)
    d = depth[:, 0]
    grid = torch.stack([xs * d, ys * d, d], 1).reshape(B, 3, -1)
    pts = Ki.bmm(grid)
    out = []
    for j in range(c.nctx):
        P = poses[j]
        q = K.bmm(P[:, :3, :3]).bmm(pts) + K.bmm(P[:, :3, 3:4])
        X, Y = (q[:, 0] / (q[:, 2] + EPS)).view(B, h, w), (q[:, 1] / (q[:, 2] + EPS)).view(B, h, w)
        Xc, Yc = X.clamp(0, w - 1), Y.clamp(0, h - 1)
        if dec is not None:
            Xc, Yc = torch.where(dec[j]["passx"], X, Xc.detach()), torch.where(dec[j]["passy"], Y, Yc.detach())
        ix = (2 * Xc / (w - 1) - 1.0 + 1.0) * ((w - 1) / 2)
        iy = (2 * Yc / (h - 1) - 1.0 + 1.0) * ((h - 1) / 2)
        out.append(G.grid_sample_bilinear_zeros_ac(c.ctx[j].double(), ix, iy) if dec is None else _sample_in_cell(c.ctx[j].double(), ix, iy, dec[j]["x0"], dec[j]["y0"]))
    return out


def photo_ref_maps(case, sampled):
    """MonoDepth2.py:L116-151 through oracle.losses.photometric_map, fp64: the maps [nmaps] of [B, h, w], clipped at the given thresholds"""
    c, A = case, case.A.double()
    maps = []
    for j in range(c.nctx):
        for x in ([sampled[j], c.ctx[j].double()] if c.automask else [sampled[j]]):
            pm = OL.photometric_map(x, A, c.ssim_w, c.C1, c.C2)[:, 0]
            if c.thr is not None:
                pm = pm.clamp(max=float(c.thr[len(maps)]))
            maps.append(pm)
    return maps


def photo_ref_reduce(case, maps, sel=None):
    """the reduced map: min over the maps (sel None), or the map `sel` names (the stored arg-min: the backward's reading)"""
    cat = torch.stack(maps, 1)
    if case.reduce_mean:
        return cat.mean(1)
    if sel is None:
        return cat.min(1)[0]
    return cat.gather(1, sel.long().clamp(max=len(maps) - 1).unsqueeze(1))[:, 0]


def photo_fwd_case(case):
    """bounds of the forward outputs; "stored": (sampled [nctx] fp32, sel uint8) for the isolated backward"""
    dec = fp32_decisions(case)
    fv = photo_fwd(V, case, dec)
    with torch.no_grad():
        S = photo_ref_sample(case, case.depth.double(), [p.double() for p in case.poses])
        maps = photo_ref_maps(case, S)
        red = photo_ref_reduce(case, maps)
    und = fv["und_sel"]
    return {"sampled": [bound(S[j], fv["sampled"][j]) for j in range(case.nctx)], "maps": bound(torch.stack(maps, 1), V.stack(fv["maps"], 1)),
            "sel": fv["sel"], "sel_alt": fv["sel_alt"], "sel_free": fv["sel_free"], "und_sel": und, "share": float(und.double().mean()), "partial": bound(ref_tile_sum(red, *FT), fv["partial"]),
            "loss": bound(red.mean(), fv["loss"]), "stored": ([s.float() for s in S], fv["sel"]), "v": fv, "dec": dec}


def photo_bwd(A, case, sampled, sel, dec=None, fault=None):
    """photo_bwd_body on the stored `sampled` [nctx] (fp32) and `sel` (uint8) -> d_depth [B, h, w], pose_partial [nblk, nctx, 12]; V only: und [B, h, w]"""
    c = case
    B, h, w = c.B, c.h, c.w
    Aa = A.inp(c.A)
    C1, C2, third, inv9 = A.k(c.C1), A.k(c.C2), A.c(1.0 / 3.0), A.c(1.0 / 9.0)
    g = A.k(c.gout) * (A.k(c.gscale) / A.k(B * h * w))
    g_mean = g / A.k(c.nctx if fault == "g_mean" else c.nmaps)
    sel = sel.long()
    dd_terms, parts = [], []
    und = torch.zeros(B, h, w, dtype=torch.bool)
    for j in range(c.nctx):
        mi = c.mi(j)
        X = A.inp(sampled[j])
        if c.reduce_mean:
            on = ~(((sel >> mi) & 1) > 0) if c.thr is not None else torch.ones(B, h, w, dtype=torch.bool)
            gw = A.where(on, g_mean, 0.0)
        else:
            on = sel == mi
            gw = A.where(on, g, 0.0)
        s = None
        if c.ssim_w > 0:
            f = ((gw.scale(-0.5) * (A.k(c.ssim_w) * third)) * inv9).map(lambda v: v.unsqueeze(1))
            cA, _, cB, cC, u_ = ssim_coef(A, X, Aa, f, C1, C2, False)
            u_ = (u_ & on.unsqueeze(1)).any(1, keepdim=True)
            und |= F.max_pool2d(u_.double(), 3, 1, 1)[:, 0] > 0
            s = ssim_gather(A, cA, cB, cC, X, Aa, fault)
        df = X.val - Aa.val
        sg = torch.sign(df).double()
        if fault == "l1_sign":
            sg = torch.where(df == 0, torch.ones_like(sg), sg)
        l1c = (1.0 - A.k(c.ssim_w)) if c.ssim_w > 0 else A.k(1.0)
        l1 = ((gw * l1c).map(lambda v: v.unsqueeze(1)).scale(sg)) * third
        ds = l1 if s is None else s + l1
        cam = make_cam(A, c.K, c.poses[j], c.sx, c.sy)
        pr = project(A, cam, c.depth, None if dec is None else dec[j])
        if not A.exact:
            und |= undecided_coord(pr, h, w)
        nw, ne, sw, se = tap_values(A, c.ctx[j], pr)
        u = lambda t: t.map(lambda v: v.unsqueeze(1))      # noqa: E731
        # Everything from here on is LINEAR in ds, and the chain uses it several times with opposite signs (dq2 = -(dX X + dY Y) / den against dq0, dq1:
        # d_depth = dX (a0 - X a2) / den + ..., a difference some hundred times smaller than its terms).  With V the error of ds must not be propagated
        # through those occurrences as if they were independent: the chain runs on ds as an exact operand (its roundings), and the error of ds enters
        # through the exact coefficient of ds in each output (lin_terms below), enclosed by V.
        ds_err, ds = (None, ds) if A.exact else (ds.err + 0.0 * ds.val, V(ds.val))
        gIx, gIy = tap_gradient(A, (ne - nw, se - sw), pr["wy"]), tap_gradient(A, (sw - nw, se - ne), pr["wx"])
        tx, ty = ds * gIx, ds * gIy
        dX = A.where(pr["passx"], A.sum([tx[:, 0], tx[:, 1], tx[:, 2]]), 0.0)
        dY = A.where(pr["passy"], A.sum([ty[:, 0], ty[:, 1], ty[:, 2]]), 0.0)
        rden = 1.0 / pr["den"]
        dq = [dX * rden, dY * rden, (-(dX * pr["X"] + dY * pr["Y"])) * rden]
        ki, kr, k = cam["ki"], cam["kr"], cam["k"]
        for i in range(3):
            dp = (dq[0] * kr[i] + dq[1] * kr[3 + i]) + dq[2] * kr[6 + i]
            dd_terms.append(dp * ((ki[3 * i] * pr["fx"] + ki[3 * i + 1] * pr["fy"]) + ki[3 * i + 2]))
        acc = [None] * 12
        for m in range(3):
            kq = (k[m] * dq[0] + k[3 + m] * dq[1]) + k[6 + m] * dq[2]
            for i in range(3):
                acc[3 * m + i] = kq * pr["p"][(i + 1) % 3 if (fault == "acc12" and m == 1 and i == 2) else i]
            acc[9 + m] = kq
        if not A.exact:
            sup = lambda v: v.val.abs() + v.err      # noqa: E731
            px, py = pr["passx"].double().unsqueeze(1), pr["passy"].double().unsqueeze(1)

            def lin(cx, cy):
                """sum_c sup |coefficient of ds_c| err(ds_c) for an output dX cx + dY cy"""
                return (sup((gIx * u(cx)).scale(px) + (gIy * u(cy)).scale(py)) * ds_err).sum(1)
            ray = [(ki[3 * i] * pr["fx"] + ki[3 * i + 1] * pr["fy"]) + ki[3 * i + 2] for i in range(3)]
            a = [V.sum([kr[3 * r + i] * ray[i] for i in range(3)]) for r in range(3)]
            dd_terms[-3] = dd_terms[-3].widen(lin((a[0] - pr["X"] * a[2]) * rden, (a[1] - pr["Y"] * a[2]) * rden))
            for m in range(3):
                e = lin((k[m] - pr["X"] * k[6 + m]) * rden, (k[3 + m] - pr["Y"] * k[6 + m]) * rden)
                acc[9 + m] = acc[9 + m].widen(e)
                for i in range(3):
                    acc[3 * m + i] = acc[3 * m + i].widen(e * sup(pr["p"][i]))
        parts.append(A.stack([tile_sum(A, a, *BT, halo=2) for a in acc], 1))
    pp = A.stack(parts, 1)                                                    # [nblk, nctx, 12]
    if fault == "partial_index":
        gy, gx = -(-h // BT[0]), -(-w // BT[1])
        pp = pp.map(lambda v: v.reshape(B, gy, gx, c.nctx, 12).permute(0, 2, 1, 3, 4).reshape(-1, c.nctx, 12))
    return {"d_depth": A.sum(dd_terms), "pose_partial": pp, "und": und}


def pose_from_partials(A, pp, B):
    """pose_grad_finalize_multi_kernel: the sum of a sample's partials in some order -> [nctx] of [B, 3, 4] (rows 0..2 of d_pose; row 3 is zero)"""
    nctx = pp.val.shape[1]
    s = pp.map(lambda v: v.reshape(B, -1, nctx, 12)).sumdim(1)                 # [B, nctx, 12]
    return [s.map(lambda v: torch.cat([v[:, j, :9].reshape(B, 3, 3), v[:, j, 9:].reshape(B, 3, 1)], 2)) for j in range(nctx)]


def photo_ref_reduced_as_stored(case, S, sel):
    """the reduced map as a function of the samples S, the selection and the clipping read from the stored `sel`"""
    c = case
    maps = photo_ref_maps(PhotoCaseView(c), S)
    sel = sel.long()
    if c.reduce_mean:
        if c.thr is not None:      # a set bit: the map was clipped at this pixel, no gradient
            maps = [torch.where(((sel >> mi) & 1) > 0, m.detach(), m) for mi, m in enumerate(maps)]
        return torch.stack(maps, 1).mean(1)
    red = photo_ref_reduce(c, maps, sel)
    return torch.where(sel == 254, red.detach(), red)


class PhotoCaseView:
    """a PhotoCase without its clip thresholds: the backward reads the clipping from `sel`, not from the values"""

    def __init__(self, c):
        self.__dict__.update(c.__dict__)
        self.thr = None


def photo_bwd_case(case, stored, sel):
    """bounds of sde_photo_bwd's outputs on the stored operands: d_depth [B, 1, h, w], pose_partial [nblk, nctx, 12], d_pose [nctx] of [B, 4, 4]"""
    c = case
    B, h, w = c.B, c.h, c.w
    dec = fp32_decisions(c)
    bv = photo_bwd(V, c, stored, sel, dec)
    und = bv["und"]
    gtot = c.gout * c.gscale
    # stage 1: dL/dS at the stored samples
    S = [s.double().requires_grad_(True) for s in stored]
    L = photo_ref_reduced_as_stored(c, S, sel).mean() * gtot
    dS = torch.autograd.grad(L, S)
    # stage 2: <dL/dS, S(depth, pose)>, the pixels left out detached; one pass per backward tile for the per-workgroup pose partials
    gy, gx = -(-h // BT[0]), -(-w // BT[1])
    dr = c.depth.double().requires_grad_(True)
    pr = [p.double().requires_grad_(True) for p in c.poses]
    Sm, Sf = photo_ref_sample(c, dr, pr), photo_ref_sample(c, dr, pr, dec)
    keep = (~und).double().unsqueeze(1)
    # (the pixels left out of d_depth still belong to the per-workgroup pose sums: there the sample function with the fp32 chain's decisions)
    per = [(dS[j] * (Sm[j] * keep + Sf[j] * (1.0 - keep))).sum(1) for j in range(c.nctx)]               # [B, h, w] per context
    d_ref = torch.zeros(B, 1, h, w, dtype=F64)
    pp_ref = torch.zeros(B, gy, gx, c.nctx, 12, dtype=F64)
    for by in range(gy):
        for bx in range(gx):
            t = sum(p[:, by * BT[0]:(by + 1) * BT[0], bx * BT[1]:(bx + 1) * BT[1]].sum() for p in per)
            gr = torch.autograd.grad(t, [dr] + pr, retain_graph=True)
            d_ref += gr[0]
            for j in range(c.nctx):
                pp_ref[:, by, bx, j, :9] = gr[1 + j][:, :3, :3].reshape(B, 9)
                pp_ref[:, by, bx, j, 9:] = gr[1 + j][:, :3, 3]
    pp_v = bv["pose_partial"]
    pp_ref = pp_ref.reshape(-1, c.nctx, 12)
    dpose_v = pose_from_partials(V, pp_v, B)
    dpose_ref = pose_from_partials(V, V(pp_ref), B)
    full = lambda t: torch.cat([t, torch.zeros(B, 1, 4, dtype=F64)], 1)      # noqa: E731
    return {"d_depth": bound(d_ref, bv["d_depth"].map(lambda v: v.unsqueeze(1)), und.unsqueeze(1)), "pose_partial": bound(pp_ref, pp_v),
            "d_pose": [Bound(full(r.val), full(v.err + 0.0 * v.val)) for r, v in zip(dpose_ref, dpose_v)], "und": und,
            "share": float((und | ~torch.isfinite(bv["d_depth"].err)).double().mean()), "v": bv}      # (an element without a finite limit counts as left out)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the photometric cases, shared by the CPU self-test and the GPU tests (each reference is built once per process)
# ---------------------------------------------------------------------------------------------------------------------------------------
# the seeds: the first of a short scan at which the share of undecided arg-min decisions (from the reference alone) is under its cap
PHOTO_SHAPES = {"4x4": (1, 4, 4, 56), "5x30": (1, 5, 30, 55), "13x29": (1, 13, 29, 64), "15x31": (1, 15, 31, 69), "2x37x75": (2, 37, 75, 100)}
PHOTO_PARAMS = {"n1": dict(nctx=1), "n2": dict(), "n3": dict(nctx=3), "n4": dict(nctx=4, seed=35), "nomask": dict(automask=False), "mean": dict(reduce_mean=True),
                "mean_nomask": dict(reduce_mean=True, automask=False, nctx=3), "l1": dict(ssim_w=0.0), "l1_mean": dict(ssim_w=0.0, reduce_mean=True), "clip_min": dict(clip=0.3, seed=28),
                "clip_mean": dict(clip=0.3, reduce_mean=True), "scaled": dict(sx=0.25, sy=0.25), "dense": dict(B=256, gscale=128.0)}
_CASES = {}


def named_case(name):
    """{"case", "fwd": photo_fwd_case, "bwd": photo_bwd_case, "stored": (sampled, sel)} of a key of PHOTO_SHAPES (default options) or PHOTO_PARAMS
    (2 x 13 x 29).  The stored samples handed to the backward equal the target frame at two pixels per sample (df == 0: the L1 term's sign is 0)."""
    if name in _CASES:
        return _CASES[name]
    if name in PHOTO_SHAPES:
        B, h, w, seed = PHOTO_SHAPES[name]
        case = photo_case(B, h, w, seed)
    else:
        kw = dict(PHOTO_PARAMS[name])
        B, clip, seed = kw.pop("B", 2), kw.pop("clip", None), kw.pop("seed", 5)
        if "sx" in kw:
            kw["sy"] = kw["sx"]
        case = photo_case(B, 13, 29, seed, **kw)
        if clip is not None:      # thresholds as LOSS.CLIP forms them (mean + clip * std of each unclipped map), from the reference
            with torch.no_grad():
                maps = photo_ref_maps(case, photo_ref_sample(case, case.depth.double(), [p.double() for p in case.poses]))
            case.thr = torch.stack([m.mean() + clip * m.std() for m in maps]).float()
    fwd = photo_fwd_case(case)
    sampled, sel = fwd["stored"]
    sampled = [s.clone() for s in sampled]
    for j, s in enumerate(sampled):
        for (y, x) in ((1, 2), (case.h - 2, case.w - 1)):
            s[:, :, y, x] = case.A[:, :, y, x]
    out = {"case": case, "fwd": fwd, "stored": (sampled, sel), "bwd": photo_bwd_case(case, sampled, sel)}
    _CASES[name] = out
    return out

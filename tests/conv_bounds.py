"""Per-element error bounds for the convolution engine from an fp64 reference (helper, no tests; imported like resnext_ref.py).

A relative-L2 error over a whole tensor cannot see one wrong pixel, one mishandled corner of a ragged tile or one reflected border column: at
2 x 96 x 160 x 128 outputs a single pixel is 1 / 30720 of the norm.  This module bounds every ELEMENT instead, with the standard a-priori bound of
an fp32 dot product (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 3.5), which holds for ANY summation order -- split-K,
slab reduces and MFMA chains included -- and needs no measured constant:

    |computed - ref| <= u_out * |ref| + (K + 3) * 2^-24 * mag + tiny

  ref   the fp64 result on the operands exactly as the kernel sees them (already rounded to the storage dtype),
  mag   the same convolution of the absolute values, conv(|x|, |w|), in fp64,
  K     the length of the fp32 accumulation (+ 1 for a bias): KH KW Cin for y, KH KW Cout for dX (the full count also for stride 2: looser, still
        valid), B OH OW for dW and dbias,
  u_out the unit roundoff of the stored result: 2^-8 bf16, 2^-11 fp16, 2^-24 fp32 (and the fp32 weight / bias gradients),
  tiny  half the smallest subnormal of the stored dtype (the rounding error of a result below the normal range).

Where the engine rounds an intermediate to the storage dtype, the bound follows the same steps:
  * ELU / ReLU are 1-Lipschitz, so the pre-activation bound carries through.  The kernels' ELU calls expm1f (conv.hip, pgemm.hip,
    conv_halo_small.hip: `t > 0.f ? t : expm1f(t)`); the HIP math API documents a maximum error of 1 ulp for expm1f in single precision, i.e.
    2 * 2^-24 relative to the result, which is added on the activated value.
  * Activation backward (nn.hip act_bwd_bias_kernel) forms dz = (g0 [+ g1]) * act'(stored y) in fp32 and stores it in the activation dtype before the
    two gradient GEMMs read it.  act'(y) as a function of the stored output (1 for y > 0, y + 1 below) is 1-Lipschitz, so
    |dz - dz_ref| <= |g| * lim_y + (u + 3 * 2^-24) * (|dz_ref| + |g| * lim_y): an OPERAND error, propagated through conv(|.|, |w|).
  * The data gradient of a reflection-padded layer is produced on the padded grid in the activation dtype and folded (reflection, 2 x 2 sums of the
    nearest up-sampling, concat split) by a second kernel in fp32 that rounds again: the padded bound goes through the same (non-negative, linear)
    fold, plus the fold's own n-term fp32 sum and final rounding.

The convolutions outside the engine follow the same scheme (Conv3x3Case, DeconvCase, Conv3dPackCase); their steps, read off the wrappers:
  * Grouped 3x3 (hip/nn.py _GroupedConv3x3, csrc/gconv.hip): the kernels convert the fp32 master weight to the activation dtype while staging it, so
    the operand is the weight rounded to that dtype; no bias, no activation, the gradient GEMMs read the incoming gradient itself.  K = 9 Cin / G
    (the block-diagonal zeros of a super-group, and of the composed route's dense weight, add exact zeros).  The weight gradient is fp32 partials
    summed by a second launch: one fp32 sum of B OH OW terms in some order.  A second backward adds a second stored dX to the first (autograd's
    add, rounded to the activation dtype) and a second sum into the fp32 weight-gradient slot: accumulated().
  * Dilated 3x3 (hip/bts.py dilated_conv3x3): sde_dilate_split / sde_dilate_merge copy elements (forward and, with their roles swapped, backward);
    each of the d^2 sub-grids goes through the engine's 3x3 padding-1 layer, whose sums are the dilated convolution's term for term.  The fp64
    dilated convolution is the reference and no rounding step is added.
  * Transposed 3x3 stride 2 (hip/nn.py _ConvTranspose2d, csrc/deconv.hip): y = relu(sum + bias) with the bias read in fp32, K = 9 Cin + 1 for the
    parity-split kernel and for the zero-insertion route (whose zero terms add nothing; that route stores the pre-activation and a second kernel
    applies ReLU to the stored value: max(., 0) of a stored value is exact, so both routes round once).  Backward: sde_act_bwd_bias_sum forms
    dz = g * [stored y > 0] and stores it in the activation dtype -- 0 or g itself, both representable, so that store is exact -- and sums dz in
    fp32 for the bias gradient (K = B 2H 2W).  The step function is not Lipschitz: where the fp64 pre-activation lies within its own limit of
    zero the sign of the computed one is not determined (`undecided`), dz may be 0 or g, an operand error of |g| that goes through
    conv(|.|, |w|) like dz_err above; everywhere else the computed and the reference mask agree and dz = g exactly.  dX is the engine's stride-2
    forward over dz (K = 9 Cout), dW its weight gradient with x in the role of the output gradient (K = B H W).
  * Conv3d(1 -> 8) pack (hip/nn.py _Conv3dPack, csrc/conv3d.hip): weight and bias are read in fp32 (not rounded); the accumulator starts at the
    bias and takes 27 fmaf (K = 27 + 1); dX sums 27 x 8 products; dW and dbias are per-thread, per-wave and per-workgroup fp32 sums and an fp64
    column sum rounded to fp32 once (K = B D H W; with K in the hundreds of thousands that worst case exceeds the gradient itself and the
    relative-L2 line of the test is the binding one -- tests/test_conv_bounds.py says where).

SDE_BOUNDS_LOG=<file>: every assertion appends "<dtype> <name> <worst error / limit>" to that file (a record of how much of the bound a run
used; the threshold is the bound itself).
"""
import os
from collections import namedtuple

import torch
import torch.nn.functional as F

E32 = 2.0 ** -24
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
TINY = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25, torch.float32: 2.0 ** -150}
# relative-L2 tolerances kept as a second assertion: the fp32 and bf16 values of test_gpu_nn.check(); fp16 = bf16 scaled by the ratio of the
# unit roundoffs (2^-11 / 2^-8)
L2_TOL = {torch.float32: 2e-5, torch.bfloat16: 1.5e-2, torch.float16: 1.5e-2 * 2.0 ** -3}
DT_NAME = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "fp16"}
ACT_NONE, ACT_ELU, ACT_RELU = 0, 1, 2

Bound = namedtuple("Bound", "ref lim")      # fp64 tensors of the result's shape


def rounded(t, dtype):
    """fp32 tensor holding exactly the values the kernel reads after the operand was stored in `dtype`."""
    return t.to(dtype).float()


def stored(ref, err, dtype):
    """Bound of a value computed with absolute error <= err and then rounded to `dtype`: |rd(c) - c| <= u |c| <= u (|ref| + err)."""
    u = U_OUT[dtype]
    return Bound(ref, u * ref.abs() + (1.0 + u) * err + TINY[dtype])


def _adjoint(fn, shapes, t):
    """t -> J^T t for a linear fn of len(shapes) inputs (data movement with 0 / 1 coefficients, or a convolution), in fp64 by autograd."""
    zs = [torch.zeros(s, dtype=torch.float64, requires_grad=True) if s is not None else None for s in shapes]
    fn(*zs).backward(t)
    return [z.grad if z is not None else None for z in zs]


class ConvCase:
    """One convolution layer of the engine: y = act(conv(src(x0, x1), w) + b) and its gradients, as fp64 references with per-element limits.

    x0 [B, C0, H0, W0], x1 (skip, [B, C1, 2 H0, 2 W0], upcat only), w [Cout, Cin, KH, KW], gys (one tensor per consumer of y): fp32 CPU tensors that
    already hold storage-dtype values (rounded()); b stays fp32 (the kernels read the bias in fp32).  src = nearest x2 up-sampling + concat (upcat),
    reflection padding (reflect): pure data movement, exact."""

    def __init__(self, x0, w, b, dtype, *, stride=1, pad=0, reflect=False, act=ACT_NONE, x1=None, upcat=False):
        self.dtype, self.stride, self.reflect, self.act, self.upcat = dtype, stride, reflect, act, upcat
        self.p = 0 if reflect else pad
        self.x0, self.x1 = x0.double(), (x1.double() if x1 is not None else None)
        self.w, self.b = w.double(), (b.double() if b is not None else None)
        self.xin = self.src(self.x0, self.x1)
        Cout, Cin, KH, KW = w.shape
        self.taps = KH * KW
        K = self.taps * Cin + (1 if b is not None else 0)
        pre = F.conv2d(self.xin, self.w, self.b, stride, self.p)
        mag = F.conv2d(self.xin.abs(), self.w.abs(), self.b.abs() if b is not None else None, stride, self.p)
        err = (K + 3) * E32 * mag
        if act == ACT_ELU:
            pre = F.elu(pre)
            err = err + 2.0 * E32 * pre.abs()        # expm1f: 1 ulp
        self.y = stored(pre, err, dtype)

    def src(self, a, s):
        t = F.interpolate(a, scale_factor=2, mode="nearest") if self.upcat else a
        if s is not None:
            t = torch.cat([t, s], 1)
        return F.pad(t, (1, 1, 1, 1), mode="reflect") if self.reflect else t

    def _conv(self, x, w):
        return F.conv2d(x, w, None, self.stride, self.p)

    def backward(self, gys, weights=True):
        """{"dX", "dSkip", "dW", "dbias"} -> Bound, for the gradients gys arriving at y (several: summed inside the activation-backward kernel).
        weights=False leaves the weight and bias gradients out (a test that does not look at them saves their fp64 convolutions)."""
        dt, u = self.dtype, U_OUT[self.dtype]
        g = sum(t.double() for t in gys)
        if self.act == ACT_NONE and len(gys) == 1:
            dz, dz_err = g, None                       # the GEMMs read the incoming gradient itself
        else:
            yr, ylim = self.y
            fp = torch.where(yr > 0, torch.ones_like(yr), yr + 1.0) if self.act == ACT_ELU else torch.ones_like(yr)
            dz = g * fp
            moved = g.abs() * ylim if self.act == ACT_ELU else torch.zeros_like(g)
            dz_err = moved + (u + 3.0 * E32) * (dz.abs() + moved) + TINY[dt]
        dz_mag = dz.abs() if dz_err is None else dz.abs() + dz_err
        out = {}
        # data gradient on the (padded) source grid
        Cout = self.w.shape[0]
        Kd = self.taps * Cout
        shp = [tuple(self.xin.shape)]
        rp = _adjoint(lambda z: self._conv(z, self.w), shp, dz)[0]
        err = (Kd + 3) * E32 * _adjoint(lambda z: self._conv(z, self.w.abs()), shp, dz_mag)[0]
        if dz_err is not None:
            err = err + _adjoint(lambda z: self._conv(z, self.w.abs()), shp, dz_err)[0]
        bp = stored(rp, err, dt)
        if not (self.reflect or self.upcat):
            out["dX"] = bp
        else:
            shapes = [tuple(self.x0.shape), tuple(self.x1.shape) if self.x1 is not None else None]
            refs = _adjoint(self.src, shapes, bp.ref)
            mags = _adjoint(self.src, shapes, bp.ref.abs())
            lims = _adjoint(self.src, shapes, bp.lim)
            terms = _adjoint(self.src, shapes, torch.ones_like(bp.ref))
            for name, r, m, l, n in zip(("dX", "dSkip"), refs, mags, lims, terms):
                if r is not None:
                    out[name] = stored(r, l + (n - 1.0).clamp(min=0) * E32 * (m + l), dt)
        if not weights:
            return out
        # weight and bias gradients: fp32 sums over B OH OW output pixels, stored in fp32
        Kw = dz.shape[0] * dz.shape[2] * dz.shape[3]
        wshape = [tuple(self.w.shape)]
        rw = _adjoint(lambda w0: self._conv(self.xin, w0), wshape, dz)[0]
        err = (Kw + 3) * E32 * _adjoint(lambda w0: self._conv(self.xin.abs(), w0), wshape, dz_mag)[0]
        if dz_err is not None:
            err = err + _adjoint(lambda w0: self._conv(self.xin.abs(), w0), wshape, dz_err)[0]
        out["dW"] = stored(rw, err, torch.float32)
        if self.b is not None:
            err = (Kw + 3) * E32 * dz_mag.sum((0, 2, 3))
            if dz_err is not None:
                err = err + dz_err.sum((0, 2, 3))
            out["dbias"] = stored(dz.sum((0, 2, 3)), err, torch.float32)
        return out


def accumulated(bound, n, dtype):
    """n results, each within `bound`, added into one tensor stored in `dtype` (a second backward into an existing gradient): n times the reference and
    the limit, and the rounding of the stored sum."""
    return stored(n * bound.ref, n * bound.lim, dtype)


class Conv3x3Case:
    """y = conv2d(x, w, None, stride, padding=dilation, dilation, groups): the grouped 3x3 (groups > 1, stride 1 | 2) and the dilated 3x3 (dilation > 1)
    operators, no bias, no activation.  x [B, Cin, H, W], w [Cout, Cin / groups, 3, 3]: fp32 CPU tensors holding storage-dtype values."""

    def __init__(self, x, w, dtype, *, groups=1, stride=1, dilation=1):
        self.dtype, self.groups, self.stride, self.dilation = dtype, groups, stride, dilation
        self.x, self.w = x.double(), w.double()
        self.taps = w.shape[2] * w.shape[3]
        K = self.taps * w.shape[1]
        self.y = stored(self._conv(self.x, self.w), (K + 3) * E32 * self._conv(self.x.abs(), self.w.abs()), dtype)

    def _conv(self, x, w):
        return F.conv2d(x, w, None, self.stride, self.dilation, self.dilation, self.groups)

    def backward(self, gy):
        """{"dX", "dW"} -> Bound for the gradient gy arriving at y (read by both gradient kernels as it is)."""
        dz = gy.double()
        Kd = self.taps * self.w.shape[0] // self.groups            # output channels of one group reach an input channel
        Kw = dz.shape[0] * dz.shape[2] * dz.shape[3]
        xs, ws = [tuple(self.x.shape)], [tuple(self.w.shape)]
        out = {}
        rp = _adjoint(lambda z: self._conv(z, self.w), xs, dz)[0]
        out["dX"] = stored(rp, (Kd + 3) * E32 * _adjoint(lambda z: self._conv(z, self.w.abs()), xs, dz.abs())[0], self.dtype)
        rw = _adjoint(lambda w0: self._conv(self.x, w0), ws, dz)[0]
        out["dW"] = stored(rw, (Kw + 3) * E32 * _adjoint(lambda w0: self._conv(self.x.abs(), w0), ws, dz.abs())[0], torch.float32)
        return out


class DeconvCase:
    """y = act(conv_transpose2d(x, w, b, stride 2, padding 1, output_padding 1)), act ACT_NONE | ACT_RELU.  x [B, Cin, H, W], w [Cin, Cout, 3, 3]: fp32 CPU
    tensors holding storage-dtype values; b fp32 or None.  `undecided`: the elements whose ReLU mask the reference cannot decide (all False without
    ReLU), `undecided_share` their fraction."""

    def __init__(self, x, w, b, dtype, *, act=ACT_NONE):
        assert act in (ACT_NONE, ACT_RELU) and tuple(w.shape[2:]) == (3, 3)
        self.dtype, self.act = dtype, act
        self.x, self.w, self.b = x.double(), w.double(), (b.double() if b is not None else None)
        K = 9 * w.shape[0] + 1
        pre = self._fwd(self.x, self.w, self.b)
        err = (K + 3) * E32 * self._fwd(self.x.abs(), self.w.abs(), self.b.abs() if b is not None else None)
        self.pre = stored(pre, err, dtype)
        if act == ACT_RELU:
            self.y = stored(F.relu(pre), err, dtype)                  # 1-Lipschitz
            self.mask = (pre > 0).double()
            self.undecided = pre.abs() <= self.pre.lim
        else:
            self.y, self.mask, self.undecided = self.pre, torch.ones_like(pre), torch.zeros_like(pre, dtype=torch.bool)
        self.undecided_share = float(self.undecided.double().mean())

    @staticmethod
    def _fwd(x, w, b=None):
        return F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1)

    @staticmethod
    def _adj(dz, w):
        """the adjoint convolution Conv2d(Cout -> Cin, 3, stride 2, padding 1), whose OIHW weight is w as it stands"""
        return F.conv2d(dz, w, None, 2, 1)

    def backward(self, gy):
        """{"dX", "dW", "dbias"} -> Bound."""
        g = gy.double()
        dz = g * self.mask
        dz_err = g.abs() * self.undecided.double()                     # dz is 0 or g there; exact elsewhere
        dz_mag = dz.abs() + dz_err
        B, Cin, H, W = self.x.shape
        Cout = self.w.shape[1]
        out = {}
        out["dX"] = stored(self._adj(dz, self.w), (9 * Cout + 3) * E32 * self._adj(dz_mag, self.w.abs()) + self._adj(dz_err, self.w.abs()), self.dtype)
        ws = [tuple(self.w.shape)]
        Kw = B * H * W
        rw = _adjoint(lambda w0: self._fwd(self.x, w0), ws, dz)[0]
        err = (Kw + 3) * E32 * _adjoint(lambda w0: self._fwd(self.x.abs(), w0), ws, dz_mag)[0] + _adjoint(lambda w0: self._fwd(self.x.abs(), w0), ws, dz_err)[0]
        out["dW"] = stored(rw, err, torch.float32)
        if self.b is not None:
            Kb = B * 4 * H * W
            out["dbias"] = stored(dz.sum((0, 2, 3)), (Kb + 3) * E32 * dz_mag.sum((0, 2, 3)) + dz_err.sum((0, 2, 3)), torch.float32)
        return out


class Conv3dPackCase:
    """y = conv3d(x.unsqueeze(1), w, b, padding=1) viewed as [B, 8 D, H, W].  x [B, D, H, W] holds storage-dtype values; w [8, 1, 3, 3, 3] and b [8] are
    read in fp32 and stay as they are."""

    def __init__(self, x, w, b, dtype):
        self.dtype = dtype
        self.x, self.w, self.b = x.double(), w.double(), b.double()
        self.F = w.shape[0]
        self.y = stored(self._fwd(self.x, self.w, self.b), (27 + 1 + 3) * E32 * self._fwd(self.x.abs(), self.w.abs(), self.b.abs()), dtype)

    @staticmethod
    def _fwd(x, w, b=None):
        B, D, H, W = x.shape
        return F.conv3d(x.unsqueeze(1), w, b, padding=1).reshape(B, w.shape[0] * D, H, W)

    def backward(self, gy):
        """{"dX", "dW", "dbias"} -> Bound."""
        dz = gy.double()
        B, D, H, W = self.x.shape
        xs, ws = [tuple(self.x.shape)], [tuple(self.w.shape)]
        Kw = B * D * H * W
        out = {}
        rp = _adjoint(lambda z: self._fwd(z, self.w), xs, dz)[0]
        out["dX"] = stored(rp, (27 * self.F + 3) * E32 * _adjoint(lambda z: self._fwd(z, self.w.abs()), xs, dz.abs())[0], self.dtype)
        rw = _adjoint(lambda w0: self._fwd(self.x, w0), ws, dz)[0]
        out["dW"] = stored(rw, (Kw + 3) * E32 * _adjoint(lambda w0: self._fwd(self.x.abs(), w0), ws, dz.abs())[0], torch.float32)
        per_f = dz.reshape(B, self.F, D, H, W)
        out["dbias"] = stored(per_f.sum((0, 2, 3, 4)), (Kw + 3) * E32 * per_f.abs().sum((0, 2, 3, 4)), torch.float32)
        return out


WORST = {}      # dtype name -> largest error / limit seen by this process


def _record(dtype, name, ratio):
    key = DT_NAME.get(dtype, str(dtype))
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    path = os.environ.get("SDE_BOUNDS_LOG")
    if path:
        with open(path, "a") as f:
            f.write(f"{key} {name} {ratio:.4f}\n")


def _worst(err, lim):
    ratio = torch.where(lim > 0, err / lim, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    i = int(ratio.argmax())
    return ratio, tuple(int(v) for v in torch.unravel_index(torch.tensor(i), err.shape)), float(ratio.flatten()[i])


def assert_within(got, bound, dtype, name, l2_tol=None):
    """No element of `got` further than bound.lim from bound.ref; then the relative L2 error below l2_tol (default: L2_TOL[dtype])."""
    assert tuple(got.shape) == tuple(bound.ref.shape), f"{name}: shape {tuple(got.shape)} != reference {tuple(bound.ref.shape)}"
    got = got.detach()
    err = (got.double() - bound.ref).abs()
    bad = ~(err <= bound.lim)                          # (a NaN fails)
    ratio, idx, worst = _worst(err, bound.lim)
    _record(dtype, name, worst)
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {err.numel()} elements exceed the per-element bound; worst at {idx}: error {float(err[idx]):.3e} > limit "
                           f"{float(bound.lim[idx]):.3e} ({worst:.1f} x; got {float(got[idx]):.6g}, reference {float(bound.ref[idx]):.6g})")
    tol = L2_TOL[dtype] if l2_tol is None else l2_tol
    e = float(err.norm() / (bound.ref.norm() + 1e-30))
    assert e < tol, f"{name}: relative L2 error {e:.3e} > {tol}"
    return worst


def assert_two_kernels(a, b, bound, dtype, name, also=None):
    """Two kernels on the same operands: each lies within bound.lim of the reference, so |a - b| <= lim_a + lim_b = 2 lim.  `also`: an extra
    per-element limit (a tensor); the tighter of the two holds."""
    a, b = a.detach().double(), b.detach().double()
    assert tuple(a.shape) == tuple(b.shape) == tuple(bound.lim.shape), f"{name}: shapes {tuple(a.shape)}, {tuple(b.shape)}, {tuple(bound.lim.shape)}"
    lim = 2.0 * bound.lim
    if also is not None:
        lim = torch.minimum(lim, also.double())
    err = (a - b).abs()
    bad = ~(err <= lim)
    ratio, idx, worst = _worst(err, lim)
    _record(dtype, name, worst)
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {err.numel()} elements of the two kernels differ by more than the sum of their bounds; worst at {idx}: "
                           f"|{float(a[idx]):.6g} - {float(b[idx]):.6g}| = {float(err[idx]):.3e} > {float(lim[idx]):.3e}")
    return worst

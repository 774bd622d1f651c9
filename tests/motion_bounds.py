"""Element-level references for the MotionLearning loss kernels of csrc/motion_loss.hip (helper, no tests; imported like photo_bounds.py).

The rules are photo_bounds.py's, sections (a) to (d) of its docstring, and the arithmetic is imported from there, not copied:

(a) Every kernel's operation sequence is written ONCE against the V / F32 interface: run with V it gives the per-element limit, run with F32 it is the
    fp32 emulation tests/test_motion_bounds.py holds against the limit (and plants faults in).  motion_loss.hip is compiled with -ffp-contract=off: fmaf is
    one rounding only where the source writes fmaf (set_kt and the project chain), every other a * b + c is two; division and sqrtf are correctly rounded
    and 1.0f / x is a division; literals (1.0f / 9.0f, 2.0f / 9.0f, 1e-2f, 1e-4f, 1e-24f, 1e-12f, 1e-5f, 1e-6f) carry their fp32 representation error (V.c).
    Every workgroup and finalize sum (sde_block_sums, sde_partial_walk, sample_sum9, the ticket finalizers, the plain loops) is an n-term sum in any order,
    gamma_(n-1) sum (|term| + err).  The atomic scatter of mc_bwd_kernel is bounded the same way, n per destination element being the number of taps that
    land on it, counted from the reference's taps: fp32 atomics add in an order nobody fixes, and the any-order bound needs none.
(b) Values come from the fp64 formulas alone (tests/motion_loss_ref.py, tests/motion_model_ref.pair_prep, autograd for the gradients); V.err alone is the
    limit.  tests/test_motion_bounds.py asserts with vjp_agrees that V.val of each hand-derived VJP is the autograd result to 1e-10 relative.
(c) Backward kernels are tested on the operands they read, each taken from the reference and rounded to fp32 (`stored`): in V such an operand is the
    reference's value with the rounding as its error, so V.val stays the exact formula and no forward decision leaks into a backward limit.  sde_rgbd_bwd
    follows photo_bounds (c) instead: its stored operands are exact, and its reference is d / d(depth, R, t) of <dL / d sampled, sampled(depth, R, t)> with
    dL / d sampled taken at the stored values (two autograd stages).  Pass 2 of sde_rgbd_fwd is such a stage too: see rgbd_pass2.
(d) Discrete decisions -- the tap cell, passx / passy, the padding flags -- are taken from the F32 run.  A pixel whose fp64 quantity lies within its V.err of
    a decision boundary is undecided, from the reference alone: a mask may take either value there, a sum that contains it carries its possible jump as
    error, and a gradient element that depends on it is left out.  Caps: 1 % of the mask pixels, 1 % of a gradient's elements; d t_B2A of motion consistency
    leaves nothing out.  Where the fp32 tap cell is not the fp64 one (a coordinate within its error of an integer) the sample is continuous across the
    cell edge; the known difference |V.val - reference| is added to that pixel's limit (triangle inequality), nothing else is.

A workgroup owns 4 rows of 64 pixels (TILE).  No constant in this file is fitted to a run.
"""
import math

import torch
import torch.nn.functional as F

import motion_loss_init as MI
import motion_loss_ref as REF
import photo_bounds as PB
from photo_bounds import (V, F32, U, SUB, F64, Bound, bound, check, record_share, record_note, vjp_agrees, project, tap_values, bilinear,      # noqa: F401
                          tap_gradient, refl_mult, tile_sum, ref_tile_sum, guarded, assert_guards, assert_equal, _record, f32, GUARD)

TILE = (4, 64)
INF = float("inf")
CAP = 0.01


def stored(A, ref):
    """(c): an operand a backward kernel reads back -- the reference's fp64 value rounded to fp32"""
    ref = ref.detach().double()
    return F32(ref.float()) if A.exact else V(ref, (ref.float().double() - ref).abs())


def un(t, dim=1):
    return t.map(lambda v: v.unsqueeze(dim))


def slab_sum(A, part, N, fault=None):
    """sde_partial_walk + block / wave sum: the partials [N * bps, ...] of each sample added up, any order -> [N, ...]"""
    p = part.map(lambda v: v.reshape(N, -1, *v.shape[1:]))
    if fault == "walk256":                        # 15: the slab walk ends after the first pass of its 256 threads
        p = p.map(lambda v: v[:, :256])
    return p.sumdim(1)


def block_sum_1d(A, t, threads):
    """t [P, n]: thread i of `threads` adds elements i, i + threads, ... in order, then sde_block_sum (wave tree, waves in order) -> [P]"""
    P, n = t.val.shape
    if not A.exact:
        return t.sumdim(1)
    k = -(-n // threads)
    v = F.pad(t.val, (0, k * threads - n)).reshape(P, k, threads)
    s = v[:, 0]
    for i in range(1, k):
        s = s + v[:, i]
    s = s.reshape(P, threads // 64, 64)
    while s.shape[-1] > 1:
        s = s[..., 0::2] + s[..., 1::2]
    return F32.sum([F32(s[:, i, 0]) for i in range(s.shape[1])])


def recip_count(A, *dims):
    """1.0f / ((float)a * (float)b * ...) as the host forms it (the product is exact at these sizes)"""
    n = math.prod(dims)
    assert n < 2 ** 24
    return A.k(1.0) / A.k(n)


# ---------------------------------------------------------------------------------------------------------------------------------------
# adaptive average pool (avgpool_fwd_kernel, avgpool_bwd_kernel; the pool of prep_pool_kernel and prep_bwd_gather_kernel)
# ---------------------------------------------------------------------------------------------------------------------------------------
def ap_bounds(H, h, fault=None):
    i = torch.arange(h)
    lo = (i * H) // h
    hi = ((i + 1) * H) // h if fault == "ap_hi_floor" else ((i + 1) * H + h - 1) // h      # 13: ap_hi floored instead of ceiled
    return lo, hi


def _ap_index(H, W, h, w, fault=None):
    """gather index [h, w, K] into the flattened source plane, its mask, and the window areas [h, w]"""
    ylo, yhi = ap_bounds(H, h, fault)
    xlo, xhi = ap_bounds(W, w, fault)
    ky, kx = int((yhi - ylo).max()), int((xhi - xlo).max())
    yy = ylo.view(h, 1, 1, 1) + torch.arange(ky).view(1, 1, ky, 1)
    xx = xlo.view(1, w, 1, 1) + torch.arange(kx).view(1, 1, 1, kx)
    ok = (yy < yhi.view(h, 1, 1, 1)) & (xx < xhi.view(1, w, 1, 1))
    idx = (yy.clamp(max=H - 1) * W + xx.clamp(max=W - 1)).expand(h, w, ky, kx)
    area = ((yhi - ylo).view(h, 1) * (xhi - xlo).view(1, w))
    return idx.reshape(h, w, -1), ok.expand(h, w, ky, kx).reshape(h, w, -1), area


def avgpool_fwd(A, src, h, w, fault=None):
    """src: A-value [P, H, W] -> [P, h, w]: the window's sum (rows, then columns) times 1.0f / area"""
    P, H, W = src.val.shape
    idx, ok, area = _ap_index(H, W, h, w, fault)
    win = src.map(lambda v: v.reshape(P, H * W)[:, idx.reshape(-1)].reshape(P, h, w, -1) * ok.to(v.dtype))
    acc = win.sumdim(3, n=area.double().expand(P, h, w)) if not A.exact else F32.sum([win[..., k] for k in range(idx.shape[-1])])
    return acc * (A.k(1.0) / A.inp(area.float()))


def avgpool_bwd(A, dout, H, W, fault=None):
    """dout: A-value [P, h, w] -> [P, H, W]: every input pixel gathers the windows that contain it, each over its area: dout * (ry / nx)"""
    P, h, w = dout.val.shape
    ylo, yhi = ap_bounds(H, h, fault)
    xlo, xhi = ap_bounds(W, w, fault)
    ry = A.k(1.0) / A.inp((yhi - ylo).float())
    wgt = un(ry, 1) / A.inp((xhi - xlo).float().view(1, w))                                 # [h, w]
    iny = (torch.arange(H).view(H, 1) >= ylo.view(1, h)) & (torch.arange(H).view(H, 1) < yhi.view(1, h))      # [H, h]
    inx = (torch.arange(W).view(W, 1) >= xlo.view(1, w)) & (torch.arange(W).view(W, 1) < xhi.view(1, w))      # [W, w]
    m = (iny.view(H, 1, h, 1) & inx.view(1, W, 1, w)).double()                              # [H, W, h, w]
    t = (dout * wgt).map(lambda v: (v.reshape(P, 1, 1, h, w) * m.to(v.dtype)).reshape(P, H, W, h * w))
    n = m.reshape(H, W, -1).sum(2)
    return t.sumdim(3, n=n.expand(P, H, W)) if not A.exact else F32(t.val.sum(3))


AVGPOOL_SIZES = [((7, 13), (3, 5)), ((13, 7), (20, 11)), ((5, 6), (1, 1)), ((9, 70), (4, 33)), ((8, 130), (4, 65))]
_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def avgpool_case(sizes, P=3):
    def build():
        (H, W), (h, w) = sizes
        g = torch.Generator().manual_seed(H * 100 + w)
        x, go = torch.randn(P, H, W, generator=g), torch.randn(P, h, w, generator=g)
        xr = x.double().requires_grad_(True)
        ref = F.adaptive_avg_pool2d(xr[None], (h, w))[0]
        ref.backward(go.double())
        vf, vb = avgpool_fwd(V, V.inp(x), h, w), avgpool_bwd(V, V.inp(go), H, W)
        return {"x": x, "gout": go, "out": bound(ref, vf), "din": bound(xr.grad, vb), "v": (vf, vb), "ref": (ref.detach(), xr.grad)}
    return cached(("avgpool", sizes, P), build)


def avgpool_emu(c, sizes, fault=None):
    (H, W), (h, w) = sizes
    return {"out": avgpool_fwd(F32, F32.inp(c["x"]), h, w, fault).val, "din": avgpool_bwd(F32, F32.inp(c["gout"]), H, W, fault).val}


def avgpool_check(c, got, name="avgpool"):
    check(got["out"], c["out"], f"{name} out")
    check(got["din"], c["din"], f"{name} din")


# ---------------------------------------------------------------------------------------------------------------------------------------
# motion smoothness (msmooth_fwd_kernel, msmooth_bwd_kernel, ticket_finalize)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _msmooth_elem(A, f):
    """f: A-value [P, H, W] -> gx, gy, root [P, H-1, W-1] of element (i, j): the corner f[i+1][j+1] against f[i+1][j] and f[i][j+1]"""
    c = f[:, 1:, 1:]
    gx, gy = c - f[:, 1:, :-1], c - f[:, :-1, 1:]
    return gx, gy, ((A.c(1e-24) + gx * gx) + gy * gy).sqrt()


def msmooth_fwd(A, f):
    """f [P, H, W] fp32 -> partial [nblk], out [1]"""
    P, H, W = f.shape
    gz = min(P, 8)
    _, _, root = _msmooth_elem(A, A.inp(f))
    cnt = torch.tensor([len(range(z, P, gz)) for z in range(gz)], dtype=F64).view(gz, 1, 1).expand(gz, H - 1, W - 1)
    per = A.sum([root.map(lambda v: F.pad(v, (0, 0, 0, 0, 0, gz * (-(-P // gz)) - P)))[k * gz:(k + 1) * gz] for k in range(-(-P // gz))], n=cnt)
    partial = tile_sum(A, per, *TILE)
    return {"partial": partial, "out": (partial.sumdim(0) * recip_count(A, P, H - 1, W - 1)).map(lambda v: v.reshape(1))}


def msmooth_bwd(A, f, gout, fault=None):
    """-> df [P, H, W]: the three elements a pixel belongs to, g = gout * scale"""
    P, H, W = f.shape
    gx, gy, root = _msmooth_elem(A, A.inp(f))
    r = A.k(1.0) / root
    pad = lambda t, l, t_, r_, b: t.map(lambda v: F.pad(v, (l, r_, t_, b)))      # noqa: E731  (left, top, right, bottom)
    t1 = pad((gx + gy) * r, 1, 1, 0, 0)                      # the element's corner f[i+1][j+1]: pixel (i + 1, j + 1)
    t2 = pad(gx * r, 0, 1, 1, 0)                             # its f[i+1][j]: pixel (i + 1, j)
    t3 = pad(gy * r, 1, 0, 0, 1)                             # its f[i][j+1]: pixel (i, j + 1)
    if fault == "smooth_edge":                               # 11: `x <= W - 2` written `x < W - 2`
        t2 = t2.scale((torch.arange(W) < W - 2).double().view(1, 1, W))
    ys, xs = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    n = ((ys >= 1) & (xs >= 1)).double() + ((ys >= 1) & (xs <= W - 2)).double() + ((ys <= H - 2) & (xs >= 1)).double()
    d = A.sum([t1, -t2, -t3], n=n.expand(P, H, W))
    return (A.k(gout) * recip_count(A, P, H - 1, W - 1)) * d


SMOOTH_PLANES = [1, 3, 9]
SMOOTH_HW = [(2, 2), (5, 66), (9, 130)]
GOUT = 1.7


def field_inputs(P, H, W, seed=0):
    """plane 0 identically zero (the 1e-24 guards) and a few exact zeros elsewhere"""
    g = torch.Generator().manual_seed(31 * P + H * W + seed)
    f = torch.randn(P, H, W, generator=g) * 0.3
    f[0] = 0.0
    if P > 1:
        f[1].view(-1)[::5] = 0.0
    return f


def msmooth_case(P, H, W):
    def build():
        f = field_inputs(P, H, W)
        fr = f.double().requires_grad_(True)
        root = torch.sqrt(1e-24 + (fr[:, 1:, 1:] - fr[:, 1:, :-1]) ** 2 + (fr[:, 1:, 1:] - fr[:, :-1, 1:]) ** 2)
        ref = REF.motion_smoothness_loss_fn(fr[None])
        assert abs(float((root.mean() - ref).detach())) <= 1e-14 * float(ref.detach()) + 1e-300
        (ref * f32(GOUT)).backward()
        fw, vb = msmooth_fwd(V, f), msmooth_bwd(V, f, GOUT)
        gz = min(P, 8)
        per = torch.stack([root.detach()[z::gz].sum(0) for z in range(gz)])
        return {"f": f, "partial": bound(ref_tile_sum(per, *TILE), fw["partial"]), "out": bound(ref.detach().reshape(1), fw["out"]), "df": bound(fr.grad, vb),
                "v": vb, "ref": fr.grad}
    return cached(("msmooth", P, H, W), build)


def msmooth_emu(c, fault=None):
    e = msmooth_fwd(F32, c["f"])
    return {"partial": e["partial"].val, "out": e["out"].val, "df": msmooth_bwd(F32, c["f"], GOUT, fault).val}


def msmooth_check(c, got, name="msmooth"):
    for k in ("partial", "out", "df"):
        check(got[k], c[k], f"{name} {k}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# motion sparsity (msparse_fwd_kernel, msparse_bwd_kernel)
# ---------------------------------------------------------------------------------------------------------------------------------------
def msparse_fwd(A, f):
    """f [P, hw] -> mean [P], partial [P], out [1]"""
    P, hw = f.shape
    a = A.inp(f).abs()
    m = block_sum_1d(A, a, 1024) / A.k(hw)
    rm = A.k(1.0) / (m + A.c(1e-24))
    t = un(m.scale(2.0)) * ((a * un(rm)) + 1.0).sqrt()
    partial = block_sum_1d(A, t, 1024)
    return {"mean": m, "partial": partial, "out": (partial.sumdim(0) * recip_count(A, P, hw)).map(lambda v: v.reshape(1))}


def msparse_bwd(A, f, mean, gout, fault=None):
    """mean: the stored per-plane mean (an A-value [P]) -> df [P, hw] = gout scale m rm sg / sqrt(|v| rm + 1)"""
    P, hw = f.shape
    a = A.inp(f).abs()
    rm = A.k(1.0) / (mean + A.c(1e-24))
    sg = torch.sign(f).double()
    if fault == "sparse_sign":                               # 12: the sign of an exact zero taken as +1
        sg = torch.where(f == 0, torch.ones_like(sg), sg)
    k = ((A.k(gout) * recip_count(A, P, hw)) * mean) * rm
    return un(k).map(lambda v: v.expand(P, hw)).scale(sg) / ((a * un(rm)) + 1.0).sqrt()


SPARSE_HW = [1, 1024, 1025]


def msparse_case(P, hw):
    def build():
        f = field_inputs(P, 1, hw, seed=5).reshape(P, hw)
        fr = f.double().requires_grad_(True)
        ref = REF.motion_sparsity_loss_fn(fr.view(1, P, 1, hw))
        (ref * f32(GOUT)).backward()
        m = fr.detach().abs().mean(1)
        fw = msparse_fwd(V, f)
        vb = msparse_bwd(V, f, stored(V, m), GOUT)
        part = (2 * m[:, None] * torch.sqrt(fr.detach().abs() / (m[:, None] + 1e-24) + 1)).sum(1)
        return {"f": f, "mean_in": m.float(), "mean": bound(m, fw["mean"]), "partial": bound(part, fw["partial"]), "out": bound(ref.detach().reshape(1), fw["out"]),
                "df": bound(fr.grad, vb), "v": vb, "ref": fr.grad}
    return cached(("msparse", P, hw), build)


def msparse_emu(c, fault=None):
    e = msparse_fwd(F32, c["f"])
    return {"mean": e["mean"].val, "partial": e["partial"].val, "out": e["out"].val, "df": msparse_bwd(F32, c["f"], F32(c["mean_in"]), GOUT, fault).val}


def msparse_check(c, got, name="msparse"):
    for k in ("mean", "partial", "out", "df"):
        check(got[k], c[k], f"{name} {k}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the image cases: view synthesis, RGB-D, weighted SSIM, motion consistency
# ---------------------------------------------------------------------------------------------------------------------------------------
# 2 x 2: the smallest admitted, every window tap reflected; 3 x 3: the centre pixel meets both double-multiplicity conditions of wssim_gather; 4 x 64: one
# tile; 5 x 65: one pixel past the tile both ways; 2 x 9 x 130: three tiles across, N = 2; 1028 x 2: 257 workgroups per sample (sde_partial_walk<., 256>
# takes a second pass, sample_sum9's 64 lanes five)
IMAGE_SHAPES = {"2x2": (1, 2, 2), "3x3": (1, 3, 3), "4x64": (1, 4, 64), "5x65": (1, 5, 65), "2x9x130": (2, 9, 130), "1028x2": (1, 1028, 2)}
OUT_OF_VIEW = ("5x65", "2x9x130")
SSIM_MODES = {"c2": (INF, 9e-6), "c1": (1e-4, INF), "both": (1e-4, 9e-4)}


def image_inputs(name):
    """motion_loss_init.inputs; at OUT_OF_VIEW the construction of test_gpu_motion_loss.out_of_view: a 0.3 rad yaw in sample 0 and a block whose t_z
    pushes its points behind camera B"""
    N, H, W = IMAGE_SHAPES[name]
    v = MI.inputs(N, H, W, seed=40 + list(IMAGE_SHAPES).index(name))
    # frame 2 darker and noisier than frame 1: with the two frames of motion_loss_init nearly equal, the SSIM distance of the warped frame lay within its
    # limit of the clamp at 0 on up to 40 % of the windows (every gradient element at 2 x 2): the input changes, never the cap
    g = torch.Generator().manual_seed(7 + H * W)
    v["frame2"] = (0.6 * v["frame2"] + 0.1 * torch.rand(N, 3, H, W, generator=g)).clamp(0, 1)
    if name in OUT_OF_VIEW:
        v["R12"][0] = MI.euler(torch.tensor([[0.0, 0.3, 0.0]]))[0]
        v["t12"][-1, 2, : max(H // 3, 1), W // 2:] = -60.0
    if name == "1028x2":      # Y is known to 5e-4 px here (q1 of about 4e4) and depth_B moves 0.3 m per row: 1.6 % of the pixels had |Z - sD| within its limit of 0,
        v["depth2"] = v["depth2"] + 1.5      # over the cap -- so depth_B is offset (the input changes, never the cap)
    return v


def geometry_ref(name):
    """the fp64 RGB-D restatement of a case (grid, occlusion mask, ...), computed once"""
    def build():
        v = image_inputs(name)
        d = {k: x.double() for k, x in v.items()}
        with torch.no_grad():
            o = REF.rgbd_consistency_loss(d["frame1"], d["frame2"], d["depth1"], d["depth2"], d["K"], d["R12"], d["t12"], 1.0, 3.0, INF, f32(9e-6))
        return v, o
    return cached(("geometry", name), build)


# ---------------------------------------------------------------------------------------------------------------------------------------
# motion consistency (mc_pixel, mc_fwd_kernel, mc_rot, mc_finalize_kernel, mc_bwd_kernel, mc_bwd_finalize_kernel)
# ---------------------------------------------------------------------------------------------------------------------------------------
def mc_taps(A, grid, H, W, dec=None):
    """grid_sample's un-normalise (align_corners) + make_taps, in the naming of photo_bounds.project.  dec: the F32 run's tap cells (required with V)."""
    out = {}
    for name, g, n in (("x", A.inp(grid[..., 0]), W), ("y", A.inp(grid[..., 1]), H)):
        i = (g + 1.0) * A.k(n - 1).scale(0.5)
        i0 = torch.floor(i.val) if dec is None else dec[name + "0"].double()
        wgt = i - A.inp(i0)
        out.update({name + "0": i0.long(), "w" + name: wgt, "e" + name: 1.0 - wgt, "i" + name: i})
    return out


FLT_MIN = 1.17549435e-38


def div_sq(A, v, den):
    """div_sq of motion_loss.hip: v / (den * den) where that square is a normal fp32 number, (v / den) / den where it is not (the 1e-24 guard alone).  The
    two are one value in exact arithmetic; where the reference cannot tell which the kernel took, the larger of the two limits holds."""
    d2 = den * den
    one, two = v / d2, (v / den) / den
    big = d2.val >= FLT_MIN
    r = A.where(big, one, two)
    if A.exact:
        return r
    near = (d2.val - FLT_MIN).abs() <= d2.err
    return V(r.val, torch.where(near, torch.maximum(one.err, two.err), r.err))


def _m3(A, R):
    """[N, 3, 3] fp32 -> 3 x 3 nested list of A-values [N]"""
    return [[A.inp(R[:, i, j]) for j in range(3)] for i in range(3)]


def mc_rot(A, R1, R2, N, g_rot=None, fault=None):
    """mc_rot for every sample -> (r [N], dR1, dR2 [N, 3, 3] or None)"""
    a, b = _m3(A, R1), _m3(A, R2)
    ident = lambda i, j: 1.0 if i == j else 0.0      # noqa: E731
    M = [[((a[i][0] * b[0][j] + a[i][1] * b[1][j]) + a[i][2] * b[2][j]) - ident(i, j) for j in range(3)] for i in range(3)]
    Am = [[a[i][j] - ident(i, j) for j in range(3)] for i in range(3)]
    Bm = [[b[i][j] - ident(i, j) for j in range(3)] for i in range(3)]
    msq = lambda m: A.sum([m[i][j] * m[i][j] for i in range(3) for j in range(3)]) / A.k(9.0)      # noqa: E731
    re, den = msq(M), (msq(Am) + msq(Bm)) + A.c(1e-24)
    r = re / den
    if g_rot is None:
        return r, None, None
    g = A.k(g_rot) / A.k(N)
    c29 = A.c(2.0 / 9.0)
    gm, gs = (g / den) * c29, div_sq(A, (-g) * re, den) * c29
    d1 = [gm * ((M[i][0] * b[j][0] + M[i][1] * b[j][1]) + M[i][2] * b[j][2]) + gs * Am[i][j] for i in range(3) for j in range(3)]
    if fault == "dR2_R1":                            # 10: dR2 formed with R1 in place of R1^T
        d2 = [gm * ((a[i][0] * M[0][j] + a[i][1] * M[1][j]) + a[i][2] * M[2][j]) + gs * Bm[i][j] for i in range(3) for j in range(3)]
    else:
        d2 = [gm * ((a[0][i] * M[0][j] + a[1][i] * M[1][j]) + a[2][i] * M[2][j]) + gs * Bm[i][j] for i in range(3) for j in range(3)]
    m33 = lambda l: A.stack(l, 1).map(lambda v: v.reshape(N, 3, 3))      # noqa: E731
    return r, m33(d1), m33(d2)


def scatter4(A, ds, pr, H, W, fault=None):
    """grid_sample's backward: ds [N, C, H, W] goes to the four taps of every pixel (taps outside receive nothing) -> ([N, C, H, W], taps per element)"""
    N, C = ds.val.shape[:2]
    wx, ex, ny, sy = un(pr["wx"]), un(pr["ex"]), un(pr["wy"]), un(pr["ey"])
    wg = [sy * ex, sy * wx, ny * ex, ny * wx]
    if fault == "scatter_swap":                      # 8: the weights sy * wx and ny * ex exchanged
        wg[1], wg[2] = wg[2], wg[1]
    base = (torch.arange(N * C) * H * W).view(N, C, 1, 1)
    vals, errs, idxs = [], [], []
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        yy, xx = pr["y0"] + dy, pr["x0"] + dx
        ok = ((xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)).unsqueeze(1).expand(N, C, H, W)
        idx = base + (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).unsqueeze(1)
        c = ds * wg[k]
        vals.append(c.val[ok])
        idxs.append(idx[ok])
        if not A.exact:
            errs.append((c.err + 0.0 * c.val)[ok])
    idx = torch.cat(idxs)
    n = torch.bincount(idx, minlength=N * C * H * W)
    flat = F32(torch.cat(vals)) if A.exact else V(torch.cat(vals), torch.cat(errs))
    return flat.segsum(idx, N * C * H * W, n).map(lambda v: v.reshape(N, C, H, W)), n.reshape(N, C, H, W)


def mc_run(A, c, dec=None, fault=None):
    """forward and backward of motion consistency on the case's operands -> dict of A-values"""
    N, H, W = c["shape"]
    pr = mc_taps(A, c["grid"], H, W, dec)
    s = bilinear(A, tap_values(A, c["tB"], pr), pr)
    tA, R = A.inp(c["tA"]), _m3(A, c["R1"])
    R = [[un(un(R[i][j])) for j in range(3)] for i in range(3)]
    s1, s2 = A.sum([tA[:, k] * tA[:, k] for k in range(3)]), A.sum([s[:, k] * s[:, k] for k in range(3)])
    e = [((R[i][0] * s[:, 0] + R[i][1] * s[:, 1]) + R[i][2] * s[:, 2]) + tA[:, i] for i in range(3)]
    E = A.sum([x * x for x in e])
    den = (s1 + s2) + A.c(1e-24)
    mask = A.inp(c["mask"][:, 0])
    inv = recip_count(A, N, H, W)
    partial = tile_sum(A, mask * (E / den), *TILE)
    r, dR1r, dR2 = mc_rot(A, c["R1"], c["R2"], N, c["g_rot"], fault)
    out = A.stack([r.sumdim(0) / A.k(N), partial.sumdim(0) * inv])
    g = (A.k(c["g_trans"]) * inv) * mask
    dden = div_sq(A, (-g) * E, den)
    de = [(g.scale(2.0) * x) / den for x in e]
    d_tA = A.stack([de[i] if fault == "no_dden" else de[i] + dden.scale(2.0) * tA[:, i] for i in range(3)], 1)      # 9: the dden term dropped
    ds = A.stack([((R[0][j] * de[0] + R[1][j] * de[1]) + R[2][j] * de[2]) + dden.scale(2.0) * s[:, j] for j in range(3)], 1)
    dRp = A.stack([tile_sum(A, de[i] * s[:, j], *TILE) for i in range(3) for j in range(3)], 1)                      # [nblk, 9]
    d_tB, taps = scatter4(A, ds, pr, H, W, fault)
    dR1 = slab_sum(A, dRp, N, fault).map(lambda v: v.reshape(N, 3, 3)) + dR1r
    return {"partial": partial, "out": out, "d_tA": d_tA, "d_tB": d_tB, "dR_partial": dRp, "dR1": dR1, "dR2": dR2, "pr": pr, "taps": taps, "s": s}


G_ROT, G_TRANS = 0.9, 1.3
MC_ROTS = ("generic", "inverse", "identity")
MC_CASES = [(n, "generic") for n in IMAGE_SHAPES] + [("4x64", "inverse"), ("4x64", "identity")]


def mc_case(name, rot="generic"):
    def build():
        v, o = geometry_ref(name)
        N, H, W = IMAGE_SHAPES[name]
        R1, R2 = v["R12"], v["R21"]
        if rot == "inverse":        # R_B2A = R_A2B^T: a 0.02 rad rotation, transposed in fp64 and then rounded -- R1 R2 - I is pure rounding noise
            R64 = MI.euler(torch.tensor([[0.02, -0.02, 0.02]], dtype=F64)).expand(N, 3, 3)
            R1, R2 = R64.float().contiguous(), R64.transpose(1, 2).float().contiguous()
        tA, tB = v["t12"], v["t21"]
        if H > 1024:                # the 257th workgroup's partial carries weight: a walk that stops after 256 must show in d R_A2B
            tA = tA.clone()
            tA[:, :, 1024:] += 0.5
        if rot == "identity":       # the 1e-24 guards alone: both rotations the identity, and a block of pixels where both translations vanish
            R1 = R2 = torch.eye(3).expand(N, 3, 3).contiguous()
            tA, tB = tA.clone(), tB.clone()
            tA[:, :, :2, :8], tB[:, :, :4, :16] = 0.0, 0.0
        c = {"shape": (N, H, W), "grid": o["coords_A_in_B"].float(), "mask": o["occlusion_mask"].float(), "R1": R1, "R2": R2, "tA": tA, "tB": tB,
             "g_rot": f32(G_ROT), "g_trans": f32(G_TRANS)}
        dec = mc_taps(F32, c["grid"], H, W)
        dec = {"x0": dec["x0"], "y0": dec["y0"]}
        g64 = c["grid"].double()
        assert torch.equal(torch.floor((g64[..., 0] + 1) * (W - 1) / 2).long(), dec["x0"]) and torch.equal(torch.floor((g64[..., 1] + 1) * (H - 1) / 2).long(), dec["y0"]), \
            "the grid is an input: its fp32 tap cells must be the fp64 ones (change the input otherwise)"
        lv = [x.double().requires_grad_(True) for x in (R1, R2, c["tA"], c["tB"])]
        s = F.grid_sample(lv[3], g64, mode="bilinear", padding_mode="zeros", align_corners=True)
        e = torch.einsum("bij,bjhw->bihw", lv[0], s) + lv[2]
        e.retain_grad()
        rot_e, trans_e = REF.motion_consistency_loss(g64, c["mask"].double(), *lv)
        te = (e ** 2).sum(1) / ((lv[2] ** 2).sum(1) + (s ** 2).sum(1) + 1e-24)       # REF's translation term with e exposed: d trans / d e for the partials
        trans2 = (c["mask"].double()[:, 0] * te).mean()
        assert abs(float((trans2 - trans_e).detach())) <= 1e-14 * abs(float(trans_e.detach())) + 1e-300
        (rot_e * c["g_rot"] + trans2 * c["g_trans"]).backward()
        if rot == "identity":
            assert bool(((s.detach().abs().sum(1) == 0) & (lv[2].detach().abs().sum(1) == 0)).any()), "a pixel whose denominator is the 1e-24 guard alone"
        rv = mc_run(V, c, dec)
        den = ((lv[2] ** 2).sum(1) + (s ** 2).sum(1) + 1e-24).detach()
        de = e.grad                # d loss / d e = g 2 e / den, from autograd
        assert float((de - (c["g_trans"] / (N * H * W)) * c["mask"].double() * 2.0 * e.detach() / den.unsqueeze(1)).abs().max()) <= 1e-12 * float(de.abs().max()) + 1e-300
        dRp_ref = torch.stack([ref_tile_sum(de[:, i] * s.detach()[:, j], *TILE) for i in range(3) for j in range(3)], 1)
        part_ref = ref_tile_sum(c["mask"].double()[:, 0] * te.detach(), *TILE)
        c.update({"dec": dec, "v": rv, "ref": {"out": torch.stack([rot_e.detach(), trans_e.detach()]), "dR1": lv[0].grad, "dR2": lv[1].grad, "d_tA": lv[2].grad,
                                                 "d_tB": lv[3].grad, "dR_partial": dRp_ref, "partial": part_ref}})
        c["bounds"] = {k: bound(c["ref"][k], rv[k]) for k in c["ref"]}
        return c
    return cached(("mc", name, rot), build)


def mc_emu(c, fault=None):
    e = mc_run(F32, c, fault=fault)
    return {k: e[k].val for k in c["ref"]}


def mc_check(c, got, name="mc", skip=()):
    for k in c["ref"]:
        if k not in skip:
            check(got[k], c["bounds"][k], f"{name} {k}")        # (nothing left out: d t_B2A included)


# ---------------------------------------------------------------------------------------------------------------------------------------
# WeightedSSIM (make_win, wssim_value, wssim_fwd_kernel, wssim_coef_kernel, wssim_gather, wssim_gather_kernel)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _taps9(t, pad=PB._reflect1):
    H, W = t.val.shape[-2:]
    p = t.map(pad)
    return [p[..., dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)]


def _inside9(H, W):
    """[9, H, W]: whether tap k of the window centred at (y, x) lies inside the image"""
    ys, xs = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    return torch.stack([(ys + dy >= 0) & (ys + dy < H) & (xs + dx >= 0) & (xs + dx < W) for dy in (-1, 0, 1) for dx in (-1, 0, 1)])


def ssim_mode(C1, C2):
    return 1 if C1 == INF else (2 if C2 == INF else 0)


def wssim_win(A, w, fault=None):
    """make_win.  w: A-value [N, 1, H, W] -> (w + 1e-2 at the nine reflected taps, avg_pool2d(w, 3, 1, padding=1): zeros outside, over 9)"""
    H, W = w.val.shape[-2:]
    wt = _taps9(w)
    ins = _inside9(H, W).double()
    zt = wt if fault == "avg_w_reflect" else [wt[k].scale(ins[k]) for k in range(9)]      # 2: avg_w summed over the reflected taps
    n = torch.full_like(w.val, 9.0, dtype=F64) if fault == "avg_w_reflect" else ins.sum(0).expand(w.val.shape)
    return [t + A.c(1e-2) for t in wt], A.sum(zt, n=n) / A.k(9.0)


def wssim_value(A, x, y, wp, aw, mode, C1, C2):
    """wssim_value: the window's weighted moments -> dict (Mom and the unclamped distance l)"""
    xt, yt = _taps9(x), _taps9(y)
    S = lambda f: A.sum([f(k) * wp[k] for k in range(9)])      # noqa: E731
    sx, sy = S(lambda k: xt[k]), S(lambda k: yt[k])
    sxx, syy, sxy = S(lambda k: xt[k] * xt[k]), S(lambda k: yt[k] * yt[k]), S(lambda k: xt[k] * yt[k])
    inv9, inv = A.c(1.0 / 9.0), A.k(1.0) / (aw + A.c(1e-2))
    mx, my = (sx * inv9) * inv, (sy * inv9) * inv
    vx, vy, vxy = (sxx * inv9) * inv - mx * mx, (syy * inv9) * inv - my * my, (sxy * inv9) * inv - mx * my
    one = A.k(1.0)
    n1 = one if mode == 1 else (mx.scale(2.0) * my) + A.k(C1)
    d1 = one if mode == 1 else (mx * mx + my * my) + A.k(C1)
    n2 = one if mode == 2 else vxy.scale(2.0) + A.k(C2)
    d2 = one if mode == 2 else (vx + vy) + A.k(C2)
    n, d = n1 * n2, d1 * d2
    return {"mx": mx, "my": my, "n1": n1, "n2": n2, "d1": d1, "d2": d2, "n": n, "d": d, "inv": inv, "l": (1.0 - n / d).scale(0.5)}


def wssim_fwd(A, x, y, w, C1, C2, fault=None):
    """x, y [N, C, H, W], w [N, 1, H, W]: A-values -> (map, avg_w, moments)"""
    wp, aw = wssim_win(A, w, fault)
    m = wssim_value(A, x, y, wp, aw, ssim_mode(C1, C2), C1, C2)
    return m["l"].maximum(0.0).minimum(1.0), aw, m


def wssim_coef(A, m, g, mode, fault=None, carry=False):
    """wssim_coef_kernel: the four coefficients per window and channel, zero where the clamp does not pass the gradient; V: the windows whose gate
    0 <= l <= 1 the reference cannot decide"""
    f = g.scale(-0.5) * A.c(1.0 / 9.0)
    rd = A.k(1.0) / m["d"]
    zero = A.k(0.0)
    an1 = zero if (mode == 1 and fault != "an1_mode1") else m["n2"] * rd          # 4: an1 not zeroed in mode 1
    an2 = zero if mode == 2 else m["n1"] * rd
    ad1 = zero if mode == 1 else (((-m["n"]) * m["d2"]) * rd) * rd
    ad2 = zero if mode == 2 else (((-m["n"]) * m["d1"]) * rd) * rd
    mx, my = m["mx"], m["my"]
    dmx = ((an1.scale(2.0) * my + ad1.scale(2.0) * mx) - mx.scale(2.0) * ad2) - my.scale(2.0) * an2
    dmy = ((an1.scale(2.0) * mx + ad1.scale(2.0) * my) - my.scale(2.0) * ad2) - mx.scale(2.0) * an2
    k = [(f * dmx) * m["inv"], (f * dmy) * m["inv"], (f * ad2) * m["inv"], (f.scale(2.0) * an2) * m["inv"]]
    l = m["l"]
    ok = (l.val >= 0) & (l.val <= 1)
    und = torch.zeros_like(ok) if A.exact else ((l.val.abs() <= l.err) | ((l.val - 1.0).abs() <= l.err))
    # carry: a window whose gate the reference cannot decide has the coefficient or 0 -- the difference enters every sum that contains it
    z = lambda c: A.where(ok, c, 0.0) if (A.exact or not carry) else A.where(ok, c, 0.0).widen(und.double() * (c.val.abs() + c.err))      # noqa: E731
    return [z(c) for c in k], und


def wssim_gather(A, k, xv, yv, fault=None):
    """wssim_gather: every pixel gathers the up to nine windows that contain it, with the multiplicity reflection gives border taps -> (gx, gy)"""
    H, W = xv.val.shape[-2:]
    my_, mx_ = refl_mult(H), refl_mult(W, "refl_mult" if fault == "gather_mult" else None)      # 1: the multiplicity dropped at px == W - 2
    pk = [c.map(PB._zero1) for c in k]
    tx, ty = [], []
    n = torch.zeros(H, W, dtype=F64)
    for ey in range(3):
        for ex in range(3):
            s = (Ellipsis, slice(ey, ey + H), slice(ex, ex + W))
            m = my_[:, ey].view(H, 1) * mx_[:, ex].view(1, W)
            n += (m > 0).double()
            tx.append(((pk[0][s] + xv.scale(2.0) * pk[2][s]) + yv * pk[3][s]).scale(m))
            ty.append(((pk[1][s] + yv.scale(2.0) * pk[2][s]) + xv * pk[3][s]).scale(m))
    n = n.expand(xv.val.shape)
    return A.sum(tx, n=n), A.sum(ty, n=n)


def dilate3(u):
    return F.max_pool2d(u.double().reshape(1, -1, *u.shape[-2:]), 3, 1, 1).reshape(u.shape) > 0


def wssim_bwd(A, x, y, w, gout, C1, C2, fault=None):
    """sde_wssim_bwd -> (dx, dy, undecided elements)"""
    _, _, m = wssim_fwd(A, x, y, w, C1, C2)
    k, und = wssim_coef(A, m, gout, ssim_mode(C1, C2), fault)
    gx, gy = wssim_gather(A, k, x, y, fault)
    wpc = w if fault == "gather_eps" else w + A.c(1e-2)                             # 3: `+ 1e-2` missing from the centre weight
    return wpc * gx, wpc * gy, dilate3(und)


def wssim_inputs(name):
    N, H, W = IMAGE_SHAPES[name]
    g = torch.Generator().manual_seed(H * W + N)
    x = MI.frames(g, N, H, W, 0.0)
    # y darker than x: the luminance distance (mu_x - mu_y)^2 / (2 d1) of mode (1e-4, inf) stays away from its clamp at 0 (with y = x + noise 2.5 % of
    # the windows lay within their limit of it, 17 % of the gradient elements after the 3 x 3 gather: over the cap, so the input changed, not the cap)
    y = (0.45 * x + 0.05 * torch.randn(N, 3, H, W, generator=g)).clamp(0, 1)
    w = torch.rand(N, 1, H, W, generator=g) * (torch.rand(N, 1, H, W, generator=g) > 0.2)
    return x, y, w, torch.randn(N, 3, H, W, generator=g)


def wssim_case(name, mode):
    def build():
        C1, C2 = (c if c == INF else f32(c) for c in SSIM_MODES[mode])
        x, y, w, go = wssim_inputs(name)
        xr, yr = x.double().requires_grad_(True), y.double().requires_grad_(True)
        mr, ar = REF.weighted_ssim(xr, yr, w.double(), C1, C2)
        mr.backward(go.double())
        vm, va, _ = wssim_fwd(V, V.inp(x), V.inp(y), V.inp(w), C1, C2)
        vdx, vdy, und = wssim_bwd(V, V.inp(x), V.inp(y), V.inp(w), V.inp(go), C1, C2)
        left = und | ~torch.isfinite(vdx.err) | ~torch.isfinite(vdy.err)
        return {"in": (x, y, w, go), "C": (C1, C2), "map": bound(mr, vm), "avg_w": bound(ar, va), "dx": bound(xr.grad, vdx, und), "dy": bound(yr.grad, vdy, und),
                "und": und, "share": float(left.double().mean()), "v": (vm, va, vdx, vdy), "ref": (mr.detach(), ar, xr.grad, yr.grad)}
    return cached(("wssim", name, mode), build)


def wssim_emu(c, fault=None):
    x, y, w, go = (F32.inp(t) for t in c["in"])
    m, a, _ = wssim_fwd(F32, x, y, w, *c["C"], fault)
    dx, dy, _ = wssim_bwd(F32, x, y, w, go, *c["C"], fault)
    return {"map": m.val, "avg_w": a.val, "dx": dx.val, "dy": dy.val}


def wssim_check(c, got, name="wssim"):
    check(got["map"], c["map"], f"{name} map")
    check(got["avg_w"], c["avg_w"], f"{name} avg_w")
    for k in ("dx", "dy"):
        if got.get(k) is not None:
            check(got[k], c[k], f"{name} {k}", True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# view synthesis with a per-pixel translation (make_cam_rt, set_kt, project, proj_valid, store_grid, view_synthesis_pp_kernel)
# ---------------------------------------------------------------------------------------------------------------------------------------
def make_cam_rt(A, K, R):
    """make_cam_rt: k, ki = k^-1, kr = K R (mul, mul, add: no fma); kt is set per pixel.  Entries [N, 1, 1]."""
    e = lambda M, r, c: A.inp(M[:, r, c].reshape(-1, 1, 1))      # noqa: E731
    k = [e(K, i // 3, i % 3) for i in range(9)]
    ki = list(k)
    ki[0], ki[4], ki[2], ki[5] = 1.0 / k[0], 1.0 / k[4], (-k[2]) / k[0], (-k[5]) / k[4]
    kr = [(k[3 * i] * e(R, 0, j) + k[3 * i + 1] * e(R, 1, j)) + k[3 * i + 2] * e(R, 2, j) for i in range(3) for j in range(3)]
    return {"k": k, "ki": ki, "kr": kr, "kt": None}


def set_kt(A, cam, t, fault=None):
    """set_kt: K @ t of every pixel, the fmaf chain of make_cam's kt.  t [N, 3, H, W] fp32."""
    if fault == "kt_pixel0":                                    # 7: kt from pixel 0's translation for every pixel
        t = t[:, :, :1, :1].expand_as(t)
    tt = [A.inp(t[:, c]) for c in range(3)]
    k = cam["k"]
    return {**cam, "kt": [k[3 * i + 2].fma(tt[2], k[3 * i + 1].fma(tt[1], k[3 * i] * tt[0])) for i in range(3)]}


def vs_project(A, K, R, t, depth, dec=None, fault=None):
    cam = set_kt(A, make_cam_rt(A, K, R), t, fault)
    pr = project(A, cam, depth, dec, eps=A.c(1e-6))
    if A.exact:
        assert bool(torch.isfinite(pr["X"].val).all()) and bool(torch.isfinite(pr["Y"].val).all()), "the cases keep X and Y finite (nan_to_num is not restated)"
    pr["cam"] = cam
    return pr


def proj_valid(A, pr, H, W):
    """-> (valid, undecided): X in [0, W - 1), Y in [0, H - 1), q2 > 0; undecided within the error of a boundary"""
    X, Y, q2 = pr["X"], pr["Y"], pr["q"][2]
    ok = (X.val >= 0) & (X.val < W - 1) & (Y.val >= 0) & (Y.val < H - 1) & (q2.val > 0)
    if A.exact:
        return ok, torch.zeros_like(ok)
    und = (X.val.abs() <= X.err) | ((X.val - (W - 1)).abs() <= X.err) | (Y.val.abs() <= Y.err) | ((Y.val - (H - 1)).abs() <= Y.err) | (q2.val.abs() <= q2.err)
    return ok, und


def decisions(pr):
    return {k: pr[k] for k in ("x0", "y0", "passx", "passy")}


def vs_run(A, c, dec=None, fault=None):
    N, H, W = c["shape"]
    pr = vs_project(A, c["K"], c["R"], c["t"], c["depth"], dec, fault)
    valid, und = proj_valid(A, pr, H, W)
    return {"sampled": bilinear(A, tap_values(A, c["img"], pr), pr), "Z": un(pr["q"][2].maximum(A.c(1e-5))), "grid": A.stack([pr["gx"], pr["gy"]], 3),
            "valid": valid.unsqueeze(1), "und": und.unsqueeze(1), "pr": pr}


def cell_mismatch(dec, grid64, H, W):
    """pixels whose fp32 tap cell is not the one the fp64 reference's grid_sample takes"""
    return (torch.floor((grid64[..., 0] + 1) * (W - 1) / 2).long() != dec["x0"]) | (torch.floor((grid64[..., 1] + 1) * (H - 1) / 2).long() != dec["y0"])


def vs_case(name):
    def build():
        v = image_inputs(name)
        N, H, W = IMAGE_SHAPES[name]
        c = {"shape": (N, H, W), "img": torch.cat([v["frame2"], v["depth2"]], 1).contiguous(), "depth": v["depth1"], "K": v["K"], "R": v["R12"], "t": v["t12"]}
        with torch.no_grad():
            r = REF.view_synthesis(c["img"].double(), c["depth"].double(), c["K"].double(), c["R"].double(), c["t"].double())
        ref = {"sampled": r[0], "Z": r[1], "grid": r[2], "valid": r[3]}
        dec = decisions(vs_project(F32, c["K"], c["R"], c["t"], c["depth"]))
        rv = vs_run(V, c, dec)
        mis = cell_mismatch(dec, r[2], H, W).unsqueeze(1)
        samp = rv["sampled"].widen(torch.where(mis, (rv["sampled"].val - r[0]).abs(), torch.zeros(1, dtype=F64)))       # docstring (d): continuity across the cell edge
        c.update({"dec": dec, "ref": ref, "v": rv, "mis": mis, "und": rv["und"], "share": float(rv["und"].double().mean()),
                  "bounds": {"sampled": bound(r[0], samp), "Z": bound(r[1], rv["Z"]), "grid": bound(r[2], rv["grid"])}})
        return c
    return cached(("vs", name), build)


def vs_emu(c, fault=None):
    e = vs_run(F32, c, fault=fault)
    return {"sampled": e["sampled"].val, "Z": e["Z"].val, "grid": e["grid"].val, "valid": e["valid"]}


def check_mask(got, ref, und, name):
    """a mask: the reference's value wherever the reference decides it, either value at an undecided pixel"""
    bad = (got.detach().cpu().bool().reshape(ref.shape) != ref.bool()) & ~und.reshape(ref.shape)
    _record(torch.float32, name, 0.0 if not bool(bad.any()) else INF)
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} decided pixels differ from the reference; first at {tuple(int(v) for v in bad.nonzero()[0])}"


def vs_check(c, got, name="view_synthesis"):
    for k in ("sampled", "Z", "grid"):
        check(got[k], c["bounds"][k], f"{name} {k}")
    check_mask(got["valid"], c["ref"]["valid"], c["und"], f"{name} valid")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the per-scale glue (prep_pool_kernel, prep_fwd_finalize_kernel, prep_scale_kernel, prep_bwd_reduce_kernel, prep_bwd_finalize_kernel,
# prep_bwd_gather_kernel)
# ---------------------------------------------------------------------------------------------------------------------------------------
# (N, H0, W0, h, w): uneven windows; N = 4 with the identity pool (the half swap n <-> n + N / 2 differs from n ^ 1 only at N = 4); a pooled grid of
# 2 x 2 workgroups per sample
PREP_SHAPES = {"N2-9x70-4x33": (2, 9, 70, 4, 33), "N4-6x10-identity": (4, 6, 10, 6, 10), "N2-10x140-5x70": (2, 10, 140, 5, 70)}
PREP_MODES = {"motion-mask": (True, True), "motion": (True, False), "no-motion": (False, False)}
PREP_COT = ("depth_r", "depth_n", "t", "m_norm", "t_sw")


def prep_inputs(shape, motion, mask):
    N, H0, W0, h, w = shape
    g = torch.Generator().manual_seed(N * 1000 + H0 * 10 + h)
    v = {"depth": torch.rand(N, 1, H0, W0, generator=g) * 30 + 2, "t_pose": torch.randn(N, 3, generator=g) * 0.3,
         "motion": torch.randn(N, 3, H0, W0, generator=g) * 0.2 if motion else None,
         "mask": (torch.rand(N, 1, H0, W0, generator=g) > 0.4).float() if mask else None}
    cot = {k: torch.randn(N, 1 if k.startswith("depth") else 3, h, w, generator=g) for k in PREP_COT}      # one cotangent per differentiable output
    return v, cot


def half_swap(N, fault=None):
    n = torch.arange(N)
    return (n ^ 1) if fault == "swap_xor" else torch.where(n < N // 2, n + N // 2, n - N // 2)      # 14: the swap index n ^ 1


def prep_fwd(A, c, fault=None):
    """sde_motion_prep_fwd on the case's inputs -> dict of A-values (None: the output does not exist in this mode)"""
    N, H0, W0, h, w = c["shape"]
    hw, normalize, v = h * w, c["normalize"], c["in"]
    depth_r = avgpool_fwd(A, A.inp(v["depth"][:, 0]), h, w)
    tp = un(un(A.inp(v["t_pose"]), 2), 3)
    m_r = None
    if v["motion"] is not None:
        mm = A.inp(v["motion"]) * A.inp(v["mask"]) if v["mask"] is not None else A.inp(v["motion"])
        m_r = avgpool_fwd(A, mm.map(lambda t: t.reshape(N * 3, H0, W0)), h, w).map(lambda t: t.reshape(N, 3, h, w))
        t0 = tp + m_r
    else:
        t0 = tp.map(lambda t: t.expand(N, 3, h, w))
    partial = A.stack([tile_sum(A, depth_r, *TILE), tile_sum(A, A.sum([t0[:, k] * t0[:, k] for k in range(3)]), *TILE)], 1)
    per = slab_sum(A, partial, N)
    mu = per[:, 0].sumdim(0) / A.k(N * hw) if normalize else A.k(1.0)
    q = (per[:, 1] / (mu * mu)) / A.k(hw)
    sq = (q + A.c(1e-12)).sqrt()
    flat = lambda t: t.map(lambda x: x.reshape(-1))      # noqa: E731
    stats = A.stack([flat(mu), flat(A.k(1.0) / mu)], 0).map(lambda x: x.reshape(-1))
    stats = A.stack([stats.map(lambda x: F.pad(x, (0, N - 2))) if N > 2 else stats, sq, q, per[:, 0], per[:, 1]], 0)      # rows: (mu, 1 / mu, ..), sq, q, per
    dn, t = (depth_r / mu, t0 / mu) if normalize else (depth_r, t0)
    sq4 = sq.map(lambda x: x.reshape(N, 1, 1, 1))
    m_norm = None if m_r is None else ((m_r / mu) if normalize else m_r) / sq4
    sw = half_swap(N, fault)
    return {"depth_r": un(depth_r), "depth_n": un(dn) if normalize else None, "t": t, "overall": t0 if normalize else None, "m_norm": m_norm,
            "depth_n_sw": un(dn).map(lambda x: x[sw]), "t_sw": t.map(lambda x: x[sw]), "partial": partial, "stats": stats}


def prep_stats_vector(st, N):
    """the rows of prep_fwd's `stats` as the kernel lays them out: mu, 1 / mu, sq [N], q [N], per [N][2]"""
    return torch.cat([st[0, :2], st[1], st[2], torch.stack([st[3], st[4]], 1).reshape(-1)])


def prep_bwd(A, c, st, fault=None):
    """sde_motion_prep_bwd.  st: the stored operands as A-values (depth_n, t, m_norm, rmu, sq, q) -> d_depth, d_motion, d_tpose, partial, bstats"""
    N, H0, W0, h, w = c["shape"]
    hw, normalize, v, cot = h * w, c["normalize"], c["in"], c["cot"]
    motion = v["motion"] is not None
    sw = half_swap(N, fault)
    gt = A.inp(cot["t"]) + A.inp(cot["t_sw"][sw])
    t = st["t"]
    zero = A.inp(torch.zeros(N, h, w))
    v0 = A.sum([A.inp(cot["m_norm"][:, k]) * st["m_norm"][:, k] for k in range(3)]) if motion else zero
    v1 = A.sum([gt[:, k] * t[:, k] for k in range(3)])
    v2 = A.inp(cot["depth_n"][:, 0]) * st["depth_n"][:, 0] if normalize else zero
    partial = A.stack([tile_sum(A, x, *TILE) for x in [v0, v1, v2] + [gt[:, k] for k in range(3)] + [t[:, k] for k in range(3)]], 1)
    p = slab_sum(A, partial, N)
    hwf, r = A.k(hw), (st["rmu"] if normalize else A.k(1.0))
    cn = ((-p[:, 0]) / (st["sq"] * st["sq"])) / hwf if motion else A.inp(torch.zeros(N))
    d_tpose = A.stack([r * (p[:, 3 + k] + cn * p[:, 6 + k]) for k in range(3)], 1)
    tot = (((p[:, 1] + cn * (st["q"] * hwf)) + p[:, 0]) + p[:, 2]).sumdim(0)
    gmu = ((-r) * tot) / A.k(N * hw) if normalize else A.k(0.0)
    g = gmu + A.inp(cot["depth_r"][:, 0])
    if normalize:
        g = g + A.inp(cot["depth_n"][:, 0]) * r
    out = {"d_depth": un(avgpool_bwd(A, g, H0, W0)), "d_motion": None, "d_tpose": d_tpose, "partial": partial,
           "bstats": A.stack([gmu.map(lambda x: x.reshape(1).expand(N)), cn] + [p[:, k] for k in range(9)], 0)}
    if motion:
        gm = (gt + cn.map(lambda x: x.reshape(N, 1, 1, 1)) * t) + A.inp(cot["m_norm"]) * (A.k(1.0) / st["sq"]).map(lambda x: x.reshape(N, 1, 1, 1))
        dm = avgpool_bwd(A, (r * gm).map(lambda x: x.reshape(N * 3, h, w)), H0, W0).map(lambda x: x.reshape(N, 3, H0, W0))
        out["d_motion"] = dm.scale(v["mask"].double()) if v["mask"] is not None else dm
    return out


def prep_bstats_vector(bs, N):
    return torch.cat([bs[0, :1], bs[1], bs[2:].t().reshape(-1)])


def prep_case(shape, mode, normalize):
    def build():
        import motion_model_ref as MM
        N, H0, W0, h, w = PREP_SHAPES[shape]
        motion, mask = PREP_MODES[mode]
        v, cot = prep_inputs(PREP_SHAPES[shape], motion, mask)
        c = {"shape": PREP_SHAPES[shape], "normalize": int(normalize), "in": v, "cot": cot}
        d = {k: None if x is None else x.double() for k, x in v.items()}
        leaves = [d[k].requires_grad_(True) for k in ("depth", "t_pose")] + ([d["motion"].requires_grad_(True)] if motion else [])
        o = MM.pair_prep(d["depth"], d["motion"], d["t_pose"], d["mask"], (h, w), bool(normalize))
        keys = [k for k in PREP_COT if o[k] is not None and (k != "depth_n" or normalize)]
        sum((o[k] * cot[k].double()).sum() for k in keys).backward()
        with torch.no_grad():
            t0 = o["overall_motion"]
            mu = o["depth_r"].mean() if normalize else torch.ones((), dtype=F64)
            q = o["t"].pow(2).mean([1, 2, 3]) * 3.0
            sq = torch.sqrt(q + 1e-12)
            per = torch.stack([o["depth_r"].sum([1, 2, 3]), t0.pow(2).sum([1, 2, 3])], 1)
            stats = torch.cat([mu.reshape(1), 1.0 / mu.reshape(1), sq, q, per.reshape(-1)])
            part = torch.stack([ref_tile_sum(o["depth_r"][:, 0], *TILE), ref_tile_sum(t0.pow(2).sum(1), *TILE)], 1)
        ref = {"depth_r": o["depth_r"], "depth_n": o["depth_n"] if normalize else None, "t": o["t"], "overall": t0 if normalize else None, "m_norm": o["m_norm"],
               "depth_n_sw": o["depth_n_sw"], "t_sw": o["t_sw"], "partial": part, "stats": stats}
        fv = prep_fwd(V, c)
        fv["stats"] = fv["stats"].map(lambda x: prep_stats_vector(x, N))
        c["stored_ref"] = {"depth_n": o["depth_n"].detach(), "t": o["t"].detach(), "m_norm": None if o["m_norm"] is None else o["m_norm"].detach(), "rmu": 1.0 / mu, "sq": sq, "q": q}
        bv = prep_bwd(V, c, {k: None if x is None else stored(V, x) for k, x in c["stored_ref"].items()})
        bv["bstats"] = bv["bstats"].map(lambda x: prep_bstats_vector(x, N))
        gref = {"d_depth": leaves[0].grad, "d_tpose": leaves[1].grad, "d_motion": leaves[2].grad if motion else None}
        c.update({"fwd": {k: bound(ref[k].detach(), fv[k]) for k in ref if ref[k] is not None}, "fv": fv, "bv": bv, "ref": ref, "gref": gref,
                  "bwd": {**{k: bound(gref[k], bv[k]) for k in gref if gref[k] is not None},
                          # scratch of the backward: no autograd counterpart -- the restated formula in exact arithmetic, whose outputs are autograd's (vjp_agrees)
                          "partial": bound(bv["partial"].val, bv["partial"]), "bstats": bound(bv["bstats"].val, bv["bstats"])}})
        return c
    return cached(("prep", shape, mode, normalize), build)


def prep_stored_f32(c):
    """what the isolated backward reads: the reference's depth_n, t, m_norm and stats, rounded to fp32"""
    s, N = c["stored_ref"], c["shape"][0]
    f = lambda x: None if x is None else x.float()      # noqa: E731
    stats = torch.cat([(1.0 / s["rmu"]).reshape(1), s["rmu"].reshape(1), s["sq"], s["q"], torch.zeros(2 * N, dtype=F64)]).float()
    return {"depth_n": f(s["depth_n"]), "t": f(s["t"]), "m_norm": f(s["m_norm"]), "stats": stats}


def prep_emu(c, fault=None):
    N = c["shape"][0]
    e = prep_fwd(F32, c, fault)
    out = {k: x.val for k, x in e.items() if x is not None and k != "stats"}
    out["stats"] = prep_stats_vector(e["stats"].val, N)
    b = prep_bwd(F32, c, {k: None if x is None else stored(F32, x) for k, x in c["stored_ref"].items()}, fault)
    out.update({"b_" + k: x.val for k, x in b.items() if x is not None and k != "bstats"})
    out["b_bstats"] = prep_bstats_vector(b["bstats"].val, N)
    return out


def prep_check(c, got, name="prep"):
    """got: forward outputs by name, backward outputs as b_<name>"""
    for k, b in c["fwd"].items():
        check(got[k], b, f"{name} {k}")
    for k, b in c["bwd"].items():
        check(got["b_" + k], b, f"{name} {k}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# RGB-D consistency (rgbd_warp_kernel, sample_m2, wssim_fwd_kernel on pass 1's outputs, rgbd_finalize_kernel; wssim_coef_kernel, rgbd_bwd_kernel,
# sum9_finalize_kernel)
# ---------------------------------------------------------------------------------------------------------------------------------------
def rgbd_fwd(A, c, dec=None, fault=None):
    """sde_rgbd_fwd -> dict of A-values (masks as bool tensors): sampled, grid, occ, err, valid, dpw, part1 [nblk, 4], part2 [nblk], stats [4, N];
    V only: und_valid, und_occ"""
    N, H, W = c["shape"]
    pr = vs_project(A, c["K"], c["R"], c["t"], c["dA"], dec, fault)
    valid, und_v = proj_valid(A, pr, H, W)
    Z = pr["q"][2].maximum(A.c(1e-5))
    sD = bilinear(A, tap_values(A, c["dB"], pr), pr)[:, 0]
    e = Z - sD
    occ = (Z.val < sD.val) & (valid if fault != "occ_no_ok" else torch.ones_like(valid))           # 5: occ without `&& ok`
    if A.exact:
        und_o = torch.zeros_like(occ)
        occ_a, valid_a = F32(occ.float()), F32(valid.float())
    else:      # (d): an undecided mask pixel enters every sum that contains it with its possible jump as error
        und_o = ((e.val.abs() <= e.err) & (valid | und_v)) | (und_v & (e.val < e.err))
        occ_a, valid_a = V(occ.double(), und_o.double()), V(valid.double(), und_v.double())
    sampled = bilinear(A, tap_values(A, c["fB"], pr), pr)
    fA = A.inp(c["fA"])
    l1 = A.sum([(sampled[:, k] - fA[:, k]).abs() * occ_a for k in range(3)])
    part1 = A.stack([tile_sum(A, x, *TILE) for x in (occ_a, (e * e) * occ_a, l1, (sD - Z).abs() * occ_a)], 1)
    out = {"sampled": sampled, "grid": A.stack([pr["gx"], pr["gy"]], 3), "occ": occ.unsqueeze(1), "err": un(e), "valid": valid.unsqueeze(1), "part1": part1,
           "und_valid": und_v.unsqueeze(1), "und_occ": und_o.unsqueeze(1), "pr": pr, "dpw": None, "part2": None}
    tot = slab_sum(A, part1, N, fault)                                                                 # [N, 4]
    nrm = tot[:, 0] + 1.0
    if c["ssim"]:
        m2 = (tot[:, 1] / nrm + A.c(1e-4)).map(lambda x: x.reshape(N, 1, 1))                         # sample_m2
        out["dpw"] = un((m2 / (e * e + m2)) * valid_a)
    out["stats"] = A.stack([tot[:, 2], tot[:, 3] / nrm, nrm], 0)                                       # rows 0, 2, 3
    if A.exact and c["ssim"]:
        _, out["part2"], out["stats1"] = rgbd_pass2(F32, c, sampled.val, e.val.unsqueeze(1), valid.unsqueeze(1), part1.val, fault)
    return out


def rgbd_pass2(A, c, sampled, err, valid, part1, fault=None, dpw=None):
    """Pass 2 of sde_rgbd_fwd on pass 1's OWN outputs (fp32 tensors, exact operands): the weight from err, valid and the sample's sums of part1
    (sample_m2), the weighted SSIM of (sampled, frame_A) and its per-workgroup and per-sample sums -> (part2 [nblk], stats row 1 [N]).
    Why on pass 1's outputs: propagated from the inputs, the error of `sampled` (some 1e-6) meets E[x^2 w] / E[w] - mu^2 against C2 = 9e-6 as if the
    moments were independent; the limit of part2 came out 4 to 120 times its value, or infinite.  So each pass is held on the operands it reads, as
    the backward kernels are: pass 1's outputs per element against the fp64 reference, pass 2 against the fp64 formula on those outputs.  The weight
    is such a boundary too (it is an output, `dpw`, and every tap's weight is the same expression): formed from (err, valid, part1) it is checked on its
    own, and the SSIM sums run on it as an exact operand (dpw given) -- m2's any-order sum error, 1.5e-5 relative at 257 partials, otherwise does to the
    moments what the error of `sampled` does.  -> (dpw, part2 [nblk], stats row 1 [N])"""
    N, H, W = c["shape"]
    tot = slab_sum(A, A.inp(part1), N, fault)
    m2 = (tot[:, 1] / (tot[:, 0] + 1.0) + A.c(1e-4)).map(lambda x: x.reshape(N, 1, 1, 1))
    e = A.inp(err)
    wv = (m2 / (e * e + m2)).scale(valid.double()) if dpw is None else A.inp(dpw)
    wp, aw = wssim_win(A, wv)
    m = wssim_value(A, A.inp(sampled), A.inp(c["fA"]), wp, aw, ssim_mode(c["C1"], c["C2"]), c["C1"], c["C2"])
    l = m["l"].maximum(0.0).minimum(1.0)
    part2 = tile_sum(A, A.sum([l[:, k] * aw[:, 0] for k in range(3)]), *TILE)
    return wv, part2, slab_sum(A, un(part2), N, fault)[:, 0]


def rgbd_pass2_bounds(c, got):
    """the fp64 formula (REF.weighted_ssim on the weight REF's lines give) on the run's own pass-1 outputs, with the limit of the chain on them"""
    N, H, W = c["shape"]
    sampled, err, valid, part1 = (got[k].detach().cpu() for k in ("sampled", "err", "valid", "part1"))
    valid = valid.reshape(N, 1, H, W) != 0
    p1 = part1.double().reshape(N, -1, 4).sum(1)
    m2 = (p1[:, 1] / (p1[:, 0] + 1) + 1e-4).view(N, 1, 1, 1)
    dpw = (m2 / (err.double() ** 2 + m2)) * valid.double()
    vd, _, _ = rgbd_pass2(V, c, sampled, err, valid, part1)
    w = got["dpw"].detach().cpu().reshape(N, 1, H, W)
    smap, avg_w = REF.weighted_ssim(sampled.double(), c["fA"].double(), w.double(), c["C1"], c["C2"])
    acc = (smap * avg_w).sum(1)
    _, vp, vs = rgbd_pass2(V, c, sampled, err, valid, part1, dpw=w)
    return bound(dpw, vd), bound(ref_tile_sum(acc, *TILE), vp), bound(acc.sum([1, 2]), vs)


RGBD_FWD_OUT = ("sampled", "grid", "err", "dpw", "part1", "stats")


def rgbd_ref(c):
    """the per-sample quantities of REF.rgbd_consistency_loss in fp64 (its own lines, kept per sample instead of averaged), checked against its losses"""
    d = {k: c[k].double() for k in ("fA", "fB", "dA", "dB", "K", "R", "t")}
    N, H, W = c["shape"]
    with torch.no_grad():
        sampled, Z, grid, valid = REF.view_synthesis(torch.cat([d["fB"], d["dB"]], 1), d["dA"], d["K"], d["R"], d["t"])
        sF, sD = sampled[:, :3], sampled[:, 3:]
        occ = (Z < sD).double() * valid.double()
        nrm = occ.sum([1, 2, 3]) + 1
        err = Z - sD
        r = {"sampled": sF, "grid": grid, "occ": occ.bool(), "err": err, "valid": valid, "Z": Z, "sD": sD}
        l1 = ((sF - d["fA"]).abs() * occ).sum(1)
        per = [occ[:, 0], (err ** 2 * occ)[:, 0], l1, ((sD - Z).abs() * occ)[:, 0]]
        r["part1"] = torch.stack([ref_tile_sum(x, *TILE) for x in per], 1)
        stats = [l1.sum([1, 2]), per[3].sum([1, 2]) / nrm, nrm]
        o = REF.rgbd_consistency_loss(d["fA"], d["fB"], d["dA"], d["dB"], d["K"], d["R"], d["t"], 1.0, 2.0 if c["ssim"] else 0.0, c["C1"], c["C2"])
        close = lambda a, b: abs(float(a) - float(b)) <= 1e-12 * abs(float(b)) + 1e-300      # noqa: E731
        assert close(stats[0].sum() / (N * 3 * H * W), o["rgb_l1_loss"]) and close(stats[1].mean(), o["depth_l1_loss"])
        if c["ssim"]:
            m2 = ((err ** 2 * occ).sum([1, 2, 3]) / nrm + 1e-4).view(-1, 1, 1, 1)
            r["dpw"] = (m2 / (err ** 2 + m2)) * valid.double()
            smap, avg_w = REF.weighted_ssim(sF, d["fA"], r["dpw"], c["C1"], c["C2"])
            acc = (smap * avg_w).sum(1)
            assert close(acc.sum() / (N * 3 * H * W), o["ssim_loss"]) and float((r["dpw"] - o["depth_proximity_weight"]).abs().max()) <= 1e-14
        r["stats"] = torch.stack(stats, 0)
    return r


RGBD_FWD_CASES = [(n, "c2") for n in IMAGE_SHAPES] + [("2x9x130", "both"), ("3x3", "c1"), ("5x65", "none")]


def rgbd_inputs(name, mode):
    v = image_inputs(name)
    C1, C2 = (x if x == INF else f32(x) for x in SSIM_MODES.get(mode, SSIM_MODES["c2"]))
    return {"shape": IMAGE_SHAPES[name], "fA": v["frame1"], "fB": v["frame2"], "dA": v["depth1"], "dB": v["depth2"], "K": v["K"], "R": v["R12"], "t": v["t12"],
            "ssim": int(mode != "none"), "C1": C1, "C2": C2}


def rgbd_fwd_case(name, mode="c2"):
    def build():
        c = rgbd_inputs(name, mode)
        N, H, W = c["shape"]
        ref = rgbd_ref(c)
        dec = decisions(vs_project(F32, c["K"], c["R"], c["t"], c["dA"]))
        assert not bool(cell_mismatch(dec, ref["grid"], H, W).any()), "the fp32 tap cells are the fp64 ones on these cases (change the input otherwise)"
        fv = rgbd_fwd(V, c, dec)
        c.update({"dec": dec, "ref": ref, "fv": fv, "und_valid": fv["und_valid"], "und_occ": fv["und_occ"],
                  "share": float((fv["und_valid"] | fv["und_occ"]).double().mean()),
                  "bounds": {k: bound(ref[k], fv[k]) for k in RGBD_FWD_OUT if fv[k] is not None}})
        return c
    return cached(("rgbd_fwd", name, mode), build)


def rgbd_fwd_emu(c, fault=None):
    e = rgbd_fwd(F32, c, fault=fault)
    out = {**{k: e[k].val for k in RGBD_FWD_OUT if e[k] is not None}, "occ": e["occ"], "valid": e["valid"]}
    if c["ssim"]:
        out["part2"], out["stats1"] = e["part2"].val, e["stats1"].val
    return out


def rgbd_fwd_check(c, got, name="rgbd_fwd"):
    for k, b in c["bounds"].items():
        check(got[k], b, f"{name} {k}")
    check_mask(got["valid"], c["ref"]["valid"], c["und_valid"], f"{name} valid")
    check_mask(got["occ"], c["ref"]["occ"], c["und_occ"], f"{name} occ")
    if c["ssim"]:
        bd, bp, bs = rgbd_pass2_bounds(c, got)
        check(got["dpw"], bd, f"{name} dpw (on pass 1's outputs)")
        check(got["part2"], bp, f"{name} part2 (on pass 1's outputs)")
        check(got["stats1"], bs, f"{name} stats row 1 (on pass 1's outputs)")


def ref_warp(c, depth, R, t, dec):
    """REF.view_synthesis restated so that it is differentiable in (depth, R, t) with the tap cell and the clamp's pass flags given (photo_bounds.
    photo_ref_sample(dec=)): the same function wherever fp64 takes the decisions of the fp32 chain -> (sampled frame_B, q2, back-projected points p)"""
    N, H, W = c["shape"]
    K = c["K"].double()
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)], 0)[None] * depth
    Kinv = K.clone()
    Kinv[:, 0, 0], Kinv[:, 1, 1] = 1.0 / K[:, 0, 0], 1.0 / K[:, 1, 1]
    Kinv[:, 0, 2], Kinv[:, 1, 2] = -K[:, 0, 2] / K[:, 0, 0], -K[:, 1, 2] / K[:, 1, 1]
    pts = Kinv.bmm(pix.reshape(N, 3, -1))
    q = K.bmm(R).bmm(pts) + K.bmm(t.reshape(N, 3, -1))
    X, Y = (q[:, 0] / (q[:, 2] + 1e-6)).view(N, H, W), (q[:, 1] / (q[:, 2] + 1e-6)).view(N, H, W)
    Xc, Yc = torch.where(dec["passx"], X, X.clamp(0, W - 1).detach()), torch.where(dec["passy"], Y, Y.clamp(0, H - 1).detach())
    ix, iy = (2 * Xc / (W - 1) - 1.0 + 1.0) * ((W - 1) / 2), (2 * Yc / (H - 1) - 1.0 + 1.0) * ((H - 1) / 2)
    return PB._sample_in_cell(c["fB"].double(), ix, iy, dec["x0"], dec["y0"]), q[:, 2].view(N, H, W), pts.view(N, 3, H, W)


def rgbd_bwd(A, c, st, g, dec=None, fault=None):
    """sde_rgbd_bwd on the stored operands st = (sampled, occ, err, dpw, nrm): fp32 tensors, exact (the reference's dL / d sampled is taken at the same
    stored values: photo_bounds docstring (c)).  g = (g_l1, g_ssim, g_dl1, gscale): [N] fp32 tensors or None.
    -> d_depth [N, H, W], d_t [N, 3, H, W], dR_partial [nblk, 9], dR [N, 3, 3]; V only: und [N, H, W], the elements left out"""
    N, H, W = c["shape"]
    sampled, occ, err, dpw, nrm = st
    g_l1, g_ssim, g_dl1, gscale = g
    X_, fA = A.inp(sampled), A.inp(c["fA"])
    per = lambda v: A.inp(v).map(lambda x: x.reshape(N, 1, 1))      # noqa: E731
    und = torch.zeros(N, H, W, dtype=torch.bool)
    zero4 = A.inp(torch.zeros(N, 3, H, W))
    ssim_term = zero4
    if c["ssim"] and g_ssim is not None:
        w = A.inp(dpw)
        wp, aw = wssim_win(A, w)
        m = wssim_value(A, X_, fA, wp, aw, ssim_mode(c["C1"], c["C2"]), c["C1"], c["C2"])
        k, u_ = wssim_coef(A, m, un((per(g_ssim) * A.k(gscale)) * aw[:, 0]), ssim_mode(c["C1"], c["C2"]), fault, carry=True)
        und |= dilate3(u_).any(1)
        gx, _ = wssim_gather(A, k, X_, fA, fault)
        ssim_term = (w + A.c(1e-2)) * gx
    df = sampled.double() - c["fA"].double()
    sg = torch.sign(df)
    l1_term = un((per(g_l1) if g_l1 is not None else A.k(0.0)) * A.inp(occ[:, 0])).map(lambda x: x.expand(N, 3, H, W)).scale(sg)
    ds = ssim_term + l1_term
    pr = vs_project(A, c["K"], c["R"], c["t"], c["dA"], dec, fault)
    cam = pr["cam"]
    if not A.exact:
        und |= PB.undecided_coord(pr, H, W)
    nw, ne, sw, se = tap_values(A, c["fB"], pr)
    # from here on everything is linear in ds and uses it with opposite signs (photo_bounds.photo_bwd): the chain runs on ds as an exact operand, and the
    # error of ds enters through its exact coefficient in each output
    ds_err, ds = (None, ds) if A.exact else (ds.err + 0.0 * ds.val, V(ds.val))
    gIx, gIy = tap_gradient(A, (ne - nw, se - sw), pr["wy"]), tap_gradient(A, (sw - nw, se - ne), pr["wx"])
    tx, ty = ds * gIx, ds * gIy
    dX = A.where(pr["passx"], A.sum([tx[:, 0], tx[:, 1], tx[:, 2]]), 0.0)
    dY = A.where(pr["passy"], A.sum([ty[:, 0], ty[:, 1], ty[:, 2]]), 0.0)
    q2 = pr["q"][2]
    se_ = torch.sign(err[:, 0].double())
    if fault == "dl1_sign":                                  # 6: the depth-L1 sign taken from sD - Z
        se_ = -se_
    on = (occ[:, 0] != 0) & (q2.val >= f32(1e-5))
    if not A.exact:
        und |= (occ[:, 0] != 0) & ((q2.val - 1e-5).abs() <= q2.err) & (g_dl1 is not None)
    gdl = per(g_dl1) / per(nrm) if g_dl1 is not None else A.k(0.0)
    dZ = A.where(on, gdl.map(lambda x: x.expand(N, H, W)).scale(se_), 0.0)
    rden = 1.0 / pr["den"]
    dq = [dX * rden, dY * rden, (-(dX * pr["X"] + dY * pr["Y"])) * rden + dZ]
    ki, kr, k = cam["ki"], cam["kr"], cam["k"]
    ray = [(ki[3 * i] * pr["fx"] + ki[3 * i + 1] * pr["fy"]) + ki[3 * i + 2] for i in range(3)]
    dd = [((dq[0] * kr[i] + dq[1] * kr[3 + i]) + dq[2] * kr[6 + i]) * ray[i] for i in range(3)]
    kq = [(k[m_] * dq[0] + k[3 + m_] * dq[1]) + k[6 + m_] * dq[2] for m_ in range(3)]
    acc = [kq[m_] * pr["p"][i] for m_ in range(3) for i in range(3)]
    if not A.exact:
        sup = lambda v: v.val.abs() + v.err      # noqa: E731
        px, py = pr["passx"].double().unsqueeze(1), pr["passy"].double().unsqueeze(1)

        def lin(cx, cy):
            return (sup((gIx * un(cx)).scale(px) + (gIy * un(cy)).scale(py)) * ds_err).sum(1)
        a = [V.sum([kr[3 * r + i] * ray[i] for i in range(3)]) for r in range(3)]
        dd[0] = dd[0].widen(lin((a[0] - pr["X"] * a[2]) * rden, (a[1] - pr["Y"] * a[2]) * rden))
        for m_ in range(3):
            e = lin((k[m_] - pr["X"] * k[6 + m_]) * rden, (k[3 + m_] - pr["Y"] * k[6 + m_]) * rden)
            kq[m_] = kq[m_].widen(e)
            for i in range(3):
                acc[3 * m_ + i] = acc[3 * m_ + i].widen(e * sup(pr["p"][i]))
    dRp = A.stack([tile_sum(A, x + A.inp(torch.zeros(N, H, W)), *TILE) for x in acc], 1)
    return {"d_depth": un(A.sum(dd)), "d_t": A.stack(kq, 1), "dR_partial": dRp, "dR": slab_sum(A, dRp, N, fault).map(lambda x: x.reshape(N, 3, 3)), "und": und, "pr": pr}


RGBD_BWD_OUT = ("d_depth", "d_t", "dR_partial", "dR")
RGBD_G = {"all": (0.8, 1.1, 0.6), "no_l1": (None, 1.1, 0.6), "no_ssim": (0.8, None, 0.6), "no_dl1": (0.8, 1.1, None)}
RGBD_BWD_CASES = [(n, "c2", "all") for n in IMAGE_SHAPES] + [("2x9x130", "both", "all"), ("3x3", "c1", "all"), ("5x65", "c2", "no_l1"), ("5x65", "c2", "no_ssim"),
                                                            ("5x65", "c2", "no_dl1"), ("5x65", "none", "all")]
GSCALE = 0.5


def rgbd_bwd_case(name, mode="c2", gsel="all"):
    def build():
        f = rgbd_fwd_case(name, mode)
        c = {k: f[k] for k in ("shape", "fA", "fB", "dA", "dB", "K", "R", "t", "ssim", "C1", "C2", "dec")}
        N, H, W = c["shape"]
        r = f["ref"]
        # (c): what the backward reads, from the reference, rounded to fp32; two pixels per sample where the stored sample equals frame_A (sign 0)
        sampled = r["sampled"].float().clone()
        for (y, x) in ((0, 1), (H - 1, 0)):
            sampled[:, :, y, x] = c["fA"][:, :, y, x]
        st = (sampled, r["occ"].float(), r["err"].float(), r["dpw"].float() if c["ssim"] else None, r["stats"][2].float())
        scale = (1.0 + 0.25 * torch.arange(N, dtype=torch.float32))
        g = tuple(None if x is None else (f32(x) * scale) for x in RGBD_G[gsel]) + (f32(GSCALE),)
        c.update({"stored": st, "g": g})
        dec = {**c["dec"]}
        bv = rgbd_bwd(V, c, st, g, dec)
        und = bv["und"] | ~torch.isfinite(bv["d_depth"].err[:, 0]) | ~torch.isfinite(bv["d_t"].err).all(1)
        # stage 1: dL / dS at the stored samples (weight, mask and normaliser are constants)
        S = sampled.double().requires_grad_(True)
        fA, occ = c["fA"].double(), st[1].double()
        L = torch.zeros((), dtype=F64)
        if g[0] is not None:
            L = L + (((S - fA).abs() * occ).sum([1, 2, 3]) * g[0].double()).sum()
        if c["ssim"] and g[1] is not None:
            smap, avg_w = REF.weighted_ssim(S, fA, st[3].double(), c["C1"], c["C2"])
            L = L + ((smap * avg_w).sum([1, 2, 3]) * g[1].double() * g[3]).sum()
        dS = torch.autograd.grad(L, S)[0] if L.requires_grad else torch.zeros_like(S)
        # stage 2: <dL / dS, S(depth, R, t)> + the depth-L1 term with the stored sign and normaliser
        lv = [c[k].double().requires_grad_(True) for k in ("dA", "R", "t")]
        Sf, q2, pts = ref_warp(c, *lv, dec)
        obj = (dS * Sf).sum()
        if g[2] is not None:
            Zc = q2.clamp(min=1e-5)
            obj = obj + ((torch.sign(st[2].double()[:, 0]) * occ[:, 0] * Zc).sum([1, 2]) * g[2].double() / st[4].double()).sum()
        gd, gR, gt = torch.autograd.grad(obj, lv)
        dRp = torch.stack([ref_tile_sum(gt[:, m_] * pts.detach()[:, i], *TILE) for m_ in range(3) for i in range(3)], 1)      # d R_mk = sum (d t_m) p_k
        assert float((dRp.reshape(N, -1, 9).sum(1).reshape(N, 3, 3) - gR).abs().max()) <= 1e-10 * float(gR.abs().max()) + 1e-300
        ref = {"d_depth": gd, "d_t": gt, "dR_partial": dRp, "dR": gR}
        u4 = und.unsqueeze(1)
        c.update({"bv": bv, "ref": ref, "und": und, "share": float(und.double().mean()),
                  "bounds": {"d_depth": bound(gd, bv["d_depth"], u4), "d_t": bound(gt, bv["d_t"], u4.expand(N, 3, H, W)), "dR_partial": bound(dRp, bv["dR_partial"]),
                             "dR": bound(gR, bv["dR"])}})
        return c
    return cached(("rgbd_bwd", name, mode, gsel), build)


def rgbd_bwd_emu(c, fault=None):
    e = rgbd_bwd(F32, c, c["stored"], c["g"], fault=fault)
    return {k: e[k].val for k in RGBD_BWD_OUT}


def rgbd_bwd_check(c, got, name="rgbd_bwd"):
    for k in RGBD_BWD_OUT:
        check(got[k], c["bounds"][k], f"{name} {k}", k in ("d_depth", "d_t"))

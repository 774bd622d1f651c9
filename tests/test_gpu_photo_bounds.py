"""GPU: the loss kernels of csrc/photometric.hip through the C ABI against tests/photo_bounds.py -- every element of every output within its own
limit from the fp64 reference, every output carved out of a guarded buffer (all of it written, the ragged last tiles included, nothing outside).

Shapes: 4 x 4 (the smallest admitted: every pixel a border pixel), 5 x 30 (two backward tiles across, h below a tile), 13 x 29 (one pixel past the 12 x 28
backward tile both ways: the 1-wide ragged tiles have threads far outside), 15 x 31 (the same for the 14 x 30 forward tile), 2 x 37 x 75; the options at
2 x 13 x 29 (photo_bounds.PHOTO_PARAMS); B = 256 at 13 x 29 = 1024 workgroups, the DENSE instantiation photo_bwd_multi_kernel<2, true>.
The backward runs on the reference's stored `sampled` and `sel` (photo_bounds docstring (c)).  The references are built once per process."""
import ctypes
import time

import pytest
import torch

import photo_bounds as PB

pytestmark = pytest.mark.gpu
dev = "cuda"
PHOTO = list(PB.PHOTO_SHAPES) + list(PB.PHOTO_PARAMS)


@pytest.fixture(scope="module")
def L():
    from simpledepthestimation_amd.hip import lib
    lib.lib()
    t0 = time.time()
    yield lib
    PB.record_note(f"time tests/test_gpu_photo_bounds.py {time.time() - t0:.1f} s (references included)")


def G(shape, dtype=torch.float32):
    return PB.guarded(shape, dtype, dev)


def _sync(L, rc, name):
    L.check(rc, name)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------------
# photometric term
# ---------------------------------------------------------------------------------------------------------------------------------------
class Launch:
    """One scale's operands on the device and its descriptor."""

    def __init__(self, L, c, B=None):
        B = c.B if B is None else B
        self.L, self.c, self.B = L, c, B
        cut = lambda t: t[:B].contiguous().to(dev)      # noqa: E731
        self.keep = [cut(c.A), cut(c.depth), cut(c.K)] + [cut(t) for t in c.ctx] + [cut(t) for t in c.poses]
        d = L.PhotoDesc()
        d.A, d.depth, d.K = (t.data_ptr() for t in self.keep[:3])
        for j in range(c.nctx):
            d.ctx[j], d.pose[j] = self.keep[3 + j].data_ptr(), self.keep[3 + c.nctx + j].data_ptr()
        d.B, d.h, d.w, d.nctx, d.automask, d.reduce_mean = B, c.h, c.w, c.nctx, int(c.automask), int(c.reduce_mean)
        d.sx, d.sy, d.ssim_w, d.C1, d.C2 = c.sx, c.sy, c.ssim_w, c.C1, c.C2
        self.thr = None if c.thr is None else c.thr.to(dev)
        d.clip_thr = 0 if self.thr is None else self.thr.data_ptr()
        self.d = d

    def fwd(self, pre=None):
        """pre: a value loss_out holds and the call accumulates into"""
        L, c, B = self.L, self.c, self.B
        lib = L.lib()
        o = {"sampled": [G((B, 3, c.h, c.w)) for _ in range(c.nctx)], "sel": G((B, c.h, c.w), torch.uint8), "maps": G((B, c.nmaps, c.h, c.w)),
             "partial": G((lib.sde_photo_num_blocks(B, c.h, c.w, 0),)), "loss": G((1,))}
        if c.reduce_mean and c.thr is None:
            o["sel"][1].zero_()            # (255 is this mode's code and the guard's sentinel)
        if pre is not None:
            o["loss"][1].fill_(pre)
        _sync(L, lib.sde_photo_fwd(ctypes.byref(self.d), L.ptr_array([s[1] for s in o["sampled"]]), L.ptr(o["sel"][1]), L.ptr(o["maps"][1]),
                                   L.ptr(o["partial"][1]), L.ptr(o["loss"][1]), 1.0, int(pre is not None), L.stream()), "sde_photo_fwd")
        return o

    def bwd(self, sampled, sel, gscale=None, pre=None):
        """sel None: a NULL pointer.  pre: (d_depth, [d_pose]) to accumulate into."""
        L, c, B = self.L, self.c, self.B
        lib = L.lib()
        self.stored = [s[:B].contiguous().to(dev) for s in sampled] + ([] if sel is None else [sel[:B].contiguous().to(dev)])
        self.gout = torch.tensor(c.gout, device=dev)
        o = {"d_depth": G((B, 1, c.h, c.w)), "pose_partial": G((lib.sde_photo_num_blocks(B, c.h, c.w, 1), c.nctx, 12)), "d_pose": [G((B, 4, 4)) for _ in range(c.nctx)]}
        if pre is not None:
            o["d_depth"][1].copy_(pre[0])
            for t, p in zip(o["d_pose"], pre[1]):
                t[1].copy_(p)
        acc = int(pre is not None)
        _sync(L, lib.sde_photo_bwd(ctypes.byref(self.d), L.ptr_array(self.stored[:c.nctx]), L.ptr(None if sel is None else self.stored[-1]), L.ptr(self.gout),
                                   c.gscale if gscale is None else gscale, L.ptr(o["d_depth"][1]), acc, L.ptr(o["pose_partial"][1]),
                                   L.ptr_array([t[1] for t in o["d_pose"]]), acc, L.stream()), "sde_photo_bwd")
        return o


def _guards(o, what):
    for k, v in o.items():
        for i, (buf, out) in enumerate(v if isinstance(v, list) else [v]):
            PB.assert_guards(buf, out, f"{what} {k}[{i}]")


@pytest.mark.parametrize("name", PHOTO)
def test_photo_fwd(L, name):
    n = PB.named_case(name)
    c, f = n["case"], n["fwd"]
    o = Launch(L, c).fwd()
    if c.reduce_mean and c.thr is None:
        sel = o.pop("sel")
        assert bool((sel[1] == 255).all()), "mean reduce without clipping: every code is 255"
        b = sel[0].cpu()
        assert bool((b[:PB.GUARD] == 255).all()) and bool((b[PB.GUARD + sel[1].numel():] == 255).all())
    else:
        PB.check_sel(o["sel"][1], f, f"photo_fwd {name} sel")
    _guards(o, f"photo_fwd {name}")
    for j in range(c.nctx):
        PB.check(o["sampled"][j][1], f["sampled"][j], f"photo_fwd {name} sampled[{j}]")
    PB.check(o["maps"][1], f["maps"], f"photo_fwd {name} maps")
    PB.check(o["partial"][1], f["partial"], f"photo_fwd {name} partial")
    PB.check(o["loss"][1], f["loss"], f"photo_fwd {name} loss_out")
    PB.record_note(f"share photo_fwd {name} sel undecided {f['share']:.5f}")


def _check_bwd(o, b, name):
    PB.check(o["d_depth"][1], b["d_depth"], f"photo_bwd {name} d_depth", True)
    PB.check(o["pose_partial"][1], b["pose_partial"], f"photo_bwd {name} pose_partial")
    for j, t in enumerate(o["d_pose"]):
        PB.check(t[1], b["d_pose"][j], f"photo_bwd {name} d_pose[{j}]")
        assert bool((t[1][:, 3] == 0).all()), "row 3 of d_pose is exactly zero"


@pytest.mark.parametrize("name", PHOTO)
def test_photo_bwd(L, name):
    n = PB.named_case(name)
    c, b = n["case"], n["bwd"]
    la = Launch(L, c)
    o = la.bwd(*n["stored"])
    _guards(o, f"photo_bwd {name}")
    _check_bwd(o, b, name)
    PB.record_share(f"photo_bwd {name} d_depth", b["share"], 0.01)
    if name == "dense":
        assert la.L.lib().sde_photo_num_blocks(c.B, c.h, c.w, 1) >= 1024, "the DENSE instantiation's grid"
        # samples 0 and 1 alone (4 workgroups per sample: the spill-free instantiation); gscale 1 / 128 of the dense launch's, so that g is the same number
        two = Launch(L, c, B=2).bwd(*n["stored"], gscale=c.gscale / 128.0)
        same = torch.equal(two["d_depth"][1], o["d_depth"][1][:2]) and torch.equal(two["pose_partial"][1], o["pose_partial"][1][:two["pose_partial"][1].shape[0]])
        PB.record_note(f"observation photo_bwd dense: samples 0 and 1 of the B = 256 launch (DENSE) equal the B = 2 launch bit for bit: {same}")


def test_photo_fwd_accumulate(L):
    """accumulate: loss_out += the scale's loss, one more fp32 addition"""
    n = PB.named_case("n2")
    f = n["fwd"]["loss"]
    pre = PB.f32(0.75)
    o = Launch(L, n["case"]).fwd(pre=pre)
    ref = f.ref + pre
    PB.check(o["loss"][1], PB.Bound(ref, f.lim + PB.U * (ref.abs() + f.lim)), "photo_fwd accumulate loss_out")


def test_photo_bwd_accumulate(L):
    """accumulate_depth / accumulate_pose: one more fp32 addition of the earlier content"""
    n = PB.named_case("n2")
    c, b = n["case"], n["bwd"]
    g = torch.Generator().manual_seed(3)
    scale = float(b["d_depth"].ref.abs().max())
    pd = torch.randn(c.B, 1, c.h, c.w, generator=g) * scale
    pp = [torch.randn(c.B, 4, 4, generator=g) * float(t.ref.abs().max()) for t in b["d_pose"]]
    o = Launch(L, c).bwd(*n["stored"], pre=(pd, pp))
    _guards(o, "photo_bwd accumulate")

    def plus(bd, p):
        ref = bd.ref + p.double()
        return PB.Bound(ref, bd.lim + PB.U * (ref.abs() + bd.lim))
    PB.check(o["d_depth"][1], plus(b["d_depth"], pd), "photo_bwd accumulate d_depth", True)
    for j, t in enumerate(o["d_pose"]):
        PB.check(t[1][:, :3], plus(PB.Bound(b["d_pose"][j].ref[:, :3], b["d_pose"][j].lim[:, :3]), pp[j][:, :3]), f"photo_bwd accumulate d_pose[{j}]")


def test_photo_bwd_null_sel_with_mean_reduce(L):
    """sel may be NULL with the 'mean' reduce and no clip thresholds: the same bits as with a sel of 255s; min reduce or thresholds refuse it."""
    n = PB.named_case("mean")
    c = n["case"]
    sampled, sel = n["stored"]
    assert bool((sel == 255).all())
    a = Launch(L, c).bwd(sampled, sel)
    z = Launch(L, c).bwd(sampled, None)
    assert torch.equal(a["d_depth"][1], z["d_depth"][1]) and torch.equal(a["pose_partial"][1], z["pose_partial"][1])
    for p, q in zip(a["d_pose"], z["d_pose"]):
        assert torch.equal(p[1], q[1])
    _guards(z, "photo_bwd null sel")
    for name in ("n2", "clip_mean"):
        m = PB.named_case(name)
        with pytest.raises(L.SdeHipError):
            Launch(L, m["case"]).bwd(m["stored"][0], None)


def test_photo_bwd_refuses_maps_below_4x4(L):
    n = PB.named_case("4x4")
    la = Launch(L, n["case"])
    la.d.h = 3
    with pytest.raises(L.SdeHipError):
        la.bwd(*n["stored"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# SSIM, smoothness, SILog
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", PB.SSIM_SHAPES, ids=str)
def test_ssim(L, shape):
    B, C, h, w = shape
    x, y, go = PB.ssim_inputs(*shape)
    c = PB.ssim_case(x, y, go)
    xd, yd, gd = x.to(dev), y.to(dev), go.to(dev)
    lib = L.lib()
    o = {"map": G(shape), "dx": G(shape), "dy": G(shape)}
    ws = torch.empty(B * C * h * w, 4, device=dev)
    _sync(L, lib.sde_ssim_fwd(L.ptr(xd), L.ptr(yd), B, C, h, w, PB.f32(1e-4), PB.f32(9e-4), L.ptr(o["map"][1]), L.stream()), "sde_ssim_fwd")
    _sync(L, lib.sde_ssim_bwd(L.ptr(xd), L.ptr(yd), L.ptr(gd), B, C, h, w, PB.f32(1e-4), PB.f32(9e-4), L.ptr(ws), L.ptr(o["dx"][1]), L.ptr(o["dy"][1]), L.stream()),
          "sde_ssim_bwd")
    _guards(o, f"ssim {shape}")
    for k in ("map", "dx", "dy"):
        PB.check(o[k][1], c[k], f"ssim {shape} {k}", k != "map")
    PB.record_share(f"ssim {shape} dx dy", c["share"], 0.01)


@pytest.mark.parametrize("shape", PB.SMOOTH_SHAPES, ids=str)
def test_smoothness(L, shape):
    B, h, w = shape
    depth, img = PB.smooth_inputs(*shape)
    c = PB.smooth_case(depth, img)
    dd, idv, gout = depth.to(dev), img.to(dev), torch.tensor(PB.f32(0.7), device=dev)
    lib = L.lib()
    nb = lib.sde_smooth_num_blocks(B, h, w)
    o = {"mean_part": G((B, PB.SM_CHUNKS)), "dn": G((B, h, w)), "loss_part": G((nb,)), "s_part": G((nb,)), "loss": G((1,)), "d_depth": G((B, 1, h, w))}
    p = lambda k: L.ptr(o[k][1])      # noqa: E731
    _sync(L, lib.sde_smooth_fwd(L.ptr(dd), L.ptr(idv), B, h, w, p("mean_part"), p("dn"), p("loss_part"), p("s_part"), p("loss"), 1.0, 0, L.stream()), "sde_smooth_fwd")
    _sync(L, lib.sde_smooth_bwd(L.ptr(dd), p("dn"), p("mean_part"), p("s_part"), L.ptr(gout), 1.0, B, h, w, p("d_depth"), 0, L.stream()), "sde_smooth_bwd")
    _guards(o, f"smooth {shape}")
    for k in o:
        PB.check(o[k][1], c[k], f"smooth {shape} {k}", k in ("dn", "d_depth"))
    PB.record_share(f"smooth {shape} dn d_depth", c["share"], 0.01)


def test_silog(L):
    est, gt = PB.silog_inputs()
    c = PB.silog_case(est, gt)
    B, _, h, w = est.shape
    H, W = gt.shape[2:]
    ed, gd, gout = est.to(dev), gt.to(dev), torch.tensor(PB.f32(0.7), device=dev)
    lib = L.lib()
    nb = lib.sde_silog_num_blocks(B, h, w)
    assert nb == c["cnt"].numel()
    o = {"part": G((nb, 3)), "stats": G((4,)), "d_est": G((B, 1, h, w))}
    _sync(L, lib.sde_silog_fwd(L.ptr(ed), L.ptr(gd), B, h, w, H, W, PB.f32(0.85), L.ptr(o["part"][1]), L.ptr(o["stats"][1]), L.stream()), "sde_silog_fwd")
    stats_in = c["stats_in"].to(dev)      # the backward in isolation: the reference's statistics, rounded to fp32
    _sync(L, lib.sde_silog_bwd(L.ptr(ed), L.ptr(gd), L.ptr(stats_in), L.ptr(gout), 1.0, PB.f32(0.85), B, h, w, H, W, L.ptr(o["d_est"][1]), 0, L.stream()), "sde_silog_bwd")
    _guards(o, "silog")
    part = o["part"][1].cpu()
    PB.assert_equal(part[:, 0].double(), c["cnt"], torch.float32, "silog count per block")
    PB.check(part[:, 1], c["s1"], "silog sum d per block")
    PB.check(part[:, 2], c["s2"], "silog sum d^2 per block")
    PB.check(o["stats"][1], c["stats"], "silog count, means, loss")
    PB.check(o["d_est"][1], c["d_est"], "silog d_est")
    assert bool((o["d_est"][1].cpu().reshape(-1)[~c["mask"]] == 0).all()), "exactly 0 where the mask is off"
    # the backward holds the shape check of the forward: ground truth smaller than the estimates is refused, nothing is launched
    with pytest.raises(L.SdeHipError):
        L.check(lib.sde_silog_bwd(L.ptr(ed), L.ptr(gd), L.ptr(stats_in), L.ptr(gout), 1.0, PB.f32(0.85), B, h, w, h - 1, W, L.ptr(o["d_est"][1]), 0, L.stream()), "sde_silog_bwd")

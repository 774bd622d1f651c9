"""GPU: the kernels of csrc/motion_loss.hip through the C ABI against tests/motion_bounds.py -- every element of every output within its own limit from
the fp64 reference, every output carved out of a guarded buffer (all of it written, the ragged last tiles included, nothing outside), masks exact outside
the pixels the reference cannot decide, tickets back at zero after each call, and every forward run twice into fresh buffers with bit-equal results
(d t_B2A, the atomic scatter, is the one sum without a fixed order).  Backward kernels run on the reference's stored operands (motion_bounds docstring
(c)).  The references are built once per process and shared with tests/test_motion_bounds.py's cases."""
import ctypes
import time

import pytest
import torch

import motion_bounds as MB

pytestmark = pytest.mark.gpu
dev = "cuda"
IMAGES = list(MB.IMAGE_SHAPES)


@pytest.fixture(scope="module")
def L():
    from simpledepthestimation_amd.hip import lib
    lib.lib()
    t0 = time.time()
    yield lib
    MB.record_note(f"time tests/test_gpu_motion_bounds.py {time.time() - t0:.1f} s (references included)")


def G(shape, dtype=torch.float32):
    return MB.guarded(tuple(shape), dtype, dev)


def D(t):
    return None if t is None else t.contiguous().to(dev)


def _sync(L, rc, name):
    L.check(rc, name)
    torch.cuda.synchronize()


def _guards(o, what):
    for k, (buf, out) in o.items():
        MB.assert_guards(buf, out, f"{what} {k}")


def _ticket(L):
    t = torch.zeros(1, dtype=torch.int32, device=dev)
    return t


def _same(a, b, what, skip=()):
    for k in a:
        if k not in skip:
            assert torch.equal(a[k][1], b[k][1]), f"{what} {k}: the second run into fresh buffers differs"


def _out(o):
    return {k: v[1] for k, v in o.items()}


# ---------------------------------------------------------------------------------------------------------------------------------------
# average pool, smoothness, sparsity
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", MB.AVGPOOL_SIZES, ids=str)
def test_avgpool(L, sizes):
    (H, W), (h, w) = sizes
    c = MB.avgpool_case(sizes)
    P = c["x"].shape[0]
    lib, x, go = L.lib(), D(c["x"]), D(c["gout"])

    def run():
        o = {"out": G((P, h, w)), "din": G((P, H, W))}
        _sync(L, lib.sde_avgpool_fwd(L.ptr(x), L.ptr(o["out"][1]), P, H, W, h, w, L.stream()), "sde_avgpool_fwd")
        _sync(L, lib.sde_avgpool_bwd(L.ptr(go), L.ptr(o["din"][1]), P, H, W, h, w, L.stream()), "sde_avgpool_bwd")
        return o
    o = run()
    _guards(o, f"avgpool {sizes}")
    MB.avgpool_check(c, _out(o), f"avgpool {sizes}")
    _same(o, run(), f"avgpool {sizes}")


@pytest.mark.parametrize("hw", MB.SMOOTH_HW, ids=str)
@pytest.mark.parametrize("P", MB.SMOOTH_PLANES)
def test_motion_smoothness(L, P, hw):
    H, W = hw
    c = MB.msmooth_case(P, H, W)
    lib, f, gout, tk = L.lib(), D(c["f"]), torch.tensor(MB.f32(MB.GOUT), device=dev), _ticket(L)
    nb = lib.sde_motion_smooth_num_blocks(P, H, W)
    assert nb == c["partial"].ref.numel()

    def run():
        o = {"partial": G((nb,)), "out": G((1,)), "df": G((P, H, W))}
        _sync(L, lib.sde_motion_smooth_fwd(L.ptr(f), P, H, W, L.ptr(o["partial"][1]), L.ptr(o["out"][1]), L.ptr(tk), L.stream()), "sde_motion_smooth_fwd")
        assert int(tk) == 0, "the ticket reads zero after the call"
        _sync(L, lib.sde_motion_smooth_bwd(L.ptr(f), L.ptr(gout), P, H, W, L.ptr(o["df"][1]), L.stream()), "sde_motion_smooth_bwd")
        return o
    o = run()
    _guards(o, f"msmooth {P} {hw}")
    MB.msmooth_check(c, _out(o), f"msmooth {P} {hw}")
    assert bool((o["df"][1][0] == 0).all()), "the flat plane's gradient is exactly zero"
    _same(o, run(), f"msmooth {P} {hw}")


@pytest.mark.parametrize("hw", MB.SPARSE_HW + [h * w for h, w in MB.SMOOTH_HW])
@pytest.mark.parametrize("P", MB.SMOOTH_PLANES)
def test_motion_sparsity(L, P, hw):
    c = MB.msparse_case(P, hw)
    lib, f, gout, tk, mean_in = L.lib(), D(c["f"]), torch.tensor(MB.f32(MB.GOUT), device=dev), _ticket(L), D(c["mean_in"])

    def run():
        o = {"mean": G((P,)), "partial": G((P,)), "out": G((1,)), "df": G((P, hw))}
        _sync(L, lib.sde_motion_sparsity_fwd(L.ptr(f), P, hw, L.ptr(o["mean"][1]), L.ptr(o["partial"][1]), L.ptr(o["out"][1]), L.ptr(tk), L.stream()), "sde_motion_sparsity_fwd")
        assert int(tk) == 0, "the ticket reads zero after the call"
        _sync(L, lib.sde_motion_sparsity_bwd(L.ptr(f), L.ptr(mean_in), L.ptr(gout), P, hw, L.ptr(o["df"][1]), L.stream()), "sde_motion_sparsity_bwd")
        return o
    o = run()
    _guards(o, f"msparse {P} {hw}")
    MB.msparse_check(c, _out(o), f"msparse {P} {hw}")
    assert bool((o["df"][1][c["f"].to(dev) == 0] == 0).all()), "exactly zero at an exact zero"
    _same(o, run(), f"msparse {P} {hw}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# view synthesis, weighted SSIM, motion consistency
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IMAGES)
def test_view_synthesis(L, name):
    c = MB.vs_case(name)
    N, H, W = c["shape"]
    lib = L.lib()
    img, depth, K, R, t = (D(c[k]) for k in ("img", "depth", "K", "R", "t"))
    C = img.shape[1]

    def run():
        o = {"sampled": G((N, C, H, W)), "Z": G((N, 1, H, W)), "grid": G((N, H, W, 2)), "valid": G((N, 1, H, W), torch.uint8)}
        _sync(L, lib.sde_view_synthesis_pp(L.ptr(img), L.ptr(depth), L.ptr(K), L.ptr(R), L.ptr(t), N, C, H, W, L.ptr(o["sampled"][1]), L.ptr(o["Z"][1]),
                                           L.ptr(o["grid"][1]), L.ptr(o["valid"][1]), L.stream()), "sde_view_synthesis_pp")
        return o
    o = run()
    _guards(o, f"view_synthesis {name}")
    assert bool((o["valid"][1] <= 1).all())
    MB.vs_check(c, _out(o), f"view_synthesis {name}")
    MB.record_share(f"view_synthesis {name} valid undecided", c["share"], MB.CAP)
    _same(o, run(), f"view_synthesis {name}")


@pytest.mark.parametrize("mode", list(MB.SSIM_MODES))
@pytest.mark.parametrize("name", IMAGES)
def test_weighted_ssim(L, name, mode):
    c = MB.wssim_case(name, mode)
    x, y, w, go = (D(t) for t in c["in"])
    N, C, H, W = x.shape
    C1, C2 = c["C"]
    lib = L.lib()
    coef = torch.empty(N, C, H, W, 4, device=dev)

    def fwd():
        o = {"map": G((N, C, H, W)), "avg_w": G((N, 1, H, W))}
        _sync(L, lib.sde_wssim_fwd(L.ptr(x), L.ptr(y), L.ptr(w), N, C, H, W, C1, C2, L.ptr(o["map"][1]), L.ptr(o["avg_w"][1]), L.stream()), "sde_wssim_fwd")
        return o

    def bwd(dx, dy):
        o = {k: G((N, C, H, W)) for k, on in (("dx", dx), ("dy", dy)) if on}
        _sync(L, lib.sde_wssim_bwd(L.ptr(x), L.ptr(y), L.ptr(w), L.ptr(go), N, C, H, W, C1, C2, L.ptr(coef), L.ptr(o["dx"][1] if dx else None),
                                   L.ptr(o["dy"][1] if dy else None), L.stream()), "sde_wssim_bwd")
        return o
    f = fwd()
    _guards(f, f"wssim {name} {mode}")
    both = bwd(True, True)
    _guards(both, f"wssim {name} {mode}")
    MB.wssim_check(c, {**_out(f), **_out(both)}, f"wssim {name} {mode}")
    MB.record_share(f"wssim {name} {mode} dx dy", c["share"], MB.CAP)
    _same(f, fwd(), f"wssim {name} {mode}")
    for only in ("dx", "dy"):         # one gradient alone: the other pointer null, the same bits
        o = bwd(only == "dx", only == "dy")
        _guards(o, f"wssim {name} {mode} {only} only")
        assert torch.equal(o[only][1], both[only][1]), f"{only} alone differs from {only} of the call with both"


@pytest.mark.parametrize("name,rot", MB.MC_CASES)
def test_motion_consistency(L, name, rot):
    c = MB.mc_case(name, rot)
    N, H, W = c["shape"]
    lib = L.lib()
    grid, mask, R1, R2, tA, tB = (D(c[k]) for k in ("grid", "mask", "R1", "R2", "tA", "tB"))
    g_rot, g_trans = torch.tensor([c["g_rot"]], device=dev), torch.tensor([c["g_trans"]], device=dev)
    nb = lib.sde_rgbd_num_blocks(N, H, W)

    def run():
        o = {"partial": G((nb,)), "out": G((2,)), "d_tA": G((N, 3, H, W)), "d_tB": G((N, 3, H, W)), "dR_partial": G((nb, 9)), "dR1": G((N, 3, 3)), "dR2": G((N, 3, 3))}
        _sync(L, lib.sde_motion_consistency_fwd(L.ptr(grid), L.ptr(mask), L.ptr(R1), L.ptr(R2), L.ptr(tA), L.ptr(tB), N, H, W, L.ptr(o["partial"][1]), L.ptr(o["out"][1]),
                                                L.stream()), "sde_motion_consistency_fwd")
        o["d_tB"][1].zero_()          # an accumulate-into buffer: its interior zeroed inside the guards
        _sync(L, lib.sde_motion_consistency_bwd(L.ptr(grid), L.ptr(mask), L.ptr(R1), L.ptr(R2), L.ptr(tA), L.ptr(tB), L.ptr(g_rot), L.ptr(g_trans), N, H, W,
                                                L.ptr(o["d_tA"][1]), L.ptr(o["d_tB"][1]), L.ptr(o["dR_partial"][1]), L.ptr(o["dR1"][1]), L.ptr(o["dR2"][1]), L.stream()),
              "sde_motion_consistency_bwd")
        return o
    o = run()
    what = f"mc {name} {rot}"
    _guards(o, what)
    got = _out(o)
    for k, t in got.items():
        assert bool(torch.isfinite(t).all()), f"{what} {k}: not finite"
    MB.mc_check(c, got, what)
    if rot == "identity":
        assert float(got["out"][0]) == 0.0 and bool((got["dR2"] == 0).all()), "both rotations the identity: every product is exact"
    _same(o, run(), what, skip=("d_tB",))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the per-scale glue
# ---------------------------------------------------------------------------------------------------------------------------------------
PREP = [(s, m, n) for s in MB.PREP_SHAPES for m in MB.PREP_MODES for n in (0, 1)]


@pytest.mark.parametrize("shape,mode,normalize", PREP)
def test_prep(L, shape, mode, normalize):
    c = MB.prep_case(shape, mode, normalize)
    N, H0, W0, h, w = c["shape"]
    v, cot = {k: D(x) for k, x in c["in"].items()}, {k: D(x) for k, x in c["cot"].items()}
    motion = v["motion"] is not None
    lib, tk = L.lib(), _ticket(L)
    nb = lib.sde_rgbd_num_blocks(N, h, w)
    what = f"prep {shape} {mode} normalize={normalize}"

    def fwd():
        o = {"depth_r": G((N, 1, h, w)), "t": G((N, 3, h, w)), "depth_n_sw": G((N, 1, h, w)), "t_sw": G((N, 3, h, w)), "partial": G((nb, 2)), "stats": G((2 + 4 * N,))}
        if normalize:
            o.update({"depth_n": G((N, 1, h, w)), "overall": G((N, 3, h, w))})
        if motion:
            o["m_norm"] = G((N, 3, h, w))
        p = lambda k: L.ptr(o[k][1] if k in o else None)      # noqa: E731
        _sync(L, lib.sde_motion_prep_fwd(L.ptr(v["depth"]), L.ptr(v["motion"]), L.ptr(v["t_pose"]), L.ptr(v["mask"]), N, H0, W0, h, w, normalize, p("depth_r"), p("depth_n"),
                                         p("t"), p("overall"), p("m_norm"), p("depth_n_sw"), p("t_sw"), p("partial"), p("stats"), L.ptr(tk), L.stream()), "sde_motion_prep_fwd")
        assert int(tk) == 0, "the ticket reads zero after the call"
        return o

    def bwd():
        s = {k: D(x) for k, x in MB.prep_stored_f32(c).items()}          # the backward in isolation: the reference's operands, rounded to fp32
        o = {"partial": G((nb, 9)), "bstats": G((1 + 10 * N,)), "d_depth": G((N, 1, H0, W0)), "d_tpose": G((N, 3))}
        if motion:
            o["d_motion"] = G((N, 3, H0, W0))
        _sync(L, lib.sde_motion_prep_bwd(L.ptr(v["mask"]), L.ptr(s["depth_n"] if normalize else None), L.ptr(s["t"]), L.ptr(s["m_norm"]), L.ptr(s["stats"]),
                                         L.ptr(cot["depth_r"]), L.ptr(cot["depth_n"] if normalize else None), L.ptr(cot["t"]), L.ptr(cot["t_sw"]),
                                         L.ptr(cot["m_norm"] if motion else None), N, H0, W0, h, w, normalize, L.ptr(o["partial"][1]), L.ptr(o["bstats"][1]), L.ptr(tk),
                                         L.ptr(o["d_depth"][1]), L.ptr(o["d_motion"][1] if motion else None), L.ptr(o["d_tpose"][1]), L.stream()), "sde_motion_prep_bwd")
        assert int(tk) == 0, "the ticket reads zero after the call"
        return o
    f, b = fwd(), bwd()
    _guards(f, what)
    _guards(b, what + " backward")
    MB.prep_check(c, {**_out(f), **{"b_" + k: t for k, t in _out(b).items()}}, what)
    _same(f, fwd(), what)
    _same(b, bwd(), what + " backward")


# ---------------------------------------------------------------------------------------------------------------------------------------
# RGB-D consistency
# ---------------------------------------------------------------------------------------------------------------------------------------
def _rgbd_desc(L, c, keep):
    t = [D(c[k]) for k in ("fA", "fB", "dA", "dB", "K", "R", "t")]
    keep.extend(t)
    d = L.RgbdDesc()
    d.frame_A, d.frame_B, d.depth_A, d.depth_B, d.K, d.R, d.t = (x.data_ptr() for x in t)
    d.N, d.H, d.W = c["shape"]
    d.ssim, d.C1, d.C2 = c["ssim"], c["C1"], c["C2"]
    return d


@pytest.mark.parametrize("name,mode", MB.RGBD_FWD_CASES)
def test_rgbd_fwd(L, name, mode):
    c = MB.rgbd_fwd_case(name, mode)
    N, H, W = c["shape"]
    lib, keep = L.lib(), []
    d = _rgbd_desc(L, c, keep)
    nb = lib.sde_rgbd_num_blocks(N, H, W)
    what = f"rgbd_fwd {name} {mode}"

    def run():
        o = {"sampled": G((N, 3, H, W)), "grid": G((N, H, W, 2)), "occ": G((N, 1, H, W)), "err": G((N, 1, H, W)), "valid": G((N, 1, H, W), torch.uint8), "part1": G((nb, 4)),
             "stats": G((4, N))}
        if c["ssim"]:
            o.update({"dpw": G((N, 1, H, W)), "part2": G((nb,))})
        p = lambda k: L.ptr(o[k][1] if k in o else None)      # noqa: E731
        _sync(L, lib.sde_rgbd_fwd(ctypes.byref(d), p("sampled"), p("grid"), p("occ"), p("err"), p("valid"), p("dpw"), p("part1"), p("part2"), p("stats"), L.stream()),
              "sde_rgbd_fwd")
        return o
    o = run()
    _guards(o, what)
    got = _out(o)
    occ = got["occ"]
    assert bool(((occ == 0) | (occ == 1)).all()) and bool((got["valid"] <= 1).all())
    stats = got.pop("stats")
    got.update({"stats": stats[[0, 2, 3]], "stats1": stats[1]})
    MB.rgbd_fwd_check(c, got, what)
    if not c["ssim"]:
        assert bool((stats[1] == 0).all()), "without the SSIM term row 1 is written as zero"
    MB.record_share(f"{what} valid / occ undecided", c["share"], MB.CAP)
    _same(o, run(), what)


@pytest.mark.parametrize("name,mode,gsel", MB.RGBD_BWD_CASES)
def test_rgbd_bwd(L, name, mode, gsel):
    c = MB.rgbd_bwd_case(name, mode, gsel)
    N, H, W = c["shape"]
    lib, keep = L.lib(), []
    d = _rgbd_desc(L, c, keep)
    nb = lib.sde_rgbd_num_blocks(N, H, W)
    sampled, occ, err, dpw, nrm = (D(t) for t in c["stored"])          # the backward in isolation: the reference's operands, rounded to fp32
    stats = torch.zeros(4, N, device=dev)
    stats[3] = nrm
    g_l1, g_ssim, g_dl1 = (D(t) for t in c["g"][:3])
    coef = torch.empty(N, 3, H, W, 4, device=dev) if c["ssim"] else None
    what = f"rgbd_bwd {name} {mode} {gsel}"

    def run():
        o = {"d_depth": G((N, 1, H, W)), "d_t": G((N, 3, H, W)), "dR_partial": G((nb, 9)), "dR": G((N, 3, 3))}
        _sync(L, lib.sde_rgbd_bwd(ctypes.byref(d), L.ptr(sampled), L.ptr(occ), L.ptr(err), L.ptr(dpw), L.ptr(stats), L.ptr(g_l1), L.ptr(g_ssim), L.ptr(g_dl1), c["g"][3],
                                  L.ptr(coef), L.ptr(o["d_depth"][1]), L.ptr(o["d_t"][1]), L.ptr(o["dR_partial"][1]), L.ptr(o["dR"][1]), L.stream()), "sde_rgbd_bwd")
        return o
    o = run()
    _guards(o, what)
    MB.rgbd_bwd_check(c, _out(o), what)
    MB.record_share(f"{what} d_depth d_t", c["share"], MB.CAP)
    _same(o, run(), what)

"""CPU self-test of tests/photo_bounds.py: the loss kernels of csrc/photometric.hip restated in fp32 (photo_bounds.F32: the kernels' operation sequences with
every operation rounded, sums in the order written, the per-workgroup sums in sde_block_sum's wave tree and wave order; the strided walks over partial slabs
as plain fp32 sums -- any order is inside the limit) stay inside the per-element limits; the hand-derived VJPs evaluated in exact
arithmetic are the fp64 autograd gradients; the part of the elements the reference cannot decide stays under its cap; and ten single planted faults are
rejected by the assertions the GPU tests call (an eleventh, a missing SILog index clamp, cannot change any admitted call: see its test)."""
import pytest
import torch

import photo_bounds as PB
from photo_bounds import F32, V
from oracle import geometry as G

PHOTO = list(PB.PHOTO_SHAPES) + list(PB.PHOTO_PARAMS)


def rejects(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the arithmetic itself
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_arithmetic_bounds_hold_on_random_expressions():
    """every operation of V against the same operation in fp32 on fp32 operands, and a cancelling chain"""
    g = torch.Generator().manual_seed(0)
    a, b, c = (torch.randn(4096, generator=g) for _ in range(3))
    p = a.abs() + 0.1
    va, vb, vc, vp = V.inp(a), V.inp(b), V.inp(c), V.inp(p)
    fa, fb, fc, fp = F32.inp(a), F32.inp(b), F32.inp(c), F32.inp(p)
    for name, v, f in (("add", va + vb, fa + fb), ("mul", va * vb, fa * fb), ("div", va / vp, fa / fp), ("fma", va.fma(vb, vc), fa.fma(fb, fc)),
                       ("exp", va.exp(), fa.exp()), ("log", vp.log(), fp.log()), ("sqrt", vp.sqrt(), fp.sqrt()), ("rcp", vp.rcp(), fp.rcp()),
                       ("var", (va * va + vb * vb).scale(0.5) - ((va + vb).scale(0.5)) * ((va + vb).scale(0.5)),
                        (fa * fa + fb * fb).scale(0.5) - ((fa + fb).scale(0.5)) * ((fa + fb).scale(0.5))),
                       ("sum", V.stack([va, vb, vc, vp]).sumdim(0), F32.sum([fa, fb, fc, fp])), ("const", va * V.c(1.0 / 9.0), fa * F32.c(1.0 / 9.0))):
        assert bool(((f.val.double() - v.val).abs() <= v.err).all()), name
    # a single rounding is not over-counted by more than the second-order terms
    assert float(((va * vb).err / (va * vb).val.abs().clamp(min=1e-30)).max()) <= 1.001 * PB.U + 1e-30
    # exact operations stay exact
    assert float(va.scale(2.0).err.max()) == 0 and float((-va).abs().err.max()) == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# SSIM
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", PB.SSIM_SHAPES[1:] + PB.SSIM_SHAPES[:1], ids=str)
def test_ssim(shape):
    x, y, go = PB.ssim_inputs(*shape)
    c = PB.ssim_case(x, y, go)
    vm, vdx, vdy = c["v"]
    PB.vjp_agrees(vm, c["ref"][0], "ssim map")
    PB.vjp_agrees(vdx, c["ref"][1], "ssim dx", c["und"])
    PB.vjp_agrees(vdy, c["ref"][2], "ssim dy", c["und"])
    PB.record_share(f"ssim {shape}", c["share"], 0.01)
    PB.check(PB.ssim_fwd(F32, F32.inp(x), F32.inp(y), PB.f32(1e-4), PB.f32(9e-4)).val, c["map"], "ssim map")
    ex, ey, _ = PB.ssim_bwd(F32, x, y, go, PB.f32(1e-4), PB.f32(9e-4))
    PB.check(ex.val, c["dx"], "ssim dx", True)
    PB.check(ey.val, c["dy"], "ssim dy", True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# SILog
# ---------------------------------------------------------------------------------------------------------------------------------------
def _silog_emu(est, gt, c, fault=None):
    gtn = PB.silog_nearest(gt, *est.shape[2:])
    mask, cnt, s1, s2 = PB.silog_fwd(F32, est, gtn, fault)
    stats = PB.silog_finalize_emu(cnt, s1.val, s2.val, 0.85)
    si = c["stats_in"]
    d = PB.silog_bwd(F32, est, gtn, (F32(si[0]), F32(si[1]), F32(si[3])), 0.7, 1.0, 0.85, fault)
    return cnt, s1.val, s2.val, stats, d.val


def _silog_check(c, cnt, s1, s2, stats, d):
    PB.assert_equal(cnt, c["cnt"], torch.float32, "silog count")
    PB.check(s1, c["s1"], "silog sum d")
    PB.check(s2, c["s2"], "silog sum d^2")
    PB.check(stats, c["stats"], "silog stats")
    PB.check(d, c["d_est"], "silog d_est")


def test_silog():
    est, gt = PB.silog_inputs()
    c = PB.silog_case(est, gt)
    assert int(c["mask"].sum()) > 8 and bool((c["gtn"] == 1.0).any()), "the case holds masked pixels and ground truth of exactly 1"
    PB.vjp_agrees(c["v"], c["d_est"].ref, "silog d_est")
    assert bool((c["d_est"].lim.reshape(-1)[~c["mask"]] == 0).all()) and bool((c["d_est"].ref.reshape(-1)[~c["mask"]] == 0).all())
    _silog_check(c, *_silog_emu(est, gt, c))


def test_silog_planted_mask_fault():
    """10: the mask `>= 1` for `> 1` (the case holds ground truth of exactly 1.0)."""
    est, gt = PB.silog_inputs()
    c = PB.silog_case(est, gt)
    rejects(_silog_check, c, *_silog_emu(est, gt, c, "silog_mask"))


def test_silog_index_clamp_cannot_be_reached():
    """11 (the nearest index not clamped to H - 1) cannot be planted so that anything changes.  For every row y < h the kernels read
    floor(fp32(y) * fp32(H / h)) <= floor((h - 1) (H / h) (1 + 2^-23)) < H -- whatever H and h are, enlarging (H < h) included, as long as h is far below
    2^23 -- so the clamp is dead code whatever the host admits (both entries admit H >= h only).  At the issue's
    5 x 7 against 12 x 20 the largest row read is floor(4 * 2.4) = 9 of 0 .. 11.  Asserted for every pair up to 64, both ways."""
    for H in range(1, 65):
        for h in range(1, 65):
            raw = (torch.arange(h, dtype=torch.float32) * torch.tensor(H / h, dtype=torch.float32)).floor()
            assert int(raw.max()) <= H - 1, (H, h)


# ---------------------------------------------------------------------------------------------------------------------------------------
# smoothness
# ---------------------------------------------------------------------------------------------------------------------------------------
def _smooth_emu(depth, img, fault=None):
    e = PB.smooth_fwd(F32, depth, img, fault)
    d = PB.smooth_bwd(F32, depth, e["dn"], e["mean_part"], e["s_part"], 0.7, 1.0)
    return {**{k: e[k].val for k in ("mean_part", "dn", "loss_part", "s_part", "loss")}, "d_depth": d.val}


def _smooth_check(c, got):
    for k in ("mean_part", "dn", "loss_part", "s_part", "loss", "d_depth"):
        PB.check(got[k], c[k], "smooth " + k, k in ("dn", "d_depth"))


@pytest.mark.parametrize("shape", PB.SMOOTH_SHAPES, ids=str)
def test_smoothness(shape):
    depth, img = PB.smooth_inputs(*shape)
    c = PB.smooth_case(depth, img)
    fw, vd = c["v"]
    PB.vjp_agrees(fw["dn"], c["dn"].ref, "smooth dn", c["und"])
    # dn / m - S / (hw m^2) cancels in fp64 too once one inverse depth is 2e6 (the clamped pixel) next to 0.03: 1e-8 of the largest gradient
    PB.vjp_agrees(vd, c["d_depth"].ref, "smooth d_depth", c["und"].unsqueeze(1), tol=1e-8)
    PB.record_share(f"smooth {shape}", c["share"], 0.01)
    if shape[1] > 2:      # the flat-depth patch's inner differences are exactly 0 in both precisions: decided, and nothing of it in the undecided set
        assert not bool(c["und"][0, 0, 0]) and float(fw["dn"].err[0, 0, 0]) < float("inf")
    _smooth_check(c, _smooth_emu(depth, img))


@pytest.mark.parametrize("fault,shape", [("smooth_left", (1, 5, 65)), ("smooth_left", (2, 9, 130)), ("smooth_nyn", (2, 9, 130)), ("smooth_nyn", (2, 2, 2))])
def test_smoothness_planted_faults(fault, shape):
    """8: the left-neighbour term dropped at x == 64 (the first column of the second 64-wide tile).  9: nyn formed with h for h - 1."""
    depth, img = PB.smooth_inputs(*shape)
    c = PB.smooth_case(depth, img)
    rejects(_smooth_check, c, _smooth_emu(depth, img, fault))


# ---------------------------------------------------------------------------------------------------------------------------------------
# photometric term
# ---------------------------------------------------------------------------------------------------------------------------------------
def _photo_emu(n, fault=None):
    c = n["case"]
    e = PB.photo_fwd(F32, c, fault=fault)
    b = PB.photo_bwd(F32, c, *n["stored"], fault=fault)
    dp = PB.pose_from_partials(F32, b["pose_partial"], c.B)
    return {"sampled": [s.val for s in e["sampled"]], "maps": torch.stack([m.val for m in e["maps"]], 1), "sel": e["sel"], "partial": e["partial"].val,
            "loss": e["loss"].val, "d_depth": b["d_depth"].val.unsqueeze(1), "pose_partial": b["pose_partial"].val,
            "d_pose": [torch.cat([t.val, torch.zeros(c.B, 1, 4)], 1) for t in dp]}


def _photo_check(n, got):
    f, b = n["fwd"], n["bwd"]
    for j, s in enumerate(got["sampled"]):
        PB.check(s, f["sampled"][j], f"photo sampled[{j}]")
    PB.check(got["maps"], f["maps"], "photo maps")
    PB.check_sel(got["sel"], f, "photo sel")
    PB.check(got["partial"], f["partial"], "photo partial")
    PB.check(got["loss"], f["loss"], "photo loss")
    PB.check(got["d_depth"], b["d_depth"], "photo d_depth", True)
    PB.check(got["pose_partial"], b["pose_partial"], "photo pose_partial")
    for j, p in enumerate(got["d_pose"]):
        PB.check(p, b["d_pose"][j], f"photo d_pose[{j}]")
        assert bool((p[:, 3] == 0).all())


@pytest.mark.parametrize("name", PHOTO)
def test_photometric(name):
    n = PB.named_case(name)
    c, f, b = n["case"], n["fwd"], n["bwd"]
    # (c): the fp32 chain's decisions are the oracle's, bit for bit
    Ks = G.scale_intrinsics(c.K, c.sx, c.sy)
    for j in range(c.nctx):
        o = G.view_synthesis(c.ctx[j], c.depth, Ks, c.poses[j][:, :3, :3], c.poses[j][:, :3, 3])
        assert torch.equal(o["fx"].long(), f["dec"][j]["x0"]) and torch.equal(o["fy"].long(), f["dec"][j]["y0"])
    # (b): formula = autograd
    PB.vjp_agrees(b["v"]["d_depth"].map(lambda v: v.unsqueeze(1)), b["d_depth"].ref, "photo d_depth", b["und"].unsqueeze(1))
    PB.vjp_agrees(b["v"]["pose_partial"], b["pose_partial"].ref, "photo pose_partial")
    for j in range(c.nctx):
        assert bool((b["d_pose"][j].ref[:, 3] == 0).all()) and bool((b["d_pose"][j].lim[:, 3] == 0).all())
    PB.record_share(f"photo d_depth {name}", b["share"], 0.01)
    _photo_check(n, _photo_emu(n))


def test_photometric_codes_of_the_clip_cases_occur():
    s = PB.named_case("clip_min")["fwd"]["sel"]
    assert bool((s == 254).any()) and bool((s < 4).any())
    m = PB.named_case("clip_mean")["fwd"]["sel"]
    assert len(torch.unique(m)) > 3 and bool(((m > 0) & (m < 15)).any()), "a non-trivial bit mask"


@pytest.mark.parametrize("name", PHOTO)
def test_forward_sel_cap(name):
    """At most 2 % of a case's arg-min decisions may be undecided from the reference alone (two smallest maps within the sum of their limits, or a map within
    its limit of its clip threshold): 0 .. 1.7 % here, 1.2 % (67 of 5 550 pixels) at 2x37x75.  That holds only because the SSIM limit treats its moments as
    dependent (photo_bounds.central, ssim_fwd): with E[x^2] and mu^2 propagated as independent quantities 17 .. 35 % of the decisions were undecided, and with
    the gradient enclosure of ssim_fwd built on independent moments still 3.2 % at 2x37x75.  The sample itself is known to 8e-5 there (median; the coordinate
    X comes from q0 = X q2 of about 2 400 through some ten roundings), and the two smallest maps lie closer than 4.1e-4 on 2 % of the pixels."""
    PB.record_share(f"photo sel {name}", PB.named_case(name)["fwd"]["share"], 0.02)


@pytest.mark.parametrize("name", PHOTO)
def test_photometric_d_depth_limit_has_power(name):
    """From the reference alone: the limit of d_depth is a small part of the value on most pixels.  A limit above |d_depth| cannot see a dropped or
    sign-flipped pixel: at most 5 % of the pixels with a gradient may have one; a limit above a tenth of |d_depth|: at most 25 %.  (Measured: 0.4 .. 2 %
    and 5 .. 18 %, the median limit 0.6 .. 3 % of the value.)  This holds because the error of ds enters the projection's VJP through its exact linear
    coefficient (photo_bwd) and the two bilinear weights are one quantity (tap_gradient); propagated as independent occurrences the median limit was 3 to
    5 times the value.  Consequences asserted on the emulation: an all-zero d_depth and one scaled by 0.5 or 1.5 are rejected."""
    n = PB.named_case(name)
    b = n["bwd"]["d_depth"]
    above, tenth, med = PB.power(b)
    PB.record_note(f"power photo d_depth {name}: limit > |value| on {above:.4f}, > 0.1 |value| on {tenth:.4f} of the pixels, median limit / |value| {med:.4f}")
    assert above <= 0.05 and tenth <= 0.25, (above, tenth, med)
    got = _photo_emu(n)["d_depth"]
    for k in (0.0, 0.5, 1.5):
        rejects(PB.check, got * k, b, "photo d_depth scaled", True)


@pytest.mark.parametrize("name", ["n2", "2x37x75", "mean"])
@pytest.mark.parametrize("fault", ["refl_mult", "seam_halo", "refl_corners"])
def test_photometric_d_depth_alone_rejects_the_window_faults(fault, name):
    """Faults 1 and 2, and the multiplicity fault at only the four pixels (1 | h-2, 1 | w-2), change a few dozen / six values of d_depth: the per-pixel
    assertion itself rejects them (not only the per-workgroup pose sums), and for faults 1 and 2 it catches more than half of the changed pixels (41 of 42, 21 of 22 at n2)."""
    n = PB.named_case(name)
    b = n["bwd"]["d_depth"]
    good, bad = _photo_emu(n)["d_depth"], _photo_emu(n, fault)["d_depth"]
    PB.check(good, b, "photo d_depth", True)
    rejects(PB.check, bad, b, "photo d_depth", True)
    changed = bad != good
    caught = changed & ((bad.double() - b.ref).abs() > b.lim)
    assert int(caught.sum()) * 2 >= int(changed.sum()) or fault == "refl_corners", (int(caught.sum()), int(changed.sum()))


PHOTO_FAULTS = [("refl_mult", "n2"), ("seam_halo", "n2"), ("g_mean", "mean"), ("l1_sign", "l1_mean"), ("l1_sign", "mean"), ("map_channel", "nomask"), ("partial_index", "n2"), ("acc12", "n2")]


@pytest.mark.parametrize("fault,name", PHOTO_FAULTS)
def test_photometric_planted_faults(fault, name):
    """1 reflection multiplicity 1 instead of 2 at gy == h - 2; 2 the window at ex = +1 dropped for the pixels of column 27; 3 g_mean divided by nctx
    instead of nmaps; 4 the L1 sign +1 at df == 0; 5 map 1 reads context 0's sample in channel 2; 6 pose_partial written at (bz gdx + bx) gdy + by;
    7 one acc12 entry using p[(k + 1) % 3].
    4 is planted where the L1 term stands alone (ssim_w = 0) and with SSIM on: all four changed pixels of d_depth exceed their limit either way."""
    n = PB.named_case(name)
    rejects(_photo_check, n, _photo_emu(n, fault))

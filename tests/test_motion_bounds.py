"""CPU self-test of tests/motion_bounds.py: the kernels of csrc/motion_loss.hip restated in fp32 (photo_bounds.F32: every operation rounded, the
per-workgroup sums in sde_block_sum's wave tree, the slab walks as plain sums) stay inside their per-element limits on every case the GPU tests run; the
hand-derived VJPs in exact arithmetic are the fp64 autograd gradients; every undecided share stays under its cap; and single planted faults (an argument
`fault=` of the emulation) are rejected by the assertion helpers the GPU tests call."""
import pytest
import torch

import motion_bounds as MB
from motion_bounds import F32, V


def rejects(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


# ---------------------------------------------------------------------------------------------------------------------------------------
# average pool
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", MB.AVGPOOL_SIZES, ids=str)
def test_avgpool(sizes):
    c = MB.avgpool_case(sizes)
    MB.vjp_agrees(c["v"][0], c["ref"][0], "avgpool out")
    MB.vjp_agrees(c["v"][1], c["ref"][1], "avgpool din")
    MB.avgpool_check(c, MB.avgpool_emu(c, sizes))


@pytest.mark.parametrize("sizes", MB.AVGPOOL_SIZES[:2] + MB.AVGPOOL_SIZES[3:4], ids=str)
def test_avgpool_planted_fault(sizes):
    """13: ap_hi floored instead of ceiled (a window loses its last row / column wherever (i + 1) H / h is no integer)."""
    c = MB.avgpool_case(sizes)
    rejects(MB.avgpool_check, c, MB.avgpool_emu(c, sizes, "ap_hi_floor"))


def test_avgpool_floor_fault_is_invisible_at_integer_ratios():
    """At (5, 6) -> (1, 1) and (8, 130) -> (4, 65) every (i + 1) H / h is an integer: floor and ceiling agree, which is why fault 13 is planted at the
    other three sizes."""
    for (H, W), (h, w) in (MB.AVGPOOL_SIZES[2], MB.AVGPOOL_SIZES[4]):
        for n, m in ((H, h), (W, w)):
            assert torch.equal(MB.ap_bounds(n, m)[1], MB.ap_bounds(n, m, "ap_hi_floor")[1])


# ---------------------------------------------------------------------------------------------------------------------------------------
# view synthesis with a per-pixel translation
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MB.IMAGE_SHAPES))
def test_view_synthesis(name):
    c = MB.vs_case(name)
    MB.vjp_agrees(c["v"]["sampled"], c["ref"]["sampled"], "sampled", c["mis"].expand_as(c["ref"]["sampled"]))      # the restated chain is the reference's formula
    MB.vjp_agrees(c["v"]["Z"], c["ref"]["Z"], "Z")
    MB.vjp_agrees(c["v"]["grid"], c["ref"]["grid"], "grid")
    MB.record_share(f"view_synthesis {name} valid undecided", c["share"], MB.CAP)
    MB.record_share(f"view_synthesis {name} tap cell differs", float(c["mis"].double().mean()), MB.CAP)
    MB.vs_check(c, MB.vs_emu(c))


@pytest.mark.parametrize("name", ["2x2", "5x65", "1028x2"])
def test_view_synthesis_planted_fault(name):
    """7: kt formed from pixel 0's translation for every pixel."""
    c = MB.vs_case(name)
    rejects(MB.vs_check, c, MB.vs_emu(c, "kt_pixel0"))


# ---------------------------------------------------------------------------------------------------------------------------------------
# RGB-D consistency
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", MB.RGBD_FWD_CASES)
def test_rgbd_fwd(name, mode):
    c = MB.rgbd_fwd_case(name, mode)
    for k in c["bounds"]:
        MB.vjp_agrees(c["fv"][k], c["ref"][k], f"rgbd_fwd {k}")
    MB.record_share(f"rgbd_fwd {name} {mode} valid / occ undecided", c["share"], MB.CAP)
    MB.rgbd_fwd_check(c, MB.rgbd_fwd_emu(c))


@pytest.mark.parametrize("name,mode,gsel", MB.RGBD_BWD_CASES)
def test_rgbd_bwd(name, mode, gsel):
    c = MB.rgbd_bwd_case(name, mode, gsel)
    u4 = c["und"].unsqueeze(1)
    for k, skip in (("d_depth", u4), ("d_t", u4.expand_as(c["ref"]["d_t"])), ("dR_partial", None), ("dR", None)):
        MB.vjp_agrees(c["bv"][k], c["ref"][k], f"rgbd_bwd {k}", skip)
    MB.record_share(f"rgbd_bwd {name} {mode} {gsel} d_depth d_t", c["share"], MB.CAP)
    MB.rgbd_bwd_check(c, MB.rgbd_bwd_emu(c))
    sampled = c["stored"][0]
    assert bool((sampled == c["fA"]).any()), "stored samples equal to frame_A occur (the L1 sign is 0 there)"


RGBD_FAULTS = [("occ_no_ok", "5x65", "fwd"), ("occ_no_ok", "2x9x130", "fwd"), ("kt_pixel0", "4x64", "fwd"), ("kt_pixel0", "1028x2", "bwd"), ("dl1_sign", "2x2", "bwd"),
               ("dl1_sign", "2x9x130", "bwd"), ("gather_mult", "3x3", "bwd"), ("gather_mult", "2x9x130", "bwd"), ("walk256", "1028x2", "fwd")]


@pytest.mark.parametrize("fault,name,which", RGBD_FAULTS)
def test_rgbd_planted_faults(fault, name, which):
    """5: occ without `&& ok` (the out-of-view cases hold pixels with Z < sD outside the projection mask); 6: the depth-L1 sign taken from sD - Z;
    7: kt from pixel 0's translation; 1: the gather multiplicity dropped at px == W - 2, through rgbd_bwd_kernel's own call of wssim_gather; 15: the
    slab walks of sample_m2 and rgbd_finalize_kernel ending after 256 of the 257 partials."""
    if which == "fwd":
        c = MB.rgbd_fwd_case(name)
        rejects(MB.rgbd_fwd_check, c, MB.rgbd_fwd_emu(c, fault))
    else:
        c = MB.rgbd_bwd_case(name)
        rejects(MB.rgbd_bwd_check, c, MB.rgbd_bwd_emu(c, fault))


def test_rgbd_bwd_limits_have_power():
    """From the reference alone: the limit of d_depth and d_t is a small part of the value on most elements (the error of d sampled enters the projection's
    VJP through its exact linear coefficient, as in photo_bounds.photo_bwd): above the value on at most 10 % of the elements with a gradient, the median
    limit below 5 % of the value.  An all-zero result and one scaled by 0.5 or 1.5 are rejected."""
    for name in ("5x65", "2x9x130"):
        c = MB.rgbd_bwd_case(name)
        got = MB.rgbd_bwd_emu(c)
        for k in ("d_depth", "d_t"):
            above, tenth, med = MB.PB.power(c["bounds"][k])
            MB.record_note(f"power rgbd_bwd {name} {k}: limit > |value| on {above:.4f}, > 0.1 |value| on {tenth:.4f}, median limit / |value| {med:.4f}")
            assert above <= 0.10 and med <= 0.05, (name, k, above, tenth, med)
            for s in (0.0, 0.5, 1.5):
                rejects(MB.check, got[k] * s, c["bounds"][k], f"rgbd_bwd {k} scaled", True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# WeightedSSIM
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MB.SSIM_MODES))
@pytest.mark.parametrize("name", list(MB.IMAGE_SHAPES))
def test_weighted_ssim(name, mode):
    c = MB.wssim_case(name, mode)
    for v, r, s in zip(c["v"], c["ref"], (None, None, c["und"], c["und"])):
        MB.vjp_agrees(v, r, f"wssim {name} {mode}", s)
    MB.record_share(f"wssim {name} {mode} dx dy", c["share"], MB.CAP)
    MB.wssim_check(c, MB.wssim_emu(c))


WSSIM_FAULTS = [("gather_mult", "3x3", "both"), ("gather_mult", "5x65", "c2"), ("gather_mult", "2x2", "c1"), ("avg_w_reflect", "2x2", "both"), ("avg_w_reflect", "5x65", "c1"),
                ("gather_eps", "4x64", "c2"), ("gather_eps", "3x3", "c1"), ("an1_mode1", "5x65", "c2"), ("an1_mode1", "2x9x130", "c2")]


@pytest.mark.parametrize("fault,name,mode", WSSIM_FAULTS)
def test_weighted_ssim_planted_faults(fault, name, mode):
    """1: the gather's multiplicity dropped at px == W - 2; 2: avg_w summed over the reflected taps instead of zero padding; 3: `+ 1e-2` missing from the
    centre weight of wssim_gather_kernel; 4: an1 not zeroed in mode 1 (C1 == inf)."""
    c = MB.wssim_case(name, mode)
    rejects(MB.wssim_check, c, MB.wssim_emu(c, fault))


def test_an1_fault_cannot_show_outside_mode_1():
    """an1 is zeroed in mode 1 only; in the other modes the planted line is the code as it stands."""
    for mode in ("c1", "both"):
        c = MB.wssim_case("5x65", mode)
        a, b = MB.wssim_emu(c), MB.wssim_emu(c, "an1_mode1")
        assert all(torch.equal(a[k], b[k]) for k in a)


# ---------------------------------------------------------------------------------------------------------------------------------------
# motion consistency
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rot", MB.MC_CASES)
def test_motion_consistency(name, rot):
    c = MB.mc_case(name, rot)
    for k, r in c["ref"].items():
        if float(r.abs().max()) > 0:
            MB.vjp_agrees(c["v"][k], r, f"mc {k}")
    for k, b in c["bounds"].items():
        assert bool(torch.isfinite(b.lim).all()) and bool(torch.isfinite(b.ref).all()), k      # nothing is left out, d t_B2A included
    MB.mc_check(c, MB.mc_emu(c))
    if rot == "inverse":      # the cancelling case: R1 R2 - I is rounding noise, the limit of rot_error is of its own size, and says so
        assert float(c["ref"]["out"][0]) < 1e-10 and float(c["bounds"]["out"].lim[0]) > float(c["ref"]["out"][0])
    if rot == "identity":
        assert float(c["ref"]["out"][0]) == 0 and bool((c["ref"]["dR1"] - c["ref"]["dR1"] == 0).all())


@pytest.mark.parametrize("name", MB.OUT_OF_VIEW)
def test_out_of_view_cases_are_what_they_say(name):
    """From the reference: clamped grid coordinates at exactly -1 and +1, taps with a neighbour outside, valid == 0 regions (points behind camera B
    among them), and many pixels that scatter into the same border cell."""
    _, o = MB.geometry_ref(name)
    c = MB.mc_case(name)
    N, H, W = c["shape"]
    g = c["grid"]
    assert bool((g[..., 0] == -1).any()) and bool((g[..., 0] == 1).any()) and bool((g == -1).any() or (g[..., 1] == 1).any())
    assert bool((c["dec"]["x0"] + 1 >= W).any()), "taps with the east neighbour outside the image"
    v = MB.vs_case(name)
    assert 0.02 < float((v["ref"]["Z"] <= 1e-5).double().mean()) and float(v["ref"]["valid"].double().mean()) < 0.9
    assert int(c["v"]["taps"].max()) >= 16, "many pixels scatter into one border cell"


@pytest.mark.parametrize("fault,name,key", [("scatter_swap", "5x65", "d_tB"), ("scatter_swap", "2x2", "d_tB"), ("no_dden", "2x9x130", "d_tA"), ("no_dden", "3x3", "d_tA"),
                                            ("dR2_R1", "4x64", "dR2"), ("walk256", "1028x2", "dR1")])
def test_motion_consistency_planted_faults(fault, name, key):
    """8: the scatter weights sy * wx and ny * ex exchanged; 9: the dden term dropped from d t_A2B; 10: dR2 formed with R1 in place of R1^T; 15: the slab
    walk of sample_sum9 ending after 256 partials (257 per sample at 1028 x 2).  Each is rejected by the output it changes, and by that output alone."""
    c = MB.mc_case(name)
    bad = MB.mc_emu(c, fault)
    rejects(MB.check, bad[key], c["bounds"][key], f"mc {key}")
    MB.mc_check(c, bad, skip=(key,) if fault != "scatter_swap" else (key,))


def test_dropped_dden_term_is_seen_where_it_is_small():
    """The issue's example: the dden term of d t_A2B on pixels where it is small against the map's maximum.  Among the pixels where the term is below 1 % of
    max |d t_A2B| (invisible to max|a - b| / max|b| at 3e-3 only if below 0.3 %, counted too) the per-element limit still rejects most of them."""
    c = MB.mc_case("2x9x130")
    good, bad, b = MB.mc_emu(c)["d_tA"], MB.mc_emu(c, "no_dden")["d_tA"], c["bounds"]["d_tA"]
    term = (bad.double() - good.double()).abs()
    small = (term > 0) & (term < 3e-3 * float(b.ref.abs().max()))
    caught = small & ((bad.double() - b.ref).abs() > b.lim)
    assert int(small.sum()) > 100 and int(caught.sum()) > 0.9 * int(small.sum()), (int(small.sum()), int(caught.sum()))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the per-scale glue
# ---------------------------------------------------------------------------------------------------------------------------------------
PREP = [(s, m, n) for s in MB.PREP_SHAPES for m in MB.PREP_MODES for n in (0, 1)]


@pytest.mark.parametrize("shape,mode,normalize", PREP)
def test_prep(shape, mode, normalize):
    c = MB.prep_case(shape, mode, normalize)
    for k, r in c["ref"].items():
        if r is not None:
            MB.vjp_agrees(c["fv"][k], r, f"prep {k}")
    for k, r in c["gref"].items():
        if r is not None:
            MB.vjp_agrees(c["bv"][k], r, f"prep d {k}")
    assert (c["gref"]["d_motion"] is None) == (mode == "no-motion")
    MB.prep_check(c, MB.prep_emu(c))


@pytest.mark.parametrize("mode,normalize", [("motion-mask", 1), ("motion", 0), ("no-motion", 1)])
def test_prep_planted_swap_fault(mode, normalize):
    """14: the swap index n ^ 1 for n <-> n + N / 2.  At N = 4 it is rejected (the swapped copies forward, d t through g_t_sw backward); at N = 2 the two
    are the same index and the emulations agree bit for bit, which is why the issue asks for N = 4."""
    c = MB.prep_case("N4-6x10-identity", mode, normalize)
    bad = MB.prep_emu(c, "swap_xor")
    rejects(MB.prep_check, c, bad)
    rejects(MB.check, bad["t_sw"], c["fwd"]["t_sw"], "prep t_sw")
    rejects(MB.check, bad["b_d_tpose"], c["bwd"]["d_tpose"], "prep d_tpose")
    c2 = MB.prep_case("N2-9x70-4x33", mode, normalize)
    a, b = MB.prep_emu(c2), MB.prep_emu(c2, "swap_xor")
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_prep_workgroups_per_sample():
    """the third shape's pooled grid spans 2 x 2 workgroups per sample: sample_sums_and_arrive walks more than one partial"""
    c = MB.prep_case("N2-10x140-5x70", "motion", 1)
    assert c["fwd"]["partial"].ref.shape[0] == 2 * 4


# ---------------------------------------------------------------------------------------------------------------------------------------
# smoothness, sparsity
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", MB.SMOOTH_HW, ids=str)
@pytest.mark.parametrize("P", MB.SMOOTH_PLANES)
def test_motion_smoothness(P, hw):
    c = MB.msmooth_case(P, *hw)
    MB.vjp_agrees(c["v"], c["ref"], "msmooth df")
    assert bool((c["ref"][0] == 0).all()) and bool(torch.isfinite(c["df"].lim).all()), "the flat plane: zero gradient, finite limit"
    MB.msmooth_check(c, MB.msmooth_emu(c))


@pytest.mark.parametrize("hw", MB.SMOOTH_HW, ids=str)
@pytest.mark.parametrize("P", [3, 9])
def test_motion_smoothness_planted_fault(P, hw):
    """11: the backward's `x <= W - 2` written `x < W - 2`: column W - 2 loses the element to its right."""
    c = MB.msmooth_case(P, *hw)
    rejects(MB.msmooth_check, c, MB.msmooth_emu(c, "smooth_edge"))


@pytest.mark.parametrize("hw", MB.SPARSE_HW + [h * w for h, w in MB.SMOOTH_HW])
@pytest.mark.parametrize("P", MB.SMOOTH_PLANES)
def test_motion_sparsity(P, hw):
    c = MB.msparse_case(P, hw)
    MB.vjp_agrees(c["v"], c["ref"], "msparse df")
    MB.msparse_check(c, MB.msparse_emu(c))


@pytest.mark.parametrize("hw", [1024, 1025])
def test_motion_sparsity_planted_fault(hw):
    """12: the sign of an exact zero taken as +1 (plane 1 holds exact zeros and a non-zero mean; on plane 0 the mean is 0 and nothing could show)."""
    c = MB.msparse_case(3, hw)
    assert bool((c["f"][1] == 0).any()) and float(c["mean_in"][1]) > 0
    rejects(MB.msparse_check, c, MB.msparse_emu(c, "sparse_sign"))

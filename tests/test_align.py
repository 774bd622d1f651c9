"""CPU: the host twins of sde_frame_align (hip/align.py) against the float64 restatement of align_ref.py -- per pixel outside the undecided
pixels, per sum with the twin's own inlier masks given, per iteration within the counted bounds --, the statuses, convergence on the room
corner, the inverse, the refusals of the binding and of the C entry points (which refuse before any launch: no GPU is needed), and
TsdfVolume.track's composition rule."""
import ctypes
import functools

import numpy as np
import pytest

import align_ref as AR
from simpledepthestimation_amd.hip import align as AL

EPS = AR.EPS
TOL = dict(dist_tol=0.03, scale_tol=0.1, min_count=32, damping=1e-4)
PIXEL_CASES = ("corner", "corner_maps", "bad_values", "corner_9x33", "plane")


def twin_step(inp, words, mode, **kw):
    kw = {**TOL, **kw}
    return AL.frame_align_host(words, inp["pred"], inp["ymap"], inp["xmap"], inp["K"], inp["model_depth"], inp["model_normal"], mode=mode,
                               min_depth=inp["min_depth"], max_depth=inp["max_depth"], **kw)


@functools.lru_cache(maxsize=None)
def states(name):
    """The states a case is examined at: fresh, and after one joint iteration of the twin (a D that is no identity, a scale that is not 1)."""
    inp = AR.case_inputs(name)
    w0 = AL.state_host()
    return (w0, twin_step(inp, w0, AL.POSE | AL.SCALE))


def terms_of(inp, words):
    return AL.align_terms_host(inp["pred"], inp["ymap"], inp["xmap"], inp["K"], inp["model_depth"], inp["model_normal"], words[:16].reshape(4, 4),
                               words[AL.SCALE_AT], inp["min_depth"], inp["max_depth"], TOL["dist_tol"], TOL["scale_tol"])


def test_defaults_are_what_the_measurements_chose():
    assert AL.DEFAULT_SCHEDULE == (3, 3, 3, 3) and AL.DEFAULTS == dict(dist_tol=0.03, scale_tol=0.1, min_count=256, damping=1e-4)
    assert (AL.POSE, AL.SCALE, AL.OK, AL.TOO_FEW, AL.SINGULAR) == (1, 2, 0, 1, 2)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("name", PIXEL_CASES)
def test_twin_against_restatement_per_pixel(name, which):
    inp = AR.case_inputs(name)
    w = states(name)[which]
    twin = terms_of(inp, w)
    want = AR.restate_terms(inp, w[:16].reshape(4, 4), w[AL.SCALE_AT], TOL["dist_tol"], TOL["scale_tol"])       # asserts the 1 % cap
    ok = ~want["undecided"]
    print(f"{name}[{which}]: {int(want['kept'].sum())} kept, {int(want['pose'].sum())} pose and {int(want['scale'].sum())} scale inliers of {ok.size}, "
          f"{int((~ok).sum())} undecided")
    for k in ("kept", "pose", "scale"):
        assert np.array_equal(twin[k][ok], want[k][ok]), k
    if name not in ("plane",):
        assert int(want["kept"].sum()) > 0.25 * ok.size
    on = ok & want["kept"]
    assert np.array_equal(twin["ix"][on], want["ix"][on]) and np.array_equal(twin["iy"][on], want["iy"][on])
    for k, b in (("r", "E_r"), ("rho", "E_rho"), ("J", "E_J")):
        err = np.abs(twin[k].astype(np.float64) - want[k])[on]
        bound = want[b][on]
        with np.errstate(all="ignore"):
            ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
        print(f"  {k}: largest error / bound {ratio:.3f}")
        assert bool(np.all(err <= bound)), k
    off = ~twin["pose"]
    assert not twin["terms"][off][:, :29].any() and not twin["terms"][~twin["scale"]][:, 29:31].any() and not twin["terms"][..., 31].any()


@pytest.mark.parametrize("mode", [AL.POSE, AL.SCALE, AL.POSE | AL.SCALE])
@pytest.mark.parametrize("name", ("corner", "corner_maps", "bad_values"))
def test_sums_solve_and_update_against_restatement(name, mode):
    """With the twin's own inlier masks given to the restatement: every total, xi, the new D and the new scale within the counted bounds."""
    inp = AR.case_inputs(name)
    w = states(name)[1]
    twin = terms_of(inp, w)
    total = AL.totals_host(AL.slab_host(twin["terms"]))
    st = dict(D=w[:16].reshape(4, 4).astype(np.float64), s=float(w[AL.SCALE_AT]))
    new, info = AR.restate_iteration(inp, st, mode, TOL["dist_tol"], TOL["scale_tol"], TOL["min_count"], TOL["damping"], masks=(twin["pose"], twin["scale"]))
    err = np.abs(total - info["total"])
    with np.errstate(all="ignore"):
        print(f"{name} mode {mode}: largest sum error / bound {float(np.nanmax(np.where(info['bound'] > 0, err / info['bound'], 0))):.3f}")
    assert bool(np.all(err <= info["bound"]))
    assert total[28] == info["count"] == twin["pose"].sum() and total[30] == info["scale_count"] == twin["scale"].sum() and total[31] == 0
    got = AL.unpack_state(twin_step(inp, w, mode))
    assert got["status"] == AL.OK == info["status"] and got["count"] == info["count"] and got["scale_count"] == info["scale_count"]
    assert abs(got["sumsq"] - info["sumsq"]) <= info["bound"][27] + EPS * info["sumsq"]
    if mode & AL.POSE:
        T, xi = AL.solve_host(total, TOL["damping"])
        print(f"  cond(A) {np.linalg.cond(info['A']):.1f}, largest xi error / bound {float((np.abs(xi - info['xi']) / info['E_xi']).max()):.3f}")
        assert bool(np.all(np.abs(xi - info["xi"]) <= info["E_xi"]))
        bound = AR.update_bound(info["xi"], info["E_xi"], st["D"])
        assert bool(np.all(np.abs(got["D"][:3].astype(np.float64) - new["D"][:3]) <= bound))
    else:
        assert got["D"].tobytes() == w[:16].tobytes()
    if mode & AL.SCALE:
        mean = info["total"][29] / info["scale_count"]
        bound = AR.SLACK * st["s"] * (info["bound"][29] / info["scale_count"] + EPS * mean) + EPS * new["s"]
        assert abs(got["scale"] - new["s"]) <= bound
    else:
        assert got["scale"] == w[AL.SCALE_AT]


def test_corner_constrains_all_six_degrees_of_freedom():
    inp = AR.case_inputs("corner")
    _, info = AR.restate_iteration(inp, dict(D=np.eye(4), s=1.0), AL.POSE, TOL["dist_tol"], TOL["scale_tol"], TOL["min_count"], TOL["damping"])
    cond = float(np.linalg.cond(info["A"]))
    print(f"corner: cond(A) = {cond:.1f} over {info['count']} inliers")
    # rotations enter through q x n with |q| up to 2.5, translations through n: a ratio of a few hundred between the extreme eigenvalues is what a
    # scene at this distance gives when every direction is seen; 2^-53 cond(A) stays ten orders of magnitude below the float32 roundings of the sums
    assert cond < 1e4


def test_fronto_parallel_plane_is_singular_and_leaves_the_state():
    inp = AR.case_inputs("plane")
    n = inp["model_normal"][inp["model_depth"] > 0]
    assert n.shape[0] > 1000 and not n[:, :2].any() and bool((n[:, 2] == -1).all())                   # exactly (0, 0, -1)
    w0 = AL.state_host()
    for mode in (AL.POSE, AL.POSE | AL.SCALE):
        w = twin_step(inp, w0, mode, dist_tol=0.1)                                                      # the depth is 4 % short: 0.07 at 1.75
        got = AL.unpack_state(w)
        assert got["status"] == AL.SINGULAR and got["count"] > 1000
        assert w[:33].tobytes() == w0[:33].tobytes()                                                    # D, Dinv and the scale: untouched
    _, info = AR.restate_iteration(inp, dict(D=np.eye(4), s=1.0), AL.POSE, 0.1, TOL["scale_tol"], TOL["min_count"], TOL["damping"])
    assert info["status"] == 2 and info["count"] > 1000
    w = twin_step(inp, w0, AL.SCALE, dist_tol=0.1)                                                      # the scale alone needs no matrix
    assert AL.unpack_state(w)["status"] == AL.OK and abs(float(w[AL.SCALE_AT]) - AR.PERTURB_SCALE) < 0.03
    assert AL.unpack_state(twin_step(inp, w0, AL.SCALE))["status"] == AL.TOO_FEW                        # ... but the pose inliers' count gates every mode


def test_empty_volume_is_too_few():
    inp = AR.case_inputs("empty")
    assert not inp["model_depth"].any() and not inp["model_normal"].any()
    w0 = AL.state_host()
    w = twin_step(inp, w0, AL.POSE | AL.SCALE)
    got = AL.unpack_state(w)
    assert got["status"] == AL.TOO_FEW and got["count"] == 0 and got["scale_count"] == 0 and got["sumsq"] == 0
    assert w[:33].tobytes() == w0[:33].tobytes()
    few = AL.unpack_state(twin_step(AR.case_inputs("corner"), w0, AL.POSE, min_count=100000))
    assert few["status"] == AL.TOO_FEW and 0 < few["count"] < 100000 and few["D"].tobytes() == np.eye(4, dtype=np.float32).tobytes()


def test_bad_depths_are_left_out():
    inp = AR.case_inputs("bad_values")
    twin = terms_of(inp, AL.state_host())
    pred = inp["pred"]
    bad = ~np.isfinite(pred) | ~(np.float32(inp["min_depth"]) < pred) | ~(pred <= np.float32(inp["max_depth"]))
    assert int(bad.sum()) > 0.1 * bad.size and not twin["kept"][bad].any() and not twin["terms"][bad].any()
    assert pred[0, 0] == np.float32(inp["max_depth"]) and not bad[0, 0]                                 # the closed end of the range is inside
    assert np.isfinite(AL.totals_host(AL.slab_host(twin["terms"]))).all()


def test_maps_with_borders_and_another_prediction_size():
    inp = AR.case_inputs("corner_maps")
    assert inp["pred"].shape == (29, 53) and inp["ymap"][0] == -1 and inp["xmap"][-1] == -1
    twin = terms_of(inp, AL.state_host())
    assert not twin["kept"][inp["ymap"] < 0].any() and not twin["kept"][:, inp["xmap"] < 0].any()
    hole = (inp["model_depth"] == 0)[twin["iy"], twin["ix"]]
    assert not (twin["kept"] & hole).any() and int(twin["kept"].sum()) > 500


def run_schedule(step, state, schedule):
    for mode in schedule:
        state = step(state, mode)
    return state


def test_convergence_on_the_corner():
    """The frame of the corner scene is seen from a camera turned by (0.6, -0.8, 0.5) degrees and moved by (0.035, -0.025, 0.04) -- about a
    voxel (0.05) -- against the predicted one, with a depth 4 % short (align_ref.PERTURB_*).  After the default schedule with the default
    tolerances the restatement's errors must be below half the initial ones (a condition on the scene), and the twin's at most 1.5 times the
    restatement's plus the counted bound: the per-iteration bounds of xi and of the update, added over the schedule along the twin's path.
    Measured: DESIGN.md section 31."""
    inp = AR.case_inputs("corner")
    kw = dict(AL.DEFAULTS)
    want_D, want_s = inp["D_true"], inp["s_true"]
    rot0, tr0 = AR.pose_error(np.eye(4), want_D)
    ref = dict(D=np.eye(4), s=1.0)
    w = AL.state_host()
    bound_D, bound_s = 0.0, 0.0
    for mode in AL.DEFAULT_SCHEDULE:
        ref, info = AR.restate_iteration(inp, ref, mode, kw["dist_tol"], kw["scale_tol"], kw["min_count"], kw["damping"])
        assert info["status"] == 0
        t = AL.align_terms_host(inp["pred"], inp["ymap"], inp["xmap"], inp["K"], inp["model_depth"], inp["model_normal"], w[:16].reshape(4, 4), w[AL.SCALE_AT],
                                inp["min_depth"], inp["max_depth"], kw["dist_tol"], kw["scale_tol"])
        st = dict(D=w[:16].reshape(4, 4).astype(np.float64), s=float(w[AL.SCALE_AT]))
        _, own = AR.restate_iteration(inp, st, mode, kw["dist_tol"], kw["scale_tol"], kw["min_count"], kw["damping"], masks=(t["pose"], t["scale"]))
        bound_D += float(AR.update_bound(own["xi"], own["E_xi"], st["D"]).max())
        bound_s += AR.SLACK * st["s"] * (own["bound"][29] / own["scale_count"] + 2 * EPS)
        w = twin_step(inp, w, mode, **kw)
        assert AL.unpack_state(w)["status"] == AL.OK
    got = AL.unpack_state(w)
    rot_r, tr_r = AR.pose_error(ref["D"], want_D)
    rot_t, tr_t = AR.pose_error(got["D"], want_D)
    s_r, s_t = abs(ref["s"] - want_s), abs(got["scale"] - want_s)
    print(f"initial: rotation {rot0:.5f} rad, translation {tr0:.5f}, scale {abs(1 - want_s):.5f}")
    print(f"restatement: rotation {rot_r:.5f}, translation {tr_r:.5f}, scale {s_r:.5f}")
    print(f"twin: rotation {rot_t:.5f}, translation {tr_t:.5f}, scale {s_t:.5f}; counted bounds {bound_D:.2e} (D), {bound_s:.2e} (scale); "
          f"{got['count']} inliers, rms {got['rms']:.4f}")
    assert rot_r < 0.5 * rot0 and tr_r < 0.5 * tr0 and s_r < 0.5 * abs(1 - want_s)
    # a rotation entry off by b moves the angle by at most 3 b, the translation by at most |t| b + b
    assert rot_t <= 1.5 * rot_r + 3 * bound_D and tr_t <= 1.5 * tr_r + 3 * bound_D and s_t <= 1.5 * s_r + bound_s


def test_inverse_times_transform_is_the_identity():
    inp = AR.case_inputs("corner")
    w = AL.state_host()
    for i, mode in enumerate(AL.DEFAULT_SCHEDULE, 1):
        w = twin_step(inp, w, mode)
        got = AL.unpack_state(w)
        D, Di = got["D"].astype(np.float64), got["Dinv"].astype(np.float64)
        # per iteration every entry of the rotation takes one rounding of the Cayley entries and four of the product: the orthogonality defect of
        # R grows by at most 3 * 5 EPS per entry; -R^T t is three products and two sums on |t| <= 1
        bound = i * 16 * EPS * (1 + np.abs(D[:3, 3]).sum())
        err = float(np.abs(Di @ D - np.eye(4)).max())
        print(f"iteration {i}: |Dinv D - I| = {err:.2e}, bound {bound:.2e}")
        assert err <= bound
        assert D[3].tolist() == [0, 0, 0, 1] and Di[3].tolist() == [0, 0, 0, 1]
        assert np.array_equal(got["Dinv"][:3, :3], got["D"][:3, :3].T)


def test_track_composed_with_compose_host_is_the_hand_computation():
    from simpledepthestimation_amd.hip.volume import compose_host
    inp = AR.case_inputs("corner")
    w = AL.track_host((inp["model_depth"], inp["model_normal"]), inp["pred"], inp["ymap"], inp["xmap"], inp["K"], min_depth=inp["min_depth"],
                      max_depth=inp["max_depth"])
    by_hand = AL.state_host()
    for mode in AL.DEFAULT_SCHEDULE:
        by_hand = AL.frame_align_host(by_hand, inp["pred"], inp["ymap"], inp["xmap"], inp["K"], inp["model_depth"], inp["model_normal"], mode=mode,
                                      min_depth=inp["min_depth"], max_depth=inp["max_depth"], **AL.DEFAULTS)
    assert w.tobytes() == by_hand.tobytes()
    got = AL.unpack_state(w)
    corrected = compose_host(got["Dinv"], inp["C"])
    f32 = np.float32
    want = np.zeros((4, 4), f32)
    want[3, 3] = 1
    for r in range(3):
        for c in range(4):
            v = f32(f32(got["Dinv"][r, 0] * inp["C"][0, c]) + f32(got["Dinv"][r, 1] * inp["C"][1, c])) + f32(got["Dinv"][r, 2] * inp["C"][2, c])
            want[r, c] = f32(v + got["Dinv"][r, 3]) if c == 3 else v
    assert corrected.tobytes() == want.tobytes()
    # world -> corrected camera = D^-1 C: closer to the frame's true pose than the predicted C was
    C_true = np.linalg.inv(inp["D_true"]) @ inp["C"].astype(np.float64)
    assert AR.pose_error(corrected, C_true)[1] < 0.5 * AR.pose_error(inp["C"], C_true)[1]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_check_align_refuses():
    good = dict(dist_tol=0.03, scale_tol=0.1, min_count=6, damping=0.0, mode=3, min_depth=0.0, max_depth=80.0)
    assert AL.check_align(**good) == (float(np.float32(0.03)), float(np.float32(0.1)), 6, 0.0, 3, 0.0, 80.0)
    for k, v in (("dist_tol", 0.0), ("dist_tol", float("nan")), ("scale_tol", -1.0), ("scale_tol", float("nan")), ("damping", -1e-3),
                 ("damping", float("nan")), ("min_count", 5), ("min_count", 6.5), ("mode", 0), ("mode", 4), ("mode", 1.0), ("mode", True),
                 ("min_depth", 80.0), ("max_depth", float("nan"))):
        with pytest.raises(ValueError):
            AL.check_align(**{**good, k: v})
    for size in ((0, 8), (8, 32769), (8,), (8.5, 8), "ab"):
        with pytest.raises(ValueError):
            AL.check_size(size)


def test_binding_refuses_host_tensors_before_the_device():
    import torch
    from simpledepthestimation_amd.hip.lib import SdeHipError
    inp = AR.case_inputs("corner_8x8")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    with pytest.raises(SdeHipError):
        AL.frame_align(t(inp["pred"]), inp["ymap"], inp["xmap"], t(inp["K"]), t(inp["model_depth"]), t(inp["model_normal"]), torch.zeros(40))
    with pytest.raises(ValueError):
        AL.frame_align(t(inp["pred"]), inp["ymap"], inp["xmap"], t(inp["K"]), t(inp["model_depth"]), t(inp["model_normal"]), torch.zeros(40), mode=0)
    with pytest.raises(SdeHipError):
        AL.AlignState((8, 8), device="cpu")


def test_library_refuses_before_any_launch():
    """Every refusal of the header, one bad argument at a time, with host buffers in place of device memory: nothing is launched."""
    from simpledepthestimation_amd.hip import lib as L
    lib = L.lib()
    assert L._PROTOS["sde_frame_align_ws_bytes"][1] is ctypes.c_size_t and len(L._PROTOS["sde_frame_align"][0]) == 21
    assert lib.sde_frame_align_ws_bytes(8, 8) == 128 and lib.sde_frame_align_ws_bytes(9, 33) == 2 * 2 * 128
    assert lib.sde_frame_align_ws_bytes(264, 264) == 33 * 9 * 128 == AL.slab_rows(264, 264) * 128
    for size in ((0, 8), (8, 0), (32769, 8), (8, 32769)):
        assert lib.sde_frame_align_ws_bytes(*size) == 0
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    off = ctypes.c_void_p(p.value + 2)
    good = dict(pred=p, ph=8, pw=8, ymap=p, xmap=p, H=8, W=8, K=p, depth=p, normal=p, lo=0.0, hi=80.0, dist=0.03, scale=0.1, min_count=6, damping=0.0,
                mode=3, state=p, ws=p, ws_bytes=128)
    nan = float("nan")
    bad = [dict(H=0), dict(W=0), dict(H=32769), dict(W=32769), dict(ph=0), dict(pw=-1), dict(pred=None), dict(ymap=None), dict(xmap=None), dict(K=None),
           dict(depth=None), dict(normal=None), dict(state=None), dict(state=off), dict(mode=0), dict(mode=4), dict(dist=0.0), dict(dist=nan),
           dict(scale=0.0), dict(scale=nan), dict(damping=-1.0), dict(damping=nan), dict(min_count=5), dict(lo=80.0), dict(lo=nan), dict(hi=nan),
           dict(ws=None), dict(ws=off), dict(ws_bytes=127)]
    for b in bad:
        a = {**good, **b}
        rc = lib.sde_frame_align(a["pred"], a["ph"], a["pw"], a["ymap"], a["xmap"], a["H"], a["W"], a["K"], a["depth"], a["normal"], a["lo"], a["hi"], a["dist"],
                                 a["scale"], a["min_count"], a["damping"], a["mode"], a["state"], a["ws"], a["ws_bytes"], None)
        assert rc == -1 and b"sde_frame_align" in lib.sde_last_error(), b
    assert lib.sde_frame_align_reset(None, None) == -1 and b"sde_frame_align_reset" in lib.sde_last_error()
    assert lib.sde_frame_align_reset(off, None) == -1


def test_header_fixes_the_state_layout():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sde_hip.h")).read()
    value = lambda k: int(re.search(r"#define %s (\d+)" % k, hdr).group(1))
    for k, v in (("SDE_ALIGN_POSE", AL.POSE), ("SDE_ALIGN_SCALE", AL.SCALE), ("SDE_ALIGN_OK", AL.OK), ("SDE_ALIGN_TOO_FEW", AL.TOO_FEW),
                 ("SDE_ALIGN_SINGULAR", AL.SINGULAR), ("SDE_ALIGN_SUMS", AL.SUMS), ("SDE_ALIGN_STATE_WORDS", AL.STATE_WORDS),
                 ("SDE_ALIGN_SCALE_AT", AL.SCALE_AT), ("SDE_ALIGN_SUMSQ_AT", AL.SUMSQ_AT), ("SDE_ALIGN_COUNT_AT", AL.COUNT_AT),
                 ("SDE_ALIGN_SCALE_COUNT_AT", AL.SCALE_COUNT_AT), ("SDE_ALIGN_STATUS_AT", AL.STATUS_AT)):
        assert value(k) == v, k
    w = AL.state_host()
    assert w[:16].reshape(4, 4).tolist() == np.eye(4).tolist() == w[16:32].reshape(4, 4).tolist() and w[32] == 1 and not w[33:].any()

"""CPU: the host twin of sde_depth_warp_fuse (hip/temporal.py: warp_fuse_host) against the float64 restatement of temporal_ref.py -- the state
equal and warped / fused within the per-element bounds derived there, outside the at most 5 % of pixels an undecided source can reach -- on the
cases the GPU test shares and on three scenes whose outcome is known beforehand; the refusals of the library, and the window rule."""
import ctypes
import functools
import os

import numpy as np
import pytest

import flow_ref as FR
import temporal_ref as TR
from simpledepthestimation_amd.hip.temporal import warp_fuse_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def reference(name):
    """Inputs and restatement of one shared case: computed once, never modified."""
    inp = TR.case_inputs(name)
    return inp, TR.restate(**inp)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", TR.CASES)
def test_twin_against_restatement(name):
    inp, want = reference(name)
    got = warp_fuse_host(**inp)
    assert got[0].dtype == np.float32 and got[1].dtype == np.uint8 and got[2].dtype == np.float32
    TR.compare(got, want, inp["cur"], name)
    again = warp_fuse_host(**inp)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


def plane_camera(h, w, f):
    return np.array([[[f, 0, (w - 1) / 2], [0, f, (h - 1) / 2], [0, 0, 1]]], dtype=np.float32)


def test_shifted_plane_over_twelve_frames():
    """A fronto-parallel plane at 10 m, the camera moving 1 m sideways per frame: 3 pixels at f = 30.  Every frame's prediction is the plane
    times a noise within 1 +- tol / 5, so that the fused map and the next prediction differ by less than tol / 2."""
    h, w, f, Z, tol, alpha = 24, 40, 30.0, 10.0, 0.05, 0.5
    K = plane_camera(h, w, f)
    T = FR.pose([0, 0, 0], [3 * Z / f, 0, 0])[None]
    rng = np.random.default_rng(12)
    state = np.zeros((1, h, w), np.float32)
    for k in range(12):
        cur = (Z * rng.uniform(1 - tol / 5, 1 + tol / 5, (1, h, w))).astype(np.float32)
        want = TR.restate(state, cur, K, T, None, alpha, tol)
        assert not want["skip"].any()                                      # an integer shift: no source is undecided, every pixel is compared
        fused, st, warped = warp_fuse_host(state, cur, K, T, None, alpha, tol)
        TR.compare((fused, st, warped), want, cur, f"frame {k}")
        if k == 0:
            assert not st.any() and np.array_equal(bits(fused), bits(cur)) and not warped.any()
        else:
            # the shift goes the right way, and exactly: with R = I and t_z = 0 the new depth is the old one, three columns to the right
            assert not want["landed"][0, :, :3].any() and want["landed"][0, :, 3:].all()
            assert np.array_equal(bits(warped[0, :, 3:]), bits(state[0, :, :-3]))
            # of the three uncovered columns the two outer ones are NEW; the rim column beside the warped map is closed by the one-ring fill
            assert bool(np.all(st[0, :, :2] == TR.NEW)) and not warped[0, :, :2].any() and np.array_equal(bits(fused[0, :, :2]), bits(cur[0, :, :2]))
            assert bool(np.all(st[0, :, 2] == (TR.FUSED | TR.FILLED)))
            col = np.pad(state[0, :, 0], 1, constant_values=np.inf)        # column 3 holds the old column 0: the rim takes the nearest of three rows
            assert np.array_equal(bits(warped[0, :, 2]), bits(np.minimum(np.minimum(col[:-2], col[1:-1]), col[2:])))
            assert bool(np.all(st[0, :, 3:] == TR.FUSED))
            assert bool(np.all(np.abs(fused[0, :, 3:] / Z - 1) <= tol / 5 + 1e-6))          # a blend of values inside the noise band stays inside it
        state = fused


def test_near_square_over_far_plane():
    """A square at 5 m in front of a plane at 20 m, the camera moving 1 m sideways: at f = 40 the plane moves 2 pixels, the square 8."""
    h, w, f, tol, alpha = 32, 48, 40.0, 0.05, 0.5
    K = plane_camera(h, w, f)
    T = FR.pose([0, 0, 0], [1.0, 0, 0])[None]
    rng = np.random.default_rng(5)
    prev = np.full((1, h, w), 20.0, np.float32)
    prev[0, 10:20, 12:22] = 5.0
    truth = np.full((1, h, w), 20.0)
    truth[0, 10:20, 20:30] = 5.0                                           # where the square is now
    truth[0, 24:28, 35:40] = 10.0                                          # something new in front of the plane: the warped plane lies FARTHER
    truth[0, 2:6, 35:40] = 40.0                                            # the plane gone: the warped plane lies NEARER
    cur = (truth * rng.uniform(1 - tol / 5, 1 + tol / 5, truth.shape)).astype(np.float32)
    want = TR.restate(prev, cur, K, T, None, alpha, tol)
    assert not want["skip"].any()
    fused, st, warped = warp_fuse_host(prev, cur, K, T, None, alpha, tol)
    TR.compare((fused, st, warped), want, cur, "square")
    # plane pixels from columns 18 .. 27 and the square land on columns 20 .. 29 of its rows: the nearer depth is kept
    assert bool(np.all(warped[0, 10:20, 20:30] == 5.0)) and bool(np.all(st[0, 10:20, 20:30] == TR.FUSED))
    # behind the square nothing lands on columns 14 .. 19; the ring fill closes one pixel on every side, the rest is NEW
    assert not want["landed"][0, 10:20, 14:20].any()
    assert bool(np.all(st[0, 11:19, 15:19] == TR.NEW)) and not warped[0, 11:19, 15:19].any()
    assert bool(np.all(st[0, 10:20, 14] & TR.FILLED)) and bool(np.all(st[0, 10:20, 19] & TR.FILLED))
    # where the current frame disagrees the prediction is kept bit for bit, and the class says which way
    assert bool(np.all(st[0, 24:28, 35:40] == TR.FARTHER)) and bool(np.all(st[0, 2:6, 35:40] == TR.NEARER))
    differs = (st & 3) >= TR.NEARER
    assert int(differs.sum()) >= 40 and np.array_equal(bits(fused)[differs], bits(cur)[differs])
    blended = (st & 3) == TR.FUSED
    assert not np.array_equal(bits(fused)[blended], bits(cur)[blended])


def test_bad_values_scatter_nothing_and_are_passed_on():
    inp, want = reference("bad_values")
    fused, st, warped = warp_fuse_host(**inp)
    cur = inp["cur"]
    for n, y, x in ((0, 2, 3), (1, 5, 5), (0, 6, 11), (1, 9, 17)):          # cur 0 or NaN: nothing to blend with
        assert st[n, y, x] & 3 == TR.NEW and bits(fused)[n, y, x] == bits(cur)[n, y, x]
    # image 1's camera has driven past the near band: those sources are behind it; others leave the image
    r = FR.restate(inp["prev"], np.arange(11, dtype=np.int32), np.arange(23, dtype=np.int32), inp["K"], inp["T"], None)
    assert bool(np.all(r["qz"][1, 3:6] < 0)) and not r["bit0"][1, 3:6].any()
    X, Y = r["X"][r["bit0"]], r["Y"][r["bit0"]]
    assert int(((np.rint(X) < 0) | (np.rint(X) >= 23) | (np.rint(Y) < 0) | (np.rint(Y) >= 11)).sum()) >= 10
    # a map that holds only unusable values scatters nothing at all
    bad = np.tile(np.array([0.0, -3.0, np.nan, np.inf], np.float32), 11 * 23 * 2 // 4 + 1)[:11 * 23 * 2].reshape(2, 11, 23)
    f2, s2, w2 = warp_fuse_host(bad, cur, inp["K"], inp["T"], None, 0.5, 0.05)
    assert not s2.any() and not w2.any() and np.array_equal(bits(f2), bits(cur))


def test_alpha_zero_keeps_the_prediction():
    inp, _ = reference("several_workgroups")
    fused, st, _ = warp_fuse_host(inp["prev"], inp["cur"], inp["K"], inp["T"], inp["motion"], 0.0, inp["tol"])
    assert np.array_equal(bits(fused), bits(inp["cur"])) and int(((st & 3) == TR.FUSED).sum()) > 100


def test_refusals_precede_any_device_call():
    """Every refusal returns SDE_ERR_ARG with a message; the pointers are never followed (they point into host memory, and this runs without a GPU)."""
    from simpledepthestimation_amd.hip import lib as L
    lib = L.lib()
    args, res = L._PROTOS["sde_depth_warp_fuse"]
    assert len(args) == 15 and res is ctypes.c_int
    assert "sde_depth_warp_fuse" in open(os.path.join(ROOT, "include", "sde_hip.h")).read()
    host = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(host))

    def call(**kw):
        a = dict(prev=p, cur=p, K=p, T=p, motion=None, N=1, h=2, w=3, alpha=0.5, tol=0.05, zbuf=p, fused=p, state=None, warped=None)
        a.update(kw)
        return lib.sde_depth_warp_fuse(a["prev"], a["cur"], a["K"], a["T"], a["motion"], a["N"], a["h"], a["w"], a["alpha"], a["tol"], a["zbuf"], a["fused"],
                                       a["state"], a["warped"], None)
    for kw in (dict(N=0), dict(N=-1), dict(h=0), dict(w=0), dict(w=-5), dict(alpha=-0.1), dict(alpha=1.0), dict(alpha=1.5), dict(alpha=float("nan")),
               dict(tol=0.0), dict(tol=-0.05), dict(tol=float("nan")), dict(prev=None), dict(cur=None), dict(K=None), dict(T=None), dict(zbuf=None),
               dict(fused=None)):
        assert call(**kw) == -1, kw
        assert b"sde_depth_warp_fuse" in lib.sde_last_error(), kw
    assert not any(host)
    from simpledepthestimation_amd.hip.temporal import check_params
    for bad in ((1.0, 0.05), (-0.5, 0.05), (float("nan"), 0.05), (0.5, 0.0), (0.5, float("nan"))):
        with pytest.raises(ValueError):
            check_params(*bad)
        with pytest.raises(ValueError):
            warp_fuse_host(np.ones((1, 2, 2), np.float32), np.ones((1, 2, 2), np.float32), np.eye(3, dtype=np.float32), np.eye(4, dtype=np.float32)[None], None, *bad)


def test_window_rule():
    from simpledepthestimation_amd.engine.predictor import temporal_args, temporal_context
    assert temporal_context((-1, 1)) == (1, False) and temporal_context((1,)) == (0, False) and temporal_context((-1,)) == (0, True)
    assert temporal_context((-2, -1, 1, 2)) == (2, False)
    for offsets in ((-2, 2), (2,), (-3,), (-4, -2)):
        with pytest.raises(ValueError, match=r"context one frame away.*offsets are \(" + str(offsets[0])):
            temporal_context(offsets)
    assert temporal_args(None) is None and temporal_args({}) == temporal_args({"alpha": 0.5, "tol": 0.05})
    for bad in ({"alpha": 1.0}, {"tol": 0}, {"beta": 1}, (0.5, 0.05)):
        with pytest.raises(ValueError):
            temporal_args(bad)

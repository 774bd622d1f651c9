"""CPU: the host twins of the TSDF volume (hip/volume.py: integrate_host, points_host, compose_host) against the float64 restatement of
volume_ref.py within its a-priori bounds, the pose chain against the inverse of accumulate_poses, the ordering / overflow / empty rules of the
points, the argument refusals of the C side, of TsdfVolume and of the predictor, and the PLY round trip.  No GPU."""
import ctypes
import functools
import os
import warnings

import numpy as np
import pytest

import volume_ref as VR
from simpledepthestimation_amd.hip import volume as HV
from simpledepthestimation_amd.hip.cloud import RECORD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_twin(vol, frames, colour=True):
    tsdf, weight, rgba = VR.fresh(vol["dims"], colour)
    keeps = []
    for fr in frames:
        keeps.append(HV.integrate_host(tsdf, weight, rgba, fr["pred"], fr["ymap"], fr["xmap"], fr["K"], fr["C"], fr["frame"] if colour else None,
                                       vol["origin"], vol["voxel"], vol["trunc"], vol["max_weight"], vol["min_depth"], vol["max_depth"]))
    return (tsdf, weight, rgba), keeps


@functools.lru_cache(maxsize=None)
def reference(name):
    """Inputs, restatement and the twin's result of one case: computed once, shared, never modified."""
    vol, frames = VR.case_inputs(name)
    got, keeps = run_twin(vol, frames)
    return vol, frames, VR.restate_integrate(vol, frames), got, keeps


@pytest.mark.parametrize("name", VR.CASES)
def test_twin_against_the_restatement(name):
    vol, frames, want, got, keeps = reference(name)
    VR.compare_integrate(got, want, name)
    tsdf, weight, rgba = got
    never = ~np.logical_or.reduce(keeps)
    assert bool(np.all(tsdf[never] == 1)) and not weight[never].any() and not rgba[never].any()          # untouched voxels keep their bytes
    assert int(np.logical_or.reduce(keeps).sum()) > 0
    plain, _ = run_twin(vol, frames, colour=False)
    assert plain[0].tobytes() == tsdf.tobytes() and plain[1].tobytes() == weight.tobytes() and plain[2] is None


def test_cases_reach_what_they_are_for():
    vol, frames, want, (tsdf, weight, rgba), keeps = reference("camera_inside")
    wz = vol["origin"][2] + (np.arange(vol["dims"][2]) + 0.5) * vol["voxel"]
    assert (wz < 0).any() and not keeps[0][wz < -0.5].any()                     # voxels behind the camera are dropped
    assert 0 < int(keeps[0].sum()) < keeps[0].size / 2                          # and most of the wide volume lies outside the picture
    vol, frames, want, (tsdf, weight, rgba), keeps = reference("saturation")
    assert len(frames) == int(vol["max_weight"]) + 2 and float(weight.max()) == vol["max_weight"] and float(want["weight"].max()) == vol["max_weight"]
    vol, frames, want, (tsdf, weight, rgba), keeps = reference("trunc_edges")
    hit = (tsdf == -1) & (weight == 1)                                          # sdf == -trunc exactly: kept, t = -1
    assert int(hit.sum()) >= 2 and bool(hit[3].any()) and int(want["skip"].sum()) >= 2
    far = (weight == 1) & (tsdf == 1)                                           # sdf > trunc: t = 1 and the colour is left alone
    assert int(far.sum()) > 50 and not rgba[far].any() and bool(rgba[hit][:, 3].all())
    vol, frames, want, (tsdf, weight, rgba), keeps = reference("two_frames")
    assert float(weight.max()) == 2 and not np.array_equal(frames[0]["C"], frames[1]["C"]) and not np.array_equal(keeps[0], keeps[1])
    vol, frames, want, got, keeps = reference("bad_values")
    p = frames[0]["pred"]
    assert np.isnan(p).any() and (p == 0).any() and (p < 0).any() and (p == np.float32(VR.MIN_DEPTH)).any() and (p == np.float32(VR.MAX_DEPTH)).any()
    assert (p > VR.MAX_DEPTH).any() and (frames[0]["ymap"] < 0).any() and p.shape != (frames[0]["ymap"].size, frames[0]["xmap"].size)


def test_depth_range_is_the_clouds_rule():
    """One voxel, one pixel: d == min_depth is dropped, d == max_depth is kept, NaN / inf / 0 / negative / beyond are dropped."""
    K, C = VR.camera(1, 1), np.eye(4, dtype=np.float32)
    K[0, 2], K[1, 2] = 0.2, -0.1
    one = np.zeros(1, np.int32)
    for d, kept in ((0.25, False), (6.0, True), (np.nan, False), (np.inf, False), (0.0, False), (-1.0, False), (6.5, False), (1.0, True)):
        tsdf, weight, rgba = VR.fresh((1, 1, 1))
        keep = HV.integrate_host(tsdf, weight, rgba, np.full((1, 1), d, np.float32), one, one, K, C, np.full((1, 1, 3), 9, np.uint8), (-0.5, -0.5, 0.5),
                                 1.0, 8.0, 64.0, 0.25, 6.0)
        assert bool(keep[0, 0, 0]) == kept and float(weight[0, 0, 0]) == float(kept), d
    tsdf, weight, rgba = VR.fresh((1, 1, 1))
    HV.integrate_host(tsdf, weight, rgba, np.ones((1, 1), np.float32), -one - 1, one, K, C, None, (-0.5, -0.5, 0.5), 1.0, 8.0, 64.0, 0.25, 6.0)
    assert not weight.any()                                                     # a map entry of -1: outside the prediction


def test_compose_chain_inverts_accumulate_poses():
    from simpledepthestimation_amd.geometry.pose_utils import accumulate_poses
    T = VR.compose_chain(300)
    C = np.eye(4, dtype=np.float32)
    for step in T:
        C = HV.compose_host(step, C)
    want = np.linalg.inv(accumulate_poses(T)[-1])
    bound_R, bound_t = VR.compose_bounds(T)
    err_R, err_t = float(np.abs(C[:3, :3] - want[:3, :3]).max()), float(np.abs(C[:3, 3] - want[:3, 3]).max())
    print(f"300 steps: rotation error {err_R:.3e} (bound {bound_R:.3e}), translation error {err_t:.3e} (bound {bound_t:.3e})")
    assert err_R <= bound_R < 1e-3 and err_t <= bound_t < 1e-1
    assert C.dtype == np.float32 and C[3].tolist() == [0, 0, 0, 1]
    assert not np.allclose(C, np.linalg.inv(want), atol=1e-2)                   # the other direction is something else
    one = HV.compose_host(T[0], np.eye(4, dtype=np.float32))
    assert one.tobytes() == T[0].tobytes()                                      # the first step onto the identity is the step itself


@pytest.mark.parametrize("name", VR.POINT_CASES)
def test_points_twin_against_the_restatement(name):
    inp = VR.point_inputs(name)
    rec, count = HV.points_host(**inp)
    want = VR.restate_points(**inp)
    VR.compare_points(rec, count, want, label=name)
    if name == "empty":
        assert count == 0 and rec.size == 0 and rec.dtype == RECORD
    else:
        assert count > 0
    if name == "f_sides":
        assert count == 2 and tuple(rec[0])[3:6] == tuple(inp["rgba"][0, 0, 0, :3]) and tuple(rec[1])[3:6] == tuple(inp["rgba"][0, 0, 2, :3])
        lighter = dict(inp, weight=np.array([[[2, 1, 2]]], np.float32))
        assert HV.points_host(**lighter)[1] == 0                                # a crossing next to an invalid neighbour gives no record
    if name == "sign_rule":                                                     # 0 and -0 count as not below zero
        row = HV.points_host(inp["tsdf"][:1, :1], inp["weight"][:1, :1], inp["rgba"][:1, :1], inp["origin"], inp["voxel"])
        assert row[1] == 2 and np.all(row[0]["y"] == row[0]["y"][0])


def test_points_order_and_overflow():
    inp = VR.point_inputs("three_axes")
    rec, count = HV.points_host(**inp)
    nz, ny, nx = inp["tsdf"].shape
    # ascending voxel, then axis: the crossings listed by three plain loops, each record on its voxel's centre off the axis and within one voxel along it
    valid, neg = inp["weight"] >= 1, inp["tsdf"] < 0
    cen = [HV.centres_np(n, o, inp["voxel"]) for n, o in zip((nx, ny, nz), inp["origin"])]
    want = [(i, j, k, a) for k in range(nz) for j in range(ny) for i in range(nx) for a, (di, dj, dk) in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1)))
            if i + di < nx and j + dj < ny and k + dk < nz and valid[k, j, i] and valid[k + dk, j + dj, i + di] and neg[k, j, i] != neg[k + dk, j + dj, i + di]]
    assert count == len(want) > 20
    for r, (i, j, k, a) in zip(rec, want):
        got, c = (r["x"], r["y"], r["z"]), (cen[0][i], cen[1][j], cen[2][k])
        assert all(got[b] == c[b] for b in range(3) if b != a) and c[a] <= got[a] <= c[a] + np.float32(1.001) * inp["voxel"], (i, j, k, a)
    assert any(i == nx - 2 and a == 0 for i, j, k, a in want) and any(j == ny - 2 and a == 1 for i, j, k, a in want)              # crossings into the last faces
    assert any(k == nz - 2 and a == 2 for i, j, k, a in want) and any(i == nx - 1 for i, j, k, a in want) and any(k == nz - 1 for i, j, k, a in want)
    cap = count // 2
    first, total = HV.points_host(cap=cap, **inp)
    assert total == count and first.size == cap and first.tobytes() == rec[:cap].tobytes()


def test_ply_round_trip(tmp_path):
    from simpledepthestimation_amd.tools.demo import ply_header
    inp = VR.point_inputs("three_axes")
    rec, count = HV.points_host(**inp)
    raw = np.zeros((count + 3, 16), np.uint8)
    raw[:count] = rec.view(np.uint8).reshape(count, 16)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert HV.write_points_ply(str(tmp_path / "a.ply"), raw, count) == (count, count)
    data = (tmp_path / "a.ply").read_bytes()
    head = ply_header(count)
    assert data.startswith(head) and np.frombuffer(data[len(head):], RECORD).tobytes() == rec.tobytes()
    with pytest.warns(UserWarning, match=f"holds {count} crossings.*room was made for 5"):
        assert HV.write_points_ply(str(tmp_path / "b.ply"), raw[:5], count) == (5, count)
    assert (tmp_path / "b.ply").read_bytes() == ply_header(5) + rec[:5].tobytes()


def test_new_entry_points_are_declared_and_bound():
    from simpledepthestimation_amd.hip import lib as L
    hdr = open(os.path.join(ROOT, "include", "sde_hip.h")).read()
    lib = L.lib()
    for name, n in (("sde_pose_compose", 3), ("sde_tsdf_integrate", 23), ("sde_tsdf_points_ws_bytes", 3), ("sde_tsdf_points", 15)):
        args, res = L._PROTOS[name]
        assert len(args) == n and name in hdr and hasattr(lib, name), name
    assert L._PROTOS["sde_tsdf_points_ws_bytes"][1] is ctypes.c_size_t
    tile, _ = VR.launch_limits()
    assert lib.sde_tsdf_points_ws_bytes(5, 3, 2) == 4 and lib.sde_tsdf_points_ws_bytes(37, 11, 5) == 4 * -(-37 * 11 * 5 // tile)
    assert lib.sde_tsdf_points_ws_bytes(1024, 1024, 1024) == 4 * (1 << 30) // tile
    for dims in ((0, 3, 2), (5, -1, 2), (1025, 1, 1), (1024, 1024, 1025)):
        assert lib.sde_tsdf_points_ws_bytes(*dims) == 0, dims


def test_refusals_precede_any_device_call():
    """Every refusal returns SDE_ERR_ARG with a message; the pointers are never followed (they point into host memory, and this runs without a GPU)."""
    from simpledepthestimation_amd.hip import lib as L
    lib = L.lib()
    host = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(host))
    origin = (ctypes.c_float * 3)(0, 0, 0)
    nan = float("nan")

    def integrate(**kw):
        a = dict(pred=p, ph=2, pw=3, ymap=p, xmap=p, H=4, W=6, frame=None, K=p, C=p, origin=origin, voxel=0.1, trunc=0.4, max_weight=64.0, lo=0.1, hi=80.0,
                 tsdf=p, weight=p, rgba=None, nx=2, ny=2, nz=2)
        a.update(kw)
        return lib.sde_tsdf_integrate(a["pred"], a["ph"], a["pw"], a["ymap"], a["xmap"], a["H"], a["W"], a["frame"], a["K"], a["C"], a["origin"], a["voxel"],
                                      a["trunc"], a["max_weight"], a["lo"], a["hi"], a["tsdf"], a["weight"], a["rgba"], a["nx"], a["ny"], a["nz"], None)
    for kw in (dict(ph=0), dict(pw=-1), dict(H=0), dict(W=0), dict(nx=0), dict(ny=-2), dict(nz=1025), dict(nx=1024, ny=1024, nz=1025), dict(voxel=0.0),
               dict(voxel=nan), dict(trunc=-1.0), dict(trunc=nan), dict(max_weight=0.0), dict(max_weight=nan), dict(lo=80.0), dict(lo=nan), dict(hi=nan),
               dict(pred=None), dict(ymap=None), dict(xmap=None), dict(K=None), dict(C=None), dict(origin=None), dict(tsdf=None), dict(weight=None),
               dict(rgba=ctypes.c_void_p(ctypes.addressof(host) + 2))):
        assert integrate(**kw) == -1, kw
        assert b"sde_tsdf_integrate" in lib.sde_last_error(), kw

    def points(**kw):
        a = dict(tsdf=p, weight=p, rgba=None, nx=2, ny=2, nz=2, origin=origin, voxel=0.1, min_weight=1.0, ws=p, ws_bytes=4, points=p, cap=8, count=p)
        a.update(kw)
        return lib.sde_tsdf_points(a["tsdf"], a["weight"], a["rgba"], a["nx"], a["ny"], a["nz"], a["origin"], a["voxel"], a["min_weight"], a["ws"], a["ws_bytes"],
                                   a["points"], a["cap"], a["count"], None)
    assert ctypes.addressof(host) % 16 == 0
    for kw in (dict(nx=0), dict(nz=2000), dict(voxel=0.0), dict(voxel=nan), dict(min_weight=0.5), dict(min_weight=nan), dict(cap=0), dict(cap=1 << 31),
               dict(tsdf=None), dict(weight=None), dict(origin=None), dict(points=None), dict(count=None), dict(ws=None), dict(ws_bytes=3),
               dict(points=ctypes.c_void_p(ctypes.addressof(host) + 8)), dict(rgba=ctypes.c_void_p(ctypes.addressof(host) + 1))):
        assert points(**kw) == -1, kw
        assert b"sde_tsdf_points" in lib.sde_last_error(), kw
    for T, C in ((None, p), (p, None)):
        assert lib.sde_pose_compose(T, C, None) == -1 and b"sde_pose_compose" in lib.sde_last_error()
    assert not any(host)


def test_volume_refuses_on_the_host():
    good = dict(dims=(4, 4, 4), voxel=0.1)
    dims, voxel, origin, trunc, max_weight, lo, hi = HV.check_params(**good)
    assert origin == tuple(float(np.float32(v)) for v in (-4 * voxel / 2, -4 * voxel / 2, 0.0)) and trunc == float(np.float32(4 * voxel)) and max_weight == 64.0
    for bad in (dict(dims=(4, 4)), dict(dims=(0, 4, 4)), dict(dims=(4, 1025, 4)), dict(dims=(4.5, 4, 4)), dict(dims=(1024, 1024, 1025)), dict(dims="abc"),
                dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=float("nan")), dict(trunc=0.0), dict(trunc=float("nan")), dict(max_weight=0.0),
                dict(max_weight=float("nan")), dict(min_depth=5.0, max_depth=5.0), dict(min_depth=float("nan")), dict(origin=(0, 0)),
                dict(origin=(0, float("inf"), 0))):
        with pytest.raises(ValueError):
            HV.check_params(**dict(good, **bad))
        with pytest.raises(ValueError):
            HV.TsdfVolume(**dict(good, **bad))                                  # refused before anything touches a device
    for bad in (0, 0.5, -1, float("nan")):
        with pytest.raises(ValueError):
            HV.check_min_weight(bad)
        with pytest.raises(ValueError):
            HV.points_host(np.ones((1, 1, 1), np.float32), np.ones((1, 1, 1), np.float32), None, (0, 0, 0), 0.1, min_weight=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HV.TsdfVolume(device="cpu", **good)


def test_demo_tool_parses_volume():
    from simpledepthestimation_amd.tools import demo
    base = ["--cfg", "c.yaml", "--input", "frames", "--pairs", "--intrinsics", "1", "2", "3", "4"]
    a = demo.parse_args(base + ["--volume", "64", "48", "32", "--voxel", "0.1", "--trunc", "0.3", "--volume-origin", "-1", "-2", "0.5", "--min-weight", "2"])
    assert a.volume == [64, 48, 32] and a.voxel == 0.1 and a.trunc == 0.3 and a.volume_origin == [-1.0, -2.0, 0.5] and a.min_weight == 2.0
    assert demo.parse_args(base).volume is None
    for bad in (["--volume", "8", "8", "8"], ["--voxel", "0.1"], ["--trunc", "0.3"], ["--volume", "8", "8", "0", "--voxel", "0.1"],
                ["--volume", "8", "8", "2000", "--voxel", "0.1"], ["--volume", "8", "8", "8", "--voxel", "0"],
                ["--volume", "8", "8", "8", "--voxel", "0.1", "--min-weight", "0.5"], ["--volume", "8", "8", "8", "--voxel", "0.1", "--trunc", "-1"]):
        with pytest.raises(SystemExit):
            demo.parse_args(base + bad)
    with pytest.raises(SystemExit):
        demo.parse_args(["--cfg", "c.yaml", "--input", "frames", "--volume", "8", "8", "8", "--voxel", "0.1"])          # needs --pairs


def test_predictor_parses_volume():
    from simpledepthestimation_amd.engine import predictor as P
    assert P.volume_arg(None) is None
    for bad in (dict(dims=(4, 4, 4)), (4, 4, 4), "volume", 3):
        with pytest.raises(ValueError, match="TsdfVolume"):
            P.volume_arg(bad)
    import inspect
    assert inspect.signature(P.PairPredictor.stream).parameters["volume"].default is None
    assert inspect.signature(P.PairPredictor.predict).parameters["volume"].default is None
    # predict and stream refuse before they look at the frames or the device: an object without __init__ run stands in for the predictor
    pp = object.__new__(P.PairPredictor)
    with pytest.raises(ValueError, match="stateless.*volume"):
        pp.predict([], np.eye(3, dtype=np.float32), volume=object())
    pp.device, pp.offsets = "cuda:0", (-1, 1)
    with pytest.raises(ValueError, match="TsdfVolume"):
        next(pp.stream(iter(()), np.eye(3, dtype=np.float32), volume=dict(dims=(4, 4, 4), voxel=0.1)))

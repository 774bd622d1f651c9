"""GPU: sde_tsdf_integrate, sde_tsdf_points and sde_pose_compose.  Every case is compared bit for bit with the host twins (hip/volume.py) and,
outside the voxels whose keep / drop decision hangs on a rounding, with the float64 restatement of volume_ref.py within its a-priori bounds;
every destination sits between guard bytes."""
import functools

import numpy as np
import pytest
import torch

import volume_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5
GUARD = 64


def guarded(shape, dtype):
    """A destination with guard bytes on both sides, everything filled with FILL: (the whole buffer, the destination view)."""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD:GUARD + nbytes].view(dtype).view(shape)


def guards_intact(buf):
    raw = buf.cpu().numpy()
    return bool((raw[:GUARD] == FILL).all() and (raw[-GUARD:] == FILL).all())


def make_volume(vol, colour=True, state=None):
    """A TsdfVolume whose arrays lie between guard bytes: fresh, or holding `state` = (tsdf, weight, rgba) host arrays."""
    from simpledepthestimation_amd.hip.volume import TsdfVolume
    v = TsdfVolume(vol["dims"], vol["voxel"], origin=vol["origin"], trunc=vol.get("trunc"), max_weight=vol.get("max_weight", 64.0),
                   min_depth=vol.get("min_depth", VR.MIN_DEPTH), max_depth=vol.get("max_depth", VR.MAX_DEPTH), colour=colour, device=DEV)
    nx, ny, nz = v.dims
    bufs = [guarded((nz, ny, nx), torch.float32), guarded((nz, ny, nx), torch.float32)] + ([guarded((nz, ny, nx, 4), torch.uint8)] if colour else [])
    v.tsdf, v.weight = bufs[0][1], bufs[1][1]
    if colour:
        v.rgba = bufs[2][1]
    v.reset()
    if state is not None:
        for dst, src in zip((v.tsdf, v.weight, v.rgba), state):
            if dst is not None:
                dst.copy_(torch.from_numpy(src))
    return v, [b for b, _ in bufs]


def read_back(v, bufs):
    torch.cuda.synchronize()
    assert all(guards_intact(b) for b in bufs), "bytes outside the volume's arrays were written"
    return v.tsdf.cpu().numpy(), v.weight.cpu().numpy(), (v.rgba.cpu().numpy() if v.rgba is not None else None)


def integrate_all(vol, frames, colour=True, with_frame=True, state=None):
    v, bufs = make_volume(vol, colour, state)
    for fr in frames:
        d = {k: torch.from_numpy(fr[k]).to(DEV) for k in ("pred", "K", "C", "frame")}
        v.integrate(d["pred"], fr["ymap"], fr["xmap"], d["K"], d["C"], frame=d["frame"] if with_frame else None)
    return read_back(v, bufs)


def twin_all(vol, frames, colour=True, with_frame=True, state=None):
    from simpledepthestimation_amd.hip.volume import integrate_host
    tsdf, weight, rgba = [None if a is None else a.copy() for a in state] if state is not None else VR.fresh(vol["dims"], colour)
    keeps = [integrate_host(tsdf, weight, rgba, fr["pred"], fr["ymap"], fr["xmap"], fr["K"], fr["C"], fr["frame"] if with_frame else None, vol["origin"],
                            vol["voxel"], vol["trunc"], vol["max_weight"], vol["min_depth"], vol["max_depth"]) for fr in frames]
    return (tsdf, weight, rgba), np.logical_or.reduce(keeps)


@functools.lru_cache(maxsize=None)
def reference(name):
    """Inputs, restatement and the twin's result of one case: computed once, shared, never modified."""
    vol, frames = VR.case_inputs(name)
    return vol, frames, VR.restate_integrate(vol, frames), twin_all(vol, frames)[0]


def same_bits(a, b):
    return all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("name", VR.CASES)
def test_integrate(name):
    vol, frames, want, twin = reference(name)
    got = integrate_all(vol, frames)
    VR.compare_integrate(got, want, name)
    for g, t, what in zip(got, twin, ("tsdf", "weight", "rgba")):
        print(f"  {what}: {int((g.view(np.uint8) != t.view(np.uint8)).sum())} bytes differ from the host twin")
        assert g.tobytes() == t.tobytes(), what
    if name == "odd_dims":
        tile, _ = VR.launch_limits()
        assert 0 < got[0].size < tile                      # one ragged workgroup
    if name == "saturation":
        assert float(got[1].max()) == vol["max_weight"] and len(frames) == int(vol["max_weight"]) + 2
    if name == "trunc_edges":
        assert int(((got[0] == -1) & (got[1] == 1)).sum()) >= 2                     # sdf == -trunc exactly is kept
        far = (got[0] == 1) & (got[1] == 1)
        assert int(far.sum()) > 50 and not got[2][far].any()                        # sdf > trunc: t = 1, colour untouched


def test_grid_stride_integrate_and_points():
    """More voxels than TILE * MAX_BLOCKS: the integrate kernel walks its grid-stride loop, and the points kernels walk more tiles than workgroups."""
    from simpledepthestimation_amd.hip.cloud import as_records
    from simpledepthestimation_amd.hip.volume import points_host
    tile, cap = VR.launch_limits()
    vol, frames, want, twin = reference("grid_stride")
    assert int(np.prod(vol["dims"])) > tile * cap
    v, bufs = make_volume(vol)
    fr = frames[0]
    d = {k: torch.from_numpy(fr[k]).to(DEV) for k in ("pred", "K", "C", "frame")}
    v.integrate(d["pred"], fr["ymap"], fr["xmap"], d["K"], d["C"], frame=d["frame"])
    got = read_back(v, bufs)
    VR.compare_integrate(got, want, "grid_stride")
    assert same_bits(got, twin)
    rec, count = points_host(twin[0], twin[1], twin[2], vol["origin"], vol["voxel"])
    assert count > 1000
    pbuf, points = guarded((count + 5, 16), torch.uint8)
    points, n = v.points(cap=count + 5, out=(points, torch.zeros(1, dtype=torch.int32, device=DEV)))
    torch.cuda.synchronize()
    assert int(n.item()) == count and guards_intact(pbuf)
    assert as_records(points, n).tobytes() == rec.tobytes()
    assert bool((points[count:].cpu().numpy() == FILL).all())                       # the slots behind the records are not touched


@pytest.mark.parametrize("name", ["two_frames", "bad_values"])
def test_with_and_without_frame_and_rgba(name):
    vol, frames, _, twin = reference(name)
    for colour, with_frame in ((False, False), (False, True), (True, False)):
        got = integrate_all(vol, frames, colour=colour, with_frame=with_frame)
        assert got[0].tobytes() == twin[0].tobytes() and got[1].tobytes() == twin[1].tobytes(), (colour, with_frame)
        assert (got[2] is None) == (not colour) and (got[2] is None or not got[2].any())          # colour is skipped: rgba keeps its zeros


def test_untouched_voxels_keep_their_bytes_and_two_runs_agree():
    vol, frames = VR.case_inputs("camera_inside")
    nx, ny, nz = vol["dims"]
    state = (np.full((nz, ny, nx), FILL, np.uint8).repeat(4).view(np.float32).reshape(nz, ny, nx).copy(),) * 2 + (np.full((nz, ny, nx, 4), FILL, np.uint8),)
    twin, kept = twin_all(vol, frames, state=state)
    a, b = integrate_all(vol, frames, state=state), integrate_all(vol, frames, state=state)
    assert same_bits(a, b) and same_bits(a, twin)
    assert 0 < int(kept.sum()) < kept.size
    for arr in a:
        assert bool((arr[~kept].view(np.uint8) == FILL).all())
    assert not bool((a[1][kept].view(np.uint8) == FILL).all())


def run_points(inp, cap=None, colour=True, slack=0):
    """-> (records of the first min(count, cap), count, the raw points buffer [cap + slack, 16]); guards checked."""
    from simpledepthestimation_amd.hip.cloud import as_records
    nz, ny, nx = inp["tsdf"].shape
    vol = dict(dims=(nx, ny, nz), voxel=float(inp["voxel"]), origin=tuple(float(o) for o in inp["origin"]))
    v, bufs = make_volume(vol, colour, state=(inp["tsdf"], inp["weight"], inp["rgba"]))
    from simpledepthestimation_amd.hip.volume import points_host
    total = points_host(**inp)[1] if cap is None else cap                           # only the room that is made depends on it
    room = max(total + slack, 1)
    pbuf, points = guarded((room, 16), torch.uint8)
    cbuf, count = guarded((1,), torch.int32)
    wbuf, ws = guarded((v.workspace_numel(),), torch.int32)
    p, c = v.points(min_weight=inp["min_weight"], cap=room, out=(points, count), workspace=ws)
    read_back(v, bufs)
    assert p.data_ptr() == points.data_ptr() and c.data_ptr() == count.data_ptr()
    assert guards_intact(pbuf) and guards_intact(cbuf) and guards_intact(wbuf), "bytes outside a destination were written"
    n = int(count.item())
    raw = points.cpu().numpy()
    return as_records(raw, min(n, room)), n, raw


@pytest.mark.parametrize("name", VR.POINT_CASES)
def test_points(name):
    from simpledepthestimation_amd.hip.volume import points_host
    inp = VR.point_inputs(name)
    twin, total = points_host(**inp)
    rec, count, raw = run_points(inp, slack=3)
    VR.compare_points(rec, count, VR.restate_points(**inp), label=name)
    assert count == total and rec.tobytes() == twin.tobytes()
    assert bool((raw[count:] == FILL).all())                                        # the slots behind the records are not touched
    if name == "several_workgroups":
        tile, _ = VR.launch_limits()
        assert inp["tsdf"].size > 4 * tile and inp["tsdf"].size % tile != 0
    if name == "two_scan_chunks":
        tile, _ = VR.launch_limits()
        assert -(-inp["tsdf"].size // tile) > tile                                  # more tiles than one chunk of the scan
    if name == "empty":
        assert count == 0


def test_points_overflow_and_no_colour():
    from simpledepthestimation_amd.hip.volume import points_host
    inp = VR.point_inputs("several_workgroups")
    twin, total = points_host(**inp)
    cap = total // 3
    rec, count, raw = run_points(inp, cap=cap)                                      # run_points checks the guards behind the cap-th record
    assert count == total > cap and rec.size == cap and rec.tobytes() == twin[:cap].tobytes()
    plain, n, _ = run_points(inp, colour=False)
    want, _ = points_host(inp["tsdf"], inp["weight"], None, inp["origin"], inp["voxel"], inp["min_weight"])
    assert n == total and plain.tobytes() == want.tobytes() and not plain["red"].any() and bool((plain["alpha"] == 255).all())
    again, n2, _ = run_points(inp)
    assert n2 == total and again.tobytes() == twin.tobytes()                        # two runs, the same bytes


def test_compose_chain():
    from simpledepthestimation_amd.hip.volume import compose_host, pose_compose
    T = VR.compose_chain(6)
    buf, C = guarded((4, 4), torch.float32)
    C.copy_(torch.eye(4, device=DEV))
    want = np.eye(4, dtype=np.float32)
    dT = torch.from_numpy(T).to(DEV)
    for k in range(T.shape[0]):
        pose_compose(dT[k], C)
        want = compose_host(T[k], want)
        assert C.cpu().numpy().tobytes() == want.tobytes(), k
    assert guards_intact(buf)


def test_capturable():
    """compose + integrate + points in one graph, replayed twice, equal two eager rounds: the pose and the volume move on with every replay."""
    vol, frames, _, _ = reference("two_frames")
    fr = frames[1]
    d = {k: torch.from_numpy(fr[k]).to(DEV) for k in ("pred", "K", "C", "frame")}
    step = torch.from_numpy(VR.compose_chain(1)[0]).to(DEV)
    results = []
    for use_graph in (False, True):
        v, bufs = make_volume(vol)
        C = d["C"].clone()
        ymap, xmap = torch.from_numpy(fr["ymap"]).to(DEV), torch.from_numpy(fr["xmap"]).to(DEV)
        points, count = torch.zeros((v.default_cap(), 16), dtype=torch.uint8, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        ws = torch.empty(v.workspace_numel(), dtype=torch.int32, device=DEV)

        def chain():
            v.integrate(d["pred"], ymap, xmap, d["K"], C, frame=d["frame"])
            v.compose(step, C)
            v.points(out=(points, count), workspace=ws)
        if use_graph:
            from simpledepthestimation_amd.hip import present as HP
            HP.ensure_checked(ymap, xmap, *fr["pred"].shape, torch.device(DEV))     # the one validation of a device pair, outside the capture
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                chain()
            g.replay()
            g.replay()
        else:
            chain()
            chain()
        results.append(read_back(v, bufs) + (C.cpu().numpy(), points.cpu().numpy(), count.cpu().numpy()))
    assert same_bits(*results) and int(results[0][5][0]) > 0 and float(results[0][1].max()) == 2


def test_binding_refuses_what_the_library_would():
    from simpledepthestimation_amd.hip import lib as L
    from simpledepthestimation_amd.hip.volume import pose_compose
    vol, frames, _, _ = reference("odd_dims")
    fr = frames[0]
    v, _ = make_volume(vol)
    d = {k: torch.from_numpy(fr[k]).to(DEV) for k in ("pred", "K", "C", "frame")}
    with pytest.raises(L.SdeHipError):
        v.integrate(d["pred"], fr["ymap"], fr["xmap"], d["K"], d["C"][:3])
    with pytest.raises(L.SdeHipError):
        v.integrate(d["pred"], fr["ymap"], fr["xmap"], d["K"], d["C"], frame=d["frame"][:-1])
    with pytest.raises(L.SdeHipError):
        v.integrate(torch.stack([d["pred"], d["pred"]]), fr["ymap"], fr["xmap"], d["K"], d["C"])
    with pytest.raises(L.SdeHipError):
        v.integrate(d["pred"].cpu(), fr["ymap"], fr["xmap"], d["K"], d["C"])
    with pytest.raises(ValueError):
        v.points(min_weight=0)
    with pytest.raises(ValueError):
        v.points(cap=0)
    with pytest.raises(L.SdeHipError):
        v.points(out=(torch.empty((4, 8), dtype=torch.uint8, device=DEV), None), cap=4)
    with pytest.raises(L.SdeHipError):
        pose_compose(d["C"][:3], d["C"])

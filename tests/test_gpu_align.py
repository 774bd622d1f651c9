"""GPU: sde_frame_align and sde_frame_align_reset.  Every case of align_ref.py is compared bit for bit with the host twins (hip/align.py): the
whole state, every info word.  The state sits between guard bytes, the workspace is pre-filled with NaN bytes, the volume's arrays and the
rendered model are read back unchanged, and the sequence render -> reset -> align x n -> compose is captured into a graph and replayed."""
import functools

import numpy as np
import pytest
import torch

import align_ref as AR
from simpledepthestimation_amd.hip import align as AL
from test_gpu_volume import DEV, FILL, guarded, guards_intact, make_volume, read_back

pytestmark = pytest.mark.gpu

KW = dict(dist_tol=0.03, scale_tol=0.1, min_count=6, damping=1e-4)
MODES = (AL.POSE, AL.SCALE, AL.POSE | AL.SCALE)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def twin_path(name, schedule, dist_tol=KW["dist_tol"], min_count=KW["min_count"]):
    """The twin's states after every iteration of `schedule` from a fresh state: computed once, shared, never modified."""
    inp = AR.case_inputs(name)
    w, out = AL.state_host(), []
    for mode in schedule:
        w = AL.frame_align_host(w, inp["pred"], inp["ymap"], inp["xmap"], inp["K"], inp["model_depth"], inp["model_normal"], mode=mode,
                                min_depth=inp["min_depth"], max_depth=inp["max_depth"], **{**KW, "dist_tol": dist_tol, "min_count": min_count})
        out.append(w)
    return tuple(out)


class Run:
    """The device side of one case: the inputs uploaded, a guarded state, a workspace full of NaN bytes."""

    def __init__(self, name):
        self.inp = inp = AR.case_inputs(name)
        self.H, self.W = inp["size"]
        self.pred, self.K, self.depth, self.normal = dev(inp["pred"]), dev(inp["K"]), dev(inp["model_depth"]), dev(inp["model_normal"])
        self.ymap, self.xmap = dev(inp["ymap"].astype(np.int32)), dev(inp["xmap"].astype(np.int32))
        self.buf, self.state = guarded((AL.STATE_WORDS,), torch.float32)
        self.ws = torch.full((AL.workspace_numel(self.H, self.W) * 4,), 0xFF, dtype=torch.uint8, device=DEV).view(torch.float32)
        assert self.ws.numel() == AL.slab_rows(self.H, self.W) * 32 and bool(torch.isnan(self.ws).all())

    def reset(self):
        from simpledepthestimation_amd.hip import lib as L
        L.check(L.lib().sde_frame_align_reset(L.ptr(self.state), L.stream()), "sde_frame_align_reset")

    def step(self, mode, **kw):
        AL.frame_align(self.pred, self.ymap, self.xmap, self.K, self.depth, self.normal, self.state, mode=mode, min_depth=self.inp["min_depth"],
                       max_depth=self.inp["max_depth"], workspace=self.ws, **{**KW, **kw})

    def words(self):
        torch.cuda.synchronize()
        assert guards_intact(self.buf), "bytes outside the state were written"
        return self.state.cpu().numpy()

    def inputs_unchanged(self):
        inp = self.inp
        return all(t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes() for t, a in (
            (self.pred, inp["pred"]), (self.K, inp["K"]), (self.depth, inp["model_depth"]), (self.normal, inp["model_normal"])))


def show(got, want, label):
    g, w = AL.unpack_state(got), AL.unpack_state(want)
    print(f"{label}: status {g['status']} / {w['status']}, count {g['count']} / {w['count']}, scale count {g['scale_count']} / {w['scale_count']}, "
          f"{int((got.view(np.uint8) != want.view(np.uint8)).sum())} bytes differ from the host twin")


def test_reset_writes_the_fresh_state_between_its_guards():
    r = Run("corner_8x8")
    assert bool((r.state.view(torch.uint8) == FILL).all())
    r.reset()
    assert r.words().tobytes() == AL.state_host().tobytes()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ("corner_8x8", "corner_9x33", "corner_maps", "corner_264", "bad_values"))
def test_iterations_match_the_twin_bit_for_bit(name, mode):
    """Two iterations of one mode from a fresh state: the second one starts from a D that is no identity and a scale that is not 1.  8 x 8 is
    one wave, 9 x 33 ragged against the 32 x 8 workgroup, corner_maps has -1 borders, holes and a prediction of another size, 264 x 264 has
    297 workgroups: more rows in the slab than the finish launch has row groups."""
    schedule = (mode, mode)
    # the small pictures: a gate wide enough for the 4 % the depth is short, so that the pose iterations have inliers
    tol = 0.1 if name in ("corner_8x8", "corner_9x33") else KW["dist_tol"]
    want = twin_path(name, schedule, tol)
    r = Run(name)
    r.reset()
    for i, m in enumerate(schedule):
        r.step(m, dist_tol=tol)
        got = r.words()
        show(got, want[i], f"{name} mode {m} iteration {i + 1}")
        assert got.tobytes() == want[i].tobytes()
    first = AL.unpack_state(want[0])                                                   # (the 8 x 8 picture's second pose step finds nothing: too few)
    assert first["status"] == AL.OK and first["count"] >= KW["min_count"] and first["scale_count"] >= KW["min_count"]
    if name == "corner_264":
        assert AL.slab_rows(r.H, r.W) == 297
    assert r.inputs_unchanged()
    slab = r.ws.cpu().numpy()
    assert np.isfinite(slab).all()                                                      # every workgroup wrote its whole row over the NaN fill


def test_default_schedule_on_the_corner_matches_the_twin_and_converges():
    want = twin_path("corner", AL.DEFAULT_SCHEDULE, AL.DEFAULTS["dist_tol"], AL.DEFAULTS["min_count"])
    r = Run("corner")
    r.reset()
    for i, m in enumerate(AL.DEFAULT_SCHEDULE):
        r.step(m, **AL.DEFAULTS)
        got = r.words()
        show(got, want[i], f"corner iteration {i + 1}")
        assert got.tobytes() == want[i].tobytes()
    u = AL.unpack_state(got)
    rot, tr = AR.pose_error(u["D"], r.inp["D_true"])
    rot0, tr0 = AR.pose_error(np.eye(4), r.inp["D_true"])
    assert rot < 0.5 * rot0 and tr < 0.5 * tr0 and abs(u["scale"] - r.inp["s_true"]) < 0.5 * abs(1 - r.inp["s_true"])


def test_both_refusal_statuses_leave_the_transform():
    fresh = AL.state_host()
    for name, status, tol in (("plane", AL.SINGULAR, 0.1), ("empty", AL.TOO_FEW, KW["dist_tol"])):
        want = twin_path(name, (AL.POSE | AL.SCALE,), tol, 32)[0]
        r = Run(name)
        r.reset()
        r.step(AL.POSE | AL.SCALE, dist_tol=tol, min_count=32)
        got = r.words()
        show(got, want, name)
        assert got.tobytes() == want.tobytes()
        assert AL.unpack_state(got)["status"] == status and got[:33].tobytes() == fresh[:33].tobytes()
    assert AL.unpack_state(got)["count"] == 0


def test_two_runs_give_the_same_bytes_whatever_the_workspace_held():
    first = None
    for fill in (0xFF, 0x00, 0x7F):
        r = Run("corner_maps")
        r.ws.view(torch.uint8).fill_(fill)
        r.reset()
        for m in (AL.SCALE, AL.POSE | AL.SCALE, AL.POSE):
            r.step(m)
        got = r.words()
        first = got if first is None else first
        assert got.tobytes() == first.tobytes()
    assert first.tobytes() == twin_path("corner_maps", (AL.SCALE, AL.POSE | AL.SCALE, AL.POSE))[-1].tobytes()


def tracked_volume(name):
    inp = AR.case_inputs(name)
    vol = dict(inp["vol"])
    v, vbufs = make_volume(vol, colour=False, state=inp["volume"])
    return inp, v, vbufs


def test_track_renders_resets_and_iterates_and_leaves_the_volume():
    inp, v, vbufs = tracked_volume("corner")
    before = read_back(v, vbufs)
    near, step, n = inp["render"]
    far = float(near) + (n - 0.5) * float(step)
    pred, K, C = dev(inp["pred"]), dev(inp["K"]), dev(inp["C"])
    state = v.track(pred, inp["ymap"], inp["xmap"], K, C, inp["size"], near=near, far=far, step=step)
    torch.cuda.synchronize()
    assert state.model_depth.cpu().numpy().tobytes() == inp["model_depth"].tobytes()
    assert state.model_normal.cpu().numpy().tobytes() == inp["model_normal"].tobytes()
    want = twin_path("corner", AL.DEFAULT_SCHEDULE, AL.DEFAULTS["dist_tol"], AL.DEFAULTS["min_count"])[-1]
    assert state.state.cpu().numpy().tobytes() == want.tobytes()
    assert state.info()["status"] == AL.OK
    after = read_back(v, vbufs)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before[:2], after[:2]))
    again = v.track(pred, inp["ymap"], inp["xmap"], K, C, inp["size"], near=near, far=far, step=step, state=state)       # the same buffers: reset first
    assert again is state and state.state.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        v.track(pred, inp["ymap"], inp["xmap"], K, C, inp["size"], schedule=())
    with pytest.raises(ValueError):
        v.track(pred, inp["ymap"], inp["xmap"], K, C, inp["size"], schedule=(1, 4))
    with pytest.raises(ValueError):
        v.track(pred, inp["ymap"], inp["xmap"], K, C, (8, 8), state=state)


def test_graph_of_render_reset_align_compose_replays_to_the_same_bytes():
    from simpledepthestimation_amd.hip.present import device_maps
    from simpledepthestimation_amd.hip.volume import compose_host
    inp, v, vbufs = tracked_volume("corner_maps")
    near, step, n = inp["render"]
    far = float(near) + (n - 0.5) * float(step)
    schedule = (AL.SCALE, AL.POSE | AL.SCALE, AL.POSE | AL.SCALE)
    pred, K, C0 = dev(inp["pred"]), dev(inp["K"]), dev(inp["C"])
    ymap, xmap = device_maps(inp["ymap"], inp["xmap"], *inp["pred"].shape, DEV)
    C = C0.clone()
    state = AL.AlignState(inp["size"], DEV)
    # the model of this case has holes cut into it after the render: the twin of the graph renders for itself
    from simpledepthestimation_amd.hip.volume import render_host
    tsdf, weight, _ = inp["volume"]
    depth, normal, _ = render_host(tsdf, weight, None, inp["K"], inp["C"], inp["size"], inp["vol"]["origin"], inp["vol"]["voxel"], near, step, n, 1)
    w = AL.track_host((depth, normal), inp["pred"], inp["ymap"], inp["xmap"], inp["K"], schedule=schedule, min_depth=inp["min_depth"],
                      max_depth=inp["max_depth"], **KW)
    want_C = compose_host(AL.unpack_state(w)["Dinv"], inp["C"])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        v.track(pred, ymap, xmap, K, C, inp["size"], schedule=schedule, near=near, far=far, step=step, state=state, **KW)
        v.compose(state.Dinv, C)
    for _ in range(2):
        C.copy_(C0)
        state.state.fill_(float("nan"))
        state.workspace.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert state.state.cpu().numpy().tobytes() == w.tobytes()
        assert C.cpu().numpy().tobytes() == want_C.tobytes()
    assert AL.unpack_state(w)["status"] == AL.OK
    read_back(v, vbufs)


def test_binding_refuses_what_the_library_would():
    from simpledepthestimation_amd.hip import lib as L
    r = Run("corner_8x8")
    r.reset()
    args = (r.pred, r.ymap, r.xmap, r.K, r.depth, r.normal, r.state)
    for bad in (dict(mode=0), dict(mode=4), dict(dist_tol=0.0), dict(scale_tol=float("nan")), dict(damping=-1.0), dict(min_count=5),
                dict(min_depth=2.0, max_depth=1.0)):
        with pytest.raises(ValueError):
            AL.frame_align(*args, workspace=r.ws, **bad)
    with pytest.raises(L.SdeHipError):
        AL.frame_align(*args, workspace=r.ws[:-1])
    with pytest.raises(L.SdeHipError):
        AL.frame_align(*args)                                                         # a bare state tensor needs a workspace
    with pytest.raises(L.SdeHipError):
        AL.frame_align(r.pred, r.ymap, r.xmap, r.K, r.depth[:4], r.normal, r.state, workspace=r.ws)
    with pytest.raises(L.SdeHipError):
        AL.frame_align(r.pred, r.ymap, r.xmap, r.K, r.depth, r.normal.cpu(), r.state, workspace=r.ws)
    with pytest.raises(L.SdeHipError):
        AL.frame_align(r.pred, r.ymap, r.xmap, r.K, r.depth, r.normal, r.state[:39], workspace=r.ws)
    assert r.words().tobytes() == AL.state_host().tobytes()                            # nothing was launched

"""GPU: PairPredictor.stream(..., volume=vol, render=...) on the tiny random-weight models of test_gpu_temporal_stream.py: every yielded
model_depth / model_normal / model_picture is, bit for bit, render_host applied to the volume and the pose replayed on the host from what the
stream itself yielded (the method of test_gpu_volume_stream.py) -- that pins the moment of the render (after the window's depth went in), the
pose, the size and the intrinsics it is taken with."""
import numpy as np
import pytest
import torch

from test_gpu_temporal_stream import DEV, HS, K_SRC, NET_H, NET_W, TEMPORAL, WS, collect, pair_cfg, sequence
from test_gpu_volume_stream import MODES, new_volume, volume_bytes, volume_params

pytestmark = pytest.mark.gpu
MODEL_KEYS = {"model_depth", "model_normal", "model_picture"}


def render_params(VOL):
    """Samples one voxel apart from half way to the near face to one voxel behind the far face: about 20 of them."""
    near = float(np.float32(VOL["origin"][2] / 2))
    return dict(normals=True, picture=True, min_weight=1, near=near, far=VOL["origin"][2] + (VOL["dims"][2] + 1) * VOL["voxel"], step=VOL["voxel"])


@pytest.fixture(scope="module", params=["MonoDepth2Model", "MotionLearningModel"])
def setup(request):
    """One model per family, an eager and a graph predictor on it, and the rendering volume stream of both, plain and temporal: computed once,
    shared, never modified."""
    from simpledepthestimation_amd.engine.predictor import PairPredictor
    from simpledepthestimation_amd.modeling import build_model
    cfg = pair_cfg(request.param)
    torch.manual_seed(21)
    model = build_model(cfg).eval()
    frames = sequence(6)
    eager, graph = PairPredictor(cfg, model=model, use_graph=False), PairPredictor(cfg, model=model, use_graph=True)
    VOL = volume_params(graph, frames)
    out = {"arch": request.param, "frames": frames, "eager": eager, "graph": graph, "vol": VOL, "render": render_params(VOL)}
    for route, pp in (("eager", eager), ("graph", graph)):
        for mode, kw in MODES.items():
            v = new_volume(VOL)
            out[f"{mode}_{route}"] = (collect(pp, frames, volume=v, render=out["render"], **kw), volume_bytes(v))
    return out


@pytest.mark.parametrize("route", ["eager", "graph"])
@pytest.mark.parametrize("mode", ["plain", "temporal"])
def test_every_render_is_the_host_twin_of_what_was_yielded(setup, route, mode):
    from simpledepthestimation_amd.hip.volume import check_render, compose_host, integrate_host, render_host
    import volume_ref as VR
    recs, got = setup[f"{mode}_{route}"]
    pp, VOL, rp = setup[route], setup["vol"], setup["render"]
    plan = pp.plan(HS, WS)
    ymap, xmap = plan.maps((NET_H, NET_W))
    H, W, near, step, n = check_render((HS, WS), rp["near"], rp["far"], rp["step"])
    assert 10 <= n <= 40
    origin, voxel = tuple(float(np.float32(o)) for o in VOL["origin"]), float(np.float32(VOL["voxel"]))
    tsdf, weight, rgba = VR.fresh(VOL["dims"])
    j = pp.offsets.index(1)
    C = np.eye(4, dtype=np.float32)
    hits = []
    for k, r in enumerate(recs):
        if k:
            C = compose_host(recs[k - 1]["pose"][j], C)
        integrate_host(tsdf, weight, rgba, r["depth_net"], np.asarray(ymap), np.asarray(xmap), K_SRC, C, setup["frames"][r["index"]], origin, voxel, VOL["trunc"],
                       VOL["max_weight"], VOL["min_depth"], VOL["max_depth"])
        want = render_host(tsdf, weight, rgba, K_SRC, C, (HS, WS), origin, voxel, near, step, n, rp["min_weight"])
        assert r["world_to_camera"].tobytes() == C.tobytes(), k
        for key, w in zip(("model_depth", "model_normal", "model_picture"), want):
            assert r[key].dtype == w.dtype and r[key].shape == w.shape, (k, key)
            print(f"{setup['arch']} {mode} {route} window {k} {key}: {int((r[key].view(np.uint8) != w.view(np.uint8)).sum())} bytes differ from the host replay")
            assert r[key].tobytes() == w.tobytes(), (k, key)
        hits.append(int((want[0] != 0).sum()))
    print(f"{setup['arch']} {mode} {route}: pixels with a surface per window {hits} of {HS * WS}")
    assert min(hits) > HS * WS // 10                                              # the model is in view in every window
    for g, w, what in zip(got, (tsdf, weight, rgba), ("tsdf", "weight", "rgba")):
        assert g.tobytes() == w.tobytes(), what


def test_eager_and_graph_agree(setup):
    for mode in MODES:
        (ra, va), (rb, vb) = setup[f"{mode}_eager"], setup[f"{mode}_graph"]
        assert all(a[k].tobytes() == b[k].tobytes() for a, b in zip(ra, rb) for k in MODEL_KEYS), mode
        assert all(x.tobytes() == y.tobytes() for x, y in zip(va, vb)), mode


def test_without_render_records_and_keys_are_unchanged(setup):
    pp, VOL = setup["graph"], setup["vol"]
    for mode, kw in MODES.items():
        v = new_volume(VOL)
        plain = collect(pp, setup["frames"], volume=v, **kw)
        recs, vol = setup[f"{mode}_graph"]
        assert len(plain) == len(recs) and all(x.tobytes() == y.tobytes() for x, y in zip(volume_bytes(v), vol))
        for a, b in zip(plain, recs):
            assert set(a) <= set(b) and set(b) - set(a) == MODEL_KEYS
            for k in a:
                assert (a[k].tobytes() == b[k].tobytes()) if isinstance(a[k], np.ndarray) else a[k] == b[k], (mode, k)
    keys = [k for s in pp._slots.values() for k in s.graphs]
    tagged = lambda k, tag: any(isinstance(e, tuple) and e and e[0] == tag for e in k)
    with_render = [k for k in keys if tagged(k, "render")]
    assert with_render and all(tagged(k, "volume") and k[-1][0] == "render" and k[-2][0] == "volume" for k in with_render)
    assert any(tagged(k, "volume") and not tagged(k, "render") and k[-1][0] == "volume" for k in keys)         # volume= alone replays the key it always had
    assert all(k[-1][1:4] == (True, True, 1.0) for k in with_render)


def test_switched_off_outputs_are_absent_and_refusals(setup):
    pp, VOL = setup["graph"], setup["vol"]
    v = new_volume(VOL)
    recs = collect(pp, setup["frames"], volume=v, present=False, render=dict(setup["render"], normals=False, picture=False))
    want = setup["plain_graph"][0]
    assert all("model_normal" not in r and "model_picture" not in r for r in recs)
    assert all(a["model_depth"].tobytes() == b["model_depth"].tobytes() for a, b in zip(recs, want))
    with pytest.raises(ValueError, match="needs volume"):
        next(pp.stream(iter(setup["frames"]), K_SRC, render=setup["render"]))
    with pytest.raises(ValueError, match="stateless"):
        pp.predict([setup["frames"][1], setup["frames"][0], setup["frames"][2]][:1 + pp.n], K_SRC, render=setup["render"])
    from simpledepthestimation_amd.hip.volume import TsdfVolume
    plain = TsdfVolume(VOL["dims"], VOL["voxel"], origin=VOL["origin"], colour=False, device=DEV)
    with pytest.raises(ValueError, match="colour"):
        next(pp.stream(iter(setup["frames"]), K_SRC, volume=plain, render=setup["render"]))

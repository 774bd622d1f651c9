"""GPU: PairPredictor.stream(..., volume=vol, track=...) on the tiny random-weight models of test_gpu_temporal_stream.py (ResNet-18, network
size 64 x 96, five 80 x 120 frames).  Everything the tracked stream does to the pose and to the volume is recomputed on the host from what the
stream itself yielded -- compose_host, render_host, the alignment twins, integrate_host -- bit for bit: that pins the order (predict, render,
align, correct, integrate), the direction of the correction (D^-1 C) and the depth that goes in (times the scale)."""
import numpy as np
import pytest
import torch

from test_gpu_temporal_stream import DEV, HS, K_SRC, NET_H, NET_W, TEMPORAL, WS, collect, pair_cfg, sequence
from test_gpu_volume_stream import DIMS, new_volume, volume_bytes, volume_params

pytestmark = pytest.mark.gpu
SCHEDULE = (2, 3, 3)
# a random-weight network's depth is smooth but means nothing: wide gates, a small count
TRACK_KW = dict(dist_tol=0.2, scale_tol=0.3, min_count=64, damping=1e-4)
MODES = {"plain": dict(present=False), "temporal": dict(temporal=TEMPORAL), "render": dict(present=False, render=dict(picture=True, normals=True))}


def track_of(VOL):
    """The render range of the tracker: the volume's own extent along z, so that the march is a few dozen samples."""
    near = float(VOL["origin"][2])
    return dict(schedule=SCHEDULE, near=near, far=near + 1.25 * DIMS[2] * VOL["voxel"], step=VOL["voxel"], **TRACK_KW)


def stream_into(pp, frames, params, **kw):
    v = new_volume(params)
    if "render" in kw:
        t = track_of(params)
        kw = dict(kw, render=dict(kw["render"], near=t["near"], far=t["far"], step=t["step"]))
    recs = collect(pp, frames, volume=v, track=track_of(params), **kw)
    return recs, volume_bytes(v)


@pytest.fixture(scope="module", params=["MonoDepth2Model", "MotionLearningModel"])
def setup(request):
    """One model per family, an eager and a graph predictor on it, and the tracked volume stream of both in every mode: computed once, shared,
    never modified."""
    from simpledepthestimation_amd.engine.predictor import PairPredictor
    from simpledepthestimation_amd.modeling import build_model
    cfg = pair_cfg(request.param)
    torch.manual_seed(21)
    model = build_model(cfg).eval()
    frames = sequence(5)
    eager, graph = PairPredictor(cfg, model=model, use_graph=False), PairPredictor(cfg, model=model, use_graph=True)
    out = {"arch": request.param, "frames": frames, "eager": eager, "graph": graph, "vol": volume_params(graph, frames)}
    for route, pp in (("eager", eager), ("graph", graph)):
        for mode, kw in MODES.items():
            out[f"{mode}_{route}"] = stream_into(pp, frames, out["vol"], **kw)
    return out


def host_replay(pp, recs, frames, VOL, render):
    """-> (per record: dict(C, words, model) of the host, the volume): the tracked chain recomputed from the yielded records."""
    from simpledepthestimation_amd.hip import align as AL
    from simpledepthestimation_amd.hip.volume import check_render, compose_host, integrate_host, render_host
    import volume_ref as VR
    plan = pp.plan(HS, WS)
    ymap, xmap = (np.asarray(m) for m in plan.maps((NET_H, NET_W)))
    tsdf, weight, rgba = VR.fresh(VOL["dims"])
    origin, voxel = tuple(np.float32(o) for o in VOL["origin"]), np.float32(VOL["voxel"])
    t = track_of(VOL)
    _, _, near, step, n = check_render((HS, WS), t["near"], t["far"], t["step"])
    j = pp.offsets.index(1)
    C = np.eye(4, dtype=np.float32)
    out = []
    for k, r in enumerate(recs):
        if k:
            C = compose_host(recs[k - 1]["pose"][j], C)                                 # the PREDICTED pose, from the corrected one before
        depth, normal, _ = render_host(tsdf, weight, rgba, K_SRC, C, (HS, WS), origin, voxel, near, step, n, 1)
        w = AL.track_host((depth, normal), r["depth_net"], ymap, xmap, K_SRC, schedule=SCHEDULE, min_depth=VOL["min_depth"], max_depth=VOL["max_depth"],
                          **TRACK_KW)
        u = AL.unpack_state(w)
        C = compose_host(u["Dinv"], C)                                                  # world -> corrected camera = D^-1 C
        integrate_host(tsdf, weight, rgba, r["depth_net"] * np.float32(u["scale"]), ymap, xmap, K_SRC, C, frames[r["index"]], origin, voxel, VOL["trunc"],
                       VOL["max_weight"], VOL["min_depth"], VOL["max_depth"])
        model = render_host(tsdf, weight, rgba, K_SRC, C, (HS, WS), origin, voxel, near, step, n, 1) if render else None
        out.append(dict(C=C, state=u, model=model))
    return out, (tsdf, weight, rgba)


@pytest.mark.parametrize("route", ["eager", "graph"])
@pytest.mark.parametrize("mode", list(MODES))
def test_tracked_stream_is_the_host_replay_of_what_was_yielded(setup, route, mode):
    from simpledepthestimation_amd.hip import align as AL
    recs, got = setup[f"{mode}_{route}"]
    pp, VOL = setup[route], setup["vol"]
    want, vol = host_replay(pp, recs, setup["frames"], VOL, mode == "render")
    print(f"{setup['arch']} {mode} {route}: status {[r['track_status'] for r in recs]}, inliers {[r['track_count'] for r in recs]}, "
          f"scale {[round(float(r['track_scale']), 4) for r in recs]}")
    first = recs[0]
    assert first["track_status"] == AL.TOO_FEW and first["track_count"] == 0 and first["track_scale"] == 1.0       # an empty volume: every ray misses
    assert first["track_delta"].tobytes() == np.eye(4, dtype=np.float32).tobytes() == first["world_to_camera"].tobytes()
    for k, (r, w) in enumerate(zip(recs, want)):
        u = w["state"]
        assert r["track_delta"].dtype == np.float32 and r["track_delta"].tobytes() == u["D"].tobytes(), k
        assert (r["track_scale"], r["track_count"], r["track_status"], r["track_rms"]) == (u["scale"], u["count"], u["status"], u["rms"]), k
        assert r["world_to_camera"].tobytes() == w["C"].tobytes(), k
        if mode == "render":
            for name, m in zip(("model_depth", "model_normal", "model_picture"), w["model"]):
                assert r[name].tobytes() == m.tobytes(), (k, name)
    assert any(r["track_status"] == AL.OK and r["track_count"] >= TRACK_KW["min_count"] for r in recs[1:])          # the tracker did run
    assert any(r["track_delta"].tobytes() != np.eye(4, dtype=np.float32).tobytes() for r in recs[1:])
    for g, w, what in zip(got, vol, ("tsdf", "weight", "rgba")):
        assert g.tobytes() == w.tobytes(), what


def test_eager_and_graph_agree(setup):
    for mode in MODES:
        (ra, va), (rb, vb) = setup[f"{mode}_eager"], setup[f"{mode}_graph"]
        assert [r["index"] for r in ra] == [r["index"] for r in rb]
        for a, b in zip(ra, rb):
            assert set(a) == set(b)
            for k in a:
                assert (a[k].tobytes() == b[k].tobytes()) if isinstance(a[k], np.ndarray) else a[k] == b[k], (mode, k)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(va, vb)), mode


def test_track_none_is_the_stream_that_never_heard_of_it(setup):
    pp, VOL, frames = setup["graph"], setup["vol"], setup["frames"]
    for kw in (dict(present=False), dict(temporal=TEMPORAL)):
        va, vb = new_volume(VOL), new_volume(VOL)
        plain = collect(pp, frames, volume=va, **kw)
        keys = {k for s in pp._slots.values() for k in s.graphs}
        none = collect(pp, frames, volume=vb, track=None, **kw)
        new = {k for s in pp._slots.values() for k in s.graphs} - keys                        # vb is another volume: a graph of its own, of the same kind
        assert not any(isinstance(e, tuple) and e and e[0] == "track" for k in new for e in k)
        assert len(plain) == len(none)
        for a, b in zip(plain, none):
            assert set(a) == set(b) and not any(k.startswith("track_") for k in b)
            for k in a:
                assert (a[k].tobytes() == b[k].tobytes()) if isinstance(a[k], np.ndarray) else a[k] == b[k], k
        assert all(x.tobytes() == y.tobytes() for x, y in zip(volume_bytes(va), volume_bytes(vb)))
    tracked = [k for s in pp._slots.values() for k in s.graphs if any(isinstance(e, tuple) and e and e[0] == "track" for e in k)]
    assert tracked and all(k[-1][1] == SCHEDULE for k in tracked)


def test_arguments_are_refused(setup):
    pp, VOL, frames = setup["graph"], setup["vol"], setup["frames"]
    v = new_volume(VOL)
    for bad, match in ((dict(track=dict()), "needs volume"), (dict(volume=v, track=dict(iterations=3)), "keys"), (dict(volume=v, track=[1, 2]), "keys"),
                       (dict(volume=v, track=dict(schedule=(4,))), "mode"), (dict(volume=v, track=dict(schedule=())), "at least one"),
                       (dict(volume=v, track=dict(schedule=(2,), scale=False)), "at least one"), (dict(volume=v, track=dict(dist_tol=0.0)), "dist_tol"),
                       (dict(volume=v, track=dict(min_count=3)), "min_count")):
        with pytest.raises(ValueError, match=match):
            next(pp.stream(iter(frames), K_SRC, **bad))
    with pytest.raises(ValueError, match="stateless"):
        pp.predict([frames[1], frames[0], frames[2]][:1 + pp.n], K_SRC, track=dict())
    from simpledepthestimation_amd.engine.predictor import track_arg
    from simpledepthestimation_amd.hip import align as AL
    assert track_arg(None, v) is None
    rng = dict(near=0.0, far=1.0, step=0.1)                                               # (this volume's own depth range is a million units)
    assert track_arg(dict(rng, scale=False), v)[0] == (AL.POSE,) * len(AL.DEFAULT_SCHEDULE) and track_arg(rng, v)[0] == AL.DEFAULT_SCHEDULE
    assert track_arg(dict(rng, schedule=(2, 3, 1), scale=False), v)[0] == (AL.POSE, AL.POSE)
    with pytest.raises(ValueError, match="samples"):
        track_arg(dict(), v)


def test_demo_tool_track_volume(tmp_path):
    """The tool end to end with --pairs --volume --track-volume --save-trajectory on five generated frames: volume.ply and trajectory.txt are
    what the tracked stream gives."""
    import yaml
    from PIL import Image
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.engine.predictor import PairPredictor
    from simpledepthestimation_amd.geometry.pose_utils import invert_pose_np
    from simpledepthestimation_amd.hip.volume import TsdfVolume
    from simpledepthestimation_amd.tools import demo
    src, dst = tmp_path / "frames", tmp_path / "out"
    src.mkdir()
    frames = sequence(5, seed=8)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(src / f"f{i:02d}.png")
    # the tool renders over the model's depth range in steps of a voxel: a range the march covers in a few hundred samples
    conf = {"MODEL": {"META_ARCHITECTURE": "MonoDepth2Model", "DEVICE": DEV, "POSE_NET": {"NAME": "PoseNet", "NUM_CONTEXTS": 2}},
            "DATASETS": {"TEST": {"PREPROCESS": [{"NAME": "LoadImg"}, {"NAME": "Resize", "IMG_H": NET_H, "IMG_W": NET_W}, {"NAME": "ToTensor"}]}}}
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(conf))
    cfg = get_cfg()
    cfg.set_new_allowed(True)
    cfg.merge_from_file(str(tmp_path / "config.yaml"))
    torch.manual_seed(7)
    pp = PairPredictor(cfg)
    p = volume_params(pp, frames)
    voxel = max(p["voxel"], float(cfg.MODEL.MAX_DEPTH) / 4096)                             # at most 4096 samples along a ray
    k = [str(v) for v in (K_SRC[0, 0], K_SRC[1, 1], K_SRC[0, 2], K_SRC[1, 2])]
    common = ["--cfg", str(tmp_path / "config.yaml"), "--input", str(src), "--output", str(dst), "--pairs", "--intrinsics"] + k
    vol_args = ["--volume"] + [str(n) for n in DIMS] + ["--voxel", repr(voxel), "--volume-origin"] + [repr(float(o)) for o in p["origin"]]
    for bad in (["--track-volume"], vol_args + ["--no-track-scale"]):
        with pytest.raises(SystemExit):
            demo.main(common + bad)
    torch.manual_seed(7)
    assert demo.main(common + vol_args + ["--track-volume", "--save-trajectory"]) == 0
    assert sorted(q.name for q in dst.iterdir()) == sorted([f"f{i:02d}.png" for i in range(1, 4)] + ["volume.ply", "trajectory.txt"])
    v = TsdfVolume(DIMS, voxel, origin=p["origin"], min_depth=float(cfg.MODEL.get("MIN_DEPTH", 0.0)), max_depth=float(cfg.MODEL.MAX_DEPTH), device=DEV)
    recs = collect(pp, frames, volume=v, track=dict(scale=True, min_weight=1.0))
    assert len(recs) == 3
    v.save_ply(str(tmp_path / "want.ply"), min_weight=1)
    assert (dst / "volume.ply").read_bytes() == (tmp_path / "want.ply").read_bytes()
    lines = (dst / "trajectory.txt").read_text().splitlines()
    assert len(lines) == 3
    for line, r in zip(lines, recs):
        W = invert_pose_np(r["world_to_camera"].astype(np.float64))
        assert [float(x) for x in line.split()] == [float(x) for x in W[:3].reshape(-1)]
    assert [float(x) for x in lines[0].split()] == [float(x) for x in np.eye(4)[:3].reshape(-1)]       # the first target is the world

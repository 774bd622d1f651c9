"""GPU: PairPredictor.stream(..., volume=vol) on the tiny random-weight models of test_gpu_temporal_stream.py (ResNet-18, network size 64 x 96,
six 80 x 120 frames): the pose chained on the device and the volume it fills are recomputed on the host with compose_host / integrate_host from
what the stream itself yielded, bit for bit: that pins the direction of the pose, the depth that goes in and the size the intrinsics are taken at."""
import numpy as np
import pytest
import torch

from test_gpu_temporal_stream import DEV, HS, K_SRC, NET_H, NET_W, TEMPORAL, WS, collect, pair_cfg, sequence

pytestmark = pytest.mark.gpu
DIMS = (24, 20, 16)


def volume_params(pp, frames):
    """A volume around what this model sees: a random-weight network's depth has no scale one could know beforehand, so the median m of the
    first window's prediction sets it -- voxels of m / 6, the near face at m / 4, four units of m wide.  Everything else is fixed."""
    m = float(np.median(next(iter(pp.stream(iter(frames), K_SRC, present=False)))["depth_net"]))
    assert np.isfinite(m) and m > 0
    voxel = float(np.float32(m / 6))
    return dict(dims=DIMS, voxel=voxel, origin=(-DIMS[0] * voxel / 2 + 0.013 * m, -DIMS[1] * voxel / 2 - 0.007 * m, m / 4), trunc=4 * voxel, max_weight=3.0,
                min_depth=0.0, max_depth=1e6)


def new_volume(params):
    from simpledepthestimation_amd.hip.volume import TsdfVolume
    return TsdfVolume(device=DEV, **params)


def volume_bytes(v):
    torch.cuda.synchronize()
    return v.tsdf.cpu().numpy(), v.weight.cpu().numpy(), v.rgba.cpu().numpy()


def stream_into(pp, frames, params, **kw):
    v = new_volume(params)
    recs = collect(pp, frames, volume=v, **kw)
    return recs, volume_bytes(v)


@pytest.fixture(scope="module", params=["MonoDepth2Model", "MotionLearningModel"])
def setup(request):
    """One model per family, an eager and a graph predictor on it, and the volume stream of both, plain and temporal: computed once, shared,
    never modified."""
    from simpledepthestimation_amd.engine.predictor import PairPredictor
    from simpledepthestimation_amd.modeling import build_model
    cfg = pair_cfg(request.param)
    torch.manual_seed(21)
    model = build_model(cfg).eval()
    frames = sequence(6)
    eager, graph = PairPredictor(cfg, model=model, use_graph=False), PairPredictor(cfg, model=model, use_graph=True)
    out = {"arch": request.param, "frames": frames, "eager": eager, "graph": graph, "vol": volume_params(graph, frames)}
    for route, pp in (("eager", eager), ("graph", graph)):
        for mode, kw in MODES.items():
            out[f"{mode}_{route}"] = stream_into(pp, frames, out["vol"], **kw)
    return out


# both modes yield `depth_net`, the depth that goes into the volume: the raw prediction without the pictures, the fused map with temporal
MODES = {"plain": dict(present=False), "temporal": dict(temporal=TEMPORAL)}


def host_replay(pp, recs, frames, VOL):
    """The pose chain and the volume recomputed on the host from the yielded records."""
    from simpledepthestimation_amd.hip.volume import compose_host, integrate_host
    import volume_ref as VR
    plan = pp.plan(HS, WS)
    ymap, xmap = plan.maps((NET_H, NET_W))
    tsdf, weight, rgba = VR.fresh(VOL["dims"])
    j = pp.offsets.index(1)
    C = np.eye(4, dtype=np.float32)
    poses = []
    for k, r in enumerate(recs):
        if k:
            C = compose_host(recs[k - 1]["pose"][j], C)
        poses.append(C)
        integrate_host(tsdf, weight, rgba, r["depth_net"], np.asarray(ymap), np.asarray(xmap), K_SRC, C, frames[r["index"]], VOL["origin"], VOL["voxel"],
                       VOL["trunc"], VOL["max_weight"], VOL["min_depth"], VOL["max_depth"])
    return poses, (tsdf, weight, rgba)


@pytest.mark.parametrize("route", ["eager", "graph"])
@pytest.mark.parametrize("mode", ["plain", "temporal"])
def test_pose_chain_and_volume_are_the_host_twins_of_what_was_yielded(setup, route, mode):
    recs, got = setup[f"{mode}_{route}"]
    pp, VOL = setup[route], setup["vol"]
    poses, want = host_replay(pp, recs, setup["frames"], VOL)
    assert recs[0]["world_to_camera"].tobytes() == np.eye(4, dtype=np.float32).tobytes()
    for k, (r, C) in enumerate(zip(recs, poses)):
        assert r["world_to_camera"].dtype == np.float32 and r["world_to_camera"].tobytes() == C.tobytes(), k
    assert not np.array_equal(recs[-1]["world_to_camera"], recs[1]["world_to_camera"])
    touched = int((got[1] > 0).sum())
    print(f"{setup['arch']} {mode} {route}: {touched} of {got[1].size} voxels touched, largest weight {float(got[1].max())}, "
          f"{int((want[0] != got[0]).sum())} tsdf values differ from the host replay")
    assert touched > 100 and float(got[1].max()) >= 2                           # the frames overlap in the volume
    for g, w, what in zip(got, want, ("tsdf", "weight", "rgba")):
        assert g.tobytes() == w.tobytes(), what
    assert bool(got[2][got[1] > 0][:, 3].max() == 255)


def test_yields_without_volume_are_unchanged(setup):
    pp = setup["graph"]
    VOL = setup["vol"]
    for mode, kw in MODES.items():
        none = collect(pp, setup["frames"], volume=None, **kw)
        recs, _ = setup[f"{mode}_graph"]
        assert len(none) == len(recs)
        for a, b in zip(none, recs):
            assert set(a) <= set(b) and set(b) - set(a) == {"world_to_camera"}
            for k in a:
                assert (a[k].tobytes() == b[k].tobytes()) if isinstance(a[k], np.ndarray) else a[k] == b[k], (mode, k)
    keys = [k for s in pp._slots.values() for k in s.graphs]
    with_volume = [k for k in keys if any(isinstance(e, tuple) and e and e[0] == "volume" for e in k)]
    assert with_volume and any(len(k) == 4 for k in keys)                       # volume=None replays the graph of the key it always had
    assert all(k[-1][1:4] == (VOL["dims"], float(np.float32(VOL["voxel"])), tuple(float(np.float32(o)) for o in VOL["origin"])) for k in with_volume)


def test_eager_and_graph_agree_and_a_second_stream_repeats(setup):
    for mode in ("plain", "temporal"):
        (ra, va), (rb, vb) = setup[f"{mode}_eager"], setup[f"{mode}_graph"]
        assert [r["index"] for r in ra] == [r["index"] for r in rb]
        assert all(a["world_to_camera"].tobytes() == b["world_to_camera"].tobytes() for a, b in zip(ra, rb))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(va, vb)), mode
    again, vol = stream_into(setup["graph"], setup["frames"], setup["vol"], temporal=TEMPORAL)          # a fresh volume, the same frames: the same bytes
    assert all(x.tobytes() == y.tobytes() for x, y in zip(vol, setup["temporal_graph"][1]))
    assert again[0]["world_to_camera"].tobytes() == np.eye(4, dtype=np.float32).tobytes()


def test_the_volume_is_the_callers(setup):
    """A second sequence into the SAME volume restarts the pose at the identity and keeps what the volume holds; predict refuses a volume."""
    pp = setup["graph"]
    v = new_volume(setup["vol"])
    first = collect(pp, setup["frames"], volume=v, present=False)
    once = volume_bytes(v)
    second = collect(pp, setup["frames"], volume=v, present=False)
    twice = volume_bytes(v)
    assert second[0]["world_to_camera"].tobytes() == np.eye(4, dtype=np.float32).tobytes()
    assert all(a["world_to_camera"].tobytes() == b["world_to_camera"].tobytes() for a, b in zip(first, second))
    assert once[0].tobytes() == setup["plain_graph"][1][0].tobytes()
    assert bool(np.all(twice[1] >= once[1])) and bool(np.any(twice[1] > once[1]))           # the second sequence went on top of the first
    with pytest.raises(ValueError, match="stateless"):
        pp.predict([setup["frames"][1], setup["frames"][0], setup["frames"][2]][:1 + pp.n], K_SRC, volume=v)
    with pytest.raises(ValueError, match="TsdfVolume"):
        next(pp.stream(iter(setup["frames"]), K_SRC, volume=dict(setup["vol"])))


def test_model_that_only_looks_back_steps_with_the_inverted_pose():
    """PoseNet with one context at -1: the step previous -> current is the inverse of the current window's pose, formed on the device term by
    term; the first window is the world and takes no step."""
    from simpledepthestimation_amd.engine.predictor import PairPredictor
    from simpledepthestimation_amd.hip.volume import compose_host
    from simpledepthestimation_amd.modeling import build_model
    cfg = pair_cfg("MonoDepth2Model")
    cfg.merge_from_other_cfg({"MODEL": {"POSE_NET": {"NUM_CONTEXTS": 1}}, "DATASETS": {"TRAIN": {"BACKWARD_CONTEXT": 1, "FORWARD_CONTEXT": 0, "STRIDE": 1}}})
    torch.manual_seed(23)
    model = build_model(cfg).eval()
    frames = sequence(5, seed=4)
    volumes = []
    for use_graph in (False, True):
        pp = PairPredictor(cfg, model=model, use_graph=use_graph)
        recs, vol = stream_into(pp, frames, volume_params(pp, frames))
        C = np.eye(4, dtype=np.float32)
        for k, r in enumerate(recs):
            if k:
                R, t = r["pose"][0, :3, :3], r["pose"][0, :3, 3]
                T = np.eye(4, dtype=np.float32)
                T[:3, :3] = R.T
                T[:3, 3] = -(R.T[:, 0] * t[0] + R.T[:, 1] * t[1] + R.T[:, 2] * t[2])
                C = compose_host(T, C)
            assert r["world_to_camera"].tobytes() == C.tobytes(), (use_graph, k)
        volumes.append(vol)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(*volumes))


def test_demo_tool_volume(tmp_path):
    """The tool end to end with --pairs --volume on six generated frames: volume.ply is what the volume stream and save_ply give."""
    import yaml
    from PIL import Image
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.engine.predictor import PairPredictor
    from simpledepthestimation_amd.hip.cloud import RECORD
    from simpledepthestimation_amd.hip.volume import TsdfVolume
    from simpledepthestimation_amd.tools import demo
    src, dst = tmp_path / "frames", tmp_path / "out"
    src.mkdir()
    frames = sequence(6, seed=8)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(src / f"f{i:02d}.png")
    conf = {"MODEL": {"META_ARCHITECTURE": "MonoDepth2Model", "DEVICE": DEV, "POSE_NET": {"NAME": "PoseNet", "NUM_CONTEXTS": 2}},
            "DATASETS": {"TEST": {"PREPROCESS": [{"NAME": "LoadImg"}, {"NAME": "Resize", "IMG_H": NET_H, "IMG_W": NET_W}, {"NAME": "ToTensor"}]}}}
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(conf))
    cfg = get_cfg()
    cfg.set_new_allowed(True)
    cfg.merge_from_file(str(tmp_path / "config.yaml"))
    torch.manual_seed(7)
    pp = PairPredictor(cfg)
    p = volume_params(pp, frames)
    k = [str(v) for v in (K_SRC[0, 0], K_SRC[1, 1], K_SRC[0, 2], K_SRC[1, 2])]
    torch.manual_seed(7)
    assert demo.main(["--cfg", str(tmp_path / "config.yaml"), "--input", str(src), "--output", str(dst), "--pairs", "--intrinsics"] + k +
                     ["--volume"] + [str(n) for n in DIMS] + ["--voxel", repr(p["voxel"]), "--volume-origin"] + [repr(float(o)) for o in p["origin"]] +
                     ["--min-weight", "2"]) == 0
    assert sorted(q.name for q in dst.iterdir()) == sorted([f"f{i:02d}.png" for i in range(1, 5)] + ["volume.ply"])
    v = TsdfVolume(DIMS, p["voxel"], origin=p["origin"], min_depth=float(cfg.MODEL.get("MIN_DEPTH", 0.0)), max_depth=float(cfg.MODEL.MAX_DEPTH), device=DEV)
    assert len(list(pp.stream(iter(frames), K_SRC, volume=v))) == 4
    written, found = v.save_ply(str(tmp_path / "want.ply"), min_weight=2)
    raw = (dst / "volume.ply").read_bytes()
    assert written == found > 0 and raw == (tmp_path / "want.ply").read_bytes()
    head = demo.ply_header(found)
    assert raw.startswith(head) and len(raw) == len(head) + found * RECORD.itemsize

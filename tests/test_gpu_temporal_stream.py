"""GPU: PairPredictor.stream(..., temporal=...) on tiny random-weight models (ResNet-18, network size 64 x 96, six 80 x 120 frames): one
MonoDepth2 (PoseNet, contexts at -1 and +1) and one MotionLearning (GoogleResNet + GoogleMotionNet, context at +1).  The fused map of every
window is recomputed on the host with warp_fuse_host from what the stream itself yielded, bit for bit: that pins the direction of the pose, the
grid of the motion field and the size the intrinsics are taken at."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HS, WS, NET_H, NET_W = 80, 120, 64, 96
STEPS = [{"NAME": "Resize", "IMG_H": NET_H, "IMG_W": NET_W}]
K_SRC = np.array([[70.0, 0, 60.3], [0, 68.0, 39.6], [0, 0, 1]], dtype=np.float32)
TEMPORAL = dict(alpha=0.5, tol=0.05)
MOTION_LOSS = {"NUM_SCALES": 1, "SSIM_WEIGHT": 3.0, "C1": "inf", "C2": 9e-6, "DEPTH_L1_WEIGHT": 0.0, "MOTION_SMOOTHNESS_WEIGHT": 1.0, "MOTION_SPARSITY_WEIGHT": 0.2,
               "ROT_CYCLE_WEIGHT": 1e-3, "TRANS_CYCLE_WEIGHT": 5e-2, "SCALE_NORMALIZE": False}


def sequence(n, seed=3):
    """n frames of one scene drifting sideways: smooth enough for the networks, different from frame to frame."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (HS // 8 + 2, WS // 8 + n + 2, 3)).astype(np.float32)
    big = np.kron(base, np.ones((8, 8, 1), np.float32))
    return [np.clip(big[4:4 + HS, 4 + 3 * i:4 + 3 * i + WS] + rng.normal(0, 4, (HS, WS, 3)), 0, 255).astype(np.uint8) for i in range(n)]


def pair_cfg(arch):
    from simpledepthestimation_amd.config import get_cfg
    cfg = get_cfg()
    cfg.set_new_allowed(True)
    if arch == "MonoDepth2Model":
        cfg.merge_from_other_cfg({"MODEL": {"META_ARCHITECTURE": arch, "POSE_NET": {"NAME": "PoseNet", "NUM_CONTEXTS": 2}}})
    else:
        cfg.merge_from_other_cfg({"MODEL": {"META_ARCHITECTURE": arch, "DEPTH_NET": {"NAME": "GoogleResNet", "NORM": "randLN"},
                                            "POSE_NET": {"NAME": "GoogleMotionNet", "USE_DEPTH": True, "SCALE_CONSTRAIN": "clip_ste"}}, "LOSS": MOTION_LOSS})
    cfg.MODEL.DEPTH_NET.ENCODER_NAME, cfg.MODEL.DEVICE, cfg.MODEL.COMPUTE_DTYPE = "18", DEV, "fp32"
    cfg.merge_from_other_cfg({"DATASETS": {"TEST": {"PREPROCESS": [{"NAME": "LoadImg"}] + STEPS + [{"NAME": "ToTensor"}]}}})
    return cfg


def collect(pp, frames, **kw):
    """The records of one stream call, copied out of the pinned buffers."""
    return [{k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in res.items()} for res in pp.stream(iter(frames), K_SRC, **kw)]


@pytest.fixture(scope="module", params=["MonoDepth2Model", "MotionLearningModel"])
def setup(request):
    """One model per family, an eager and a graph predictor on it, and the temporal stream of both: computed once, shared, never modified."""
    from simpledepthestimation_amd.engine.predictor import PairPredictor
    from simpledepthestimation_amd.modeling import build_model
    cfg = pair_cfg(request.param)
    torch.manual_seed(21)
    model = build_model(cfg).eval()
    frames = sequence(6)
    eager, graph = PairPredictor(cfg, model=model, use_graph=False), PairPredictor(cfg, model=model, use_graph=True)
    return {"arch": request.param, "frames": frames, "eager": eager, "graph": graph, "rec_eager": collect(eager, frames, temporal=TEMPORAL),
            "rec_graph": collect(graph, frames, temporal=TEMPORAL)}


def host_fusion(pp, recs, with_motion):
    """The fused maps recomputed on the host from the yielded records: window k from the fused map of k - 1, the raw prediction of k, and the
    pose (and motion field) window k - 1 yielded for its context at +1."""
    from simpledepthestimation_amd.hip.temporal import warp_fuse_host
    j = pp.offsets.index(1)
    K_net = np.asarray(pp.plan(HS, WS).intrinsics(K_SRC), dtype=np.float32)
    out = []
    for k in range(1, len(recs)):
        motion = recs[k - 1]["motion"][:1] if with_motion else None
        out.append(warp_fuse_host(recs[k - 1]["depth_net"][None], recs[k]["depth_net_raw"][None], K_net, recs[k - 1]["pose"][j][None], motion, **TEMPORAL))
    return out


def test_first_window_is_the_raw_prediction(setup):
    for recs in (setup["rec_eager"], setup["rec_graph"]):
        first = recs[0]
        assert first["depth_net"].shape == (NET_H, NET_W) and first["temporal_state"].dtype == np.uint8 and first["temporal_state"].shape == (NET_H, NET_W)
        assert first["depth_net"].tobytes() == first["depth_net_raw"].tobytes() and not first["temporal_state"].any()


def test_graph_replay_equals_eager(setup):
    """The eager run before each slot's capture must not advance the state: with it, windows 0 and 1 of the graph route would be fused twice."""
    a, b = setup["rec_eager"], setup["rec_graph"]
    n = 4 if setup["arch"] == "MonoDepth2Model" else 5
    assert [r["index"] for r in a] == [r["index"] for r in b] and len(a) == n
    for ra, rb in zip(a, b):
        assert sorted(ra) == sorted(rb)
        for k in ("depth_net", "temporal_state", "depth_net_raw", "depth", "canvas"):
            assert ra[k].tobytes() == rb[k].tobytes(), (ra["index"], k)


@pytest.mark.parametrize("route", ["rec_eager", "rec_graph"])
def test_every_window_is_the_host_twin_of_what_was_yielded(setup, route):
    recs = setup[route]
    pp = setup["graph"]
    with_motion = setup["arch"] == "MotionLearningModel"
    assert ("motion" in recs[0]) == with_motion
    want = host_fusion(pp, recs, with_motion)
    for k, (fused, state, _) in enumerate(want, start=1):
        counts = np.bincount(state.ravel() & 3, minlength=4).tolist()
        print(f"{setup['arch']} {route} window {k}: classes {counts}, filled {int((state & 4).astype(bool).sum())}")
        assert recs[k]["depth_net"].tobytes() == fused[0].tobytes(), k
        assert recs[k]["temporal_state"].tobytes() == state[0].tobytes(), k
        assert counts[1] > 0                                                 # something was fused: the state did carry over
    # the fused map is what the pictures show: DepthPredictor's present kernel on it
    from simpledepthestimation_amd.hip.present import depth_present
    ymap, xmap = pp._maps_on_device(pp.plan(HS, WS), (NET_H, NET_W))
    last = recs[-1]
    frame = torch.from_numpy(setup["frames"][last["index"]])[None].to(DEV)
    canvas, depth, _ = depth_present(torch.from_numpy(last["depth_net"])[None].to(DEV), ymap, xmap, pp.vmax, pp.gamma, frame=frame, want_depth=True, want_u16=False)
    assert np.array_equal(depth[0].cpu().numpy(), last["depth"]) and np.array_equal(canvas[0].cpu().numpy(), last["canvas"])
    assert not np.array_equal(last["depth_net"], last["depth_net_raw"])


def test_without_temporal_nothing_changes(setup):
    pp = setup["graph"]
    plain = collect(pp, setup["frames"])
    none = collect(pp, setup["frames"], temporal=None)
    assert len(plain) == len(none) == len(setup["rec_graph"])
    for a, b, t in zip(plain, none, setup["rec_graph"]):
        assert sorted(a) == sorted(b) and "depth_net" not in a and "temporal_state" not in a and "depth_net_raw" not in a
        for k in a:
            assert (a[k].tobytes() == b[k].tobytes()) if isinstance(a[k], np.ndarray) else a[k] == b[k], k
        # pose, flow and motion of the temporal stream are the plain stream's: they read the raw prediction
        for k in ("pose", "flow", "flow_valid", "flow_canvas", "pose_next") + (("motion",) if "motion" in a else ()):
            assert a[k].tobytes() == t[k].tobytes(), k
    keys = [k for s in pp._slots.values() for k in s.graphs]
    assert any(len(k) == 4 for k in keys) and any(len(k) == 5 and k[4] == (0.5, float(np.float32(0.05))) for k in keys)
    with pytest.raises(ValueError, match="stateless"):
        pp.predict([setup["frames"][1], setup["frames"][0], setup["frames"][2]][:1 + pp.n], K_SRC, temporal=TEMPORAL)


def test_rigid_only_warps_without_the_motion_field(setup):
    pp = setup["graph"]
    recs = collect(pp, setup["frames"], temporal=TEMPORAL, rigid_only=True)
    want = host_fusion(pp, recs, with_motion=False)
    for k, (fused, state, _) in enumerate(want, start=1):
        assert recs[k]["depth_net"].tobytes() == fused[0].tobytes() and recs[k]["temporal_state"].tobytes() == state[0].tobytes(), k
    differs = any(r["depth_net"].tobytes() != m["depth_net"].tobytes() for r, m in zip(recs[1:], setup["rec_graph"][1:]))
    assert differs == (setup["arch"] == "MotionLearningModel")            # the motion field does enter where there is one; MonoDepth2's warp is rigid already


def test_second_stream_starts_from_an_empty_state(setup):
    again = collect(setup["graph"], setup["frames"], temporal=TEMPORAL)
    for a, b in zip(again, setup["rec_graph"]):
        assert a["depth_net"].tobytes() == b["depth_net"].tobytes() and a["temporal_state"].tobytes() == b["temporal_state"].tobytes()
    assert not again[0]["temporal_state"].any()
    other = collect(setup["graph"], setup["frames"][2:], temporal=dict(alpha=0.25, tol=0.05))          # other frames, another alpha: another graph key
    assert not other[0]["temporal_state"].any() and other[0]["depth_net"].tobytes() == other[0]["depth_net_raw"].tobytes()


def test_demo_tool_stabilise(tmp_path):
    """The tool end to end with --pairs --stabilise --save-state --save-depth --save-cloud on six generated frames: what it writes is what the
    temporal stream yields."""
    import yaml
    from PIL import Image
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.engine.predictor import PairPredictor
    from simpledepthestimation_amd.hip.cloud import RECORD, as_records
    from simpledepthestimation_amd.hip.temporal import STATE_COLOURS
    from simpledepthestimation_amd.tools import demo
    src, dst = tmp_path / "frames", tmp_path / "out"
    src.mkdir()
    frames = sequence(6, seed=8)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(src / f"f{i:02d}.png")
    conf = {"MODEL": {"META_ARCHITECTURE": "MonoDepth2Model", "DEVICE": DEV, "POSE_NET": {"NAME": "PoseNet", "NUM_CONTEXTS": 2}},
            "DATASETS": {"TEST": {"PREPROCESS": [{"NAME": "LoadImg"}] + STEPS + [{"NAME": "ToTensor"}]}}}
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(conf))
    k = [str(v) for v in (K_SRC[0, 0], K_SRC[1, 1], K_SRC[0, 2], K_SRC[1, 2])]
    torch.manual_seed(7)
    assert demo.main(["--cfg", str(tmp_path / "config.yaml"), "--input", str(src), "--output", str(dst), "--pairs", "--stabilise", "--stabilise-alpha", "0.25",
                      "--save-state", "--save-depth", "--save-cloud", "--intrinsics"] + k) == 0
    stems = [f"f{i:02d}" for i in range(1, 5)]
    assert sorted(p.name for p in dst.iterdir()) == sorted(s + e for s in stems for e in (".png", "_state.png", "_depth.png", ".ply"))
    cfg = get_cfg()
    cfg.set_new_allowed(True)
    cfg.merge_from_file(str(tmp_path / "config.yaml"))
    torch.manual_seed(7)
    pp = PairPredictor(cfg)
    cloud = dict(min_depth=float(cfg.MODEL.get("MIN_DEPTH", 0.0)), max_depth=float(cfg.MODEL.MAX_DEPTH), step=1)
    seen = 0
    for res in pp.stream(iter(frames), K_SRC, temporal=dict(alpha=0.25, tol=0.05), want_u16=True, cloud=cloud):
        stem = stems[res["index"] - 1]
        assert np.array_equal(np.asarray(Image.open(dst / (stem + ".png"))), res["canvas"])
        assert np.array_equal(np.asarray(Image.open(dst / (stem + "_state.png"))), STATE_COLOURS[res["temporal_state"] & 3])
        assert np.array_equal(np.asarray(Image.open(dst / (stem + "_depth.png"))), res["depth_u16"])
        rec = as_records(res["points"], res["count"])[0]
        raw = (dst / (stem + ".ply")).read_bytes()
        assert raw.startswith(demo.ply_header(rec.size)) and raw[len(demo.ply_header(rec.size)):] == rec.astype(RECORD).tobytes()
        seen += 1
    assert seen == 4
    with pytest.raises(SystemExit):
        demo.parse_args(["--cfg", "c.yaml", "--input", "frames", "--stabilise"])
    with pytest.raises(SystemExit):
        demo.parse_args(["--cfg", "c.yaml", "--input", "frames", "--pairs", "--intrinsics", "1", "2", "3", "4", "--save-state"])
    with pytest.raises(SystemExit):
        demo.parse_args(["--cfg", "c.yaml", "--input", "frames", "--pairs", "--intrinsics", "1", "2", "3", "4", "--stabilise", "--stabilise-alpha", "1.0"])


def test_model_that_only_looks_back_inverts_its_pose():
    """PoseNet with one context at -1: the step previous -> current is the inverse of the current window's pose, formed on the device term by
    term; the host repeats it in float32 and the fused maps agree bit for bit, eager and from the graph."""
    from simpledepthestimation_amd.engine.predictor import PairPredictor
    from simpledepthestimation_amd.hip.temporal import warp_fuse_host
    from simpledepthestimation_amd.modeling import build_model
    cfg = pair_cfg("MonoDepth2Model")
    cfg.merge_from_other_cfg({"MODEL": {"POSE_NET": {"NUM_CONTEXTS": 1}}, "DATASETS": {"TRAIN": {"BACKWARD_CONTEXT": 1, "FORWARD_CONTEXT": 0, "STRIDE": 1}}})
    torch.manual_seed(23)
    model = build_model(cfg).eval()
    frames = sequence(5, seed=4)
    routes = []
    for use_graph in (False, True):
        pp = PairPredictor(cfg, model=model, use_graph=use_graph)
        assert pp.offsets == (-1,) and pp.next_context == (0, True)
        recs = collect(pp, frames, temporal=TEMPORAL)
        assert [r["index"] for r in recs] == [1, 2, 3, 4] and not recs[0]["temporal_state"].any()
        K_net = np.asarray(pp.plan(HS, WS).intrinsics(K_SRC), dtype=np.float32)
        for k in range(1, len(recs)):
            R, t = recs[k]["pose"][0, :3, :3], recs[k]["pose"][0, :3, 3]
            T = np.eye(4, dtype=np.float32)
            T[:3, :3] = R.T
            T[:3, 3] = -(R.T[:, 0] * t[0] + R.T[:, 1] * t[1] + R.T[:, 2] * t[2])
            fused, state, _ = warp_fuse_host(recs[k - 1]["depth_net"][None], recs[k]["depth_net_raw"][None], K_net, T[None], None, **TEMPORAL)
            assert recs[k]["depth_net"].tobytes() == fused[0].tobytes() and recs[k]["temporal_state"].tobytes() == state[0].tobytes(), (use_graph, k)
            assert int(((state & 3) == 1).sum()) > 0
        routes.append(recs)
    for a, b in zip(*routes):
        assert a["depth_net"].tobytes() == b["depth_net"].tobytes()

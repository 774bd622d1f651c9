"""GPU: sde_pair_flow against the restatement of its definition (flow_ref.py), PairPredictor and the demo tool's --pairs mode.

Kernel, per case: the validity map equal outside the edge band of flow_ref.py (at most 1 % of the pixels); the flow within the per-element
bound wherever bit 0 is set -- first order in 2^-24 from the order of operations include/sde_hip.h documents, nothing measured from the kernel --
and exactly (0, 0) elsewhere; the colours within +-1 per channel outside the pixels the restatement places next to the wheel's wrap or to
radius 1 (at most 0.5 %); the frame on top bit for bit.  And every pixel of the flow and of both validity bits, bit for bit, against the host
twin of the camera the geometry kernels share (hip/twins.py: pinhole_project_np): the bound above would let a reordering pass, the twin does not."""
import functools

import numpy as np
import pytest
import torch

import flow_ref as FR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5
GUARD = 64


@functools.lru_cache(maxsize=None)
def reference(name):
    """Inputs, restatement and colours of one case: computed once, shared, never modified."""
    inp = FR.case_inputs(name)
    want = FR.restate(inp["pred"], inp["ymap"], inp["xmap"], inp["K"], inp["T"], inp["motion"])
    rgb, skip = FR.colours(want["flow"], want["bit0"], want["bound"], inp["max_flow"], FR.wheel())
    return inp, want, rgb, skip


def on_device(inp):
    return {k: (torch.from_numpy(v).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in inp.items()}


def guarded(shape, dtype):
    """A destination with guard bytes on both sides, everything filled with FILL: (the whole buffer, the destination view)."""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD:GUARD + nbytes].view(dtype).view(shape)


def run(inp, with_frame=True, want=(True, True, True)):
    """-> (flow, valid, canvas) host arrays (None when not asked for); the guards of every destination are checked."""
    from simpledepthestimation_amd.hip.flow import pair_flow
    d = on_device(inp)
    N, H, W = inp["pred"].shape[0], inp["ymap"].size, inp["xmap"].size
    rows = 2 * H if with_frame else H
    bufs = [guarded(s, t) for s, t in (((N, H, W, 2), torch.float32), ((N, H, W), torch.uint8), ((N, rows, W, 3), torch.uint8))]
    out = pair_flow(d["pred"], d["ymap"], d["xmap"], d["K"], d["T"], motion=d["motion"], max_flow=inp["max_flow"], frame=d["frame"] if with_frame else None,
                    want_flow=want[0], want_valid=want[1], want_canvas=want[2], out=tuple(b[1] if w else None for b, w in zip(bufs, want)))
    torch.cuda.synchronize()
    res = []
    for (buf, view), o, w in zip(bufs, out, want):
        raw = buf.cpu().numpy()
        assert bool((raw[:GUARD] == FILL).all() and (raw[-GUARD:] == FILL).all()), "bytes outside a destination were written"
        if w:
            assert o.data_ptr() == view.data_ptr()
            res.append(view.cpu().numpy())
        else:
            assert o is None and bool((raw == FILL).all()), "an output that was not asked for was written"
            res.append(None)
    return res


@pytest.mark.parametrize("name", FR.CASES)
def test_pair_flow(name):
    inp, want, rgb, skip = reference(name)
    flow, valid, canvas = run(inp)
    N, H, W = valid.shape
    edge = want["edge1"]
    print(f"{name}: {N} x {H} x {W}, valid counts {np.bincount(valid.ravel(), minlength=4).tolist()}, edge band {int(edge.sum())}, colour skips {int(skip.sum())}")
    assert float(edge.mean()) <= 0.01 and float(skip.mean()) <= 0.005
    assert np.array_equal(valid[~edge], want["valid"][~edge])
    b0 = (valid & 1).astype(bool)
    assert bool(np.all(flow[~b0] == 0.0))
    cmp = b0 & want["bit0"]
    err = np.abs(flow.astype(np.float64) - want["flow"])[cmp]
    ratio = err / want["bound"][cmp]
    print(f"  flow: {int(cmp.sum())} pixels, largest error {float(err.max()):.3e}, largest error / bound = {float(ratio.max()):.3f}")
    assert bool(np.all(err <= want["bound"][cmp]))
    frame_rows, colour_rows = canvas[:, :H], canvas[:, H:]
    assert np.array_equal(frame_rows, inp["frame"]), "the frame on top"
    cc = cmp & ~skip | (~b0 & ~want["bit0"])
    diff = np.abs(colour_rows.astype(np.int16) - rgb.astype(np.int16))[cc]
    print(f"  colours: {int(cc.sum())} pixels, largest difference {int(diff.max())}, differing bytes {int((diff > 0).sum())}")
    assert int(diff.max()) <= 1
    assert bool(np.all(colour_rows[~b0] == 0))
    if name == "maps_with_outside":
        assert bool(np.all(valid[:, 0] == 0) and np.all(valid[:, -1] == 0) and np.all(valid[:, :, :2] == 0) and np.all(valid[:, :, -1] == 0))
        assert bool(np.all(valid[:, 1:-1, 2:-1] & 1))
    if name == "ragged_tile":
        assert W % FR.TILE != 0 and W >= FR.TILE + 3 and (H * W) % 4 != 0
    if name == "per_pixel_motion":
        rigid = FR.restate(inp["pred"], inp["ymap"], inp["xmap"], inp["K"], inp["T"], None)
        assert float(np.abs(rigid["flow"] - want["flow"]).max()) > 100 * float(want["bound"].max())       # the motion does enter
    if name == "nan_zero_and_behind":
        assert bool(np.all(valid[1, 3:6] == 0) and np.all(valid[0, 3:6] & 1))
        for n, y, x in ((0, 0, 4), (1, 8, 2), (0, 7, 7), (1, 0, 0), (0, 9, 20), (1, 10, 1)):
            assert valid[n, y, x] == 0 and not flow[n, y, x].any()
    # the colours alone, without the frame
    _, _, alone = run(inp, with_frame=False, want=(False, False, True))
    assert np.array_equal(alone, colour_rows)


@functools.lru_cache(maxsize=None)
def twin(name):
    """The kernel's own fp32 arithmetic on the host (hip/twins.py: pinhole_project_np, the camera every geometry kernel shares) on the restored
    fp32 inputs of one case -> (flow [N,H,W,2] float32, valid [N,H,W] uint8), the bits sde_pair_flow must write."""
    from simpledepthestimation_amd.hip.twins import pinhole_project_np
    inp = FR.case_inputs(name)
    d, inside = FR.restore(inp["pred"], inp["ymap"], inp["xmap"])
    m = FR.restore(inp["motion"], inp["ymap"], inp["xmap"])[0] if inp["motion"] is not None else None
    N, H, W = d.shape
    f32 = np.float32
    fu, fv = np.arange(W, dtype=f32)[None, :], np.arange(H, dtype=f32)[:, None]
    flow, valid = np.zeros((N, H, W, 2), f32), np.zeros((N, H, W), np.uint8)
    with np.errstate(all="ignore"):
        for n in range(N):
            _, _, qz, X, Y = pinhole_project_np(d[n], inp["K"][n], inp["T"][n], m[n] if m is not None else None)
            b0 = inside & np.isfinite(d[n]) & (d[n] > 0) & (qz > 0) & np.isfinite(X) & np.isfinite(Y)
            b1 = b0 & (X >= 0) & (X < f32(W - 1)) & (Y >= 0) & (Y < f32(H - 1))
            flow[n, ..., 0], flow[n, ..., 1] = np.where(b0, X - fu, f32(0)), np.where(b0, Y - fv, f32(0))
            valid[n] = b0.astype(np.uint8) | (b1.astype(np.uint8) << 1)
    return flow, valid


@pytest.mark.parametrize("name", FR.CASES)
def test_pair_flow_equals_the_host_twin_bit_for_bit(name):
    """Every pixel, no edge band: the flow's bytes and both validity bits are those of the shared camera's fp32 operations in their order."""
    want_flow, want_valid = twin(name)
    flow, valid, _ = run(reference(name)[0], want=(True, True, False))
    differing = int((flow.view(np.uint32) != want_flow.view(np.uint32)).sum())
    print(f"{name}: {differing} of {flow.size} flow values and {int((valid != want_valid).sum())} of {valid.size} validity bytes differ from the host twin")
    assert np.array_equal(valid & 1, want_valid & 1), "bit 0"
    assert np.array_equal(valid & 2, want_valid & 2), "bit 1"
    assert flow.tobytes() == want_flow.tobytes()


def test_two_runs_give_equal_bytes_and_unrequested_outputs_stay_untouched():
    inp, _, _, _ = reference("per_pixel_motion")
    a = run(inp)
    b = run(inp)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, True, False)):
        got = run(inp, want=want)                                   # run() checks the sentinels of what was left out
        for g, full, w in zip(got, a, want):
            assert (g is not None) == w and (g is None or g.tobytes() == full.tobytes())


def test_refused_arguments_launch_nothing():
    """Every refusal returns SDE_ERR_ARG with a message and leaves the destinations as they were."""
    from simpledepthestimation_amd.hip import lib as L
    from simpledepthestimation_amd.hip.flow import flow_wheel, pair_flow
    inp, _, _, _ = reference("maps_with_outside")
    d = on_device(inp)
    wheel = flow_wheel(DEV)
    flow = torch.full((2, 9, 14, 2), -77.0, device=DEV)
    valid = torch.full((2, 9, 14), FILL, dtype=torch.uint8, device=DEV)
    canvas = torch.full((2, 9, 14, 3), FILL, dtype=torch.uint8, device=DEV)
    lib = L.lib()

    def call(**kw):
        a = dict(pred=L.ptr(d["pred"]), N=2, ph=6, pw=10, ymap=L.ptr(d["ymap"]), xmap=L.ptr(d["xmap"]), H=9, W=14, K=L.ptr(d["K"]), T=L.ptr(d["T"]), motion=None,
                 wheel=L.ptr(wheel), ncols=55, max_flow=2.0, frame=None, flow=L.ptr(flow), valid=L.ptr(valid), canvas=L.ptr(canvas))
        a.update(kw)
        return lib.sde_pair_flow(a["pred"], a["N"], a["ph"], a["pw"], a["ymap"], a["xmap"], a["H"], a["W"], a["K"], a["T"], a["motion"], a["wheel"], a["ncols"],
                                 a["max_flow"], a["frame"], a["flow"], a["valid"], a["canvas"], L.stream())
    for kw in (dict(N=0), dict(H=0), dict(W=-1), dict(ph=0), dict(pw=0), dict(max_flow=0.0), dict(max_flow=-1.0), dict(max_flow=float("nan")), dict(ncols=0),
               dict(ncols=-3), dict(ncols=257), dict(pred=None), dict(ymap=None), dict(xmap=None), dict(K=None), dict(T=None),
               dict(flow=None, valid=None, canvas=None), dict(wheel=None)):
        assert call(**kw) == -1, kw
        assert b"sde_pair_flow" in lib.sde_last_error(), kw
    torch.cuda.synchronize()
    assert bool((flow == -77.0).all() and (valid == FILL).all() and (canvas == FILL).all())
    assert call(wheel=None, canvas=None) == 0                              # no canvas: no wheel needed
    assert call() == 0                                                     # the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert not bool((valid == FILL).any()) and not bool((flow == -77.0).any())
    with pytest.raises(ValueError):
        pair_flow(d["pred"], d["ymap"], d["xmap"], d["K"], d["T"], max_flow=0.0)
    with pytest.raises(ValueError):
        pair_flow(d["pred"], d["ymap"], d["xmap"], d["K"], d["T"], want_flow=False, want_valid=False, want_canvas=False)
    with pytest.raises(L.SdeHipError):
        pair_flow(d["pred"], d["ymap"], d["xmap"], d["K"], d["T"][:, :3])


# ---- PairPredictor ---------------------------------------------------------------------------------------------------------------------------
HS, WS = 120, 200
STEPS = [{"NAME": "Resize", "IMG_H": 96, "IMG_W": 160}]
K_SRC = np.array([[116.0, 0, 100.3], [0, 114.0, 59.6], [0, 0, 1]], dtype=np.float32)
MAX_FLOW = 0.05 * WS                                      # the default: 5 % of the frame's width


def sequence(n, seed=3):
    """n frames of one scene drifting sideways: smooth enough for the networks, different from frame to frame."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (HS // 8 + 2, WS // 8 + n + 2, 3)).astype(np.float32)
    big = np.kron(base, np.ones((8, 8, 1), np.float32))
    return [np.clip(big[4:4 + HS, 4 + 3 * i:4 + 3 * i + WS] + rng.normal(0, 4, (HS, WS, 3)), 0, 255).astype(np.uint8) for i in range(n)]


def pair_cfg(arch, use_depth=True):
    from simpledepthestimation_amd.config import get_cfg
    cfg = get_cfg()
    cfg.set_new_allowed(True)
    if arch == "MonoDepth2Model":
        cfg.merge_from_other_cfg({"MODEL": {"META_ARCHITECTURE": arch, "POSE_NET": {"NAME": "PoseNet", "NUM_CONTEXTS": 2}}})
    else:
        cfg.merge_from_other_cfg({"MODEL": {"META_ARCHITECTURE": arch, "DEPTH_NET": {"NAME": "GoogleResNet", "NORM": "randLN"},
                                            "POSE_NET": {"NAME": "GoogleMotionNet", "USE_DEPTH": use_depth, "SCALE_CONSTRAIN": "clip_ste"}},
                                  "LOSS": {"NUM_SCALES": 1, "SSIM_WEIGHT": 3.0, "C1": "inf", "C2": 9e-6, "DEPTH_L1_WEIGHT": 0.0, "MOTION_SMOOTHNESS_WEIGHT": 1.0,
                                           "MOTION_SPARSITY_WEIGHT": 0.2, "ROT_CYCLE_WEIGHT": 1e-3, "TRANS_CYCLE_WEIGHT": 5e-2, "SCALE_NORMALIZE": False}})
    cfg.MODEL.DEPTH_NET.ENCODER_NAME, cfg.MODEL.DEVICE, cfg.MODEL.COMPUTE_DTYPE = "18", DEV, "fp32"
    cfg.merge_from_other_cfg({"DATASETS": {"TEST": {"PREPROCESS": [{"NAME": "LoadImg"}] + STEPS + [{"NAME": "ToTensor"}]}}})
    return cfg


def build(cfg, seed):
    from simpledepthestimation_amd.modeling import build_model
    torch.manual_seed(seed)
    return build_model(cfg).eval()


@pytest.fixture(scope="module")
def mono():
    from simpledepthestimation_amd.engine.predictor import PairPredictor
    cfg = pair_cfg("MonoDepth2Model")
    model = build(cfg, 11)
    return {"cfg": cfg, "model": model, "frames": sequence(6), "eager": PairPredictor(cfg, model=model, use_graph=False),
            "graph": PairPredictor(cfg, model=model, use_graph=True)}


def prepared(pp, frames):
    """The window as the predictor prepares it: [1+n,3,h,w] float32 on the device, and the size plan."""
    t = torch.from_numpy(np.stack(frames)).to(DEV)
    plan = pp.plan(HS, WS)
    img, _ = pp._aug.prep(t, pp._no_jitter(len(frames)), plan.h, plan.w, tabs=(plan.xtab, plan.ytab))
    return img, plan


def direct_flow(pp, plan, out, motion=None):
    from simpledepthestimation_amd.hip.flow import pair_flow
    n = out["pose"].shape[0]
    ymap, xmap = pp._maps_on_device(plan, out["depth_net"].shape[-2:])
    return pair_flow(out["depth_net"].expand(n, -1, -1), ymap, xmap, torch.from_numpy(K_SRC).to(DEV), out["pose"], motion=motion, max_flow=MAX_FLOW)


def same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def test_pair_predictor_monodepth2(mono):
    from simpledepthestimation_amd.engine.predictor import DepthPredictor
    window = [mono["frames"][1], mono["frames"][0], mono["frames"][2]]          # the target, then the contexts at -1 and +1
    pp = mono["eager"]
    assert pp.offsets == (-1, 1) and pp.n == 2 and pp.next_context == (1, False)
    e = pp.predict(window, K_SRC)
    assert sorted(e) == ["canvas", "depth", "depth_net", "flow", "flow_canvas", "flow_valid", "motion", "pose"] and e["motion"] is None
    assert tuple(e["pose"].shape) == (2, 4, 4) and tuple(e["flow"].shape) == (2, HS, WS, 2) and tuple(e["flow_valid"].shape) == (2, HS, WS)
    assert tuple(e["flow_canvas"].shape) == (2, HS, WS, 3) and tuple(e["depth"].shape) == (1, HS, WS) and tuple(e["canvas"].shape) == (1, 2 * HS, WS, 3)
    assert tuple(e["depth_net"].shape) == (1, 96, 160)
    # the pose network called directly on the same prepared input
    img, plan = prepared(pp, window)
    with torch.no_grad():
        direct = torch.cat(mono["model"].pose_net({"pose_net_input": torch.cat([img[0:1], img[1:2], img[2:3]], 1)})["pose_pred"], 0)
    assert torch.equal(e["pose"], direct)
    assert not torch.equal(e["pose"][0], e["pose"][1]) and not torch.equal(e["pose"][0], torch.eye(4, device=DEV))
    # the flow is the kernel's, from the predictor's own network output and poses
    flow, valid, canvas = direct_flow(pp, plan, e)
    assert torch.equal(e["flow"], flow) and torch.equal(e["flow_valid"], valid) and torch.equal(e["flow_canvas"], canvas)
    assert bool((e["flow_valid"] & 1).all()) and float(e["flow"].abs().max()) > 0
    print(f"  |flow| up to {float(e['flow'].abs().max()):.3f} px, pose translations {e['pose'][:, :3, 3].tolist()}")
    # eager and graph replay: the first call captures, the second only replays
    for _ in range(2):
        same(mono["graph"].predict(window, K_SRC), e)
    # the target's depth outputs are DepthPredictor's
    d = DepthPredictor(mono["cfg"], model=mono["model"], use_graph=False).predict(window[0], intrinsics=K_SRC)
    assert torch.equal(d["depth"], e["depth"]) and torch.equal(d["canvas"], e["canvas"]) and torch.equal(d["depth_net"], e["depth_net"])
    # present=False leaves the pictures out, a larger max_flow changes only the colours
    q = mono["graph"].predict(window, K_SRC, present=False)
    assert q["canvas"] is None and q["depth"] is None and q["flow_canvas"] is None and torch.equal(q["flow"], e["flow"])
    m = mono["graph"].predict(window, K_SRC, max_flow=4 * MAX_FLOW)
    assert torch.equal(m["flow"], e["flow"]) and not torch.equal(m["flow_canvas"], e["flow_canvas"])
    with pytest.raises(ValueError, match="context frame"):
        pp.predict(window[:2], K_SRC)
    with pytest.raises(ValueError, match="intrinsics"):
        pp.predict(window, None)


@pytest.mark.parametrize("use_depth", [True, False])
def test_pair_predictor_motion_learning(use_depth):
    from simpledepthestimation_amd.engine.predictor import PairPredictor
    cfg = pair_cfg("MotionLearningModel", use_depth)
    model = build(cfg, 12)
    pp = PairPredictor(cfg, model=model, use_graph=True)
    assert pp.offsets == (1,) and pp.next_context == (0, False)
    window = sequence(2, seed=5)
    o = pp.predict(window, K_SRC)
    assert tuple(o["pose"].shape) == (1, 4, 4) and tuple(o["motion"].shape) == (1, 3, 96, 160) and tuple(o["flow"].shape) == (1, HS, WS, 2)
    assert float(o["motion"].abs().max()) > 0
    # the pose network on the stacked both-directions input, of which the first half is target -> context
    img, plan = prepared(pp, window)
    with torch.no_grad():
        depth_all = model.run_depth_net({"img": img})["depth_pred"][0] if use_depth else None
        x = pp.pose_input(img, depth_all)
        assert tuple(x.shape) == (2, 8 if use_depth else 6, 96, 160)
        pb = model.pose_net({"pose_net_input": x})
    assert torch.equal(o["pose"], pb["pose_pred"][:1]) and torch.equal(o["motion"], pb["motion_pred"][:1])
    # the motion field enters the flow ...
    flow, valid, canvas = direct_flow(pp, plan, o, motion=o["motion"])
    assert torch.equal(o["flow"], flow) and torch.equal(o["flow_valid"], valid) and torch.equal(o["flow_canvas"], canvas)
    # ... unless rigid_only asks for the camera's share alone
    r = pp.predict(window, K_SRC, rigid_only=True)
    flow_r, valid_r, canvas_r = direct_flow(pp, plan, r, motion=None)
    assert torch.equal(r["flow"], flow_r) and torch.equal(r["flow_valid"], valid_r) and torch.equal(r["flow_canvas"], canvas_r)
    assert torch.equal(r["pose"], o["pose"]) and torch.equal(r["motion"], o["motion"]) and torch.equal(r["depth"], o["depth"])
    assert not torch.equal(r["flow"], o["flow"])
    same(pp.predict(window, K_SRC), o)


def test_stream_yields_the_records_of_predict(mono):
    frames = mono["frames"]
    want = {t: mono["eager"].predict([frames[t], frames[t - 1], frames[t + 1]], K_SRC) for t in range(1, 5)}
    seen = []
    for res in mono["graph"].stream(iter(frames), K_SRC):
        t = res["index"]
        seen.append(t)
        assert sorted(res) == ["canvas", "depth", "flow", "flow_canvas", "flow_valid", "index", "pose", "pose_next"]
        w = want[t]
        assert np.array_equal(res["depth"], w["depth"][0].cpu().numpy()) and np.array_equal(res["canvas"], w["canvas"][0].cpu().numpy())
        for k in ("pose", "flow", "flow_valid", "flow_canvas"):
            assert np.array_equal(res[k], w[k].cpu().numpy()), (t, k)
        assert np.array_equal(res["pose_next"], w["pose"][1].cpu().numpy())            # the context at +1, as it is
    assert seen == [1, 2, 3, 4]
    assert [r["index"] for r in mono["graph"].stream(iter(frames[:2]), K_SRC)] == []        # no full window
    rigid = list(mono["graph"].stream(iter(frames[:3]), K_SRC, present=False, rigid_only=True))
    assert len(rigid) == 1 and sorted(rigid[0]) == ["depth_net", "flow", "flow_valid", "index", "pose", "pose_next"]


def test_demo_tool_pairs(tmp_path):
    """The tool end to end with --pairs --save-flow --save-trajectory on six generated frames."""
    import yaml
    from PIL import Image
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.engine.predictor import PairPredictor
    from simpledepthestimation_amd.hip.flow import read_flo
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
    assert demo.main(["--cfg", str(tmp_path / "config.yaml"), "--input", str(src), "--output", str(dst), "--pairs", "--save-flow", "--save-trajectory",
                      "--intrinsics"] + k) == 0
    stems = [f"f{i:02d}" for i in range(1, 5)]
    assert sorted(p.name for p in dst.iterdir()) == sorted([s + e for s in stems for e in (".png", "_flow.png", ".flo")] + ["trajectory.txt"])
    cfg = get_cfg()
    cfg.set_new_allowed(True)
    cfg.merge_from_file(str(tmp_path / "config.yaml"))
    torch.manual_seed(7)
    pp = PairPredictor(cfg)
    Kf = np.array([[float(k[0]), 0, float(k[2])], [0, float(k[1]), float(k[3])], [0, 0, 1]], dtype=np.float32)
    steps = []
    for res in pp.stream(iter(frames), Kf):
        stem = stems[res["index"] - 1]
        assert np.array_equal(read_flo(str(dst / (stem + ".flo"))), res["flow"][1])
        assert np.array_equal(np.asarray(Image.open(dst / (stem + "_flow.png"))), res["flow_canvas"][1])
        assert np.array_equal(np.asarray(Image.open(dst / (stem + ".png"))), res["canvas"])
        steps.append((res["pose"].copy(), res["pose_next"]))
    traj = np.loadtxt(str(dst / "trajectory.txt"))
    assert traj.shape == (6, 12)                                                       # one line per frame
    assert np.array_equal(traj[0], np.eye(4)[:3].reshape(-1))
    from simpledepthestimation_amd.geometry.pose_utils import accumulate_poses, invert_pose_np
    rel = [invert_pose_np(steps[0][0][0])] + [s[1] for s in steps]                     # the step into frame 1, then frame -> next frame
    assert np.array_equal(traj, accumulate_poses(np.stack(rel))[:, :3].reshape(6, 12))

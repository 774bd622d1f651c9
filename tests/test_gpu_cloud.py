"""GPU: sde_depth_cloud and sde_img_to_points against the restatement of their definitions (cloud_ref.py), and the predictor's cloud option.

Compacted cloud, per case: count, order, colours and z exact; x and y within the per-element bound of cloud_ref.py -- 2^-24 * k * |d| *
(|Kinv00 u| + |Kinv02|) with k = K_BOUND = 5, the number of float32 roundings in the evaluation order include/sde_hip.h documents (1 / fx, * u,
cx / fx, +, * d).  The order is checked against the (u, v) the restatement keeps, never against what the kernel wrote.
The x, y, z bytes of every record are also compared with the host twin of the camera the geometry kernels share (hip/twins.py:
pinhole_project_np): the bound would let a reordering pass, the twin does not.

Dense mode: forward and the four gradients against the float64 restatement, relative to the maximum, within 4 x the restatement's own
float32-vs-float64 deviation on the same inputs (printed), floor 2e-5: the rule of tests/test_gpu_bts_densenet.py."""
import functools

import numpy as np
import pytest
import torch

import cloud_ref as CR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64            # guard bytes in front of and behind the points: a multiple of 16, the records need that alignment
FILL = 0xA5
FLOOR = 2e-5


@functools.lru_cache(maxsize=None)
def reference(name):
    """Inputs and restatement of one case: computed once, shared, never modified."""
    inp = CR.case_inputs(name)
    return inp, CR.cloud(inp["pred"], inp["ymap"], inp["xmap"], inp["K"], inp["min_depth"], inp["max_depth"], inp["step"], inp["frame"])


def run_cloud(inp, workspace=None):
    from simpledepthestimation_amd.hip.cloud import as_records, depth_cloud
    N, H, W = inp["pred"].shape[0], inp["ymap"].size, inp["xmap"].size
    cap = CR.capacity(H, W, inp["step"])
    buf = torch.full((GUARD + N * cap * 16 + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    points = buf[GUARD:GUARD + N * cap * 16].view(N, cap, 16)
    cbuf = torch.full((N + 2,), -77, dtype=torch.int32, device=DEV)
    frame = torch.from_numpy(inp["frame"]).to(DEV) if inp["frame"] is not None else None
    p, c = depth_cloud(torch.from_numpy(inp["pred"]).to(DEV), torch.from_numpy(inp["ymap"]).to(DEV), torch.from_numpy(inp["xmap"]).to(DEV),
                       torch.from_numpy(inp["K"]).to(DEV), inp["min_depth"], inp["max_depth"], inp["step"], frame=frame, out=(points, cbuf[1:N + 1]),
                       workspace=workspace)
    torch.cuda.synchronize()
    assert p.data_ptr() == points.data_ptr() and tuple(p.shape) == (N, cap, 16)
    raw = buf.cpu().numpy()
    assert bool((raw[:GUARD] == FILL).all() and (raw[-GUARD:] == FILL).all()), "bytes outside the points buffer were written"
    cnt = cbuf.cpu().numpy()
    assert cnt[0] == -77 and cnt[-1] == -77
    return as_records(points, cnt[1:N + 1]), cnt[1:N + 1], raw[GUARD:-GUARD].reshape(N, cap, 16)


def check_records(recs, want):
    assert len(recs) == len(want)
    for n, (r, w) in enumerate(zip(recs, want)):
        assert r.shape == (w["u"].size,), (n, r.shape, w["u"].size)
        assert np.array_equal(r["z"].view(np.int32), w["z"].view(np.int32)), f"frame {n}: z (order or value)"           # a copy: bit-exact
        got_rgba = np.stack([r["red"], r["green"], r["blue"], r["alpha"]], 1)
        assert np.array_equal(got_rgba, w["rgba"]), f"frame {n}: colours"
        for i, f in enumerate(("x", "y")):
            err = np.abs(r[f].astype(np.float64) - w["xyz"][:, i])
            worst = float((err / np.maximum(w["bound"][:, i], 1e-300)).max()) if err.size else 0.0
            print(f"  frame {n} {f}: {r.size} records, largest error / bound = {worst:.3f}")
            assert bool(np.all(err <= w["bound"][:, i])), f"frame {n}: {f} off by up to {worst:.2f} x its bound"


@pytest.mark.parametrize("name", CR.CASES)
def test_depth_cloud(name):
    inp, want = reference(name)
    recs, cnt, raw = run_cloud(inp)
    cap = raw.shape[1]
    print(f"{name}: counts {cnt.tolist()} of capacity {cap}")
    assert cnt.tolist() == [w["u"].size for w in want]
    check_records(recs, want)
    if name == "all_kept":
        assert cnt.tolist() == [cap]
    if name == "none_kept":
        assert cnt.tolist() == [0] and bool((raw == FILL).all())                     # nothing written at all
    if name == "two_frames_different_counts":
        assert cnt[0] != cnt[1] and min(cnt) > CR.TILE
    if name == "scan_wider_than_one_wave":
        assert 64 < -(-cap // CR.TILE) <= CR.TILE
    if name == "scan_more_than_one_chunk":
        assert -(-cap // CR.TILE) > CR.TILE
    if name == "maps_with_outside":
        assert want[0]["v"].min() >= 7 and want[0]["u"].min() >= 4 and want[0]["u"].max() < 44      # the -1 border gives 0: dropped
    if name == "step_3_odd_sizes":
        assert cap == 13 * 21 and bool(np.all(want[0]["u"] % 3 == 0) and np.all(want[0]["v"] % 3 == 0))
    if name == "nan_inf_and_bounds":
        # kept: max_depth itself, the value above min_depth, the value below max_depth, 40; dropped: NaN, +-inf, min_depth, its lower
        # neighbour, max_depth's upper neighbour, +-0, -5, 1e-38, 3e38
        assert [(int(v), int(u)) for u, v in zip(want[0]["u"], want[0]["v"])] == [(0, 4), (1, 1), (1, 2), (2, 2)]
    if name == "no_frame":
        assert bool((want[0]["rgba"] == 255).all())


@functools.lru_cache(maxsize=None)
def twin(name):
    """The kernel's own fp32 arithmetic on the host (hip/twins.py: pinhole_project_np, the camera every geometry kernel shares) -> per frame
    the float32 [count,3] coordinates sde_depth_cloud must write, in raster order; the keep decision is the restatement's."""
    from simpledepthestimation_amd.hip.twins import pinhole_project_np
    inp, want = reference(name)
    full = CR.restore(inp["pred"], inp["ymap"], inp["xmap"])
    out = []
    for n, w in enumerate(want):
        px, py, _, _, _ = pinhole_project_np(full[n], inp["K"][n], np.eye(4, dtype=np.float32))
        out.append(np.stack([px[w["v"], w["u"]], py[w["v"], w["u"]], full[n][w["v"], w["u"]]], 1).astype(np.float32))
    return out


@pytest.mark.parametrize("name", CR.CASES)
def test_depth_cloud_equals_the_host_twin_bit_for_bit(name):
    """count, and the x, y, z bytes of every record up to count, are those of the shared camera's fp32 operations in their order."""
    want = twin(name)
    recs, cnt, _ = run_cloud(reference(name)[0])
    assert cnt.tolist() == [w.shape[0] for w in want]
    for n, (r, w) in enumerate(zip(recs, want)):
        got = np.stack([r["x"], r["y"], r["z"]], 1)
        print(f"{name} frame {n}: {int((got.view(np.uint32) != w.view(np.uint32)).sum())} of {got.size} coordinates differ from the host twin")
        assert got.tobytes() == w.tobytes(), f"frame {n}"


def test_depth_cloud_is_deterministic_and_ignores_workspace_contents():
    """Two runs, one on a workspace full of garbage: the same bytes (no atomics decide placement, the scan reads only what the count wrote)."""
    from simpledepthestimation_amd.hip.cloud import workspace_numel
    inp, want = reference("two_frames_different_counts")
    _, c0, raw0 = run_cloud(inp)
    ws = torch.randint(-2 ** 31, 2 ** 31 - 1, (workspace_numel(2, 37, 61, 1) + 5,), dtype=torch.int32, device=DEV)
    tail = ws[-5:].clone()
    _, c1, raw1 = run_cloud(inp, workspace=ws)
    assert np.array_equal(c0, c1) and np.array_equal(raw0, raw1) and torch.equal(ws[-5:], tail)


def test_refused_arguments_launch_nothing():
    """Every refusal returns SDE_ERR_ARG and leaves the destinations as they were."""
    from simpledepthestimation_amd.hip import lib as L
    from simpledepthestimation_amd.hip.cloud import depth_cloud
    inp, _ = reference("one_partial_block")
    pred, ymap, xmap, K = (torch.from_numpy(inp[k]).to(DEV) for k in ("pred", "ymap", "xmap", "K"))
    points = torch.full((1, 15, 16), FILL, dtype=torch.uint8, device=DEV)
    count = torch.full((1,), -77, dtype=torch.int32, device=DEV)
    ws = torch.zeros(4, dtype=torch.int32, device=DEV)
    lib = L.lib()

    def call(**kw):
        a = dict(pred=L.ptr(pred), N=1, ph=3, pw=5, ymap=L.ptr(ymap), xmap=L.ptr(xmap), H=3, W=5, frame=None, K=L.ptr(K), lo=1.0, hi=80.0, step=1,
                 ws=L.ptr(ws), ws_bytes=16, points=L.ptr(points), count=L.ptr(count))
        a.update(kw)
        return lib.sde_depth_cloud(a["pred"], a["N"], a["ph"], a["pw"], a["ymap"], a["xmap"], a["H"], a["W"], a["frame"], a["K"], a["lo"], a["hi"], a["step"],
                                   a["ws"], a["ws_bytes"], a["points"], a["count"], L.stream())
    for kw in (dict(N=0), dict(H=0), dict(W=0), dict(ph=-1), dict(step=0), dict(lo=80.0), dict(lo=81.0), dict(pred=None), dict(ymap=None), dict(xmap=None),
               dict(K=None), dict(points=None), dict(count=None), dict(ws=None), dict(ws_bytes=3), dict(points=L.ptr(points.view(-1)[8:]))):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((points == FILL).all()) and int(count[0]) == -77
    assert call() == 0                                                     # the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert int(count[0]) == reference("one_partial_block")[1][0]["u"].size
    with pytest.raises(ValueError):
        depth_cloud(pred, ymap, xmap, K, 1.0, 80.0, step=0)
    with pytest.raises(L.SdeHipError):
        depth_cloud(pred, ymap, xmap, K, 1.0, 80.0, workspace=torch.zeros(0, dtype=torch.int32, device=DEV))


# ---- dense mode ------------------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def dense_reference(H, W, per_pixel):
    depth, R, t, cot = CR.dense_inputs(H, W, per_pixel, seed=H * 100 + W + int(per_pixel))
    f64 = CR.img_to_points_grads(depth, R, t, cot, torch.float64)
    f32 = CR.img_to_points_grads(depth, R, t, cot, torch.float32)
    tols = tuple(max(4 * rel(a, b), FLOOR) for a, b in zip(f32, f64))
    print(f"  img_to_points {H}x{W} per-pixel t {per_pixel}: restatement float32 vs float64 (points, ddepth, dR, dt) "
          + ", ".join(f"{rel(a, b):.2e}" for a, b in zip(f32, f64)))
    return (depth, R, t, cot), f64, tols


@pytest.mark.parametrize("per_pixel", [False, True])
@pytest.mark.parametrize("H, W", [(5, 7), (33, 47)])          # one workgroup with tail lanes; seven partial-sum rows, the last one ragged
def test_img_to_points(H, W, per_pixel):
    from simpledepthestimation_amd.geometry.camera import img_to_points
    (depth, R, t, cot), want, tols = dense_reference(H, W, per_pixel)
    d, r, tt = (x.to(DEV).requires_grad_(True) for x in (depth, R, t))
    p = img_to_points(d, r, tt)
    (p * cot.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert p.dtype == torch.float32 and tuple(p.shape) == (2, 3, H, W) and tuple(tt.grad.shape) == tuple(t.shape)
    for name, got, w, tol in zip(("points", "ddepth", "dR", "dt"), (p.detach(), d.grad, r.grad, tt.grad), want, tols):
        e = rel(got.cpu(), w)
        print(f"  {name}: {e:.2e} (tolerance {tol:.2e})")
        assert e <= tol, (name, e, tol)
    again = img_to_points(d.detach(), r.detach(), tt.detach())
    assert torch.equal(again, p.detach())


def test_img_to_points_gradient_of_a_subset():
    """Only the inputs that ask for a gradient get one: depth alone skips the twelve sums (no workspace, one launch) and gives the ddepth of the
    full backward bit for bit; R alone and t alone give theirs."""
    from simpledepthestimation_amd.geometry.camera import img_to_points
    (depth, R, t, cot), _, _ = dense_reference(33, 47, False)
    full = [x.to(DEV).requires_grad_(True) for x in (depth, R, t)]
    (img_to_points(*full) * cot.to(DEV)).sum().backward()
    for k in range(3):
        ins = [x.to(DEV).requires_grad_(i == k) for i, x in enumerate((depth, R, t))]
        (img_to_points(*ins) * cot.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        assert [x.grad is not None for x in ins] == [i == k for i in range(3)]
        assert torch.equal(ins[k].grad, full[k].grad), k
    (_, _, tp, _), _, _ = dense_reference(33, 47, True)
    ins = [depth.to(DEV), R.to(DEV), tp.to(DEV).requires_grad_(True)]
    (img_to_points(*ins) * cot.to(DEV)).sum().backward()
    assert torch.equal(ins[2].grad, cot.to(DEV).reshape(2, 3, -1))


def test_img_to_points_equals_the_reference_recording():
    """The reference's own float32 output (tests/golden/cloud.npz): a point is a sum of four float32 terms evaluated in some order -- within 8
    roundings of the sum of the terms' magnitudes on either side, 16 between the two."""
    import os
    from simpledepthestimation_amd.geometry.camera import img_to_points
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cloud.npz"))
    terms = np.abs(g["grid"].astype(np.float64) * g["depth"].astype(np.float64))
    for t_name in ("t1", "tp"):
        got = img_to_points(*(torch.from_numpy(g[k]).to(DEV) for k in ("depth", "R", t_name))).cpu().numpy()
        tt = np.abs(g[t_name].astype(np.float64)).reshape((2, 3, 1, 1) if t_name == "t1" else (2, 3, 5, 7))
        mag = np.einsum("bck,bkhw->bchw", np.abs(g["R"].astype(np.float64)), terms) + tt
        assert bool(np.all(np.abs(got.astype(np.float64) - g["points_" + t_name]) <= 16 * 2.0 ** -24 * mag)), t_name


# ---- the predictor ---------------------------------------------------------------------------------------------------------------------------
STEPS = [{"NAME": "CropTopTo", "IMG_H": 88}, {"NAME": "Resize", "IMG_H": 64, "IMG_W": 192}]
CLOUD = dict(min_depth=0.0, max_depth=80.0, step=1)      # every pixel under the eight border rows: the depth head's output lies in (0, 80]
K_SRC = np.array([[120.5, 0, 80.2], [0, 118.0, 47.6], [0, 0, 1]], dtype=np.float32)


@pytest.fixture(scope="module")
def sup():
    from oracle import models as OM
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.engine.predictor import DepthPredictor
    from simpledepthestimation_amd.modeling import build_model
    cfg = get_cfg()
    cfg.MODEL.META_ARCHITECTURE, cfg.MODEL.DEPTH_NET.ENCODER_NAME, cfg.MODEL.DEVICE, cfg.MODEL.COMPUTE_DTYPE = "SupDepthModel", "18", DEV, "fp32"
    cfg.merge_from_other_cfg({"DATASETS": {"TEST": {"PREPROCESS": [{"NAME": "LoadImg"}] + STEPS + [{"NAME": "ToTensor"}]}}})
    model = build_model(cfg)
    model.load_state_dict(OM.init_state_dict(18, seed=1), strict=True)
    model.eval()
    frames = np.random.default_rng(3).integers(0, 256, (2, 96, 160, 3), dtype=np.uint8)
    return {"frames": frames, "eager": DepthPredictor(cfg, model=model, use_graph=False), "graph": DepthPredictor(cfg, model=model, use_graph=True)}


def same_records(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_predict_with_cloud_eager_graph_and_direct(sup):
    from simpledepthestimation_amd.hip.cloud import as_records, depth_cloud
    frames = sup["frames"]
    base = sup["eager"].predict(frames)
    assert sorted(base) == ["canvas", "depth", "depth_net", "depth_u16"]                      # without cloud: the keys of before, nothing else
    # the lower limit is the median of the restored depth under the border rows: about half of the pixels are dropped, whatever the weights give
    inside = base["depth"][:, 8:]
    cut = dict(min_depth=float(inside.median()), max_depth=80.0, step=1)
    assert float(inside.min()) < cut["min_depth"] < float(inside.max())
    e = sup["eager"].predict(frames, intrinsics=K_SRC, cloud=cut)
    assert sorted(e) == ["canvas", "count", "depth", "depth_net", "depth_u16", "points"]
    assert tuple(e["points"].shape) == (2, 96 * 160, 16) and e["points"].dtype == torch.uint8 and e["points"].is_cuda
    assert tuple(e["count"].shape) == (2,) and e["count"].dtype == torch.int32
    assert torch.equal(e["depth"], base["depth"]) and torch.equal(e["canvas"], base["canvas"])
    er = as_records(e["points"], e["count"])
    # the cloud of the returned depth: identity maps over the restored map, the same K, the frames' colours
    ident = (np.arange(96, dtype=np.int32), np.arange(160, dtype=np.int32))
    dp, dc = depth_cloud(e["depth"], *ident, torch.from_numpy(K_SRC).to(DEV), cut["min_depth"], cut["max_depth"], 1, frame=torch.from_numpy(frames).to(DEV))
    assert torch.equal(dc, e["count"]) and same_records(as_records(dp, dc), er)
    # ... and of the restatement on that depth: the top eight rows (CropTopTo) are outside
    want = CR.cloud(e["depth"].cpu().numpy(), *ident, np.stack([K_SRC, K_SRC]), cut["min_depth"], cut["max_depth"], 1, frames)
    print(f"predict: counts {e['count'].tolist()} of capacity {96 * 160}")
    assert e["count"].tolist() == [w["u"].size for w in want] and all(w["v"].min() >= 8 for w in want)
    assert 0 < sum(e["count"].tolist()) < 2 * 88 * 160
    check_records(er, want)
    for _ in range(2):                                   # the first call captures, the second only replays
        g = sup["graph"].predict(frames, intrinsics=K_SRC, cloud=cut)
        assert torch.equal(g["count"], e["count"]) and same_records(as_records(g["points"], g["count"]), er)
        assert torch.equal(g["depth"], e["depth"])
    K2 = K_SRC.copy()
    K2[0, 0] = 200.0                                     # the replayed graph reads the intrinsics given now
    g2 = as_records(*(sup["graph"].predict(frames, intrinsics=K2, cloud=cut)[k] for k in ("points", "count")))
    e2 = as_records(*(sup["eager"].predict(frames, intrinsics=K2, cloud=cut)[k] for k in ("points", "count")))
    assert same_records(g2, e2) and not same_records(g2, er)
    s3 = sup["graph"].predict(frames, intrinsics=K_SRC, cloud=dict(min_depth=0.0, max_depth=80.0, step=3))
    assert tuple(s3["points"].shape) == (2, 32 * 54, 16) and s3["count"].tolist() == [29 * 54] * 2          # rows 9, 12, ... 93 of 96, every third column
    want3 = CR.cloud(e["depth"].cpu().numpy(), *ident, np.stack([K_SRC, K_SRC]), 0.0, 80.0, 3, frames)
    check_records(as_records(s3["points"], s3["count"]), want3)
    assert sorted(sup["graph"].predict(frames)) == ["canvas", "depth", "depth_net", "depth_u16"]
    with pytest.raises(ValueError, match="intrinsics"):
        sup["graph"].predict(frames, cloud=cut)


def test_stream_yields_the_records_of_predict(sup):
    from simpledepthestimation_amd.hip.cloud import as_records
    frames = [np.random.default_rng(40 + i).integers(0, 256, (96, 160, 3), dtype=np.uint8) for i in range(3)]
    want = []
    for f in frames:
        o = sup["eager"].predict(f, intrinsics=K_SRC, cloud=CLOUD)
        want.append((as_records(o["points"], o["count"])[0], o["depth"][0].cpu().numpy()))
    n = 0
    for i, res in enumerate(sup["graph"].stream(iter(frames), intrinsics=K_SRC, cloud=CLOUD)):
        assert sorted(res) == ["canvas", "count", "depth", "points"]
        assert res["points"].shape == (1, 96 * 160, 16) and res["count"].shape == (1,)
        assert np.array_equal(res["depth"], want[i][1])
        assert same_records(as_records(res["points"], res["count"]), [want[i][0]])
        n += 1
    assert n == 3
    assert sorted(next(iter(sup["graph"].stream(iter(frames[:1]))))) == ["canvas", "depth"]


def test_demo_tool_writes_a_ply(tmp_path):
    """The tool end to end with --save-cloud: a PLY the minimal reader of test_cloud.py loads, with the records predict gives for that frame."""
    import yaml
    from PIL import Image
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.engine.predictor import DepthPredictor
    from simpledepthestimation_amd.hip.cloud import as_records
    from simpledepthestimation_amd.tools import demo
    from test_cloud import read_ply
    src, dst = tmp_path / "frames", tmp_path / "out"
    src.mkdir()
    frame = np.random.default_rng(50).integers(0, 256, (96, 160, 3), dtype=np.uint8)
    Image.fromarray(frame).save(src / "a.png")
    conf = {"MODEL": {"META_ARCHITECTURE": "SupDepthModel", "DEVICE": DEV},
            "DATASETS": {"TEST": {"PREPROCESS": [{"NAME": "LoadImg"}] + STEPS + [{"NAME": "ToTensor"}]}}}
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(conf))
    torch.manual_seed(7)
    assert demo.main(["--cfg", str(tmp_path / "config.yaml"), "--input", str(src), "--output", str(dst), "--save-cloud", "--cloud-step", "2",
                      "--intrinsics", "120.5", "118", "80.2", "47.6"]) == 0
    assert sorted(p.name for p in dst.iterdir()) == ["a.ply", "a.png"]
    cfg = get_cfg()
    cfg.set_new_allowed(True)
    cfg.merge_from_file(str(tmp_path / "config.yaml"))
    torch.manual_seed(7)
    o = DepthPredictor(cfg).predict(frame, intrinsics=K_SRC, cloud=dict(min_depth=0.0, max_depth=float(cfg.MODEL.MAX_DEPTH), step=2))
    want, = as_records(o["points"], o["count"])
    got, _ = read_ply(dst / "a.ply")
    assert got.shape == (int(o["count"][0]),) and got.size > 0 and got.tobytes() == want.tobytes()

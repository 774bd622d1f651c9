"""GPU: sde_depth_present against the float64 restatement of its definition (present_ref.py), DepthPredictor against the composed route (CPU
preprocess chain -> model -> torch gather through backward_maps), its graph replay, its stream and the demo tool end to end."""
import os

import numpy as np
import pytest
import torch

import present_ref as PR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 37          # guard elements in front of and behind every buffer: an odd count, so no view starts on a 16-byte boundary
STEPS = [{"NAME": "CropTopTo", "IMG_H": 72}, {"NAME": "Resize", "IMG_H": 64, "IMG_W": 192}]


def guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_intact(buf, fill):
    return bool((buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all())


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lut():
    from simpledepthestimation_amd.utils.colormap import magma_u8
    return magma_u8()


@pytest.fixture(scope="module")
def refs(lut):
    """The float64 reference of every (case, N), computed once."""
    out = {}
    for name in PR.CASES:
        for N in (1, 3):
            pred, frame, ymap, xmap = PR.case_inputs(name, N)
            out[name, N] = (pred, frame, ymap, xmap) + PR.reference(pred, ymap, xmap, lut)
    return out


@pytest.mark.parametrize("want_depth, want_u16", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("with_frame", [True, False])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("name", PR.CASES)
def test_present_kernel(refs, lut, name, N, with_frame, want_depth, want_u16):
    from simpledepthestimation_amd.hip.present import depth_present
    pred, frame, ymap, xmap, full, u16, idx, boundary, other = refs[name, N]
    H, W = ymap.size, xmap.size
    share = float(boundary.mean())
    print(f"{name} N={N}: boundary share {share:.4%} of {boundary.size} pixels")
    assert share <= 0.01
    rows = 2 * H if with_frame else H
    cbuf, canvas = guarded((N, rows, W, 3), torch.uint8, 0xA5)
    dbuf, depth = guarded((N, H, W), torch.float32, -7.25)
    ubuf, du16 = guarded((N, H, W), torch.int16, 0x5A5A)
    _, pred_d = guarded(pred.shape, torch.float32, 0.0)             # the inputs too start off any 16-byte boundary
    pred_d.copy_(torch.from_numpy(pred))
    fr_d = None
    if with_frame:
        _, fr_d = guarded(frame.shape, torch.uint8, 0)
        fr_d.copy_(torch.from_numpy(frame))
    c, d, u = depth_present(pred_d, torch.from_numpy(ymap).to(DEV), torch.from_numpy(xmap).to(DEV), PR.VMAX, PR.GAMMA, lut=torch.from_numpy(lut).to(DEV),
                            frame=fr_d, want_depth=want_depth, want_u16=want_u16, out=(canvas, depth if want_depth else None, du16 if want_u16 else None))
    torch.cuda.synchronize()
    assert c.data_ptr() == canvas.data_ptr() and (d is None) == (not want_depth) and (u is None) == (not want_u16)
    assert guards_intact(cbuf, 0xA5) and guards_intact(dbuf, -7.25) and guards_intact(ubuf, 0x5A5A)
    if want_depth:
        assert np.array_equal(depth.cpu().numpy().view(np.int32), full.view(np.int32))          # bit for bit, NaN and -3.5 included
    else:
        assert bool((dbuf == -7.25).all())
    if want_u16:
        assert np.array_equal(du16.cpu().numpy().view(np.uint16), u16)
    else:
        assert bool((ubuf == 0x5A5A).all())
    got = canvas.cpu().numpy()
    if with_frame:
        assert np.array_equal(got[:, :H], frame)
        got = got[:, H:]
    exact = np.all(got == lut[idx], axis=-1)
    either = exact | np.all(got == lut[other], axis=-1)
    assert bool(np.all(np.where(boundary, either, exact))), f"{int((~np.where(boundary, either, exact)).sum())} colour pixels differ"


def test_present_default_table_and_new_tensors(refs, lut):
    """Without lut / out: the magma table, fresh outputs; maps given as host arrays are validated and uploaded."""
    from simpledepthestimation_amd.hip.lib import SdeHipError
    from simpledepthestimation_amd.hip.present import depth_present
    pred, frame, ymap, xmap, full, u16, idx, boundary, other = refs["resize_pad", 1]
    c, d, u = depth_present(torch.from_numpy(pred).to(DEV), ymap, xmap, PR.VMAX)
    assert u is None and tuple(c.shape) == (1, ymap.size, xmap.size, 3)
    assert np.array_equal(d.cpu().numpy().view(np.int32), full.view(np.int32))
    got = c.cpu().numpy()
    assert bool(np.all(np.all(got == lut[idx], -1) | (boundary & np.all(got == lut[other], -1))))
    bad = torch.from_numpy(ymap).to(DEV).clone()
    bad[-1] = pred.shape[1]                                       # one row past the prediction: refused on the host, nothing is launched
    with pytest.raises(SdeHipError):
        depth_present(torch.from_numpy(pred).to(DEV), bad, torch.from_numpy(xmap).to(DEV), PR.VMAX)


# ---- the predictor -------------------------------------------------------------------------------------------------------------------------
def make_cfg(meta, dtype):
    from simpledepthestimation_amd.config import get_cfg
    cfg = get_cfg()
    cfg.MODEL.META_ARCHITECTURE, cfg.MODEL.DEPTH_NET.ENCODER_NAME, cfg.MODEL.DEVICE, cfg.MODEL.COMPUTE_DTYPE = meta, "18", DEV, dtype
    cfg.merge_from_other_cfg({"DATASETS": {"TEST": {"PREPROCESS": [{"NAME": "LoadImg"}] + STEPS + [{"NAME": "ToTensor"}]}}})
    return cfg


def frames_of(n, hw=(80, 200), seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n,) + hw + (3,), dtype=np.uint8)


def composed(model, frames, K=None):
    """The route the package offered before: CPU chain per frame (it moves the intrinsics too), model(batch), torch gather through backward_maps."""
    from simpledepthestimation_amd.data.preprocess import build_preprocess
    from simpledepthestimation_amd.evaluation.depth_evaluation import backward_maps
    import simpledepthestimation_amd.data.preprocess.augmentation, simpledepthestimation_amd.data.preprocess.formating  # noqa: F401,E401
    imgs, Ks, meta = [], [], None
    for f in frames:
        data = {"img": f.copy(), "metadata": {}}
        if K is not None:
            data["intrinsics"] = K.copy()
        for s in STEPS + [{"NAME": "ToTensor"}]:
            data = build_preprocess(s).forward(data)
        imgs.append(data["img"])
        Ks.append(data.get("intrinsics"))
        meta = data["metadata"]
    batch = {"img": torch.stack(imgs)}
    if K is not None:
        batch["intrinsics"] = torch.from_numpy(np.stack(Ks))
    with torch.no_grad():
        pred = model(batch)["depth_pred"].float()[:, 0]
    rows, cols = backward_maps(tuple(pred.shape[-2:]), meta, [s["NAME"] for s in STEPS])
    ry, cx = torch.from_numpy(rows).to(DEV).long(), torch.from_numpy(cols).to(DEV).long()
    inside = (ry >= 0)[:, None] & (cx >= 0)[None, :]
    full = torch.where(inside[None], pred[:, ry.clamp(min=0)][:, :, cx.clamp(min=0)], torch.zeros((), device=DEV))
    return pred, full


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@pytest.fixture(scope="module", params=["fp32", "bf16"])
def sup(request):
    from oracle import models as OM
    from simpledepthestimation_amd.engine.predictor import DepthPredictor
    from simpledepthestimation_amd.modeling import build_model
    cfg = make_cfg("SupDepthModel", request.param)
    model = build_model(cfg)
    model.load_state_dict(OM.init_state_dict(18, seed=1), strict=True)
    model.eval()
    frames = frames_of(3)
    ref_net, ref_full = composed(model, frames)
    return {"cfg": cfg, "model": model, "frames": frames, "ref_net": ref_net, "ref_full": ref_full,
            "eager": DepthPredictor(cfg, model=model, use_graph=False), "graph": DepthPredictor(cfg, model=model, use_graph=True)}


def test_predict_equals_composed_route(sup):
    out = sup["eager"].predict(sup["frames"])
    assert tuple(out["depth"].shape) == (3, 80, 200) and tuple(out["depth_net"].shape) == (3, 64, 192) and tuple(out["canvas"].shape) == (3, 160, 200, 3)
    assert torch.equal(bits(out["depth_net"]), bits(sup["ref_net"]))
    assert torch.equal(bits(out["depth"]), bits(sup["ref_full"]))
    assert bool((out["depth"][:, :8] == 0).all()) and bool((out["depth"][:, 8:] > 0).all())       # CropTopTo(72) of 80 rows: eight rows of zeros on top
    assert np.array_equal(out["canvas"][:, :80].cpu().numpy(), sup["frames"])


def test_graph_replay_equals_eager(sup):
    e = sup["eager"].predict(sup["frames"], want_u16=True)
    for _ in range(2):                                   # the first call captures, the second only replays
        g = sup["graph"].predict(sup["frames"], want_u16=True)
        for k in ("depth", "depth_net", "canvas", "depth_u16"):
            assert torch.equal(bits(g[k]), bits(e[k])), k
    other = frames_of(3, seed=9)                          # the replayed graph reads what is uploaded now, not what it was captured with
    assert torch.equal(bits(sup["graph"].predict(other)["depth"]), bits(sup["eager"].predict(other)["depth"]))
    assert not torch.equal(bits(sup["graph"].predict(other)["depth"]), bits(e["depth"]))


def test_batch_equals_single_frames(sup):
    whole = sup["graph"].predict(sup["frames"])
    for n in range(3):
        one = sup["graph"].predict(sup["frames"][n])
        assert tuple(one["depth"].shape) == (1, 80, 200)
        for k in ("depth", "depth_net", "canvas"):
            assert torch.equal(bits(one[k][0]), bits(whole[k][n])), (k, n)


def test_predict_without_present_and_without_frame(sup):
    out = sup["eager"].predict(sup["frames"][0], present=False)
    assert out["depth"] is None and out["canvas"] is None and torch.equal(bits(out["depth_net"][0]), bits(sup["ref_net"][0]))
    bare = sup["eager"].predict(sup["frames"][0], frame_in_canvas=False)
    both = sup["eager"].predict(sup["frames"][0])
    assert tuple(bare["canvas"].shape) == (1, 80, 200, 3) and torch.equal(bare["canvas"], both["canvas"][:, 80:])


def test_monodepth2_goes_through_the_eval_path():
    from simpledepthestimation_amd.engine.predictor import DepthPredictor
    from simpledepthestimation_amd.modeling import build_model
    torch.manual_seed(3)
    cfg = make_cfg("MonoDepth2Model", "fp32")
    model = build_model(cfg).eval()
    frames = frames_of(1, seed=4)
    ref_net, ref_full = composed(model, frames)
    out = DepthPredictor(cfg, model=model).predict(frames[0])
    assert torch.equal(bits(out["depth_net"]), bits(ref_net)) and torch.equal(bits(out["depth"]), bits(ref_full))


def test_bts_takes_its_intrinsics_through_the_chain():
    """BtsModel reads the focal length: without intrinsics its KeyError comes through, with them the predictor moves them as the chain's steps do."""
    from simpledepthestimation_amd.engine.predictor import DepthPredictor
    from simpledepthestimation_amd.modeling import build_model
    torch.manual_seed(5)
    cfg = make_cfg("SupDepthModel", "fp32")
    cfg.MODEL.DATASET, cfg.MODEL.DEPTH_NET.NAME, cfg.MODEL.DEPTH_NET.ENCODER_NAME, cfg.MODEL.DEPTH_NET.BTS_SIZE = "kitti", "BtsModel", "resnet50_bts", 128
    model = build_model(cfg).eval()
    frames = frames_of(2, seed=6)
    K = np.array([[721.5, 0, 100.2], [0, 721.5, 43.7], [0, 0, 1]], dtype=np.float32)
    ref_net, ref_full = composed(model, frames, K)
    eager, graph = DepthPredictor(cfg, model=model, use_graph=False), DepthPredictor(cfg, model=model, use_graph=True)
    with pytest.raises(KeyError, match="intrinsics"):
        eager.predict(frames)
    e = eager.predict(frames, intrinsics=K)
    assert torch.equal(bits(e["depth_net"]), bits(ref_net)) and torch.equal(bits(e["depth"]), bits(ref_full))
    for _ in range(2):
        g = graph.predict(frames, intrinsics=np.stack([K, K]))
        assert torch.equal(bits(g["depth"]), bits(e["depth"])) and torch.equal(g["canvas"], e["canvas"])
    K2 = K.copy()
    K2[0, 0] = K2[1, 1] = 500.0                      # the replayed graph reads the intrinsics given now
    assert torch.equal(bits(graph.predict(frames, intrinsics=K2)["depth"]), bits(eager.predict(frames, intrinsics=K2)["depth"]))
    assert not torch.equal(bits(graph.predict(frames, intrinsics=K2)["depth"]), bits(e["depth"]))


def test_stream(sup):
    """Five frames, the third of another size: results in order, equal to predict's, and still intact when the next one is requested."""
    p = sup["graph"]
    frames = [frames_of(1, seed=20 + i)[0] for i in range(5)]
    frames[2] = frames_of(1, hw=(84, 208), seed=22)[0]
    want = []
    for f in frames:
        o = sup["eager"].predict(f)
        want.append((o["depth"][0].cpu().numpy(), o["canvas"][0].cpu().numpy()))
    it = p.stream(iter(frames))
    prev = None
    for i in range(5):
        res = next(it)                                   # requesting result i ...
        if prev is not None:                             # ... leaves result i-1 as it was handed out
            assert np.array_equal(prev["depth"], want[i - 1][0]) and np.array_equal(prev["canvas"], want[i - 1][1])
        assert res["depth"].shape == frames[i].shape[:2] and res["canvas"].shape == (2 * frames[i].shape[0], frames[i].shape[1], 3)
        assert np.array_equal(res["depth"].view(np.int32), want[i][0].view(np.int32)), i
        assert np.array_equal(res["canvas"], want[i][1]), i
        prev = res
    with pytest.raises(StopIteration):
        next(it)


def test_demo_tool_end_to_end(tmp_path):
    """Three small PNGs and a YAML config with the chain and no weights file (the model keeps its seeded initialisation)."""
    import yaml
    from PIL import Image
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.engine.predictor import DepthPredictor
    from simpledepthestimation_amd.evaluation.depth_evaluation import write_depth
    from simpledepthestimation_amd.tools import demo
    src, dst = tmp_path / "frames", tmp_path / "out"
    src.mkdir()
    frames = frames_of(3, seed=30)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(src / f"f{2 - i}.png")               # names in reverse: the tool sorts
    conf = {"MODEL": {"META_ARCHITECTURE": "SupDepthModel", "DEVICE": DEV},                 # the default encoder: ResNet-18
            "DATASETS": {"TEST": {"PREPROCESS": [{"NAME": "LoadImg"}] + STEPS + [{"NAME": "ToTensor"}]}}}
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(conf))
    torch.manual_seed(7)
    assert demo.main(["--cfg", str(tmp_path / "config.yaml"), "--input", str(src), "--output", str(dst), "--save-depth"]) == 0
    cfg = get_cfg()
    cfg.set_new_allowed(True)
    cfg.merge_from_file(str(tmp_path / "config.yaml"))
    torch.manual_seed(7)
    out = DepthPredictor(cfg).predict(frames)
    assert sorted(os.listdir(dst)) == ["f0.png", "f0_depth.png", "f1.png", "f1_depth.png", "f2.png", "f2_depth.png"]
    for i in range(3):
        pic = np.asarray(Image.open(dst / f"f{2 - i}.png"))
        assert pic.shape == (160, 200, 3) and np.array_equal(pic[:80], frames[i])
        assert np.array_equal(pic[80:], out["canvas"][i, 80:].cpu().numpy())
        write_depth(out["depth"][i].cpu().numpy(), str(tmp_path / "want.png"))
        assert np.array_equal(np.asarray(Image.open(dst / f"f{2 - i}_depth.png")), np.asarray(Image.open(tmp_path / "want.png")))
        assert open(dst / f"f{2 - i}_depth.png", "rb").read() == open(tmp_path / "want.png", "rb").read()
    assert demo.main(["--cfg", str(tmp_path / "config.yaml"), "--input", str(src / "f1.png"), "--output", str(tmp_path / "bare"), "--no-frame"]) == 0
    assert np.asarray(Image.open(tmp_path / "bare" / "f1.png")).shape == (80, 200, 3)

"""GPU: the Waymo data path on the device -- the existing prep, mask-dilation and metric kernels at the geometry Waymo brings (CropTopTo + a 4-6x
reduction, tap-compacted uploads with host-given tables, masks through the prefetcher), and the three Waymo projects end to end over the synthetic
tree of tests/waymo_tree.py.  Everything on the data side is integer / index logic: bit-identical to the CPU chain.  The evaluation part compares
float reductions at the tolerance tests/test_evaluation.py uses for sde_depth_metrics (2e-5 relative, 1e-7 absolute)."""
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from simpledepthestimation_amd.data.preprocess import build_preprocess
from waymo_tree import make_waymo_tree, project_cfg, seeded_batches

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _chain(on_device, crop, h, w, jitter_prob):
    extra = {"ON_DEVICE": on_device} if on_device else {}
    steps = [dict(NAME="CropTopTo", IMG_H=crop)] if crop else []
    steps += [dict(NAME="Resize", IMG_H=h, IMG_W=w, **extra), dict(NAME="RandomFlip"), dict(NAME="RandomImageAug", JITTER_PROB=jitter_prob, **extra), dict(NAME="ToTensor")]
    return [build_preprocess(s) for s in steps]


def _run(chain, sample, seed):
    random.seed(seed); torch.manual_seed(seed); np.random.seed(seed)
    d = {k: ([a.copy() for a in v] if isinstance(v, list) else (v.copy() if isinstance(v, np.ndarray) else dict(v))) for k, v in sample.items()}
    for p in chain:
        d = p.forward(d)
    return d


def _sample(rng, Hs, Ws):
    return {"img": rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8), "ctx_img": [rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)],
            "intrinsics": np.array([[2055.0, 0, Ws / 2], [0, 2055.0, Hs / 2], [0, 0, 1]], np.float32), "metadata": {}}


def _same(got, want):
    got, want = (torch.as_tensor(np.asarray(x)) if not torch.is_tensor(x) else x.detach().cpu() for x in (got, want))
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)


# (source sizes of the three samples in modes (i) / (ii), in mode (iii), rows CropTopTo keeps, destination)
GEOMETRY = {"crop_6x": ([(56, 96)] * 3, [(56, 96), (62, 100), (56, 96)], 48, (8, 16)),                # 56 x 96 cropped to 48 x 96, then 6x both ways
            "odd_ratio": ([(40, 97)] * 3, [(40, 97), (40, 97), (43, 99)], 0, (10, 24))}                # non-integer ratio, odd width, no crop


@pytest.mark.parametrize("case", sorted(GEOMETRY))
@pytest.mark.parametrize("mode", ["plain", "taps_collated", "taps_two_sizes"])
def test_prep_kernels_at_waymo_geometry(case, mode):
    """sde_image_prep_u8(_multi) behind CropTopTo at a 4-6x reduction: full frames with the plain tables, cut-down frames with the host-given tables
    (one pair for a stacked batch; per-sample pairs, grouped by size and table, for a batch of two source sizes) -- all equal to the CPU chain."""
    from simpledepthestimation_amd.data.build import collate_samples
    from simpledepthestimation_amd.data.device_aug import DeviceImageAug
    same, two, crop, (h, w) = GEOMETRY[case]
    sizes = two if mode == "taps_two_sizes" else same
    rng = np.random.default_rng(17)
    samples = [_sample(rng, Hs, Ws) for Hs, Ws in sizes]
    probs = [1.0, 0.0, 1.0]                                            # the second sample is not jittered
    cpu = [_run(_chain(False, crop, h, w, p), s, 300 + i) for i, (s, p) in enumerate(zip(samples, probs))]
    raw = [_run(_chain(True if mode == "plain" else "taps", crop, h, w, p), s, 300 + i) for i, (s, p) in enumerate(zip(samples, probs))]
    assert raw[1]["aug_params"][4] < 0 and raw[0]["aug_params"][4] >= 0 and [r["flip"] for r in raw] == [c["flip"] for c in cpu]
    batch = collate_samples(raw)
    if mode == "plain":
        assert "device_taps" not in batch and torch.is_tensor(batch["img_u8"]) and batch["img_u8"].shape[1:3] == ((crop or sizes[0][0]), sizes[0][1])
    elif mode == "taps_collated":
        assert torch.is_tensor(batch["img_u8"]) and len(batch["device_taps"]) == 2 and torch.is_tensor(batch["device_taps"][0])
        assert batch["img_u8"].shape[1] <= 2 * h and batch["img_u8"].shape[2] <= 2 * w
    else:
        assert isinstance(batch["img_u8"], list) and isinstance(batch["device_taps"], list) and len(batch["device_taps"]) == 3
        assert len({tuple(f.shape) for f in batch["img_u8"]}) == 2 or len({t[0].tobytes() + t[1].tobytes() for t in batch["device_taps"]}) == 2
    out = DeviceImageAug(DEV)(batch)
    torch.cuda.synchronize()
    assert not ({"device_taps", "img_u8", "ctx_img_u8", "aug_params", "device_resize"} & set(out)) and out["flip"] == cpu[0]["flip"]
    assert out["img"].is_cuda and out["img"].shape == (3, 3, h, w)
    assert _same(out["img"], torch.stack([c["img"] for c in cpu])), "jittered target frames differ"
    assert _same(out["img_orig"], torch.stack([c["img_orig"] for c in cpu]))
    assert len(out["ctx_img"]) == len(out["ctx_img_orig"]) == 1
    assert _same(out["ctx_img"][0], torch.stack([c["ctx_img"][0] for c in cpu])), "jittered context frames differ"
    assert _same(out["ctx_img_orig"][0], torch.stack([c["ctx_img_orig"][0] for c in cpu]))
    assert not torch.equal(out["img"][0], out["img_orig"][0]) and torch.equal(out["img"][1], out["img_orig"][1])


def test_given_tables_are_checked_on_the_host_before_any_launch():
    """The kernel indexes the frames with whatever the tables hold, so tables that do not fit the frames never reach it."""
    from simpledepthestimation_amd.data.device_aug import DeviceImageAug
    from simpledepthestimation_amd.data.preprocess.augmentation import compact_taps
    from simpledepthestimation_amd.hip.lib import SdeHipError
    aug = DeviceImageAug(DEV)
    xt, yt = compact_taps(96, 16)[1], compact_taps(48, 8)[1]
    frames = torch.zeros(1, 16, 32, 3, dtype=torch.uint8)
    params = torch.tensor([[1.0, 1.0, 1.0, 0.0, -1.0, -1.0, -1.0, -1.0]])
    ok = aug({"img_u8": frames, "aug_params": params, "device_resize": (8, 16), "device_taps": (xt, yt)})
    assert ok["img"].shape == (1, 3, 8, 16) and float(ok["img"].abs().sum()) == 0.0
    bad = xt.copy(); bad[-1, 1] = 32                                   # one past the last column
    for tabs in ((bad, yt), (xt, yt[:-1]), (xt.astype(np.int64), yt), (yt, xt)):
        with pytest.raises(SdeHipError):
            aug({"img_u8": frames, "aug_params": params, "device_resize": (8, 16), "device_taps": tabs})
    with pytest.raises(SdeHipError):                                   # a frame smaller than the tables were made for
        aug({"img_u8": frames[:, :15], "aug_params": params, "device_resize": (8, 16), "device_taps": (xt, yt)})
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def small_tree(tmp_path_factory):
    return make_waymo_tree(str(tmp_path_factory.mktemp("waymo_small")))


@pytest.fixture(scope="module")
def net_tree(tmp_path_factory):
    """200 x 580 frames: CropTopTo 192, then 3x down to 64 x 192, the smallest size the tiny-model tests of the three nets run at."""
    return make_waymo_tree(str(tmp_path_factory.mktemp("waymo_net")), seed=1, size=(200, 580))


def _assert_batch_equals(got, want, keys):
    for k in keys:
        if isinstance(want[k], list):
            assert isinstance(got[k], list) and len(got[k]) == len(want[k]), k
            for i, (a, b) in enumerate(zip(got[k], want[k])):
                assert _same(a, b), (k, i)
        elif isinstance(want[k], bool):
            assert got[k] == want[k], k
        else:
            assert _same(got[k], want[k]), k


def test_taps_loader_through_the_prefetcher_delivers_the_cpu_batches(small_tree):
    from simpledepthestimation_amd.data import DevicePrefetcher
    from simpledepthestimation_amd.data.device_aug import DeviceImageAug
    from simpledepthestimation_amd.hip import motion_loss as HM
    cpu = seeded_batches(project_cfg("MotionLearningWaymo", small_tree, 48, 8, 16), 2, seed=11)
    tap = seeded_batches(project_cfg("MotionLearningWaymo", small_tree, 48, 8, 16, on_device="taps"), 2, seed=11)
    assert all("device_taps" in b and b["img_u8"].shape == (2, 16, 32, 3) for b in tap)
    n = 0
    for got, want in zip(DevicePrefetcher(tap, DEV, device_aug=DeviceImageAug(DEV), pick_stream=False), cpu):
        torch.cuda.synchronize()
        assert set(got) == set(want) and got["img"].is_cuda and got["mask"].is_cuda and got["ctx_mask"][0].is_cuda
        _assert_batch_equals(got, want, ("img", "img_orig", "ctx_img", "ctx_img_orig", "intrinsics", "mask", "ctx_mask", "flip"))
        assert got["metadata"] == want["metadata"]
        both = torch.cat([torch.as_tensor(want["mask"]), torch.as_tensor(want["ctx_mask"][0])], 0)
        assert float(both[:, :, 0, :].sum()) > 0 and float(both[:, :, :, -1].sum()) > 0          # rectangles on the border
        ref = F.max_pool2d((both > 0).float(), 17, stride=1, padding=8)
        assert torch.equal(HM.dilate_mask(torch.cat([got["mask"], got["ctx_mask"][0]], 0), 8).cpu(), ref)
        ref = F.max_pool2d((both > 0).float(), 3, stride=1, padding=1)                        # and at a radius that leaves structure at 8 x 16
        assert torch.equal(HM.dilate_mask(torch.cat([got["mask"], got["ctx_mask"][0]], 0), 1).cpu(), ref) and 0 < float(ref.mean()) < 1
        n += 1
    assert n == 2


class _Recording:
    """A loader that keeps a host copy of the first batch it hands over."""

    def __init__(self, inner):
        self.inner, self.first = inner, None

    def __len__(self):
        return len(self.inner)

    def __iter__(self):
        for b in self.inner:
            if self.first is None:
                torch.cuda.synchronize()
                self.first = {k: ([x.detach().cpu().clone() for x in v] if isinstance(v, list) and v and torch.is_tensor(v[0]) else
                                  (v.detach().cpu().clone() if torch.is_tensor(v) else v)) for k, v in b.items()}
            yield b


@pytest.mark.parametrize("project", ["MotionLearningWaymo", "MonoDepth2Waymo", "SupervisedWaymo"])
def test_waymo_projects_train_end_to_end(net_tree, tmp_path, project):
    """get_project_cfg(..., datasets=True) over the tree -> WaymoDepth loader ("taps") -> DevicePrefetcher + DeviceImageAug -> do_train for two steps."""
    from simpledepthestimation_amd.data import DevicePrefetcher
    from simpledepthestimation_amd.data.device_aug import DeviceImageAug
    from simpledepthestimation_amd.engine.loops import do_train
    from simpledepthestimation_amd.modeling import build_model

    def cfg_for(on_device):
        cfg = project_cfg(project, net_tree, 192, 64, 192, on_device=on_device)
        if project != "MotionLearningWaymo":
            cfg.MODEL.DEPTH_NET.ENCODER_NAME = "18"             # the YAML's "18pt" asks for ImageNet weights
        cfg.MODEL.DEVICE = DEV
        cfg.OUTPUT_DIR, cfg.LOG_PERIOD, cfg.SOLVER.MAX_EPOCHS, cfg.TEST.EVAL_PERIOD, cfg.SOLVER.CHECKPOINT_PERIOD = str(tmp_path / "out"), 1, 1, 0, 100
        return cfg
    cpu = seeded_batches(cfg_for(False), 2, seed=21)
    tap = seeded_batches(cfg_for("taps"), 2, seed=21)
    if project == "SupervisedWaymo":             # RandomCrop, no Resize: the frames go up as they are
        assert "device_taps" not in tap[0] and tap[0]["img_u8"].shape == (2, 64, 192, 3)
    else:
        assert tap[0]["img_u8"].shape == (2, 128, 384, 3) and tap[0]["device_taps"][0].shape == (192, 4)
    cfg = cfg_for("taps")
    torch.manual_seed(5)
    model = build_model(cfg)
    before = [p.detach().clone() for p in model.parameters()]
    loader = _Recording(DevicePrefetcher(tap, DEV, device_aug=DeviceImageAug(DEV), pick_stream=False))
    rec = do_train(cfg, model, loader, None)
    torch.cuda.synchronize()
    assert [r["iteration"] for r in rec] == [1, 2] and all(np.isfinite(r["total_loss"]) for r in rec)
    losses = [k for k in rec[0] if k.endswith("_loss") and k != "total_loss"]
    assert losses and all(np.isfinite(r[k]) for r in rec for k in losses)
    grads = [p.grad.flatten() for p in model.parameters() if p.grad is not None]
    flat = torch.cat(grads)
    assert flat.numel() > 1e6 and bool(torch.isfinite(flat).all()) and float(flat.abs().sum()) > 0
    changed = sum(int(not torch.equal(a, p.detach())) for a, p in zip(before, model.parameters()))
    assert changed >= len(grads) // 2 and all(bool(torch.isfinite(p).all()) for p in model.parameters())
    keys = [k for k in cpu[0] if k != "metadata"]
    assert set(loader.first) == set(cpu[0]) and {"img", "img_orig", "intrinsics", "flip"} <= set(keys)
    if project == "MotionLearningWaymo":
        assert {"mask", "ctx_mask", "ctx_img", "ctx_img_orig"} <= set(keys) and len(cpu[0]["ctx_img"]) == 1
    elif project == "MonoDepth2Waymo":
        assert {"ctx_img", "ctx_img_orig"} <= set(keys) and len(cpu[0]["ctx_img"]) == 2
    else:
        assert "depth" in keys and cpu[0]["depth"].shape == (2, 1, 64, 192)
    _assert_batch_equals(loader.first, cpu[0], keys)


@pytest.mark.parametrize("gt_scale", [True, False])
def test_evaluation_over_the_waymo_test_chain(small_tree, gt_scale):
    """MonoDepth2's Waymo test chain (LoadDepth KEEP_ORIG, ClipDepth, CropTopTo, Resize) through inference_on_dataset and the four kitti_evaluators ==
    the numpy restatement on the same predictions: Resize.backward, CropTopTo.backward, Garg window, optional median scaling, the seven metrics."""
    from oracle import evaluation as OE
    from simpledepthestimation_amd.data import build_detection_test_loader
    from simpledepthestimation_amd.evaluation import build_evaluator, inference_on_dataset
    cfg = project_cfg("MonoDepth2Waymo", small_tree, 48, 8, 16)
    cfg.TEST.GT_SCALE = gt_scale
    assert [s["NAME"] for s in cfg.DATASETS.TEST.PREPROCESS] == ["LoadImg", "LoadDepth", "ClipDepth", "CropTopTo", "Resize", "ToTensor"]

    class Stub(torch.nn.Module):
        def forward(self, inputs):
            img = inputs["img"].to(DEV)
            return {"depth_pred": 2.0 + 75.0 * (0.5 * img[:, :1] + 0.3 * img[:, 1:2] + 0.2 * img[:, 2:])}

    loader = build_detection_test_loader(cfg)
    evs = build_evaluator(cfg, None)
    assert len(evs) == 4 and evs[0].preprocess_chain == ["CropTopTo", "Resize"]
    model = Stub()
    res = inference_on_dataset(model, loader, evs)
    assert list(res) == [e.tag for e in evs]
    rows = {e.tag: [] for e in evs}
    with torch.no_grad():
        for b in loader:
            pred = model(b)["depth_pred"][0, 0].cpu().numpy()
            full = loader.dataset.get_prediction({"depth_pred": pred, "metadata": dict(b["metadata"][0])})["depth_pred"]
            gt = b["depth_orig"][0]
            assert full.shape == gt.shape == (56, 96) and not full[:8].any()
            for e in evs:
                r = OE.process_image(full, gt, np.arange(56), np.arange(96), "garg", e.min_depth, e.max_depth, gt_scale)
                if r is not None:
                    rows[e.tag].append(r)
    names = ("abs_rel", "sq_rel", "rms", "log_rms", "d1", "d2", "d3")
    for e in evs:
        assert len(rows[e.tag]) == 9                                    # every frame of the tree has ground truth in every range
        want = np.mean(np.array(rows[e.tag], np.float64), axis=0)
        assert list(res[e.tag]) == list(names)
        np.testing.assert_allclose([res[e.tag][n] for n in names], want[2:], rtol=2e-5, atol=1e-7, err_msg=e.tag)

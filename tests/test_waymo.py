"""CPU: the Waymo data path (data/datasets/waymo.py, LoadMask / LoadLidar, Resize ON_DEVICE: "taps", the Waymo project configs).

Pinned by tests/golden/waymo.npz = what the reference's OWN WaymoDepth class (index, context filter, sample dicts, batch_collator) gives on the
synthetic tree of tests/waymo_tree.py (scripts/gen_golden_waymo.py).  Decoding cannot be run from the reference (cv2): LoadMask / LoadImg / LoadLidar are
pinned by round trips.  The tap-compacted upload is integer index logic: everything is compared with equality."""
import json
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN, _Golden
from simpledepthestimation_amd.config import get_project_cfg
from simpledepthestimation_amd.data import DATASET_REGISTRY, DevicePrefetcher, WaymoDepth, build_detection_test_loader, build_detection_train_loader
from simpledepthestimation_amd.data.preprocess import PREPROCESS_REGISTRY, build_preprocess
from simpledepthestimation_amd.data.preprocess import augmentation as A
from waymo_tree import CASES, SEGMENTS, dataset_cfg, fake_samples, make_waymo_tree, project_cfg, seeded_batches


@pytest.fixture(scope="module")
def gw():
    return _Golden(os.path.join(GOLDEN, "waymo.npz"))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("waymo"))
    return root, make_waymo_tree(root)


def _rel(v, root):
    if isinstance(v, str):
        return os.path.relpath(v, root) if v.startswith(root) else v
    if isinstance(v, list):
        return [_rel(x, root) for x in v]
    if isinstance(v, dict):
        return {str(k): _rel(x, root) for k, x in v.items()}
    return v


def _case(tree, tag):
    kw = dict(CASES[tag])
    if kw.get("MASK_ROOT"):
        kw["MASK_ROOT"] = tree[1][2]
    return kw


# ---------------------------------------------------------------------------------------------------------------- index, samples, collation

@pytest.mark.parametrize("tag", sorted(CASES))
def test_index_context_and_samples_vs_reference(gw, tree, tag):
    root, t = tree
    kw = _case(tree, tag)
    assert DATASET_REGISTRY.get("WaymoDepth") is WaymoDepth
    ds = WaymoDepth(dataset_cfg(t, **kw), None)
    assert [json.dumps([m[0], m[1], {str(k): v for k, v in m[2].items()}], sort_keys=True) for m in ds.metadatas] == list(gw[f"{tag}.metadatas"])
    assert ds.valid_inds == list(gw[f"{tag}.valid_inds"]) and len(ds) == len(gw[f"{tag}.valid_inds"])
    assert [json.dumps(c) for c in ds.context_list] == list(gw[f"{tag}.context"])
    for idx, ctx in enumerate(ds.context_list):                       # a context never crosses a segment
        assert all(ds.metadatas[j][0] == ds.metadatas[idx][0] for j in ctx)
    times = [m[1] for m in ds.metadatas]
    for seg, _, _ in SEGMENTS:                                         # sorted inside each segment although the pickle's keys are not
        own = [x for m, x in zip(ds.metadatas, times) if m[0] == seg]
        assert own == sorted(own) and len(own) > 0
    n = int(gw[f"{tag}.n_items"])
    items = [ds[i] for i in range(n)]
    cams = kw.get("USE_CAMS", ["FRONT"])
    assert all(isinstance(it, list) and len(it) == len(cams) for it in items) and [len(it) for it in items] == list(gw[f"{tag}.n_cams"])
    flat = [d for it in items for d in it]
    assert [json.dumps(_rel(d["metadata"], root), sort_keys=True) for d in flat] == list(gw[f"{tag}.item_meta"])
    K = np.stack([d["intrinsics"] for d in flat])
    assert K.dtype == np.float32 and K.shape[1:] == (3, 3) and np.array_equal(K, gw[f"{tag}.K"])
    for d in flat:
        assert ("mask_dir" in d["metadata"]) == ("ctx_mask_dir" in d["metadata"]) == ("MASK_ROOT" in kw)
        assert d["metadata"]["img_dir"].endswith(".jpg") and d["metadata"]["depth_dir"].endswith(".png") and d["metadata"]["cam"] in cams
        assert len(d["metadata"]["ctx_img_dir"]) == kw.get("FORWARD_CONTEXT", 0) + kw.get("BACKWARD_CONTEXT", 0)
        assert os.path.isfile(d["metadata"]["img_dir"]) and all(os.path.isfile(p) for p in d["metadata"]["ctx_img_dir"])


def test_the_two_stated_deviations(tree):
    _, t = tree
    one = WaymoDepth(dataset_cfg(t, USE_CAMS="FRONT"), None)           # a bare string names one camera (the reference would look up 'F', 'R', ...)
    assert one.use_cams == ["FRONT"] and len(one[0]) == 1 and one[0][0]["metadata"]["cam"] == "FRONT"
    assert WaymoDepth(dataset_cfg(t), None).use_cams == ["FRONT"] and len(WaymoDepth(dataset_cfg(t), None)) == 9
    with pytest.raises(ValueError, match="STRIDE"):
        WaymoDepth(dataset_cfg(t, FORWARD_CONTEXT=1), None)            # STRIDE defaults to 0
    assert len(WaymoDepth(dataset_cfg(t, STRIDE=0), None)) == 9         # without contexts the stride is never read


def test_batch_collator_vs_reference(gw, tree):
    ds = WaymoDepth(dataset_cfg(tree[1]), None)
    b = ds.batch_collator(fake_samples())
    assert sorted(b.keys()) == list(gw["collate.keys"])
    assert [f"{k}:{type(b[k]).__name__}:{type(b[k][0]).__name__ if isinstance(b[k], list) else ''}" for k in sorted(b.keys())] == list(gw["collate.types"])
    for k in ("img", "img_orig", "intrinsics", "depth", "mask"):
        want = gw[f"collate.{k}"]
        assert torch.is_tensor(b[k]) and tuple(b[k].shape) == want.shape and b[k].numpy().dtype == want.dtype and np.array_equal(b[k].numpy(), want), k
    assert b["mask"].shape == (6, 1, 4, 6) and b["depth"].shape == (6, 1, 4, 6) and b["img"].shape == (6, 3, 4, 6)          # 3 samples x 2 cameras
    for k in ("ctx_img", "ctx_img_orig", "ctx_depth", "ctx_mask"):
        assert isinstance(b[k], list) and len(b[k]) == int(gw[f"collate.{k}.n"])
        for i, a in enumerate(b[k]):
            want = gw[f"collate.{k}.{i}"]
            assert isinstance(a, np.ndarray) and a.shape == want.shape and a.dtype == want.dtype and np.array_equal(a, want), (k, i)
    assert b["ctx_mask"][0].shape == (6, 1, 4, 6) and b["ctx_img"][0].shape == (6, 3, 4, 6)
    assert b["flip"] is True and bool(gw["collate.flip"]) is True                                     # the first sample's
    assert [json.dumps(m, sort_keys=True) for m in b["metadata"]] == list(gw["collate.metadata"]) and len(b["depth_orig"]) == int(gw["collate.depth_orig.n"])


def _raw_sample(r, shape, taps=None, nctx=1):
    d = {"img_u8": r.integers(0, 256, shape + (3,), dtype=np.uint8), "ctx_img_u8": [r.integers(0, 256, shape + (3,), dtype=np.uint8) for _ in range(nctx)],
         "aug_params": r.random(8).astype(np.float32), "device_resize": (4, 6), "flip": False, "intrinsics": np.eye(3, dtype=np.float32)}
    if taps is not None:
        d["device_taps"] = taps
    return d


def test_batch_collator_on_device_entries(tree):
    """Frames of one size are stacked in the worker (with ONE table pair), frames of different sizes -- or of one size but two tables -- stay lists."""
    ds = WaymoDepth(dataset_cfg(tree[1]), None)
    r = np.random.default_rng(0)
    tabs = lambda H, W: (A.compact_taps(W, 6)[1], A.compact_taps(H, 4)[1])
    same = [[_raw_sample(r, (8, 12), tabs(24, 36)), _raw_sample(r, (8, 12), tabs(24, 36))], [_raw_sample(r, (8, 12), tabs(24, 36))]]
    b = ds.batch_collator(same)
    assert torch.is_tensor(b["img_u8"]) and b["img_u8"].shape == (3, 8, 12, 3) and b["img_u8"].dtype == torch.uint8
    assert isinstance(b["ctx_img_u8"], list) and b["ctx_img_u8"][0].shape == (3, 8, 12, 3) and b["aug_params"].shape == (3, 8)
    assert np.array_equal(b["img_u8"][1].numpy(), same[0][1]["img_u8"]) and np.array_equal(b["ctx_img_u8"][0][2].numpy(), same[1][0]["ctx_img_u8"][0])
    xt, yt = b["device_taps"]
    assert torch.is_tensor(xt) and xt.dtype == torch.int32 and xt.shape == (6, 4) and yt.shape == (4, 4)
    assert np.array_equal(xt.numpy(), tabs(24, 36)[0]) and np.array_equal(yt.numpy(), tabs(24, 36)[1])
    plain = ds.batch_collator([[_raw_sample(r, (8, 12))], [_raw_sample(r, (8, 12))]])
    assert torch.is_tensor(plain["img_u8"]) and "device_taps" not in plain
    mixed = ds.batch_collator([[_raw_sample(r, (8, 12), tabs(24, 36))], [_raw_sample(r, (8, 11), tabs(24, 33))]])
    assert isinstance(mixed["img_u8"], list) and mixed["img_u8"][1].shape == (8, 11, 3) and isinstance(mixed["ctx_img_u8"][0], list)
    assert isinstance(mixed["device_taps"], list) and len(mixed["device_taps"]) == 2 and np.array_equal(mixed["device_taps"][1][0], tabs(24, 33)[0])
    # one compacted shape from two source heights (28 and 32 rows both keep 8): the tables differ, so nothing may be stacked under one pair
    assert A.compact_taps(28, 4)[0].size == A.compact_taps(32, 4)[0].size == 8 and not np.array_equal(A.compact_taps(28, 4)[1], A.compact_taps(32, 4)[1])
    two = ds.batch_collator([[_raw_sample(r, (8, 12), tabs(28, 36))], [_raw_sample(r, (8, 12), tabs(32, 36))]])
    assert isinstance(two["img_u8"], list) and isinstance(two["device_taps"], list) and np.array_equal(two["device_taps"][1][1], tabs(32, 36)[1])
    # and the KITTI reader's collator carries the same additions
    kb = DATASET_REGISTRY.get("KittiDepthV2").batch_collator(None, [s[0] for s in same])
    assert torch.is_tensor(kb["img_u8"]) and kb["img_u8"].shape == (2, 8, 12, 3) and np.array_equal(kb["device_taps"][0].numpy(), tabs(24, 36)[0])


# ---------------------------------------------------------------------------------------------------------------- loading

def test_load_mask_img_lidar_round_trips(tmp_path):
    from PIL import Image
    assert {"LoadMask", "LoadLidar"} <= set(PREPROCESS_REGISTRY._obj_map) if hasattr(PREPROCESS_REGISTRY, "_obj_map") else True
    r = np.random.default_rng(4)
    m8, m16 = r.integers(0, 256, (9, 13), dtype=np.uint8), r.integers(0, 65536, (9, 13)).astype(np.uint16)
    m16[0, 0], m16[0, 1] = 65535, 256
    Image.fromarray(m8).save(tmp_path / "m8.png"); Image.fromarray(m16).save(tmp_path / "m16.png")
    d = build_preprocess({"NAME": "LoadMask"}).forward({"metadata": {"mask_dir": str(tmp_path / "m8.png"), "ctx_mask_dir": [str(tmp_path / "m16.png"), str(tmp_path / "m8.png")]}})
    assert d["mask"].dtype == np.float32 and d["mask"].shape == (9, 13) and np.array_equal(d["mask"], m8.astype(np.float32))
    assert len(d["ctx_mask"]) == 2 and d["ctx_mask"][0].dtype == np.float32 and np.array_equal(d["ctx_mask"][0], m16.astype(np.float32)) and np.array_equal(d["ctx_mask"][1], d["mask"])
    none = build_preprocess({"NAME": "LoadMask"}).forward({"metadata": {"mask_dir": str(tmp_path / "m8.png"), "ctx_mask_dir": []}})
    assert none["ctx_mask"] == []
    missing = str(tmp_path / "nope.png")
    with pytest.raises(AssertionError, match="does not exist"):
        build_preprocess({"NAME": "LoadMask"}).forward({"metadata": {"mask_dir": missing, "ctx_mask_dir": []}})
    with pytest.raises(AssertionError, match="does not exist"):
        build_preprocess({"NAME": "LoadImg"}).forward({"metadata": {"img_dir": str(tmp_path / "nope.jpg")}})
    # JPEG: LoadImg returns what Pillow decodes (parity with cv2's decoder is not pinned)
    y, x = np.mgrid[0:24, 0:40]
    rgb = np.stack([(7 * y + x) % 256, (3 * x + 100) % 256, (5 * y + 2 * x) % 256], -1).astype(np.uint8)
    Image.fromarray(rgb).save(tmp_path / "f.jpg", quality=90)
    with Image.open(tmp_path / "f.jpg") as im:
        want = np.asarray(im.convert("RGB")).copy()
    d = build_preprocess({"NAME": "LoadImg", "WITH_CTX": True}).forward({"metadata": {"img_dir": str(tmp_path / "f.jpg"), "ctx_img_dir": [str(tmp_path / "f.jpg")]}})
    assert d["img"].dtype == np.uint8 and d["img"].shape == (24, 40, 3) and np.array_equal(d["img"], want) and np.array_equal(d["ctx_img"][0], want)
    assert np.abs(want.astype(int) - rgb.astype(int)).mean() < 8                     # and it is the picture that was written, up to JPEG's loss
    # lidar
    scan = r.normal(size=(17, 4)).astype(np.float32)
    scan.tofile(tmp_path / "s.bin")
    md = {"metadata": {"lidar_dir": str(tmp_path / "s.bin"), "ctx_lidar_dir": [str(tmp_path / "s.bin")]}}
    d = build_preprocess({"NAME": "LoadLidar", "LOAD_DIM": 4, "USE_DIM": 3}).forward({"metadata": dict(md["metadata"])})
    assert d["lidar"].dtype == np.float32 and np.array_equal(d["lidar"], scan[:, :3]) and "ctx_lidar" not in d
    d = build_preprocess({"NAME": "LoadLidar", "LOAD_DIM": 4, "USE_DIM": [0, 1, 3], "WITH_CTX": True}).forward({"metadata": dict(md["metadata"])})
    assert np.array_equal(d["lidar"], scan[:, [0, 1, 3]]) and len(d["ctx_lidar"]) == 1 and np.array_equal(d["ctx_lidar"][0], scan[:, [0, 1, 3]])
    assert np.array_equal(build_preprocess({"NAME": "LoadLidar"}).forward({"metadata": dict(md["metadata"])})["lidar"], scan[:, :3])          # the defaults: 4 and 3
    with pytest.raises(NotImplementedError):
        build_preprocess({"NAME": "LoadLidar"}).forward({"metadata": {"lidar_dir": str(tmp_path / "s.npy")}})


# ---------------------------------------------------------------------------------------------------------------- tap compaction

def _resize_with_tables(img, xtab, ytab):
    """resize_linear_u8's arithmetic (and sde_image_prep_u8's resize_px) reading the source through given [dst][4] tables."""
    x0, x1, a0, a1 = (xtab[:, i].astype(np.int64) for i in range(4))
    y0, y1, b0, b1 = (ytab[:, i].astype(np.int64) for i in range(4))
    src = img.astype(np.int64)
    rows = src[:, x0, :] * a0[None, :, None] + src[:, x1, :] * a1[None, :, None]
    out = (((b0[:, None, None] * (rows[y0] >> 4)) >> 16) + ((b1[:, None, None] * (rows[y1] >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def _taps_sample(r, H, W, nctx=1):
    return {"img": r.integers(0, 256, (H, W, 3), dtype=np.uint8), "ctx_img": [r.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(nctx)],
            "intrinsics": np.array([[2055.0, 0, W / 2], [0, 2050.0, H / 2], [0, 0, 1]], np.float32), "metadata": {},
            "mask": (r.random((H, W)) < 0.3).astype(np.float32), "depth": np.where(r.random((H, W)) < 0.2, r.random((H, W)) * 70, 0).astype(np.float32)}


def _clone(d):
    return {k: (v.copy() if isinstance(v, np.ndarray) else ([a.copy() for a in v] if isinstance(v, list) else dict(v))) for k, v in d.items()}


# source (H, W) -> destination (h, w); compacts: whether any row or column can be dropped
TAP_CASES = [((1152, 1920), (192, 320), True), ((768, 1920), (192, 480), True), ((375, 375), (192, 192), False), ((56, 96), (8, 16), True),
             ((53, 53), (7, 7), True), ((7, 7), (20, 20), False), ((375, 96), (192, 16), True), ((40, 97), (10, 24), True)]


@pytest.mark.parametrize("src,dst,compacts", TAP_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_tap_compacted_frames_resize_to_the_same_bytes(src, dst, compacts):
    (H, W), (h, w) = src, dst
    r = np.random.default_rng(H * 7 + W)
    s = _taps_sample(r, H, W)
    plain = build_preprocess({"NAME": "Resize", "IMG_H": h, "IMG_W": w, "ON_DEVICE": True}).forward(_clone(s))
    step = build_preprocess({"NAME": "Resize", "IMG_H": h, "IMG_W": w, "ON_DEVICE": "taps"})
    got = step.forward(_clone(s))
    got2 = step.forward(_clone(s))                                     # the step caches its tables per source size: a second frame gets the same
    # everything but the frames is what ON_DEVICE: True gives
    for k in ("intrinsics", "mask", "depth"):
        assert np.array_equal(got[k], plain[k]), k
    assert got["metadata"] == plain["metadata"] == {"h_before_resize": H, "w_before_resize": W} and tuple(got["device_resize"]) == (h, w)
    if not compacts:
        assert "device_taps" not in got and np.array_equal(got["img"], s["img"]) and np.array_equal(got["ctx_img"][0], s["ctx_img"][0])
        assert set(got) == set(plain)
        return
    xtab, ytab = got["device_taps"]
    assert xtab.dtype == np.int32 and ytab.dtype == np.int32 and xtab.shape == (w, 4) and ytab.shape == (h, 4)
    ch, cw = got["img"].shape[:2]
    assert ch <= min(H, 2 * h) and cw <= min(W, 2 * w) and (ch < H or cw < W) and got["ctx_img"][0].shape == got["img"].shape
    assert 0 <= xtab[:, :2].min() and xtab[:, :2].max() == cw - 1 and 0 <= ytab[:, :2].min() and ytab[:, :2].max() == ch - 1
    for axis_src, axis_dst, tab in ((W, w, xtab), (H, h, ytab)):        # weights untouched, taps renumbered monotonically
        s0, s1, w0, w1 = A._linear_coefs(axis_src, axis_dst)
        used = np.unique(np.concatenate([s0, s1]))
        assert np.array_equal(tab[:, 2], w0) and np.array_equal(tab[:, 3], w1) and np.array_equal(used[tab[:, 0]], s0) and np.array_equal(used[tab[:, 1]], s1)
    for full, cut in ((s["img"], got["img"]), (s["ctx_img"][0], got["ctx_img"][0])):
        assert np.array_equal(_resize_with_tables(cut, xtab, ytab), A.resize_linear_u8(full, w, h))
    assert np.array_equal(got2["img"], got["img"]) and np.array_equal(got2["device_taps"][0], xtab) and np.array_equal(got2["device_taps"][1], ytab)
    assert set(got) == set(plain) | {"device_taps"}


def test_waymo_reductions_keep_one_ninth_and_one_quarter():
    """The arithmetic the mode exists for: 1152 x 1920 -> 192 x 320 reads 384 x 640 source pixels, 768 x 1920 -> 192 x 480 reads 384 x 960."""
    assert A.compact_taps(1152, 192)[0].size == 384 and A.compact_taps(1920, 320)[0].size == 640 and A.compact_taps(768, 192)[0].size == 384
    assert A.compact_taps(1920, 480)[0].size == 960 and A.compact_taps(375, 192)[0].size == 375 and A.compact_taps(7, 20)[0].size == 7


def test_true_and_false_are_untouched_by_the_new_mode():
    r = np.random.default_rng(9)
    s = _taps_sample(r, 56, 96)
    host = build_preprocess({"NAME": "Resize", "IMG_H": 8, "IMG_W": 16}).forward(_clone(s))
    assert host["img"].shape == (8, 16, 3) and np.array_equal(host["img"], A.resize_linear_u8(s["img"], 16, 8)) and "device_resize" not in host and "device_taps" not in host
    dev = build_preprocess({"NAME": "Resize", "IMG_H": 8, "IMG_W": 16, "ON_DEVICE": True}).forward(_clone(s))
    assert np.array_equal(dev["img"], s["img"]) and "device_taps" not in dev and tuple(dev["device_resize"]) == (8, 16)


def _chain(on_device, h=8, w=16, jitter_prob=1.0):
    extra = {"ON_DEVICE": on_device} if on_device else {}
    return [build_preprocess(dict(NAME="Resize", IMG_H=h, IMG_W=w, **extra)), build_preprocess(dict(NAME="RandomFlip")),
            build_preprocess(dict(NAME="RandomImageAug", JITTER_PROB=jitter_prob, **extra)), build_preprocess(dict(NAME="ToTensor"))]


def _run(chain, sample, seed):
    random.seed(seed); torch.manual_seed(seed); np.random.seed(seed)
    d = _clone(sample)
    for p in chain:
        d = p.forward(d)
    return d


def test_taps_chain_draws_the_same_random_numbers_as_the_cpu_chain():
    r = np.random.default_rng(3)
    s = _taps_sample(r, 48, 96, nctx=2)
    for seed in range(6):
        cpu, dev, tap = _run(_chain(False), s, seed), _run(_chain(True), s, seed), _run(_chain("taps"), s, seed)
        assert cpu["flip"] == dev["flip"] == tap["flip"] and np.array_equal(cpu["intrinsics"], tap["intrinsics"]) and cpu["metadata"] == tap["metadata"]
        assert np.array_equal(tap["aug_params"], dev["aug_params"]) and np.array_equal(tap["mask"], cpu["mask"])
        assert "img" not in tap and tap["img_u8"].shape == (16, 32, 3) and tap["img_u8"].flags["C_CONTIGUOUS"] and len(tap["ctx_img_u8"]) == 2
        assert dev["img_u8"].shape == (48, 96, 3) and "device_taps" not in dev and tuple(tap["device_resize"]) == (8, 16)
        aug = _chain(False)[2]
        random.seed(seed); torch.manual_seed(seed)
        _ = random.random() > 0.5                                     # RandomFlip's draw
        assert random.random() < 1.0
        aug.get_params()
        assert np.allclose(tap["aug_params"], [aug.b, aug.c, aug.s, aug.h] + [float(i) for i in aug.fn_idx], rtol=0, atol=0)
        # and the frames the device would produce from the cut-down upload are the CPU chain's un-jittered ones
        xtab, ytab = tap["device_taps"]
        assert torch.equal(torch.from_numpy(_resize_with_tables(tap["img_u8"], xtab, ytab)).permute(2, 0, 1).float().div(255), cpu["img_orig"])
        assert torch.equal(torch.from_numpy(_resize_with_tables(tap["ctx_img_u8"][1], xtab, ytab)).permute(2, 0, 1).float().div(255), cpu["ctx_img_orig"][1])
    assert _run(_chain("taps", jitter_prob=0.0), s, 1)["aug_params"][4] < 0


# ---------------------------------------------------------------------------------------------------------------- configs

def _flat(d, prefix=""):
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(_flat(v, prefix + k + "."))
        else:
            out[prefix + k] = tuple(v) if isinstance(v, (list, tuple)) and not (v and isinstance(v[0], dict)) else v
    return out


def _yaml_chain(project):
    """The reference's resnet18_waymo.yaml merged over its Base_waymo.yaml, from the parsed mappings under tests/golden/."""
    import yaml
    from simpledepthestimation_amd.config import get_cfg
    with open(os.path.join(GOLDEN, "configs.json")) as f:
        stored = json.load(f)
    with open(os.path.join(GOLDEN, "configs_waymo.json")) as f:
        stored.update(json.load(f))
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("Base_waymo.yaml", "resnet18_waymo.yaml"):
            with open(os.path.join(tmp, name), "w") as f:
                f.write(yaml.safe_dump(stored[f"{project}/{name}"], sort_keys=False))
        cfg = get_cfg()
        cfg.set_new_allowed(True)
        cfg.merge_from_file(os.path.join(tmp, "resnet18_waymo.yaml"))
    return cfg


@pytest.mark.parametrize("name,project", [("MotionLearningWaymo", "MotionLearning"), ("MonoDepth2Waymo", "MonoDepth2"), ("SupervisedWaymo", "Supervised")])
def test_embedded_waymo_projects_equal_the_yaml_chain(name, project):
    from simpledepthestimation_amd.config.defaults import PROJECT_BASE, PROJECT_DATASETS
    ref = _yaml_chain(project)
    want = _flat(ref)
    embedded = dict(PROJECT_BASE[name], DATASETS=PROJECT_DATASETS[name])
    checked = 0
    for k, v in _flat(embedded).items():
        if k.endswith(".PREPROCESS"):
            node = ref
            for part in k.split(".")[:-1]:
                node = node[part]
            assert [dict(s) for s in node.PREPROCESS] == [dict(s) for s in v], k
        else:
            assert k in want and want[k] == v, (k, want.get(k), v)
        checked += 1
    assert checked >= 25
    cfg = get_project_cfg(name, datasets=True)
    got = _flat(cfg)
    for split in ("TRAIN", "TEST"):                   # every key the YAML gives a dataset block is embedded, with its value
        for k, v in ref.DATASETS[split].items():
            if k == "PREPROCESS":
                assert [dict(s) for s in cfg.DATASETS[split].PREPROCESS] == [dict(s) for s in v]
            elif k not in ("IMG_WIDTH", "IMG_HEIGHT"):
                assert got[f"DATASETS.{split}.{k}"] == (tuple(v) if isinstance(v, (list, tuple)) else v), (split, k)
    for k in ("MODEL", "LOSS", "SOLVER", "TEST"):
        assert _flat(cfg[k]) == _flat(ref[k]), k
    assert tuple(cfg.EVALUATORS) == tuple(ref.EVALUATORS) and cfg.LOG_PERIOD == ref.LOG_PERIOD
    assert cfg.DATASETS.TRAIN.NAME == "WaymoDepth" and cfg.DATASETS.TEST.NAME == "WaymoDepth"
    assert ("MASK_ROOT" in cfg.DATASETS.TRAIN) == (name == "MotionLearningWaymo") and "MASK_ROOT" not in cfg.DATASETS.TEST


def test_datasets_are_merged_only_when_asked():
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.config.defaults import PROJECT_BASE
    plain, with_ds = get_project_cfg("MotionLearningWaymo"), get_project_cfg("MotionLearningWaymo", datasets=True)
    assert _flat(plain.DATASETS) == _flat(get_cfg().DATASETS) and plain.DATASETS.TRAIN.NAME == "" and "DATASETS" not in PROJECT_BASE["MotionLearningWaymo"]
    for k in plain:
        if k != "DATASETS":
            assert plain[k] == with_ds[k], k
    assert [s["NAME"] for s in with_ds.DATASETS.TRAIN.PREPROCESS] == ["LoadImg", "LoadMask", "CropTopTo", "Resize", "RandomFlip", "RandomImageAug", "ToTensor"]
    with_ds.DATASETS.TRAIN.PREPROCESS[0]["NAME"] = "x"                 # a copy: the table is not written through
    assert get_project_cfg("MotionLearningWaymo", datasets=True).DATASETS.TRAIN.PREPROCESS[0]["NAME"] == "LoadImg"
    with pytest.raises(KeyError):
        get_project_cfg("MonoDepth2", datasets=True)                  # the KITTI projects embed no dataset block


# ---------------------------------------------------------------------------------------------------------------- loaders

def _seg_index(md):
    return [s[0] for s in SEGMENTS].index(md["segment"])


def test_train_loader_contract_over_the_tree(tree):
    """MotionLearning's Waymo chain (LoadImg+ctx, LoadMask, CropTopTo, Resize, RandomFlip, RandomImageAug, ToTensor) at 56 x 96 -> crop 48 -> 8 x 16."""
    _, t = tree
    cfg = project_cfg("MotionLearningWaymo", t, 48, 8, 16)
    tl = build_detection_train_loader(cfg)
    assert isinstance(tl.dataset, WaymoDepth) and len(tl.dataset) == 7 and len(tl) == 3          # 4 + 3 frames have a successor in their segment; drop_last
    batches = list(tl)
    b = batches[0]
    assert b["img"].shape == (2, 3, 8, 16) and b["img"].dtype == torch.float32 and 0 <= float(b["img"].min()) and float(b["img"].max()) <= 1
    assert b["img_orig"].shape == (2, 3, 8, 16) and isinstance(b["ctx_img"], list) and len(b["ctx_img"]) == 1 and b["ctx_img"][0].shape == (2, 3, 8, 16)
    assert b["ctx_img_orig"][0].shape == (2, 3, 8, 16) and b["ctx_img"][0].dtype == np.float32
    assert torch.is_tensor(b["mask"]) and b["mask"].shape == (2, 1, 8, 16) and b["mask"].dtype == torch.float32 and float(b["mask"].max()) > 0
    assert isinstance(b["ctx_mask"], list) and len(b["ctx_mask"]) == 1 and b["ctx_mask"][0].shape == (2, 1, 8, 16) and b["ctx_mask"][0].dtype == np.float32
    assert b["intrinsics"].shape == (2, 3, 3) and b["intrinsics"].dtype == torch.float32 and isinstance(b["flip"], bool) and len(b["metadata"]) == 2
    for i, md in enumerate(b["metadata"]):
        si = _seg_index(md)                     # the tree's K: fx = 2055.5 + 3.25 si, cx = 48 + 1.5 si, cy = 28 - 2.25 si; crop takes 8 rows, then x 16/96, y 8/48
        K = np.array([[np.float32(2055.5 + 3.25 * si), 0, np.float32(48 + 1.5 * si)], [0, np.float32(2055.5 + 3.25 * si), np.float32(28 - 2.25 * si)], [0, 0, 1]], np.float32)
        K[1, 2] -= 8
        K[0, 0] *= 16 / 96; K[0, 2] *= 16 / 96; K[1, 1] *= 8 / 48; K[1, 2] *= 8 / 48
        assert np.array_equal(b["intrinsics"][i].numpy(), K), (i, b["intrinsics"][i], K)
        assert (md["crop_y_start"], md["h_before_crop"], md["w_before_crop"], md["h_before_resize"], md["w_before_resize"]) == (8, 56, 96, 48, 96)
        # the mask is the file's rectangles, cropped and nearest-resized
        want = A.resize_nearest(__import__("simpledepthestimation_amd.data.preprocess.loading", fromlist=["x"]).read_mask_png(md["mask_dir"])[8:], 16, 8)
        assert np.array_equal(b["mask"][i, 0].numpy(), want)
    from simpledepthestimation_amd.engine.trainer import HipTrainer
    assert HipTrainer._kind(b["mask"]) == "array" and HipTrainer._kind(b["ctx_mask"]) == "arrays" and HipTrainer._kind(b["metadata"]) == "opaque"
    # two cameras: the camera dimension goes into the batch (first segment only: the second has one camera)
    cfg2 = project_cfg("MotionLearningWaymo", t, 48, 8, 16)
    cfg2.DATASETS.TRAIN.USE_CAMS = ["FRONT", "FRONT_LEFT"]
    ds2 = WaymoDepth(cfg2.DATASETS.TRAIN, cfg2)
    b2 = ds2.batch_collator([ds2[0], ds2[1]])
    assert b2["img"].shape == (4, 3, 8, 16) and b2["mask"].shape == (4, 1, 8, 16) and [m["cam"] for m in b2["metadata"]] == ["FRONT", "FRONT_LEFT"] * 2


def test_test_loader_contract_and_backward_maps(tree):
    """MonoDepth2's Waymo test chain: LoadImg, LoadDepth KEEP_ORIG, ClipDepth, CropTopTo, Resize, ToTensor."""
    _, t = tree
    cfg = project_cfg("MonoDepth2Waymo", t, 48, 8, 16)
    te = build_detection_test_loader(cfg)
    tb = list(te)
    assert len(tb) == len(te.dataset) == 9 and tb[0]["img"].shape == (1, 3, 8, 16) and tb[0]["depth"].shape == (1, 1, 8, 16)
    assert isinstance(tb[0]["depth_orig"], list) and tb[0]["depth_orig"][0].shape == (56, 96) and float(tb[0]["depth_orig"][0].max()) > 80 >= float(tb[0]["depth"].max())
    md = tb[0]["metadata"][0]
    assert (md["crop_y_start"], md["h_before_crop"], md["w_before_crop"], md["h_before_resize"], md["w_before_resize"]) == (8, 56, 96, 48, 96)
    assert [m["metadata"][0]["frame_time"] for m in tb[:5]] == sorted(m["metadata"][0]["frame_time"] for m in tb[:5])          # InferenceSampler: dataset order
    pred = te.dataset.get_prediction({"depth_pred": np.arange(128, dtype=np.float32).reshape(8, 16) + 1, "metadata": md})["depth_pred"]
    assert pred.shape == (56, 96) and not pred[:8].any() and pred[8:].all() and pred[8, 0] == 1 and pred[-1, -1] == 128
    # Supervised's Waymo chains: RandomCrop instead of Resize in training, full-size crop at test
    cfg = project_cfg("SupervisedWaymo", t, 48, 32, 64)
    b = next(iter(build_detection_train_loader(cfg)))
    assert b["img"].shape == (2, 3, 32, 64) and b["depth"].shape == (2, 1, 32, 64) and "ctx_img" not in b and "mask" not in b
    sb = next(iter(build_detection_test_loader(cfg)))
    assert sb["img"].shape == (1, 3, 48, 96) and sb["depth"].shape == (1, 1, 48, 96) and sb["depth_orig"][0].shape == (56, 96)


def test_taps_loader_and_the_prefetcher_pass_through(tree):
    """The three train chains draw the same batches; under "taps" the frames arrive cut down with one table pair, and DevicePrefetcher hands `mask`,
    `ctx_mask` and `device_taps` over unchanged in value."""
    _, t = tree
    cpu = seeded_batches(project_cfg("MotionLearningWaymo", t, 48, 8, 16), 2, seed=5)
    dev = seeded_batches(project_cfg("MotionLearningWaymo", t, 48, 8, 16, on_device=True), 2, seed=5)
    tap = seeded_batches(project_cfg("MotionLearningWaymo", t, 48, 8, 16, on_device="taps"), 2, seed=5)
    for c, d, p in zip(cpu, dev, tap):
        assert [m["img_dir"] for m in c["metadata"]] == [m["img_dir"] for m in p["metadata"]] and c["flip"] == d["flip"] == p["flip"]
        assert torch.equal(c["mask"], p["mask"]) and np.array_equal(c["ctx_mask"][0], p["ctx_mask"][0]) and torch.equal(c["intrinsics"], p["intrinsics"])
        assert torch.equal(d["aug_params"], p["aug_params"]) and d["img_u8"].shape == (2, 48, 96, 3) and p["img_u8"].shape == (2, 16, 32, 3)
        assert "device_taps" not in d and "device_taps" not in c and p["ctx_img_u8"][0].shape == (2, 16, 32, 3)
        xt, yt = (x.numpy() for x in p["device_taps"])
        for i in range(2):
            got = torch.from_numpy(_resize_with_tables(p["img_u8"][i].numpy(), xt, yt)).permute(2, 0, 1).float().div(255)
            assert torch.equal(got, c["img_orig"][i])
            got = torch.from_numpy(_resize_with_tables(p["ctx_img_u8"][0][i].numpy(), xt, yt)).permute(2, 0, 1).float().div(255)
            assert np.array_equal(got.numpy(), c["ctx_img_orig"][0][i])
    pf = list(DevicePrefetcher(tap, "cpu"))
    assert len(pf) == 2
    for a, b in zip(pf, tap):
        assert torch.equal(a["mask"], b["mask"]) and isinstance(a["ctx_mask"], list) and np.array_equal(np.asarray(a["ctx_mask"][0]), b["ctx_mask"][0])
        assert a["device_taps"] is b["device_taps"] and torch.equal(a["img_u8"], b["img_u8"]) and a["metadata"] == b["metadata"]

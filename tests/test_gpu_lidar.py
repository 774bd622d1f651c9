"""GPU: sde_lidar_depth against the float64 restatement of lidar_ref.py, every case into an output buffer pre-filled with NaN (an element the
kernel leaves unwritten fails the finiteness check) with guard elements around it.  Exact cases use unambiguous inputs (lidar_ref's docstring:
occupancy equal, values within 8 * 2^-24 * sum |m2k p_k| at the winning point, bit-equal with vel_depth); `borders` and `rejects` use inputs
that are exact in float32, so nothing is ambiguous there; the robustness case takes unfiltered points and checks what holds for them."""
import functools

import numpy as np
import pytest
import torch

import lidar_ref as LR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64


def run(points, counts, projs, origins, H, W, **kw):
    """points: list of [n_b, 3 or 4] arrays (padded to a common cap, or kw['cap']) -> [B,H,W] float32 numpy; checks the guards."""
    from simpledepthestimation_amd.hip.lidar import lidar_depth
    cap = kw.pop("cap", None) or max(1, max(len(p) for p in points))
    stride = points[0].shape[1]
    B = len(points)
    host = np.full((B, cap, stride), np.nan, np.float32)          # rows behind count[b] hold NaN: reading them would show
    for b, p in enumerate(points):
        host[b, :len(p)] = p
    buf = torch.full((GUARD + B * H * W + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    out = buf[GUARD:GUARD + B * H * W].view(B, 1, H, W)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(DEV)
    got = lidar_depth(up(host, np.float32), up(counts, np.int32), up(projs, np.float32), up(origins, np.int32), H, W, out=out, **kw)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (B, 1, H, W)
    raw = buf.cpu().numpy()
    assert np.isnan(raw[:GUARD]).all() and np.isnan(raw[-GUARD:]).all(), "elements outside the output were written"
    return raw[GUARD:-GUARD].reshape(B, H, W).copy()


@functools.lru_cache(maxsize=None)
def ragged_inputs():
    proj = LR.kitti_proj()
    p, share = LR.unambiguous(40, 72000, proj, (0, 0), 37, 61)          # one draw, one dropped share, cut into the three scans
    assert len(p) >= 1 + 257 + 70001
    return proj, [p[:1], p[1:258], p[258:258 + 70001]], share


def test_empty_and_single():
    proj = LR.kitti_proj()
    p, _ = LR.unambiguous(7, 40, proj, (0, 0), 3, 4, margin=0.0)
    inside = [q for q in p if LR.reference(q[None], proj, (0, 0), 3, 4)[0].any()]
    got = run([np.zeros((0, 3), np.float32), inside[0][None]], [0, 1], [proj, proj], [(0, 0), (0, 0)], 3, 4, cap=5)
    assert not got[0].any() and (got[1] != 0).sum() == 1
    LR.compare(got[1], inside[0][None], proj, (0, 0), tag="single")


def test_collisions():
    proj = LR.kitti_proj()
    pts, dropped = LR.unambiguous(2, 3000, proj, (0, 0), 5, 7)
    assert dropped <= LR.MAX_DROPPED
    got = run([pts], [len(pts)], [proj], [(0, 0)], 5, 7, front_only=False)
    ref = LR.compare(got[0], pts, proj, (0, 0), front_only=False, tag="collisions")
    assert (ref != 0).all()              # 35 pixels, about 60 candidates each


@pytest.mark.parametrize("stride", [3, 4])
def test_ragged_batch_and_reproducible(stride):
    proj, pts, share = ragged_inputs()
    assert share <= LR.MAX_DROPPED
    feed = [p if stride == 3 else np.concatenate([p, np.full((len(p), 1), np.nan, np.float32)], 1) for p in pts]      # the fourth column is never read
    args = (feed, [1, 257, 70001], [proj] * 3, [(0, 0)] * 3, 37, 61)
    got = run(*args, cap=70016, front_only=False)
    for b in range(3):
        LR.compare(got[b], pts[b], proj, (0, 0), front_only=False, tag=f"ragged[{b}] stride {stride}")
    assert (got[2] != 0).sum() > 2000
    again = run(*args, cap=70016, front_only=False)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


def test_window_is_a_slice_of_the_full_map():
    proj = LR.kitti_proj()
    pts, dropped = LR.unambiguous(9, 6000, proj, (0, 0), 32, 64)
    assert dropped <= LR.MAX_DROPPED
    full = run([pts], [len(pts)], [proj], [(0, 0)], 32, 64)[0]
    LR.compare(full, pts, proj, (0, 0), tag="window: full map")
    win = run([pts, pts], [len(pts)] * 2, [proj] * 2, [(13, 5), (0, 24)], 8, 16)
    assert np.array_equal(win[0].view(np.uint32), full[5:13, 13:29].view(np.uint32)) and (win[0] != 0).sum() > 60
    assert np.array_equal(win[1].view(np.uint32), full[24:32, 0:16].view(np.uint32))


def test_borders_half_even_and_the_one_based_offset():
    """proj maps (x, y, z) to (u, v, w) = (x, y, z); the points are (c z, r z, z) with z a power of two, so u / w = c and v / w = r exactly."""
    H, W = 4, 6
    proj = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
    cols = [0.0, 1.0, float(W), W + 1.0, 0.5, 1.5, 2.5, 3.5, W + 0.5]          # rint - 1 -> -1, 0, W-1, W, (0.5 -> 0) -1, (1.5 -> 2) 1, (2.5 -> 2) 1, (3.5 -> 4) 3, (6.5 -> 6) 5
    rows = [0.0, 1.0, float(H), H + 1.0, 0.5, 1.5, 2.5, 3.5, H + 0.5]
    pts = np.array([(c * z, r * z, z) for z in (2.0, 4.0) for c in cols for r in rows], np.float32)
    got = run([pts], [len(pts)], [proj], [(0, 0)], H, W, front_only=False)[0]
    ref, _ = LR.reference(pts, proj, (0, 0), H, W, front_only=False)
    want_cols, want_rows = {0, W - 1, 1, 3, 5}, {0, H - 1, 1, 3}
    occupied = np.argwhere(got != 0)
    assert set(occupied[:, 1]) == want_cols and set(occupied[:, 0]) == want_rows
    assert np.array_equal(got, ref.astype(np.float32)) and set(np.unique(got)) == {0.0, 2.0}


def test_rejects():
    proj = np.array([[1, 0, 2, 0], [0, 1, 2, 0], [0, 0, 1, 0]], np.float32)      # pixel = (x / z + 2, y / z + 2) - 1, depth z
    nan, inf = np.nan, np.inf
    pts = np.array([(nan, 0, 1), (0, nan, 1), (0, 0, nan), (inf, 0, 1), (0, -inf, 1), (0, 0, inf), (0, 0, -inf),      # non-finite coordinates
                    (0, 0, 0), (0, 0, -1), (1, 1, -2),                                                                # w <= 0 (the last one would mirror into the image)
                    (-2, 0, 2), (-1, -1, 1),                                                                          # x < 0: kept only without FRONT_ONLY
                    (2, 2, 2), (1, 1, 1)], np.float32)
    on = run([pts], [len(pts)], [proj], [(0, 0)], 4, 4, front_only=True)[0]
    off = run([pts], [len(pts)], [proj], [(0, 0)], 4, 4, front_only=False)[0]
    want_on = np.zeros((4, 4), np.float32)
    want_on[2, 2] = 1.0                                                  # (2,2,2) and (1,1,1) share pixel (2, 2): the closer one
    want_off = want_on.copy()
    want_off[1, 0], want_off[0, 0] = 2.0, 1.0
    assert np.array_equal(on, want_on) and np.array_equal(off, want_off)
    for fo, got in ((True, on), (False, off)):
        assert np.array_equal(got, LR.reference(pts, proj, (0, 0), 4, 4, front_only=fo)[0].astype(np.float32))


def test_clip_and_vel_depth():
    proj = LR.kitti_proj()
    pts, dropped = LR.unambiguous(12, 5000, proj, (0, 0), 24, 48, depth=(0.3, 120.0))
    assert dropped <= LR.MAX_DROPPED
    for vel, clip in ((False, 80.0), (True, None), (True, 60.0)):
        got = run([pts], [len(pts)], [proj], [(0, 0)], 24, 48, vel_depth=vel, max_depth=clip)[0]
        LR.compare(got, pts, proj, (0, 0), vel_depth=vel, max_depth=clip, tag=f"vel_depth={vel} clip={clip}")
        assert clip is None or (got.max() == np.float32(clip) and (got == np.float32(clip)).sum() > 5)


def test_unfiltered_points_stay_sane():
    """No filter: a pixel may go to the neighbour the float64 rounding would not choose, so the checks are the ones that hold anyway."""
    proj, H, W = LR.kitti_proj(), 37, 61
    pts = LR.aimed_points(77, 30000, proj, (0, 0), H, W)
    got = run([pts], [len(pts)], [proj], [(0, 0)], H, W, front_only=False)[0]
    ref, _ = LR.reference(pts, proj, (0, 0), H, W, front_only=False)
    assert np.isfinite(got).all() and (got >= 0).all()
    col, row, w = LR.project64(pts, proj)
    m = proj.astype(np.float64)
    bound = 8 * 2.0 ** -24 * (np.abs(m[2, 0] * pts[:, 0]) + np.abs(m[2, 1] * pts[:, 1]) + np.abs(m[2, 2] * pts[:, 2]) + abs(m[2, 3]))
    for y, x in np.argwhere(got != 0):
        near = (np.abs(col - 1 - x) <= 1.0) & (np.abs(row - 1 - y) <= 1.0) & (w > 0)
        assert (np.abs(w[near] - float(got[y, x])) <= bound[near]).any(), (y, x, got[y, x])
    n_amb = int(LR.ambiguous(pts, proj, (0, 0), H, W).sum())
    print(f"unfiltered: {int((got != 0).sum())} / {int((ref != 0).sum())} non-zero pixels, {n_amb} ambiguous points, {int((got != ref.astype(np.float32)).sum())} pixels differ")
    assert abs(int((got != 0).sum()) - int((ref != 0).sum())) <= n_amb


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kitti_raw"))
    split, scans = LR.make_kitti_tree(root)
    return root, split, scans


def _batches(tree, on_device):
    from simpledepthestimation_amd.data.datasets.kitti_v2 import KittiDepthV2
    root, split, _ = tree
    chain = [dict(NAME="LoadImg"), dict(NAME="LoadLidar"), dict(NAME="LidarDepth", ON_DEVICE=on_device, KEEP_ORIG=True, MAX_POINTS=4096),
             dict(NAME="ClipDepth", MAX_DEPTH=80.0), dict(NAME="KBCrop"), dict(NAME="ToTensor")]
    ds = KittiDepthV2(LR.dataset_cfg(root, split, chain), None)
    return ds.batch_collator([ds[0], ds[1], ds[2]])


def test_device_aug_end_to_end_and_evaluator(tree):
    from simpledepthestimation_amd.config import get_project_cfg
    from simpledepthestimation_amd.data.device_aug import DeviceImageAug
    from simpledepthestimation_amd.evaluation.depth_evaluation import kitti_evaluator
    host, raw = _batches(tree, False), _batches(tree, True)
    static = {"depth": torch.full((3, 1, 352, 1216), float("nan"), device=DEV)}
    dev = DeviceImageAug(DEV)(raw, None, static)
    torch.cuda.synchronize()
    assert not [k for k in dev if k.startswith("lidar")] and dev["depth"] is static["depth"]
    scans = list(tree[2].values())
    proj = LR.kitti_proj()
    for b in range(3):
        x0, y0 = raw["lidar_window"][b, :2].tolist()
        LR.compare(dev["depth"][b, 0].cpu().numpy(), scans[b], proj, (x0, y0), max_depth=80.0, tag=f"device batch[{b}]")
        assert np.array_equal(dev["depth"][b, 0].cpu().numpy(), host["depth"][b, 0].numpy())
        full = dev["depth_orig"][b]
        assert full.is_cuda and tuple(full.shape) == LR.FRAMES[b][3] == host["depth_orig"][b].shape
        LR.compare(full.cpu().numpy(), scans[b], proj, (0, 0), tag=f"device depth_orig[{b}]")
    assert (host["depth"] == 80.0).sum() > 50
    # the evaluator takes the device tensors as they are; prediction = gt * r with r away from the 1.25^k thresholds
    cfg = get_project_cfg("MonoDepth2")
    cfg.TEST.GT_SCALE = False
    results = []
    for depth_orig in (dev["depth_orig"], host["depth_orig"]):
        ev = kitti_evaluator(cfg)
        ev.preprocess_chain = ["KBCrop"]
        gt = [torch.as_tensor(d).to(DEV) for d in depth_orig]
        pred = torch.stack([g[m["kb_y_start"]:m["kb_y_start"] + 352, m["kb_x_start"]:m["kb_x_start"] + 1216] * 1.1 for g, m in zip(gt, host["metadata"])])[:, None]
        ev.process({"depth_orig": depth_orig, "metadata": host["metadata"]}, {"depth_pred": pred + (pred == 0) * 5.0})
        results.append(ev.evaluate()["kitti evaluator"])
    for k in results[0]:
        assert results[0][k] == pytest.approx(results[1][k], rel=1e-5, abs=1e-9), k
    assert results[0]["abs_rel"] == pytest.approx(0.1, rel=1e-3) and results[0]["d1"] == 1.0


def test_export_tool_kernel_path_equals_host_path(tree, tmp_path):
    from simpledepthestimation_amd.tools import export_gt_depth
    root, split, _ = tree
    outs = {}
    for mode, extra in (("host", ["--host"]), ("device", ["--batch", "2"])):          # --batch 2: a full batch of the first size, then the flushes at the end
        out = str(tmp_path / mode)
        assert export_gt_depth.main(["--data-root", root, "--split", split, "--out", out] + extra) == 0
        outs[mode] = out
    for date, drive, img_id, size in LR.FRAMES:
        a, b = (np.load(export_gt_depth.out_path(outs[m], date, drive, LR.CAM, img_id))["velodyne_depth"] for m in ("host", "device"))
        assert a.shape == size and a.dtype == np.float32 and np.array_equal(a, b) and (a != 0).sum() > 500


def test_prefetcher_hands_device_depth_over(tree):
    from simpledepthestimation_amd.data.build import DevicePrefetcher
    from simpledepthestimation_amd.data.device_aug import DeviceImageAug
    host, raw = _batches(tree, False), _batches(tree, True)
    got = list(DevicePrefetcher([raw, raw], DEV, device_aug=DeviceImageAug(DEV), pick_stream=False))
    torch.cuda.synchronize()
    assert len(got) == 2
    for b in got:
        assert not [k for k in b if k.startswith("lidar")] and b["depth"].is_cuda
        assert torch.equal(b["depth"].cpu(), host["depth"])

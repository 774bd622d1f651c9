"""CPU: raw LiDAR scans -> depth ground truth without a GPU.  The host twin (hip.lidar.lidar_depth_np) against the float64 restatement of
lidar_ref.py on unambiguous inputs (bound and input filter: lidar_ref's docstring); the LidarDepth step in host mode against the window / clip
bookkeeping of device mode, bit for bit; KittiDepthV2 with DEPTH_TYPE "lidar" over a miniature tree; the export tool's --host path."""
import ctypes
import os
import random

import numpy as np
import pytest

import lidar_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("H,W,n,seed", [(375, 1242, 60000, 1), (5, 7, 3000, 2)])
@pytest.mark.parametrize("vel_depth", [False, True])
def test_host_twin_matches_the_float64_restatement(H, W, n, seed, vel_depth):
    from simpledepthestimation_amd.hip.lidar import lidar_depth_np
    proj = LR.kitti_proj()
    pts, dropped = LR.unambiguous(seed, n, proj, (0, 0), H, W)
    print(f"{H}x{W}: {dropped:.4f} of {n} points dropped as ambiguous")
    assert dropped <= LR.MAX_DROPPED
    got = lidar_depth_np(pts, proj, (0, 0), H, W, vel_depth=vel_depth, front_only=False)
    ref = LR.compare(got, pts, proj, (0, 0), vel_depth=vel_depth, front_only=False, tag=f"np {H}x{W} vel_depth={vel_depth}")
    assert (ref != 0).sum() > (30 if H == 5 else 30000)
    clipped = lidar_depth_np(pts, proj, (0, 0), H, W, vel_depth=vel_depth, front_only=False, max_depth=40.0)
    assert np.array_equal(clipped, np.minimum(got, np.float32(40.0)))


def test_host_twin_window_is_a_slice_of_the_full_map():
    from simpledepthestimation_amd.hip.lidar import lidar_depth_np
    proj = LR.kitti_proj()
    pts = LR.aimed_points(5, 4000, proj, (0, 0), 32, 64)
    full = lidar_depth_np(pts, proj, (0, 0), 32, 64)
    assert np.array_equal(lidar_depth_np(pts, proj, (13, 5), 8, 16), full[5:13, 13:29]) and (full != 0).sum() > 1000


def test_step_registered_and_prototype_bound():
    from simpledepthestimation_amd.data.preprocess import build_preprocess
    from simpledepthestimation_amd.data.preprocess.loading import LidarDepth
    from simpledepthestimation_amd.hip import lib as L
    step = build_preprocess({"NAME": "LidarDepth"})
    assert isinstance(step, LidarDepth)
    assert (step.vel_depth, step.front_only, step.keep_orig_for_eval, step.on_device, step.max_points) == (False, True, False, False, 131072)
    args, res = L._PROTOS["sde_lidar_depth"]
    assert len(args) == 13 and res is ctypes.c_int
    assert "sde_lidar_depth" in open(os.path.join(ROOT, "include", "sde_hip.h")).read()
    assert hasattr(L.lib(), "sde_lidar_depth")


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    from simpledepthestimation_amd.hip import lib as L
    f = L.lib().sde_lidar_depth
    one = ctypes.c_void_p(64)          # never dereferenced: every call below is refused (or returns) before any launch
    ok = dict(pts=one, cap=8, stride=3, count=one, B=1, proj=one, origin=one, H=4, W=4, flags=2, max_depth=0.0, depth=one)
    order = ("pts", "cap", "stride", "count", "B", "proj", "origin", "H", "W", "flags", "max_depth", "depth")
    call = lambda **kw: f(*[{**ok, **kw}[k] for k in order], None)
    for bad in (dict(stride=2), dict(stride=5), dict(H=0), dict(W=-1), dict(cap=0), dict(B=-1), dict(flags=4), dict(pts=None), dict(count=None), dict(proj=None),
                dict(origin=None), dict(depth=None)):
        assert call(**bad) < 0, bad
        assert b"sde_lidar_depth" in L.lib().sde_last_error(), bad
    assert call(B=0) == 0 and call(B=0, pts=None, count=None, proj=None, origin=None, depth=None) == 0


def test_binding_refuses_cpu_tensors_and_wrong_shapes():
    import torch
    from simpledepthestimation_amd.hip.lib import SdeHipError
    from simpledepthestimation_amd.hip.lidar import lidar_depth
    with pytest.raises(SdeHipError):
        lidar_depth(torch.zeros(1, 8, 3), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 3, 4), torch.zeros(1, 2, dtype=torch.int32), 4, 4)
    with pytest.raises(SdeHipError):
        lidar_depth(torch.zeros(1, 8, 5), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 3, 4), torch.zeros(1, 2, dtype=torch.int32), 4, 4)


def _chain(on_device, keep_orig=False):
    from simpledepthestimation_amd.data.preprocess import build_preprocess
    return [build_preprocess(s) for s in (dict(NAME="LoadLidar"), dict(NAME="LidarDepth", ON_DEVICE=on_device, KEEP_ORIG=keep_orig), dict(NAME="ClipDepth", MAX_DEPTH=80.0),
                                          dict(NAME="KBCrop"), dict(NAME="RandomCrop", IMG_H=96, IMG_W=320))]


def _sample(tmp_path, seed=3, n=20000, H=375, W=1242):
    proj = LR.kitti_proj()
    pts = LR.aimed_points(seed, n, proj, (0, 0), H, W, depth=(1.0, 120.0))
    path = os.path.join(tmp_path, "scan.bin")
    np.concatenate([pts, np.ones((n, 1), np.float32)], 1).astype(np.float32).tofile(path)
    make = lambda: {"img": np.zeros((H, W, 3), np.uint8), "lidar_proj": proj.copy(), "intrinsics": np.eye(3, dtype=np.float32), "metadata": {"lidar_dir": path}}
    return pts, proj, make


def test_device_mode_bookkeeping_equals_host_mode(tmp_path):
    """The same chain and seed in both modes: the same crops are drawn, the RNG ends in the same state, and projecting into the recorded window
    with the recorded clip gives the host-mode depth bit for bit."""
    from simpledepthestimation_amd.hip.lidar import lidar_depth_np
    pts, proj, make = _sample(str(tmp_path))
    out, states = {}, {}
    for mode in (False, True):
        random.seed(11)
        d = make()
        for step in _chain(mode, keep_orig=True):
            d = step.forward(d)
        out[mode], states[mode] = d, random.getstate()
    host, dev = out[False], out[True]
    assert states[False] == states[True]
    assert "lidar" not in host and "lidar" not in dev and "depth" not in dev and "lidar_proj" not in host
    assert host["depth"].shape == (96, 320) and host["depth"].dtype == np.float32 and host["depth_orig"].shape == (375, 1242)
    assert dev["lidar_points"].shape == (131072, 3) and dev["lidar_points"].dtype == np.float32 and dev["lidar_count"].dtype == np.int32
    assert dev["lidar_window"].dtype == np.int32 and dev["lidar_window"].tolist()[2:] == [320, 96]
    md = host["metadata"]
    assert dev["lidar_window"].tolist()[:2] == [md["kb_x_start"] + md["rand_x_start"], md["kb_y_start"] + md["rand_y_start"]]
    assert float(dev["lidar_clip"]) == 80.0 and int(dev["lidar_flags"]) == 2 and dev["lidar_window_orig"].tolist() == [0, 0, 1242, 375]
    n = int(dev["lidar_count"])
    assert n == int((pts[:, 0] >= 0).sum()) and not dev["lidar_points"][n:].any()
    x0, y0, w, h = dev["lidar_window"].tolist()
    again = lidar_depth_np(dev["lidar_points"][:n], dev["lidar_proj"], (x0, y0), h, w, front_only=True, max_depth=float(dev["lidar_clip"]))
    assert np.array_equal(again, host["depth"]) and (host["depth"] != 0).sum() > 300 and host["depth"].max() == 80.0
    full = lidar_depth_np(dev["lidar_points"][:n], dev["lidar_proj"], (0, 0), 375, 1242)
    assert np.array_equal(full, host["depth_orig"]) and full.max() > 80.0


def test_crop_top_moves_the_window(tmp_path):
    from simpledepthestimation_amd.data.preprocess import build_preprocess
    _, _, make = _sample(str(tmp_path), n=100)
    d = make()
    for step in (build_preprocess(dict(NAME="LoadLidar")), build_preprocess(dict(NAME="LidarDepth", ON_DEVICE=True)), build_preprocess(dict(NAME="CropTopTo", IMG_H=300))):
        d = step.forward(d)
    assert d["lidar_window"].tolist() == [0, 75, 1242, 300] and "lidar_window_orig" not in d


def test_resize_behind_device_mode_raises_and_overflow_raises(tmp_path):
    from simpledepthestimation_amd.data.preprocess import build_preprocess
    _, _, make = _sample(str(tmp_path), n=500)
    d = make()
    for step in (build_preprocess(dict(NAME="LoadLidar")), build_preprocess(dict(NAME="LidarDepth", ON_DEVICE=True))):
        d = step.forward(d)
    with pytest.raises(ValueError, match="host mode"):
        build_preprocess(dict(NAME="Resize", IMG_H=192, IMG_W=640)).forward(d)
    d = build_preprocess(dict(NAME="LoadLidar")).forward(make())
    with pytest.raises(ValueError, match="MAX_POINTS"):
        build_preprocess(dict(NAME="LidarDepth", ON_DEVICE=True, MAX_POINTS=100)).forward(d)
    host = build_preprocess(dict(NAME="LidarDepth", MAX_POINTS=100)).forward(build_preprocess(dict(NAME="LoadLidar")).forward(make()))      # host mode has no capacity
    assert host["depth"].shape == (375, 1242)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kitti_raw"))
    split, scans = LR.make_kitti_tree(root)
    return root, split, scans


def test_dataset_with_depth_type_lidar(tree):
    from simpledepthestimation_amd.data.datasets.kitti_v2 import KittiDepthV2, read_calib
    from simpledepthestimation_amd.geometry.camera import velo_to_image
    root, split, scans = tree
    ds = KittiDepthV2(LR.dataset_cfg(root, split, []), None)
    assert len(ds) == 3 and ds.with_depth
    s = ds[0]
    assert s["metadata"]["depth_dir"] == "" and s["metadata"]["lidar_dir"].endswith("velodyne_points/data/0000000000.bin")
    cam, velo = read_calib(os.path.join(root, "2011_09_26", "calib_cam_to_cam.txt")), read_calib(os.path.join(root, "2011_09_26", "calib_velo_to_cam.txt"))
    R, T = np.eye(4), np.eye(4)
    R[:3, :3] = cam["R_rect_00"].astype(np.float64).reshape(3, 3)
    T[:3, :3], T[:3, 3] = velo["R"].astype(np.float64).reshape(3, 3), velo["T"].astype(np.float64)
    want = (cam["P_rect_02"].astype(np.float64).reshape(3, 4) @ R @ T).astype(np.float32)
    assert s["lidar_proj"].dtype == np.float32 and s["lidar_proj"].shape == (3, 4) and np.array_equal(s["lidar_proj"], want)
    assert np.array_equal(velo_to_image(cam, velo, "image_02"), want) and np.array_equal(want, LR.kitti_proj())
    assert not np.array_equal(velo_to_image(cam, velo, "image_03"), want)
    # the existence filter looks at the scan, not at a depth file
    os.rename(s["metadata"]["lidar_dir"], s["metadata"]["lidar_dir"] + ".away")
    try:
        assert len(KittiDepthV2(LR.dataset_cfg(root, split, []), None)) == 2
    finally:
        os.rename(s["metadata"]["lidar_dir"] + ".away", s["metadata"]["lidar_dir"])
    with pytest.raises(NotImplementedError):
        KittiDepthV2(LR.dataset_cfg(root, split, [], DEPTH_TYPE="bogus"), None)


HOST_CHAIN = [dict(NAME="LoadImg"), dict(NAME="LoadLidar"), dict(NAME="LidarDepth", KEEP_ORIG=True), dict(NAME="ToTensor")]


def test_host_mode_samples_match_the_restatement_and_collate(tree):
    from simpledepthestimation_amd.data.datasets.kitti_v2 import KittiDepthV2
    root, split, scans = tree
    ds = KittiDepthV2(LR.dataset_cfg(root, split, HOST_CHAIN), None)
    entries = list(scans)
    for i in (0, 2):
        s = ds[i]
        H, W = LR.FRAMES[i][3]
        assert s["depth"].shape == (H, W)
        LR.compare(s["depth"], scans[entries[i]], LR.kitti_proj(), (0, 0), tag=f"tree frame {i}")
    dev_chain = [dict(NAME="LoadImg"), dict(NAME="LoadLidar"), dict(NAME="LidarDepth", ON_DEVICE=True, KEEP_ORIG=True, MAX_POINTS=4096), dict(NAME="KBCrop"), dict(NAME="ToTensor")]
    dd = KittiDepthV2(LR.dataset_cfg(root, split, dev_chain), None)
    b = dd.batch_collator([dd[0], dd[2]])
    import torch
    assert tuple(b["lidar_points"].shape) == (2, 4096, 3) and b["lidar_count"].dtype == torch.int32 and tuple(b["lidar_count"].shape) == (2,)
    assert b["lidar_window"].tolist() == [[13, 23, 1216, 352], [5, 18, 1216, 352]] and b["lidar_window_orig"].tolist() == [[0, 0, 1242, 375], [0, 0, 1226, 370]]
    assert tuple(b["lidar_proj"].shape) == (2, 3, 4) and b["lidar_clip"].tolist() == [0.0, 0.0] and b["lidar_flags"].tolist() == [2, 2]


def test_export_tool_host_path_round_trips_through_load_depth(tree, tmp_path):
    from simpledepthestimation_amd.data.datasets.kitti_v2 import KittiDepthV2
    from simpledepthestimation_amd.tools import export_gt_depth
    root, split, _ = tree
    out = str(tmp_path / "gt")
    assert export_gt_depth.main(["--data-root", root, "--split", split, "--out", out, "--host"]) == 0
    lidar = KittiDepthV2(LR.dataset_cfg(root, split, HOST_CHAIN), None)
    cached = KittiDepthV2(LR.dataset_cfg(root, split, [dict(NAME="LoadImg"), dict(NAME="LoadDepth", KEEP_ORIG=True), dict(NAME="ToTensor")],
                                         DEPTH_TYPE="velodyne", DEPTH_ROOT=out), None)
    assert len(cached) == 3
    for i in range(3):
        a, b = lidar[i], cached[i]
        assert b["metadata"]["depth_dir"].endswith(f"proj_depth/velodyne/image_02/{LR.FRAMES[i][2]}.npz")
        assert a["depth"].dtype == b["depth"].dtype and np.array_equal(a["depth"], b["depth"]) and (a["depth"] != 0).sum() > 500

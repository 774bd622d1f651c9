"""CPU: the flow restatement (flow_ref.py) and points_to_img against the reference's recording (tests/golden/flow.npz, written by
scripts/gen_golden_flow.py), the trajectory helpers, the .flo file and the colour wheel.  Nothing here needs a GPU."""
import os
import struct

import numpy as np
import pytest
import torch

import flow_ref as FR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flow.npz")
RECORDED = ("rigid", "motion")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def restated(g, case):
    d = g[case + "_depth"][:, 0]
    H, W = d.shape[1:]
    motion = g[case + "_motion"] if case == "motion" else None
    return FR.restate(d, np.arange(H, dtype=np.int32), np.arange(W, dtype=np.int32), g[case + "_K"], g[case + "_T"], motion)


@pytest.mark.parametrize("case", RECORDED)
def test_restatement_agrees_with_the_reference_recording(golden, case):
    """The reference evaluates the same projection in float32 in another order (K R and K t first); its result lies within the bound of the
    float64 restatement, its mask equals bit 1 outside the edge band, and the band holds at most 1 % of the pixels."""
    r = restated(golden, case)
    coords = golden[case + "_coords"].astype(np.float64)
    for i, (name, E) in enumerate((("X", r["EX"]), ("Y", r["EY"]))):
        err = np.abs(coords[..., i] - r[name])
        print(f"{case} {name}: largest error / bound = {float((err / E).max()):.3f}")
        assert bool(np.all(err <= E)), name
    mask = golden[case + "_mask"][..., 0]
    assert float(r["edge1"].mean()) <= 0.01
    assert np.array_equal(mask[~r["edge1"]], r["bit1"][~r["edge1"]])
    assert 0.2 < float(mask.mean()) < 0.95                                 # both outcomes occur
    assert bool(np.all(np.abs(golden[case + "_Z"][..., 0] - r["qz"]) <= 8 * FR.EPS * (np.abs(r["qz"]) + 60.0)))


@pytest.mark.parametrize("case", RECORDED)
def test_points_to_img_equals_the_recording(golden, case):
    """The package's points_to_img on the recorded points, K R and K t, on the CPU: two float32 evaluations of one expression, so within the
    restatement's bound of each other; same shapes, dtypes and mask."""
    from simpledepthestimation_amd.geometry.camera import points_to_img
    r = restated(golden, case)
    coords, Z, mask = points_to_img(*(torch.from_numpy(golden[f"{case}_{k}"]) for k in ("points", "KR", "Kt")))
    assert coords.dtype == torch.float32 and Z.dtype == torch.float32 and mask.dtype == torch.bool
    for got, name in ((coords, "coords"), (Z, "Z"), (mask, "mask")):
        assert tuple(got.shape) == golden[f"{case}_{name}"].shape, name
    diff = np.abs(coords.numpy().astype(np.float64) - golden[case + "_coords"])
    assert bool(np.all(diff[..., 0] <= r["EX"]) and np.all(diff[..., 1] <= r["EY"]))
    assert bool(np.all(np.abs(Z.numpy() - golden[case + "_Z"]) <= 8 * FR.EPS * (np.abs(golden[case + "_Z"]) + 60.0)))
    keep = ~r["edge1"]
    assert np.array_equal(mask.numpy()[..., 0][keep], golden[case + "_mask"][..., 0][keep])


def test_points_to_img_gradient():
    from simpledepthestimation_amd.geometry.camera import points_to_img
    g = np.load(GOLDEN)
    pts = torch.from_numpy(g["motion_points"][:, :, 2:5, 3:7]).double().contiguous().requires_grad_(True)
    R = torch.from_numpy(g["motion_KR"]).double().requires_grad_(True)
    for t_np in (g["rigid_Kt"], g["motion_Kt"].reshape(2, 3, 10, 16)[:, :, 2:5, 3:7].reshape(2, 3, 12)):
        t = torch.from_numpy(np.ascontiguousarray(t_np)).double().requires_grad_(True)
        assert torch.autograd.gradcheck(lambda p, r, tt: points_to_img(p, r, tt)[:2], (pts, R, t), eps=1e-6, atol=1e-6, rtol=1e-5)
    with pytest.raises(ValueError):
        points_to_img(pts[:, :2], R, t)


def test_accumulate_poses():
    from simpledepthestimation_amd.geometry.pose_utils import accumulate_poses
    eye = np.tile(np.eye(4), (5, 1, 1))
    W = accumulate_poses(eye)
    assert W.shape == (6, 4, 4) and W.dtype == np.float64 and np.array_equal(W, np.tile(np.eye(4), (6, 1, 1)))
    # a pure translation: the camera moves 0.5 m forward per step, so a point's coordinates in the next frame drop by 0.5: T = [I | (0, 0, -0.5)]
    step = np.eye(4)
    step[2, 3] = -0.5
    W = accumulate_poses(torch.from_numpy(np.tile(step, (4, 1, 1))).float())
    assert np.allclose(W[:, :3, 3], np.stack([np.zeros(5), np.zeros(5), 0.5 * np.arange(5)], 1), atol=1e-12)
    assert np.array_equal(W[:, :3, :3], np.tile(np.eye(3), (5, 1, 1)))
    # a constant yaw of 6 degrees with a forward step: sixty steps close the circle
    a = np.deg2rad(6.0)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    T[:3, 3] = [0.0, 0.0, -1.0]
    W = accumulate_poses(np.tile(T, (60, 1, 1)))
    assert np.abs(W[60] - np.eye(4)).max() <= 1e-9
    radius = np.linalg.norm(W[:, :3, 3] - W[:60, :3, 3].mean(0), axis=1)
    assert np.ptp(radius[:60]) <= 1e-9 and radius[0] > 5.0                   # the positions lie on one circle (1 / (2 sin 3 deg) = 9.55 m)
    with pytest.raises(ValueError):
        accumulate_poses(np.eye(4))


def test_write_kitti_poses_round_trip(tmp_path):
    from simpledepthestimation_amd.geometry.pose_utils import accumulate_poses, write_kitti_poses
    rng = np.random.default_rng(5)
    rel = np.stack([FR.pose(rng.uniform(-3, 3, 3), rng.uniform(-1, 1, 3)) for _ in range(7)])
    W = accumulate_poses(rel)
    path = tmp_path / "trajectory.txt"
    write_kitti_poses(str(path), W)
    back = np.loadtxt(str(path))
    assert back.shape == (8, 12) and np.array_equal(back, W[:, :3].reshape(8, 12))
    assert path.read_text().splitlines()[0].split() == ["1.0", "0.0", "0.0", "0.0", "0.0", "1.0", "0.0", "0.0", "0.0", "0.0", "1.0", "0.0"]
    with pytest.raises(ValueError):
        write_kitti_poses(str(path), np.eye(4))


def test_flo_round_trip_and_header(tmp_path):
    from simpledepthestimation_amd.hip.flow import read_flo, write_flo
    rng = np.random.default_rng(6)
    flow = rng.standard_normal((5, 7, 2)).astype(np.float32)
    flow[0, 0] = [np.float32(-0.0), np.float32(1e-42)]
    flow[1, 2] = [np.inf, np.float32(3.4e38)]
    path = str(tmp_path / "a.flo")
    write_flo(path, flow)
    raw = open(path, "rb").read()
    assert raw[:4] == b"PIEH" and struct.unpack("<f", raw[:4])[0] == 202021.25
    assert struct.unpack("<ii", raw[4:12]) == (7, 5) and len(raw) == 12 + 5 * 7 * 2 * 4
    assert raw[12:20] == flow[0, 0].tobytes()
    back = read_flo(path)
    assert back.dtype == np.float32 and back.shape == (5, 7, 2) and back.tobytes() == flow.tobytes()
    write_flo(path, torch.from_numpy(flow))
    assert open(path, "rb").read() == raw
    with pytest.raises(ValueError):
        write_flo(path, flow.astype(np.float64))
    with pytest.raises(ValueError):
        write_flo(path, flow[..., 0])
    open(path, "wb").write(raw[:-4])
    with pytest.raises(ValueError):
        read_flo(path)
    open(path, "wb").write(b"JUNK" + raw[4:])
    with pytest.raises(ValueError):
        read_flo(path)


def test_flow_wheel():
    from simpledepthestimation_amd.hip.flow import WHEEL_SEGMENTS, wheel_u8
    w = wheel_u8()
    assert w.shape == (55, 3) and w.dtype == np.uint8 and WHEEL_SEGMENTS == (15, 6, 4, 11, 13, 6)
    assert np.array_equal(w, FR.wheel())
    # a segment starts at a pure colour (every channel 0 or 255) and ramps one channel: the lengths are the distances between the pure rows
    pure = [i for i, r in enumerate(w) if all(int(c) in (0, 255) for c in r)]
    assert pure == [0, 15, 21, 25, 36, 49]
    assert np.diff(pure + [55]).tolist() == [15, 6, 4, 11, 13, 6]
    assert [w[i].tolist() for i in pure] == [[255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 255]]
    assert bool(np.all(w.max(1) == 255) and np.all(w.min(1) == 0))
    assert w[14].tolist() == [255, 238, 0] and w[54].tolist() == [255, 0, 43]                 # floor(255 * 14 / 15), 255 - floor(255 * 5 / 6)


def test_restatement_cases_are_well_conditioned():
    """The GPU cases' inputs keep the restatement inside the range its first-order bound is written for (restate asserts qz), have both valid
    classes, and exclude little."""
    table = FR.wheel()
    for name in FR.CASES:
        i = FR.case_inputs(name)
        r = FR.restate(i["pred"], i["ymap"], i["xmap"], i["K"], i["T"], i["motion"])
        _, skip = FR.colours(r["flow"], r["bit0"], r["bound"], i["max_flow"], table)
        assert float(r["edge1"].mean()) <= 0.01 and float(skip.mean()) <= 0.005, name
        assert bool(r["bit1"].any() and (r["bit0"] & ~r["bit1"]).any()), name
        assert i["xmap"].size % FR.TILE != 0
    i = FR.case_inputs("ragged_tile")
    assert i["xmap"].size >= FR.TILE + 3 and FR.TILE == 1024
    r = FR.restate(**{k: FR.case_inputs("nan_zero_and_behind")[k] for k in ("pred", "ymap", "xmap", "K", "T", "motion")})
    assert bool((r["qz"][1, 3:6] < 0).all() and (~r["bit0"][1, 3:6]).all()) and bool(r["bit0"][0, 3:6].all())

"""CPU: the host twin of sde_tsdf_render (hip/volume.py: render_host) against the float64 restatement of render_ref.py on every shared case, the
analytic scenes against their closed form, and the argument errors that are raised before anything touches a device."""
import functools
import inspect

import numpy as np
import pytest

import render_ref as RR


@functools.lru_cache(maxsize=None)
def twin(name):
    """The twin's result of one case: computed once, shared, never modified."""
    from simpledepthestimation_amd.hip.volume import render_host
    inp = RR.case_inputs(name)
    return render_host(inp["tsdf"], inp["weight"], inp["rgba"], inp["K"], inp["C"], inp["size"], inp["origin"], inp["voxel"], inp["near"], inp["step"], inp["n"],
                       inp["min_weight"])


@pytest.mark.parametrize("name", RR.CASES)
def test_twin_against_restatement(name):
    inp, got = RR.case_inputs(name), twin(name)
    H, W = inp["size"]
    assert got[0].dtype == np.float32 and got[0].shape == (H, W) and got[1].dtype == np.float32 and got[1].shape == (H, W, 3)
    assert (got[2] is None) == (inp["rgba"] is None) and (got[2] is None or (got[2].dtype == np.uint8 and got[2].shape == (H, W, 4)))
    want = RR.restate(inp)                                                    # asserts that at most MAX_EXCLUDED of the pixels are undecided
    RR.compare(got, want, name)
    hit = got[0] != 0
    hits = int(hit.sum())
    if name in ("all_miss", "flat_dims") or name in RR.BAD_POSE:
        assert hits == 0 and not got[1].any() and not got[2].any()
    elif name == "camera_inside":
        assert hits == hit.size
    else:
        assert 0 < hits < hit.size
    if got[2] is not None:
        assert bool((got[2][hit][:, 3] == 255).all())
    length = np.linalg.norm(got[1].astype(np.float64), axis=-1)
    if name == "zero_sample":                                                 # t == 0 hits (the <= of the rule), one whole step behind the positive sample
        i = int(want["index"][hit][0])
        assert bool((want["index"][hit] == i).all())
        s_prev = np.float32(inp["near"]) + np.float32(i - 1) * np.float32(inp["step"])
        assert bool((got[0][hit] == s_prev + np.float32(inp["step"]) * np.float32(1)).all())
        assert not got[1].any()                                               # all eight corners 0: a gradient of length 0, the normal is zeros
    else:
        assert bool(np.all(np.abs(length[hit] - 1) < 1e-6)) and not length[~hit].any()
    if name == "axis_parallel":
        assert float(inp["K"][0, 2]) == 9 and float(inp["K"][1, 2]) == 6 and hit[6, 9]
    if name == "beyond_far":                                                  # both kinds: a surface between samples 0 and 1, and one behind the last sample
        s = [float(np.float32(inp["near"]) + np.float32(i) * np.float32(inp["step"])) for i in range(inp["n"])]
        assert inp["n"] == 3 and bool(((got[0] > s[0]) & (got[0] <= s[1])).any())
        nrm, point = RR.plane_field((2, 2, 2), inp["origin"], inp["voxel"], (0.8, 0.0, -1.0), (0.0, 0.0, 1.5), 0.5)[1], (0.0, 0.0, 1.5)
        behind = (nrm @ np.asarray(point)) / (np.stack([(np.arange(W) - float(inp["K"][0, 2])) / float(inp["K"][0, 0]), np.zeros(W), np.ones(W)], -1) @ nrm)
        assert bool((behind > s[-1] + 0.01).any()) and not hit[:, behind > s[-1] + 0.01].any()
    if name == "back_face_first":                                             # the hit is the far face of the slab: the near one, negative to positive, was passed
        assert float(got[0][hit].min()) > 2.15
    if name == "holes":
        plain = twin("oblique_plane")[0] != 0                                 # the same scene without the holes
        assert int((plain & ~hit).sum()) > 100 and int((plain & hit).sum()) > 100 and not (hit & ~plain).any()
    if name == "min_weight_2":
        from simpledepthestimation_amd.hip.volume import render_host
        one = render_host(inp["tsdf"], inp["weight"], inp["rgba"], inp["K"], inp["C"], inp["size"], inp["origin"], inp["voxel"], inp["near"], inp["step"],
                          inp["n"], 1)[0] != 0
        assert int((one & ~hit).sum()) > 100 and not (hit & ~one).any()


@pytest.mark.parametrize("name", RR.ANALYTIC)
def test_analytic_scene_in_closed_form(name):
    """A tsdf that is linear in space: trilinear interpolation and the interpolation between two samples are exact in exact arithmetic, so the
    restatement of the EXACT field gives the ray / plane intersection and the plane's normal, and its bounds -- with the counted cost of storing
    the field as float32 in them -- hold for the twin.  Nothing is tuned."""
    inp, got = RR.case_inputs(name), twin(name)
    ex = inp["exact"]
    assert float(np.abs(inp["tsdf"].astype(np.float64) - ex["tsdf"])[inp["weight"] >= 1].max()) <= float(ex["err"].max())
    want = RR.restate(inp, ex["tsdf"], ex["err"])
    depth, normal = RR.closed_form(inp)
    ok = want["hit"] & ~want["skip"]
    assert int(ok.sum()) > 100
    assert float(np.abs(want["depth"] - depth)[ok].max()) < 1e-12 and float(np.abs(want["normal"] - normal)[ok].max()) < 1e-12
    RR.compare(got, want, name + " (exact field)")
    err, nerr = np.abs(got[0] - depth)[ok], np.abs(got[1] - normal)[ok]
    print(f"{name}: largest distance from the closed form: depth {float(err.max()):.3e} (bound {float(want['depth_bound'][ok].max()):.3e}), "
          f"normal {float(nerr.max()):.3e} (bound {float(want['normal_bound'][ok].max()):.3e})")
    assert bool(np.all(err <= want["depth_bound"][ok] + 1e-12)) and bool(np.all(nerr <= want["normal_bound"][ok] + 1e-12))
    assert float(want["depth_bound"][ok].max()) < 1e-4 and float(want["normal_bound"][ok].max()) < 1e-4           # the bounds say something


def test_the_march_is_complete_and_computed_from_the_index():
    """One ray through a 2 x 2 x 4 grid whose numbers can be followed by hand: the crossing lies at g_z = 1.5, z = 2 exactly."""
    from simpledepthestimation_amd.hip.volume import render_host
    f32 = np.float32
    tsdf = np.zeros((4, 2, 2), f32)
    tsdf[0], tsdf[1], tsdf[2], tsdf[3] = 0.5, 0.25, -0.25, -0.5
    K, C = np.array([[4, 0, 0.5], [0, 4, 0.5], [0, 0, 1]], f32), np.eye(4, dtype=f32)
    args = dict(K=K, C=C, size=(1, 1), origin=(f32(-1.0), f32(-1.0), f32(0.0)), voxel=f32(1.0), near=f32(0.75), step=f32(0.5), n=6)
    depth, normal, picture = render_host(tsdf, np.ones_like(tsdf), None, min_weight=1, **args)
    assert picture is None and float(depth[0, 0]) == 2.0 and normal[0, 0].tolist() == [0.0, 0.0, -1.0]
    weight = np.ones_like(tsdf)
    weight[2] = 0                                                             # no cell around the crossing is valid any more
    assert float(render_host(tsdf, weight, None, min_weight=1, **args)[0][0, 0]) == 0
    assert float(render_host(tsdf, np.ones_like(tsdf), None, min_weight=1, **dict(args, n=3))[0][0, 0]) == 0          # the crossing lies behind sample 2


def test_sample_count_and_refusals():
    from simpledepthestimation_amd.hip import volume as HV
    assert HV.check_render((13, 19), 0.5, 3.0, 0.1) == (13, 19, 0.5, float(np.float32(0.1)), 25)
    assert HV.check_render((1, 1), 0.0, 1.0, 0.25)[4] == 4 and HV.check_render((1, 1), 0.0, 1.0, 0.3)[4] == 4
    assert HV.check_render((1, 1), 1.0, 1.5, 2.0)[4] == 1
    assert HV.check_render((1, 1), 0.0, 65536.0, 1.0)[4] == HV.MAX_SAMPLES
    near, step = np.float32(0.3), np.float32(0.11)                            # from the fp32 values, in float64
    assert HV.check_render((2, 2), 0.3, 4.5, 0.11)[4] == int(np.ceil((float(np.float32(4.5)) - float(near)) / float(step)))
    for size in ((0, 4), (4, 0), (4,), (4, 4, 4), (4.5, 4), "ab", None, (HV.MAX_PICTURE + 1, 4)):
        with pytest.raises(ValueError, match="size"):
            HV.check_render(size, 0.0, 1.0, 0.1)
    for near, far, step in ((0.0, 1.0, 0.0), (0.0, 1.0, -0.1), (0.0, 1.0, np.nan), (np.nan, 1.0, 0.1), (0.0, np.inf, 0.1), (0.0, 1.0, np.inf)):
        with pytest.raises(ValueError, match="finite"):
            HV.check_render((4, 4), near, far, step)
    for near, far, step in ((1.0, 1.0, 0.1), (2.0, 1.0, 0.1), (0.0, 65537.0, 1.0), (0.0, 1.0, 1e-6)):
        with pytest.raises(ValueError, match="samples"):
            HV.check_render((4, 4), near, far, step)
    # the binding refuses before it looks at the tensors or the device: an object without __init__ run stands in for the volume
    v = object.__new__(HV.TsdfVolume)
    v.min_depth, v.max_depth, v.voxel, v.rgba, v.dims = 0.0, 80.0, 0.1, None, (4, 4, 4)
    with pytest.raises(ValueError, match="colour"):
        v.render(None, None, (4, 4))
    with pytest.raises(ValueError, match="min_weight"):
        v.render(None, None, (4, 4), picture=False, min_weight=0.5)
    with pytest.raises(ValueError, match="samples"):
        v.render(None, None, (4, 4), picture=False, step=1e-4)
    with pytest.raises(ValueError, match="size"):
        v.render(None, None, (4, 0), picture=False)
    with pytest.raises(ValueError, match="min_weight"):
        HV.render_host(np.ones((2, 2, 2), np.float32), np.ones((2, 2, 2), np.float32), None, np.eye(3), np.eye(4), (1, 1), (0, 0, 0), 0.1, 0.1, 0.1, 3, min_weight=0)
    sig = inspect.signature(HV.TsdfVolume.render).parameters
    assert [sig[k].default for k in ("near", "far", "step", "min_weight", "normals", "picture", "out")] == [None, None, None, 1, True, True, None]


def test_predictor_parses_render():
    from simpledepthestimation_amd.engine import predictor as P
    from simpledepthestimation_amd.hip.volume import TsdfVolume
    v = object.__new__(TsdfVolume)                                            # stands in for a volume: render_arg reads its parameters only
    v.min_depth, v.max_depth, v.voxel, v.colour = 0.5, 20.0, float(np.float32(0.1)), True
    assert P.render_arg(None, None) is None and P.render_arg(None, v) is None
    assert P.render_arg({}, v) == (True, True, 1.0, 0.5, 20.0, float(np.float32(0.1)))
    assert P.render_arg(dict(normals=False, picture=False, min_weight=2, near=1, far=3, step=0.5), v) == (False, False, 2.0, 1.0, 3.0, 0.5)
    with pytest.raises(ValueError, match="needs volume"):
        P.render_arg(dict(normals=True), None)
    for bad in (True, "all", (True, True), dict(normal=True), dict(cap=4)):
        with pytest.raises(ValueError, match="render must be"):
            P.render_arg(bad, v)
    with pytest.raises(ValueError, match="min_weight"):
        P.render_arg(dict(min_weight=0), v)
    with pytest.raises(ValueError, match="samples"):
        P.render_arg(dict(step=1e-5), v)
    v.colour = False
    with pytest.raises(ValueError, match="colour"):
        P.render_arg({}, v)
    assert P.render_arg(dict(picture=False), v)[:2] == (True, False)
    assert inspect.signature(P.PairPredictor.stream).parameters["render"].default is None
    assert inspect.signature(P.PairPredictor.predict).parameters["render"].default is None
    pp = object.__new__(P.PairPredictor)                                      # predict and stream refuse before they look at the frames or the device
    with pytest.raises(ValueError, match="stateless.*render"):
        pp.predict([], np.eye(3, dtype=np.float32), render=dict(normals=True))
    pp.device, pp.offsets = "cuda:0", (-1, 1)
    with pytest.raises(ValueError, match="needs volume"):
        next(pp.stream(iter(()), np.eye(3, dtype=np.float32), render=dict(normals=True)))


def test_demo_tool_parses_render_volume():
    from simpledepthestimation_amd.tools import demo
    base = ["--cfg", "c.yaml", "--input", "frames", "--pairs", "--intrinsics", "1", "2", "3", "4"]
    vol = ["--volume", "64", "48", "32", "--voxel", "0.1"]
    a = demo.parse_args(base + vol + ["--render-volume", "--save-normals"])
    assert a.render_volume and a.save_normals
    a = demo.parse_args(base + vol)
    assert not a.render_volume and not a.save_normals
    for bad in (["--render-volume"], vol + ["--save-normals"], ["--save-normals"], ["--render-volume", "--save-normals"]):
        with pytest.raises(SystemExit):
            demo.parse_args(base + bad)
    with pytest.raises(SystemExit):
        demo.parse_args(["--cfg", "c.yaml", "--input", "frames"] + vol + ["--render-volume"])                       # needs --pairs
    d = demo.model_depth_u16(np.array([[0.0, 1.0, 2.5, 300.0, -1.0, np.nan]], np.float32))
    assert d.dtype == np.uint16 and d.tolist() == [[0, 255, 637, 65535, 0, 0]]
    n = demo.normal_picture(np.array([[[0, 0, -1], [0, 0, 0], [1, 0, 0]]], np.float32))
    assert n.dtype == np.uint8 and n.tolist() == [[[127, 127, 0], [127, 127, 127], [255, 127, 127]]]

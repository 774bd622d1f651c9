"""CPU: GoogleResNet (GoogleResNet.py:L126-171) builds with the reference's state-dict layout, config keys and error cases."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD_PATH = os.path.join(ROOT, "tests", "golden", "google.npz")
GOLD = np.load(GOLD_PATH)
CASES = [("18", "randLN", False), ("18", "BN", False), ("50", "randLN", True)]
NEW_ENTRY_POINTS = ["sde_randln_chunks", "sde_randln_fwd", "sde_randln_bwd", "sde_bilinear2_fwd", "sde_bilinear2_bwd", "sde_softplus_head_fwd",
                    "sde_softplus_head_bwd"]


def google_cfg(enc="18", norm="randLN", learn_scale=False, dtype="fp32"):
    from simpledepthestimation_amd.config import get_cfg
    cfg = get_cfg()
    cfg.MODEL.DEPTH_NET.NAME, cfg.MODEL.DEPTH_NET.ENCODER_NAME = "GoogleResNet", enc
    cfg.MODEL.DEPTH_NET.NORM, cfg.MODEL.DEPTH_NET.LEARN_SCALE, cfg.MODEL.COMPUTE_DTYPE = norm, learn_scale, dtype
    return cfg


@pytest.mark.parametrize("ci", [0, 1, 2, "r34"])
def test_state_dict_names_and_shapes_equal_the_reference(ci):
    import torch
    from simpledepthestimation_amd.modeling.depth_net import build_depth_net
    enc, norm, ls = ("34", "randLN", False) if ci == "r34" else CASES[ci]
    p = "r34_" if ci == "r34" else f"case{ci}_"
    m = build_depth_net(google_cfg(enc, norm, ls))
    sd = m.state_dict()
    assert list(sd) == list(GOLD[p + "names"])
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == list(GOLD[p + "shapes"])
    assert "encoder.encoder.layer2.0.downsample.0.weight" in sd and "encoder.encoder.layer2.0.downsample.1.weight" not in sd
    assert ("decoder.scale" in sd) == ls
    # a reference checkpoint loads with strict=True
    m.load_state_dict({k: torch.zeros(v.shape, dtype=v.dtype) for k, v in sd.items()}, strict=True)


def test_reference_yaml_depth_net_block():
    from oracle import ref_harness
    path = os.path.join(ref_harness.REF_ROOT, "projects", "MotionLearning", "configs", "resnet18.yaml")
    if not os.path.exists(path):
        pytest.skip("reference checkout not present")
    import yaml
    with open(path) as f:
        dn = yaml.safe_load(f)["MODEL"]["DEPTH_NET"]
    assert dn == {"NAME": "GoogleResNet", "ENCODER_NAME": "18pt", "UPSAMPLE_DEPTH": False, "LEARN_SCALE": False, "NORM": "randLN",
                  "NOISE_STDDEV": 0.5, "RAMPUP_ITERS": 10000}
    from simpledepthestimation_amd.config import get_cfg
    cfg = get_cfg()
    for k in dn:
        assert k in cfg.MODEL.DEPTH_NET, k


def test_pretrained_encoders_raise_like_depth_resnet():
    from simpledepthestimation_amd.modeling.depth_net import build_depth_net
    with pytest.raises(RuntimeError, match="ImageNet weights cannot be downloaded") as e1:
        build_depth_net(google_cfg("18pt"))
    cfg = google_cfg("18pt")
    cfg.MODEL.DEPTH_NET.NAME = "DepthResNet"
    with pytest.raises(RuntimeError) as e2:
        build_depth_net(cfg)
    assert str(e1.value) == str(e2.value)


def test_bad_norm_and_fp16_raise():
    from simpledepthestimation_amd.modeling.depth_net import build_depth_net
    with pytest.raises(ValueError, match="NORM"):
        build_depth_net(google_cfg(norm="GN"))
    with pytest.raises(NotImplementedError, match="fp16"):
        build_depth_net(google_cfg(dtype="fp16"))


@pytest.mark.parametrize("hw,match", [((64, 200), "divisible by 32"), ((48, 192), "divisible by 32"), ((32, 32), "2 pixels")])
def test_input_size_errors(hw, match):
    import torch
    from simpledepthestimation_amd.modeling.depth_net import build_depth_net
    m = build_depth_net(google_cfg())
    x = torch.zeros(1, hw[0], hw[1], 4)             # the size checks come before any kernel
    with pytest.raises(ValueError, match=match):
        m({"depth_net_input_nhwc": x})


def test_bn_model_accepts_one_pixel_layer4():
    import torch
    from simpledepthestimation_amd.modeling.depth_net import build_depth_net
    m = build_depth_net(google_cfg(norm="BN"))
    assert not m._rand_norms
    with pytest.raises(Exception) as e:            # passes the size checks, then needs the GPU
        m({"depth_net_input_nhwc": torch.zeros(1, 32, 32, 4)})
    assert "pixels" not in str(e.value)


def test_ramp_formula():
    from simpledepthestimation_amd.modeling.depth_net.GoogleResNet import noise_ramp
    assert noise_ramp(0.5, 10000, 1) == pytest.approx(0.5 * (1 / 10000) ** 2)
    assert noise_ramp(0.5, 10000, 5000) == pytest.approx(0.125)
    assert noise_ramp(0.5, 10000, 10000) == 0.5
    assert noise_ramp(0.5, 10000, 20000) == 0.5


def test_set_stddev_reaches_every_norm():
    from simpledepthestimation_amd.layers.hip_modules import HipRandLayerNorm
    from simpledepthestimation_amd.modeling.depth_net import build_depth_net
    m = build_depth_net(google_cfg())
    norms = [x for x in m.modules() if isinstance(x, HipRandLayerNorm)]
    assert len(norms) == 1 + 2 * 8 and all(x.stddev == 0.5 for x in norms)       # reference default 0.5
    m.set_stddev(0.125)
    assert all(x.stddev == 0.125 and float(x.noise_stddev) == 0.125 for x in norms)
    assert not any("noise_stddev" in k for k in m.state_dict())


def test_max_pool_shortcut_is_refused():
    from simpledepthestimation_amd.layers.hip_modules import HipBatchNorm2d
    from simpledepthestimation_amd.layers.resnet_encoder import BasicBlock, ResNet
    r = ResNet(BasicBlock, [1, 1, 1, 1], HipBatchNorm2d, shortcut_norm=False)
    with pytest.raises(NotImplementedError, match="max-pool"):
        r._make_layer(BasicBlock, 512, 1, stride=2)


def test_new_config_keys_and_existing_defaults():
    from simpledepthestimation_amd.config import get_cfg
    cfg = get_cfg()
    dn = cfg.MODEL.DEPTH_NET
    assert (dn.NORM, dn.NOISE_STDDEV, dn.RAMPUP_ITERS, dn.LEARN_SCALE) == ("randLN", 0.5, 0, False)
    assert dn.NAME == "DepthResNet" and dn.ENCODER_NAME == "18" and not dn.UPSAMPLE_DEPTH and dn.VERSION == "1A" and dn.BTS_SIZE == 512
    assert cfg.MODEL.DATASET == "" and not (dn.BN_NO_TRACK or dn.FIX_1ST_CONV or dn.FIX_1ST_CONVS)


def test_new_entry_points_are_declared_and_bound():
    from simpledepthestimation_amd.hip import google  # noqa: F401
    from simpledepthestimation_amd.hip import lib as L
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sde_hip.h")).read(), flags=re.S)
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L._PROTOS, name
    if L.available():
        L.lib()


def test_golden_file_holds_arrays_only():
    assert all(GOLD[k].dtype != object for k in GOLD.files)
    assert os.path.getsize(GOLD_PATH) < 1 << 20

"""CPU: GooglePoseNet / GoogleMotionNet build from the config with the reference's state dict (tests/golden/motion.npz), their config keys merge,
and the new C entry points never synchronise.  The arithmetic is checked on the GPU (tests/test_gpu_motion_net.py)."""
import os
import re

import numpy as np
import pytest
import torch

import motion_init
from simpledepthestimation_amd.config import get_cfg
from simpledepthestimation_amd.modeling.pose_net import POSE_NET_REGISTRY, build_pose_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "motion.npz"))

# MODEL.POSE_NET of the reference's projects/MotionLearning/configs/Base.yaml and resnet18.yaml (data, copied)
BASE_YAML = """
MODEL:
  POSE_NET:
    NAME: "GoogleMotionNet"
    USE_DEPTH: True
    GROUP_NORM: False
    MASK_MOTION: True
    LEARN_SCALE: True
    BURN_IN_ITERS: 20000
"""
RESNET18_YAML = """
_BASE_: "./Base.yaml"
MODEL:
  POSE_NET:
    SCALE_CONSTRAIN: "clip_ste"
"""


def build(case, dtype="fp32"):
    return build_pose_net(motion_init.case_cfg(get_cfg(), case, dtype))


def test_both_names_build_from_the_default_config():
    for name in ("GooglePoseNet", "GoogleMotionNet"):
        cfg = get_cfg()
        cfg.MODEL.POSE_NET.NAME = name
        net = build_pose_net(cfg)
        assert type(net).__name__ == name and name in POSE_NET_REGISTRY
    assert abs(sum(p.numel() for p in net.parameters()) - 44.18e6) < 0.01e6       # GoogleMotionNet: 44 M parameters


@pytest.mark.parametrize("ci", range(len(motion_init.CASES)))
def test_state_dict_names_order_and_shapes_equal_the_reference(ci):
    net = build(motion_init.CASES[ci])
    sd = net.state_dict()
    names = [str(n) for n in GOLD[f"case{ci}_names"]]
    shapes = [tuple(int(s) for s in str(v).split(",") if s) for v in GOLD[f"case{ci}_shapes"]]
    assert list(sd) == names
    assert [tuple(v.shape) for v in sd.values()] == shapes
    if motion_init.CASES[ci][4]:
        assert names[:2] == ["rot_scale", "trans_scale"] and sd["rot_scale"].dim() == 0
    net.load_state_dict({n: torch.zeros(s) for n, s in zip(names, shapes)}, strict=True)      # a zero-filled reference state dict loads strictly
    assert all(float(v.abs().sum()) == 0 for v in net.state_dict().values())


def test_initialisation():
    torch.manual_seed(0)
    for constrain, scale in (("clip", 0.01), ("clip_ste", 0.01), ("softplus", 0.4)):
        net = build(("GoogleMotionNet", True, constrain, True, True, True))
        assert net.rot_scale.item() == pytest.approx(scale) and net.trans_scale.item() == pytest.approx(scale)
        for n, p in net.named_parameters():
            if n.endswith(".0.bias") or n == "conv8.bias":
                assert float(p.abs().sum()) == 0, n
        w = net.refiner3.conv21[0].weight                    # xavier-uniform: |w| <= sqrt(6 / (fan_in + fan_out))
        bound = (6.0 / ((w.shape[0] + w.shape[1]) * 9)) ** 0.5
        assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound
        assert "refiner0.conv1.1.weight" not in net.state_dict() and "refiner1.conv1.1.weight" in net.state_dict()
        assert net.motion_weight == 1.0


def test_reference_config_blocks_merge(tmp_path):
    cfg = get_cfg()
    pn = cfg.MODEL.POSE_NET
    assert (pn.USE_DEPTH, pn.GROUP_NORM, pn.MASK_MOTION, pn.LEARN_SCALE, pn.SCALE_CONSTRAIN, pn.BURN_IN_ITERS) == (True, False, True, True, "clip", 20000)
    assert pn.NAME == "PoseNet"
    (tmp_path / "Base.yaml").write_text(BASE_YAML)
    (tmp_path / "resnet18.yaml").write_text(RESNET18_YAML)
    cfg.merge_from_file(str(tmp_path / "resnet18.yaml"))
    assert cfg.MODEL.POSE_NET.NAME == "GoogleMotionNet" and cfg.MODEL.POSE_NET.SCALE_CONSTRAIN == "clip_ste"
    net = build_pose_net(cfg)
    assert net.scale_constrain == "clip_ste" and net.mask_motion and net.learn_scale and net.burn_in_iters == 20000


def test_unknown_constraint_and_fp16_raise():
    with pytest.raises(NotImplementedError):
        build(("GoogleMotionNet", False, "sigmoid", True, True, True))
    for name in ("GoogleMotionNet", "GooglePoseNet"):
        with pytest.raises(NotImplementedError):
            build((name, False, "clip", True, True, True), "fp16")
    build(("GoogleMotionNet", False, "clip", True, True, True), "bf16")


def test_posenet_builds_the_same_keys():
    cfg = get_cfg()
    keys = list(build_pose_net(cfg).state_dict())
    want = [f"conv{i}.{j}.{k}" for i in range(1, 8) for j in (0, 1) for k in ("weight", "bias")] + ["pose_pred.weight", "pose_pred.bias"]
    assert keys == want
    cfg.MODEL.POSE_NET.GROUP_NORM, cfg.MODEL.POSE_NET.LEARN_SCALE = False, False          # the new keys are not PoseNet's
    assert list(build_pose_net(cfg).state_dict()) == want


def test_new_entry_points_do_not_synchronise():
    src = open(os.path.join(ROOT, "simpledepthestimation_amd", "csrc", "motion.hip")).read()
    assert not re.search(r"hip(Stream|Device)Synchronize|hipEventSynchronize|hipMemcpy\s*\(", src)
    py = open(os.path.join(ROOT, "simpledepthestimation_amd", "hip", "motion.py")).read()
    assert not re.search(r"\.item\(\)|\.cpu\(\)|\.tolist\(\)|synchronize", py)

"""CPU: the ResNet-101 and ResNeXt-101 32x8d encoders of BtsModel (MODEL.DEPTH_NET.ENCODER_NAME resnet101_bts / resnext101_bts; reference list:
BTSNet.py:L278-313) build with torchvision's state-dict layout, and the grouped-convolution plumbing beneath them refuses what it cannot run."""
import json
import os
import re

import numpy as np
import pytest
import torch

import resnext_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "bts.npz"))
NEW_ENTRY_POINTS = ["sde_gconv3x3_stats_rows", "sde_gconv3x3_fwd", "sde_gconv3x3_dgrad", "sde_gconv3x3_wgrad_ws_bytes", "sde_gconv3x3_wgrad"]
NETS = {"resnet101_bts": (resnext_ref.resnet101, 44_549_160), "resnext101_bts": (resnext_ref.resnext101_32x8d, 88_791_336)}


def bts_cfg(size=128, name="resnet50_bts"):
    """The reference's Supervised/bts_r50.yaml with another encoder name."""
    from simpledepthestimation_amd.config import get_cfg
    with open(os.path.join(ROOT, "tests", "golden", "configs.json")) as f:
        entry = json.load(f)["Supervised/bts_r50.yaml"]
    cfg = get_cfg()
    cfg.MODEL.DATASET = entry["MODEL"]["DATASET"]
    for k, v in entry["MODEL"]["DEPTH_NET"].items():
        cfg.MODEL.DEPTH_NET[k] = v
    cfg.MODEL.DEPTH_NET.BTS_SIZE, cfg.MODEL.DEPTH_NET.ENCODER_NAME = size, name
    return cfg


@pytest.fixture(scope="module", params=list(NETS))
def built(request):
    from simpledepthestimation_amd.modeling.depth_net import build_depth_net
    torch.manual_seed(0)
    return request.param, build_depth_net(bts_cfg(128, name=request.param)), NETS[request.param][0]()


def test_builds_with_the_bts_decoder_widths(built):
    name, model, _ = built
    assert type(model).__name__ == "BtsModel" and model.encoder.encoder_name == name
    assert model.encoder.feat_out_channels == [64, 256, 512, 1024, 2048]
    assert list(model.encoder.num_ch_enc) == [64, 256, 512, 1024, 2048]


def test_state_dict_equals_the_restatement_and_loads_both_ways(built):
    name, model, ref = built
    ours, theirs = model.encoder.base_model.state_dict(), ref.state_dict()
    assert list(ours) == list(theirs)
    assert [tuple(v.shape) for v in ours.values()] == [tuple(v.shape) for v in theirs.values()]
    assert sum(p.numel() for p in model.encoder.base_model.parameters()) == NETS[name][1] == sum(p.numel() for p in ref.parameters())
    model.encoder.base_model.load_state_dict(theirs, strict=True)
    assert torch.equal(model.encoder.base_model.layer3[22].conv2.weight, ref.layer3[22].conv2.weight)
    ref.load_state_dict(model.encoder.base_model.state_dict(), strict=True)
    # ... and under the reference's checkpoint prefix
    assert "encoder.base_model.layer3.22.bn2.running_var" in model.state_dict()


def test_grouped_layer_shapes(built):
    name, model, _ = built
    from simpledepthestimation_amd.layers.hip_modules import HipConv2d, HipGroupedConv2d
    bm = model.encoder.base_model
    if name == "resnext101_bts":
        assert tuple(bm.layer1[0].conv2.weight.shape) == (256, 8, 3, 3) and tuple(bm.layer4[0].conv2.weight.shape) == (2048, 64, 3, 3)
        grouped = [m for m in bm.modules() if isinstance(m, HipGroupedConv2d)]
        assert len(grouped) == 33 and all(m.groups == 32 for m in grouped)
        assert [m.stride for m in (bm.layer1[0].conv2, bm.layer2[0].conv2, bm.layer3[0].conv2, bm.layer4[0].conv2)] == [1, 2, 2, 2]
        assert not hasattr(grouped[0], "_pack_shapes") and not hasattr(grouped[0], "_packed")       # WeightPacker passes these layers by
    else:
        assert tuple(bm.layer1[0].conv2.weight.shape) == (64, 64, 3, 3)
        assert not any(isinstance(m, HipGroupedConv2d) for m in bm.modules()) and isinstance(bm.layer3[22].conv2, HipConv2d)


def test_set_misc_freezes_the_same_names_as_for_resnet50(built):
    name, model, _ = built
    frozen = {n for n, p in model.named_parameters() if not p.requires_grad}
    enc = [n for n, _ in model.named_parameters() if n.startswith("encoder.")]
    assert frozen == {n for n in enc if "base_model.conv1" in n or ".bn" in n}
    assert "encoder.base_model.conv1.weight" in frozen and "encoder.base_model.layer3.22.bn2.weight" in frozen
    assert "encoder.base_model.layer2.0.downsample.1.weight" not in frozen and "encoder.base_model.layer1.0.conv2.weight" not in frozen
    # the ResNet-50 rule itself, from the golden file: every frozen name of that network is frozen here too
    r50_trainable = set(GOLD["trainable_none"])
    r50_frozen = {n for n in GOLD["names"] if n.startswith("encoder.") and n.endswith((".weight", ".bias")) and "running" not in n and n not in r50_trainable}
    assert {n for n in r50_frozen if ".fc." not in n} <= frozen


def test_default_encoder_is_unchanged():
    """ResnetEncoder(50) / resnet50_bts build exactly the parent's network: the golden key, shape and trainable lists still hold."""
    from simpledepthestimation_amd.layers.hip_modules import HipGroupedConv2d
    from simpledepthestimation_amd.layers.resnet_encoder import ResnetEncoder
    from simpledepthestimation_amd.modeling.depth_net import build_depth_net
    sd = build_depth_net(bts_cfg(512)).state_dict()            # (the golden names and shapes are the BTS_SIZE 512 network's, the trainable list BTS_SIZE 128's)
    assert list(sd) == list(GOLD["names"]) and [",".join(str(s) for s in v.shape) for v in sd.values()] == list(GOLD["shapes"])
    assert [n for n, p in build_depth_net(bts_cfg(128)).named_parameters() if p.requires_grad] == list(GOLD["trainable_none"])
    enc = ResnetEncoder(50)
    assert ["encoder.base_model." + k[len("encoder."):] for k in enc.state_dict()] == [n for n in GOLD["names"] if n.startswith("encoder.")]
    assert not any(isinstance(x, HipGroupedConv2d) for x in enc.modules())
    assert tuple(enc.encoder.layer2[0].conv2.weight.shape) == (128, 128, 3, 3) and enc.encoder.layer2[0].conv2.stride == 2


def test_resnext50_geometry_builds_below_the_refused_name():
    """resnext50_bts stays refused (tests/test_bts.py), but the containers build its network: 32 groups of 4 channels in layer 1."""
    from simpledepthestimation_amd.layers.resnet_encoder import ResnetEncoder
    enc = ResnetEncoder(50, groups=32, width_per_group=4)
    ref = resnext_ref.resnext50_32x4d()
    assert [(k, tuple(v.shape)) for k, v in enc.encoder.state_dict().items()] == [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    assert sum(p.numel() for p in enc.encoder.parameters()) == 25_028_904
    assert tuple(enc.encoder.layer1[0].conv2.weight.shape) == (128, 4, 3, 3)
    with pytest.raises(ValueError, match="BasicBlock"):
        ResnetEncoder(18, groups=32, width_per_group=4)


@pytest.mark.parametrize("channels,groups,stride", [(32, 16, 1), (24, 3, 1), (256, 2, 1), (64, 8, 3), (64, 5, 1)])
def test_grouped_module_refuses_unsupported_geometry(channels, groups, stride):
    from simpledepthestimation_amd.layers.hip_modules import HipGroupedConv2d
    with pytest.raises(NotImplementedError, match="channels / groups in"):
        HipGroupedConv2d(channels, groups, stride)


def test_grouped_module_initialises_like_torch():
    from simpledepthestimation_amd.layers.hip_modules import HipGroupedConv2d
    torch.manual_seed(3)
    ours = HipGroupedConv2d(64, 8, 2)
    torch.manual_seed(3)
    theirs = torch.nn.Conv2d(64, 64, 3, 2, 1, groups=8, bias=False)
    assert torch.equal(ours.weight, theirs.weight) and ours.bias is None and list(ours.state_dict()) == ["weight"]


def test_new_entry_points_are_declared_and_bound():
    from simpledepthestimation_amd.hip import lib as L
    from simpledepthestimation_amd.hip import nn  # noqa: F401
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sde_hip.h")).read(), flags=re.S)
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L._PROTOS, name
    if L.available():
        lib = L.lib()
        # shape-only queries answer without a GPU: the workload's first grouped layer (bf16, 8 x 88 x 176 x 256, 32 groups), and a refusal
        assert lib.sde_gconv3x3_stats_rows(8, 88, 176, 256, 32, 1, L.BF16) > 0
        assert lib.sde_gconv3x3_wgrad_ws_bytes(8, 88, 176, 256, 32, 1, L.BF16) % (256 * 9 * 16 * 4) == 0
        assert lib.sde_gconv3x3_stats_rows(8, 88, 176, 256, 128, 1, L.BF16) == -1 and b"not supported" in lib.sde_last_error()

"""CPU: the DenseNet-121 encoder of BtsModel (MODEL.DEPTH_NET.ENCODER_NAME densenet121_bts; reference list: BTSNet.py:L283-311) builds with
torchvision's state-dict layout and the reference's frozen set, the containers also build DenseNet-161's geometry, and the dense-block entry
points are declared, bound and refuse what they cannot run."""
import ctypes
import json
import os
import re

import pytest
import torch

import densenet_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ["sde_dense_stats", "sde_dense_bwd_rows", "sde_dense_bn_relu_fwd", "sde_dense_bn_relu_bwd", "sde_dense_grad_gather",
                    "sde_avgpool2x2_fwd", "sde_avgpool2x2_bwd"]


def bts_cfg(size=128, fix1=False, fix2=False, name="densenet121_bts"):
    """The reference's Supervised/bts_r50.yaml with another encoder name."""
    from simpledepthestimation_amd.config import get_cfg
    with open(os.path.join(ROOT, "tests", "golden", "configs.json")) as f:
        entry = json.load(f)["Supervised/bts_r50.yaml"]
    cfg = get_cfg()
    cfg.MODEL.DATASET = entry["MODEL"]["DATASET"]
    for k, v in entry["MODEL"]["DEPTH_NET"].items():
        cfg.MODEL.DEPTH_NET[k] = v
    cfg.MODEL.DEPTH_NET.BTS_SIZE, cfg.MODEL.DEPTH_NET.FIX_1ST_CONV, cfg.MODEL.DEPTH_NET.FIX_1ST_CONVS = size, fix1, fix2
    cfg.MODEL.DEPTH_NET.ENCODER_NAME = name
    return cfg


@pytest.fixture(scope="module")
def built():
    from simpledepthestimation_amd.modeling.depth_net import build_depth_net
    torch.manual_seed(0)
    return build_depth_net(bts_cfg()), densenet_ref.densenet121()


def test_builds_with_the_bts_decoder_widths(built):
    model, _ = built
    assert type(model).__name__ == "BtsModel" and model.encoder.encoder_name == "densenet121_bts"
    assert model.encoder.feat_out_channels == [64, 64, 128, 256, 1024]
    assert model.decoder.fc == [64, 64, 128, 256, 1024]


def test_state_dict_equals_the_restatement_and_loads_both_ways(built):
    model, ref = built
    ours, theirs = model.encoder.base_model.state_dict(), ref.state_dict()
    assert list(ours) == list(theirs)
    assert [tuple(v.shape) for v in ours.values()] == [tuple(v.shape) for v in theirs.values()]
    assert sum(p.numel() for p in model.encoder.base_model.parameters()) == 6_953_856 == sum(p.numel() for p in ref.parameters())
    model.encoder.base_model.load_state_dict(theirs, strict=True)
    assert torch.equal(model.encoder.base_model.denseblock3.denselayer24.conv2.weight, ref.denseblock3.denselayer24.conv2.weight)
    ref.load_state_dict(model.encoder.base_model.state_dict(), strict=True)
    assert "encoder.base_model.denseblock3.denselayer24.conv2.weight" in model.state_dict()
    assert "encoder.base_model.norm5.num_batches_tracked" in model.state_dict()


def test_initialisation_is_torchvisions():
    from simpledepthestimation_amd.layers.densenet_encoder import DenseNetFeatures
    torch.manual_seed(5)
    ours = DenseNetFeatures(16, (2, 2, 2, 2), 32)
    torch.manual_seed(5)
    ref = densenet_ref.DenseNetFeatures(16, (2, 2, 2, 2), 32)
    a, b = ours.state_dict(), ref.state_dict()
    assert list(a) == list(b)
    assert float(ours.denseblock1.denselayer1.norm1.weight.detach().min()) == 1.0 and float(ours.norm5.bias.detach().abs().max()) == 0.0
    w = ours.denseblock2.denselayer1.conv2.weight
    assert abs(float(w.detach().std()) - (2.0 / (w.shape[1] * 9)) ** 0.5) < 0.1 * (2.0 / (w.shape[1] * 9)) ** 0.5        # kaiming_normal_, fan_in


def test_densenet161_geometry_builds_below_the_refused_name():
    """densenet161_bts stays refused (tests/test_bts.py), but the containers build its network."""
    from simpledepthestimation_amd.layers.densenet_encoder import DenseNetEncoder
    from simpledepthestimation_amd.modeling.depth_net import build_depth_net
    enc = DenseNetEncoder(48, (6, 12, 36, 24), 96)
    ref = densenet_ref.densenet161()
    assert [(k, tuple(v.shape)) for k, v in enc.base_model.state_dict().items()] == [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    assert sum(p.numel() for p in enc.base_model.parameters()) == 26_472_000
    assert enc.base_model.norm5.num_features == 2208 and enc.feat_out_channels == [96, 96, 192, 384, 2208]
    assert enc.base_model.transition3.norm.num_features == 384 + 36 * 48
    with pytest.raises(NotImplementedError, match="densenet121_bts"):
        build_depth_net(bts_cfg(name="densenet161_bts"))


@pytest.mark.parametrize("fix1,fix2,extra", [(False, False, []), (True, False, ["denseblock1.denselayer1"]),
                                             (False, True, ["denseblock1.denselayer1", "denseblock1.denselayer2"])])
def test_set_misc_freezes_the_non_resnet_branch(fix1, fix2, extra):
    from simpledepthestimation_amd.modeling.depth_net import build_depth_net
    model = build_depth_net(bts_cfg(128, fix1, fix2))
    frozen = {n for n, p in model.named_parameters() if not p.requires_grad}
    enc = [n for n, _ in model.encoder.named_parameters()]
    rule = ["conv0", "norm"] + extra
    assert frozen == {"encoder." + n for n in enc if any(s in n for s in rule)}
    assert "encoder.base_model.conv0.weight" in frozen and "encoder.base_model.denseblock4.denselayer16.norm2.bias" in frozen
    assert "encoder.base_model.transition2.norm.weight" in frozen and "encoder.base_model.transition2.conv.weight" not in frozen
    assert ("encoder.base_model.denseblock1.denselayer1.conv1.weight" in frozen) == (fix1 or fix2)
    assert ("encoder.base_model.denseblock1.denselayer2.conv2.weight" in frozen) == fix2
    assert "encoder.base_model.denseblock1.denselayer3.conv1.weight" not in frozen
    assert not any(n.startswith("decoder.") for n in frozen)


def test_resnet_branch_of_set_misc_is_unchanged():
    from simpledepthestimation_amd.modeling.depth_net import build_depth_net
    model = build_depth_net(bts_cfg(128, True, False, name="resnet50_bts"))
    frozen = {n for n, p in model.named_parameters() if not p.requires_grad}
    enc = [n for n, _ in model.named_parameters() if n.startswith("encoder.")]
    assert frozen == {n for n in enc if "base_model.conv1" in n or ".bn" in n or "base_model.layer1.0" in n}


def test_new_entry_points_are_declared_and_bound():
    from simpledepthestimation_amd.hip import dense as HD
    from simpledepthestimation_amd.hip import lib as L
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sde_hip.h")).read(), flags=re.S)
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L._PROTOS, name
    assert int(re.search(r"#define\s+SDE_DENSE_MAX\s+(\d+)", hdr).group(1)) == HD.DENSE_MAX == 40
    assert ctypes.sizeof(HD.DenseDesc) == 40 * 8 + 40 * 4 + 8
    if L.available():
        lib = L.lib()
        # shape-only queries answer without a GPU: DenseNet-121's widest layer at 8 x 22 x 76 (bf16), one tiny shape, and the refusals
        assert 1 <= lib.sde_dense_bwd_rows(8 * 22 * 76, 1024, L.BF16) <= 64
        assert lib.sde_dense_bwd_rows(2, 16, L.F32) == 1
        assert lib.sde_dense_bwd_rows(64, 12, L.BF16) < 0 and b"multiple of 8" in lib.sde_last_error()
        assert lib.sde_dense_bwd_rows(64, 16, L.F16) < 0 and b"fp32 and bf16 only" in lib.sde_last_error()
        d = HD.DenseDesc()
        d.n = 41
        assert lib.sde_dense_bn_relu_fwd(ctypes.byref(d), 4, L.BF16, None, None, None, None, None, 0.1, 1e-5, None, None, None) < 0
        assert b"1..40 pieces" in lib.sde_last_error()

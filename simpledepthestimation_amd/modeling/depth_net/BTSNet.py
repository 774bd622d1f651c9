"""BtsModel = ResNet-50 / ResNet-101 / ResNeXt-101 32x8d / DenseNet-121 encoder + BTS decoder (reference: detectron2/modeling/depth_net/BTSNet.py:L281-413).

State-dict keys equal the reference's (``encoder.base_model.layer3.5.bn2.running_var``, ``decoder.get_depth.0.weight`` ...), so its
checkpoints load with ``strict=True``.  The encoder is this package's ResNet encoder (layers/resnet_encoder.py) with its torchvision module
registered under ``base_model``; the reference's `encoder` returns the same five features (relu, layer1..layer4).  ``densenet121_bts`` is
layers/densenet_encoder.py: torchvision's ``densenet121().features`` under ``base_model``, features relu0, pool0, transition1, transition2, norm5.
"""
import logging

import torch
import torch.nn as nn

from ...hip import nn as HN
from ...layers.bts_decoder import BtsDecoder
from ...layers.densenet_encoder import DenseNetEncoder
from ...layers.hip_modules import HipBatchNorm2d
from ...layers.resnet_encoder import ResnetEncoder
from .build import DEPTH_NET_REGISTRY
from .DepthResNet import compute_dtype

logger = logging.getLogger(__name__)

# MODEL.DEPTH_NET.ENCODER_NAME -> (layers, groups, width per group) of the torchvision network the reference wraps (BTSNet.py:L291-306)
_ENCODERS = {"resnet50_bts": (50, 1, 64), "resnet101_bts": (101, 1, 64), "resnext101_bts": (101, 32, 8)}
# ... -> (growth rate, block config, stem channels) of the torchvision DenseNet (BTSNet.py:L283-286).  The containers also build DenseNet-161's
# geometry (48, (6, 12, 36, 24), 96); that name is not enabled
_DENSENETS = {"densenet121_bts": (32, (6, 12, 24, 16), 64)}
_SUPPORTED = sorted(list(_ENCODERS) + list(_DENSENETS))


class BtsEncoder(ResnetEncoder):
    """ResnetEncoder whose torchvision-shaped module is named ``base_model`` (the reference's `encoder` wrapper, L281-335)."""

    def __init__(self, encoder_name):
        if encoder_name not in _ENCODERS:
            raise NotImplementedError(f"BtsModel encoder {encoder_name!r} is not on the HIP path; supported: {_SUPPORTED}")
        num_layers, groups, width = _ENCODERS[encoder_name]
        super().__init__(num_layers, groups=groups, width_per_group=width)
        self.encoder_name = encoder_name
        self.base_model = self._modules.pop("encoder")
        self.feat_out_channels = [64, 256, 512, 1024, 2048]
        logger.info(f"{encoder_name}: torchvision initialisation (ImageNet weights cannot be fetched here); "
                    "load pretrained weights through MODEL.WEIGHTS or load_state_dict")

    @property
    def encoder(self):       # ResnetEncoder.forward reads self.encoder
        return self.base_model


class BtsDenseNetEncoder(DenseNetEncoder):
    """DenseNetEncoder under the reference's encoder names (L283-286)."""

    def __init__(self, encoder_name):
        growth, blocks, stem = _DENSENETS[encoder_name]
        super().__init__(growth, blocks, stem)
        self.encoder_name = encoder_name
        logger.info(f"{encoder_name}: torchvision initialisation (ImageNet weights cannot be fetched here); "
                    "load pretrained weights through MODEL.WEIGHTS or load_state_dict")


def build_encoder(encoder_name):
    return BtsDenseNetEncoder(encoder_name) if encoder_name in _DENSENETS else BtsEncoder(encoder_name)


def set_misc(model, bn_no_track_stats, fix_first_conv_block, fix_first_conv_blocks):
    """BTSNet.py:L374-413: freeze encoder parameters by substring match on their names (``.bn`` does not match ``downsample.1``).  Encoders whose
    name does not contain ``resne`` take the reference's other branch (L387-404): ``conv0``, ``norm`` and the first dense layer(s)."""
    if bn_no_track_stats:
        # bn_init_as_tf: m.eval() on every BatchNorm -- the training loop's model.train() undoes it, as in the reference
        for m in model.modules():
            if isinstance(m, HipBatchNorm2d):
                m.eval()
    if "resne" in model.encoder_name:
        fixing = ["base_model.conv1", ".bn"]
        if fix_first_conv_blocks:
            fixing += ["base_model.layer1.0", "base_model.layer1.1"]
        elif fix_first_conv_block:
            fixing += ["base_model.layer1.0"]
    else:
        fixing = ["conv0", "norm"]
        if fix_first_conv_blocks:
            fixing += ["denseblock1.denselayer1", "denseblock1.denselayer2"]
        elif fix_first_conv_block:
            fixing += ["denseblock1.denselayer1"]
    for name, child in model.named_children():
        if "encoder" not in name:
            continue
        for name2, p in child.named_parameters():
            if any(x in name2 for x in fixing):
                p.requires_grad = False
    return model


@DEPTH_NET_REGISTRY.register()
class BtsModel(nn.Module):
    def __init__(self, cfg, **kwargs):
        super().__init__()
        dn = cfg.MODEL.DEPTH_NET
        self.encoder_name = dn.ENCODER_NAME
        self.encoder = build_encoder(dn.ENCODER_NAME)
        self.decoder = BtsDecoder(cfg.MODEL.DATASET, cfg.MODEL.MAX_DEPTH, self.encoder.feat_out_channels, dn.BTS_SIZE)
        self.dtype = compute_dtype(cfg)
        set_misc(self, dn.BN_NO_TRACK, dn.FIX_1ST_CONV, dn.FIX_1ST_CONVS)

    def forward(self, batch):
        """Adds depth_8x8, depth_4x4, depth_2x2, reduc_1x1 ([B,1,H,W] fp32) and depth_pred = [final_depth] (BTSNet.py:L350-371)."""
        if "intrinsics" not in batch:
            raise KeyError("BtsModel needs batch['intrinsics'] ([B,3,3]): the decoder reads the focal length intrinsics[:, 0, 0]")
        flip = bool(batch.get("flip", False))
        x = batch.get("depth_net_input_nhwc")
        if x is None:
            x = HN.prep_input(batch["depth_net_input"], None, None, self.dtype, flip)
        focal = batch["intrinsics"][:, 0, 0].float().contiguous()
        feats = self.encoder(x)
        d8, d4, d2, r1, final = self.decoder(feats, focal, flip)
        if flip:      # final_depth is mirrored inside its head kernel; the auxiliary maps are mirrored here
            d8, d4, d2, r1 = [torch.flip(d, [3]) for d in (d8, d4, d2, r1)]
        batch.update({"depth_8x8": d8, "depth_4x4": d4, "depth_2x2": d2, "reduc_1x1": r1, "depth_pred": [final]})
        return batch

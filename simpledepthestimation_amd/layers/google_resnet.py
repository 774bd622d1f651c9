"""GoogleResNet's encoder and decoder on the HIP path.

Reference: detectron2/modeling/depth_net/GoogleResNet.py:L21-68 (ResnetEncoder over detectron2/layers/resnet.py:L35-59's ResNetTF) and L72-123
(DepthDecoder: five UpsampleBlocks = bilinear x2 (align_corners) -> 3x3 conv + ReLU -> cat(skip) -> 3x3 conv + ReLU, then out_conv and softplus).
Attribute / state-dict names follow the reference (``encoder.encoder.layer2.0.downsample.0.weight``, ``decoder.blocks.3.iconv.bias``).

The encoder is layers/resnet_encoder.py's, in its bare-shortcut variant with the configured norm layer; only the decoder lives here.
"""
import numpy as np
import torch
import torch.nn as nn

from ..hip import bts as HB
from ..hip import google as HG
from .hip_modules import HipBatchNorm2d, HipConv2d, HipRandLayerNorm
from .resnet_encoder import ResnetEncoder

NORMS = {"BN": HipBatchNorm2d, "randLN": HipRandLayerNorm, None: HipBatchNorm2d}


class GoogleResnetEncoder(ResnetEncoder):
    """ResNetTF-18/34/50: the projection shortcut is a bare 1x1 convolution, built only where the width changes."""

    def __init__(self, num_layers, norm_layer=HipBatchNorm2d):
        super().__init__(num_layers, norm_layer=norm_layer, shortcut_norm=False)


def _conv3x3(cin, cout):
    return HipConv2d(cin, cout, 3, 1, 1, bias=True)


class UpsampleBlock(nn.Module):
    """GoogleResNet.py:L106-123: bilinear x2 (align_corners=True) -> upconv + ReLU [-> cat(skip)] -> iconv + ReLU."""

    def __init__(self, channel_in, channel_out, channel_cat=None):
        super().__init__()
        self.channel_out, self.channel_cat = int(channel_out), (int(channel_cat) if channel_cat else None)
        self.upconv = _conv3x3(channel_in, channel_out)
        self.iconv = _conv3x3(channel_out + (self.channel_cat or 0), channel_out)

    def forward(self, x, y=None):
        # the conv engine's epilogue applies no ReLU (ELU only): a separate ReLU pass, whose backward is the engine's activation backward
        out = HB.relu(self.upconv(HG.bilinear2(x)))
        if y is not None:
            out = HB.cat([(out, self.channel_out), (y, self.channel_cat)])
        return HB.relu(self.iconv(out))


class GoogleDepthDecoder(nn.Module):
    """GoogleResNet.py:L72-103.  ``scale`` (LEARN_SCALE) is a parameter the forward pass never reads, as in the reference."""

    def __init__(self, num_ch_enc, learn_scale=False):
        super().__init__()
        self.num_ch_enc = num_ch_enc
        self.num_ch_dec = np.array([16, 32, 64, 128, 256])
        self.scale = nn.Parameter(torch.ones(1), requires_grad=True) if learn_scale else None
        self.blocks = nn.ModuleList()
        for i in range(4, -1, -1):
            c_in = num_ch_enc[-1] if i == 4 else self.num_ch_dec[i + 1]
            c_cat = num_ch_enc[i - 1] if i > 0 else None
            self.blocks.append(UpsampleBlock(c_in, self.num_ch_dec[i], c_cat))
        self.out_conv = _conv3x3(self.num_ch_dec[0], 1)
        for m in self.modules():
            if isinstance(m, HipConv2d):
                nn.init.xavier_uniform_(m.weight.data)
                m.bias.data.zero_()

    def forward(self, features, flip=False):
        """features: the encoder's five NHWC maps -> depth [B,1,H,W] fp32 (softplus of out_conv; mirrored along x when flip)."""
        out = features[-1]
        for y, block in zip(features[-2::-1] + [None], self.blocks):
            out = block(out, y)
        return HG.softplus_head(self.out_conv(out), flip)

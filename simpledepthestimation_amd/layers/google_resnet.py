"""GoogleResNet's encoder and decoder on the HIP path.

Reference: detectron2/modeling/depth_net/GoogleResNet.py:L21-68 (ResnetEncoder over detectron2/layers/resnet.py:L35-59's ResNetTF) and L72-123
(DepthDecoder: five UpsampleBlocks = bilinear x2 (align_corners) -> 3x3 conv + ReLU -> cat(skip) -> 3x3 conv + ReLU, then out_conv and softplus);
GoogleResNetv2.py:L80-170 (the same ResNet-18 under other names, and a decoder that up-samples with a transposed convolution).
Attribute / state-dict names follow the reference (``encoder.encoder.layer2.0.downsample.0.weight``, ``decoder.blocks.3.iconv.bias``).

The encoder is layers/resnet_encoder.py's, in its bare-shortcut variant with the configured norm layer; only the decoder lives here.
"""
import numpy as np
import torch
import torch.nn as nn

from ..hip import bts as HB
from ..hip import google as HG
from ..hip import nn as HN
from .hip_modules import HipBatchNorm2d, HipConv2d, HipConvTranspose2d, HipRandLayerNorm
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


class _Decoder(nn.Module):
    """What the two decoders share: [scale,] blocks, out_conv in the reference's registration order, xavier-uniform weights with zero biases, and the walk
    over the encoder's features (deepest first, the last block without a skip) into the softplus head."""

    def _build(self, blocks, c_last, learn_scale):
        self.scale = nn.Parameter(torch.ones(1), requires_grad=True) if learn_scale else None
        self.blocks = nn.ModuleList(blocks)
        self.out_conv = _conv3x3(c_last, 1)
        for m in self.modules():
            if isinstance(m, (HipConv2d, HipConvTranspose2d)):
                nn.init.xavier_uniform_(m.weight.data)
                m.bias.data.zero_()

    def forward(self, features, flip=False):
        """features: the encoder's five NHWC maps -> depth [B,1,H,W] fp32 (softplus of out_conv; mirrored along x when flip)."""
        out = features[-1]
        for y, block in zip(features[-2::-1] + [None], self.blocks):
            out = block(out, y)
        return HG.softplus_head(self.out_conv(out), flip)


class GoogleDepthDecoder(_Decoder):
    """GoogleResNet.py:L72-103.  ``scale`` (LEARN_SCALE) is a parameter the forward pass never reads, as in the reference."""

    def __init__(self, num_ch_enc, learn_scale=False):
        super().__init__()
        self.num_ch_enc = num_ch_enc
        self.num_ch_dec = np.array([16, 32, 64, 128, 256])
        blocks = []
        for i in range(4, -1, -1):
            c_in = num_ch_enc[-1] if i == 4 else self.num_ch_dec[i + 1]
            c_cat = num_ch_enc[i - 1] if i > 0 else None
            blocks.append(UpsampleBlock(c_in, self.num_ch_dec[i], c_cat))
        self._build(blocks, self.num_ch_dec[0], learn_scale)


# ---------------------------------------------------------------------------------------------------------------
# GoogleResNetv2 (detectron2/modeling/depth_net/GoogleResNetv2.py:L80-170)
# ---------------------------------------------------------------------------------------------------------------
class GoogleResnetEncoderV2(GoogleResnetEncoder):
    """GoogleResNetv2.py:L80-124: the same bare-shortcut ResNet-18 (layers/resnet_encoder.py's skeleton and forward walk) under the v2 file's names --
    no wrapper level (``encoder.conv1``, not ``encoder.encoder.conv1``), the shortcut a bare convolution (``downsample.weight``, not
    ``downsample.0.weight``) registered ahead of the block's conv1, and no ``fc``.  Only the state dict is renamed, on its way out and in."""

    def __init__(self, norm_layer=HipBatchNorm2d):
        super().__init__(18, norm_layer)
        del self.encoder.fc
        self._register_state_dict_hook(self._to_reference_names)
        self._register_load_state_dict_pre_hook(self._from_reference_names)

    @staticmethod
    def _to_reference_names(module, sd, prefix, local_metadata):
        mine = [k for k in sd if k.startswith(prefix)]
        out = []
        for k in mine:
            name = k[len(prefix) + len("encoder."):].replace("downsample.0.", "downsample.")
            if ".downsample." in name:                   # the reference's block registers its shortcut first
                block = name[:name.index("downsample.")]
                out.insert(next(i for i, (n, _) in enumerate(out) if n.startswith(block)), (name, sd.pop(k)))
            else:
                out.append((name, sd.pop(k)))
        for name, v in out:
            sd[prefix + name] = v

    @staticmethod
    def _from_reference_names(sd, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        for k in [k for k in sd if k.startswith(prefix) and not k.startswith(prefix + "encoder.")]:
            sd[prefix + "encoder." + k[len(prefix):].replace("downsample.", "downsample.0.")] = sd.pop(k)


class UpsampleBlockV2(nn.Module):
    """GoogleResNetv2.py:L127-138: upconv = ConvTranspose2d(3, stride 2, padding 1, output_padding 1) + ReLU [-> cat(skip)] -> iconv + ReLU."""

    def __init__(self, channel_in, channel_out, channel_cat=None):
        super().__init__()
        self.channel_out, self.channel_cat = int(channel_out), (int(channel_cat) if channel_cat else None)
        self.upconv = HipConvTranspose2d(channel_in, channel_out, 3, stride=2, padding=1, output_padding=1, bias=True)
        self.iconv = _conv3x3(channel_out + (self.channel_cat or 0), channel_out)

    def forward(self, x, y=None):
        out = self.upconv(x, act=HN.ACT_RELU)            # bias + ReLU in the transposed convolution's epilogue
        if y is not None:
            out = HB.cat([(out, self.channel_out), (y, self.channel_cat)])
        return HB.relu(self.iconv(out))


class GoogleDepthDecoderV2(_Decoder):
    """GoogleResNetv2.py:L141-170: five UpsampleBlockV2 over the fixed ResNet-18 widths, skips out3, out2, out1, out0, none."""

    def __init__(self, learn_scale=False):
        super().__init__()
        self.channels = [512, 256, 128, 64, 32, 16]
        self.enc_channels = [256, 128, 64, 64, None]
        blocks = [UpsampleBlockV2(c_in, c_out, c_mid) for c_in, c_out, c_mid in zip(self.channels[:-1], self.channels[1:], self.enc_channels)]
        self._build(blocks, self.channels[-1], learn_scale)

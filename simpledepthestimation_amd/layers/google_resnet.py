"""GoogleResNet's encoder (ResNetTF) and decoder on the HIP path.

Reference: detectron2/layers/resnet.py:L35-59 (ResNetTF: torchvision's ResNet whose projection shortcut is a bare 1x1 convolution, no norm
layer) under detectron2/modeling/depth_net/GoogleResNet.py:L21-68 (ResnetEncoder: relu(norm(conv1)), layer1(maxpool), layer2-4) and
L72-123 (DepthDecoder: five UpsampleBlocks = bilinear x2 (align_corners) -> 3x3 conv + ReLU -> cat(skip) -> 3x3 conv + ReLU, then out_conv and
softplus).  Attribute / state-dict names follow the reference (``encoder.encoder.layer2.0.downsample.0.weight``, ``decoder.blocks.3.iconv.bias``).

This is a sibling of layers/resnet_encoder.py, not a variant of it: that encoder (DepthResNet, BtsModel) keeps its BatchNorm'd shortcut.
"""
import numpy as np
import torch
import torch.nn as nn

from ..hip import bts as HB
from ..hip import google as HG
from ..hip import nn as HN
from .hip_modules import HipBatchNorm2d, HipConv2d, HipRandLayerNorm, conv_bn


def conv_norm(conv, norm, x, residual=None, relu=True, n_out=1):
    """conv -> norm [-> + residual] [-> ReLU] for either norm layer (BatchNorm takes its statistics from the convolution's epilogue)."""
    if isinstance(norm, HipBatchNorm2d):
        return conv_bn(conv, norm, x, residual, relu, n_out)
    return norm(conv(x), residual, relu, n_out)


class BasicBlockTF(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride, downsample, norm_layer):
        super().__init__()
        self.conv1 = HipConv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = norm_layer(planes)
        self.conv2 = HipConv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = norm_layer(planes)
        self.downsample = downsample

    def forward(self, x, n_out=1):
        xa, xb = x if isinstance(x, tuple) else (x, x)       # two aliases of the block input: one per consumer
        idt = xb if self.downsample is None else self.downsample[0](xb)
        out = conv_norm(self.conv1, self.bn1, xa)
        return conv_norm(self.conv2, self.bn2, out, residual=idt, relu=True, n_out=n_out)


class BottleneckTF(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride, downsample, norm_layer):
        super().__init__()
        self.conv1 = HipConv2d(inplanes, planes, 1, 1, 0, bias=False)
        self.bn1 = norm_layer(planes)
        self.conv2 = HipConv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = norm_layer(planes)
        self.conv3 = HipConv2d(planes, planes * 4, 1, 1, 0, bias=False)
        self.bn3 = norm_layer(planes * 4)
        self.downsample = downsample

    def forward(self, x, n_out=1):
        xa, xb = x if isinstance(x, tuple) else (x, x)
        idt = xb if self.downsample is None else self.downsample[0](xb)
        out = conv_norm(self.conv1, self.bn1, xa)
        out = conv_norm(self.conv2, self.bn2, out)
        return conv_norm(self.conv3, self.bn3, out, residual=idt, relu=True, n_out=n_out)


class ResNetTF(nn.Module):
    """torchvision-shaped container (conv1, bn1, layer1..4, fc); ``fc`` is kept only so checkpoints load."""

    def __init__(self, block, layers, norm_layer, num_classes=1000):
        super().__init__()
        self.norm_layer = norm_layer
        self.inplanes = 64
        self.conv1 = HipConv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = norm_layer(64)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2)
        self.fc = nn.Linear(512 * block.expansion, num_classes)
        for m in self.modules():
            if isinstance(m, HipConv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(HipConv2d(self.inplanes, planes * block.expansion, 1, stride, 0, bias=False))
        elif stride != 1:
            raise NotImplementedError("ResNetTF's max-pool shortcut (resnet.py:L47-48) is not on the HIP path")
        layers = [block(self.inplanes, planes, stride, downsample, self.norm_layer)]
        self.inplanes = planes * block.expansion
        layers += [block(self.inplanes, planes, 1, None, self.norm_layer) for _ in range(1, blocks)]
        return nn.Sequential(*layers)


_SPECS = {18: (BasicBlockTF, [2, 2, 2, 2]), 34: (BasicBlockTF, [3, 4, 6, 3]), 50: (BottleneckTF, [3, 4, 6, 3])}
NORMS = {"BN": HipBatchNorm2d, "randLN": HipRandLayerNorm, None: HipBatchNorm2d}


class GoogleResnetEncoder(nn.Module):
    def __init__(self, num_layers, norm_layer=HipBatchNorm2d):
        super().__init__()
        if num_layers not in _SPECS:
            raise ValueError("{} is not a valid number of resnet layers".format(num_layers))
        self.num_ch_enc = np.array([64, 64, 128, 256, 512])
        block, layers = _SPECS[num_layers]
        self.encoder = ResNetTF(block, layers, norm_layer)
        if num_layers > 34:
            self.num_ch_enc[1:] *= 4

    def forward(self, x):
        """x: NHWC normalised image (channels padded).  Returns the 5 NHWC feature maps."""
        e = self.encoder
        split = torch.is_grad_enabled()      # aliases only matter for backward

        def run(layer, x, last_n):
            """Every block output but the last gets two aliases (conv1 + shortcut of the next block), the last one `last_n`."""
            blocks = list(layer)
            for i, blk in enumerate(blocks):
                x = blk(x, n_out=(2 if i + 1 < len(blocks) else last_n) if split else 1)
            return x

        if split:
            f0, f0_pool = conv_norm(e.conv1, e.bn1, x, n_out=2)          # decoder skip + max-pool
            o1 = run(e.layer1, HN.max_pool_3x3_s2(f0_pool, n_out=2), 3)
            o2 = run(e.layer2, (o1[1], o1[2]), 3)
            o3 = run(e.layer3, (o2[1], o2[2]), 3)
            f4 = run(e.layer4, (o3[1], o3[2]), 1)
            return [f0, o1[0], o2[0], o3[0], f4]
        f0 = conv_norm(e.conv1, e.bn1, x)
        f1 = run(e.layer1, HN.max_pool_3x3_s2(f0), 1)
        f2 = run(e.layer2, f1, 1)
        f3 = run(e.layer3, f2, 1)
        return [f0, f1, f2, f3, run(e.layer4, f3, 1)]


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

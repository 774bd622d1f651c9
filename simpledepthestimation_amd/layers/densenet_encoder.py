"""DenseNet encoder (torchvision ``densenet121().features``) on the HIP path, for BtsModel (reference: BTSNet.py:L283-290, L318-333).

Module tree and state-dict keys are torchvision's: ``conv0``, ``norm0``, ``denseblockK.denselayerL.{norm1,conv1,norm2,conv2}``,
``transitionK.{norm,conv}``, ``norm5`` (the parameter-free relu / pool members are not modules here), so its checkpoints load with
``strict=True``.  Initialisation as torchvision: kaiming-normal convolutions, BatchNorm 1 / 0.

A dense block never concatenates: it is a hip.dense.DenseBlock of pieces, and ``norm1`` / the transition's ``norm`` / ``norm5`` run as
hip.dense.dense_bn_relu over them (hip.dense.DENSE_DIRECT = False: the composed route through cat + channel_stats + BatchNorm).  The two
convolutions and ``norm2`` of a layer are the ordinary HipConv2d / conv_bn.
"""
import torch
import torch.nn as nn

from ..hip import bts as HB
from ..hip import dense as HD
from ..hip import nn as HN
from .hip_modules import HipBatchNorm2d, HipConv2d, conv_bn


class DenseLayer(nn.Module):
    def __init__(self, in_channels, growth_rate, bn_size):
        super().__init__()
        self.norm1 = HipBatchNorm2d(in_channels)
        self.conv1 = HipConv2d(in_channels, bn_size * growth_rate, 1, 1, 0, bias=False)
        self.norm2 = HipBatchNorm2d(bn_size * growth_rate)
        self.conv2 = HipConv2d(bn_size * growth_rate, growth_rate, 3, 1, 1, bias=False)

    def forward(self, blk):
        """Reads the block's pieces, files its own output as the next one."""
        y = conv_bn(self.conv1, self.norm2, HD.dense_bn_relu(blk, self.norm1))
        if blk.track:
            y, stats = self.conv2(y, bn_stats=True)
        else:
            y, stats = self.conv2(y), None
        return HD.dense_piece(y, blk, stats)


class DenseBlockModule(nn.Module):
    def __init__(self, num_layers, in_channels, growth_rate, bn_size):
        super().__init__()
        for i in range(num_layers):
            self.add_module(f"denselayer{i + 1}", DenseLayer(in_channels + i * growth_rate, growth_rate, bn_size))
        self.out_channels = in_channels + num_layers * growth_rate
        if num_layers + 1 > HD.DENSE_MAX:
            raise NotImplementedError(f"a dense block of {num_layers} layers has more than {HD.DENSE_MAX} pieces")

    def forward(self, x, norm_after):
        """x: the block input.  Returns (the block input as its first piece, relu(norm_after(block output))): the norm behind the block is the
        transition's or norm5."""
        track = any(m.training for m in self.modules() if isinstance(m, HipBatchNorm2d)) or norm_after.training
        blk = HD.DenseBlock(self.out_channels, track)
        x = x.contiguous()
        first = HD.dense_piece(x, blk, HB.channel_stats(x) if (track and HD.DENSE_DIRECT) else None)
        for layer in self.children():
            layer(blk)
        out = HD.dense_bn_relu(blk, norm_after)
        blk.close()
        return first, out


class Transition(nn.Module):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.norm = HipBatchNorm2d(in_channels)
        self.conv = HipConv2d(in_channels, out_channels, 1, 1, 0, bias=False)


class DenseNetFeatures(nn.Module):
    """torchvision's DenseNet.features for any growth_rate / block_config / num_init_features (DenseNet-161: 48, (6, 12, 36, 24), 96)."""

    def __init__(self, growth_rate=32, block_config=(6, 12, 24, 16), num_init_features=64, bn_size=4):
        super().__init__()
        if growth_rate % 8 or num_init_features % 8:
            raise NotImplementedError("DenseNet on the HIP path needs growth_rate and num_init_features that are multiples of 8")
        self.conv0 = HipConv2d(3, num_init_features, 7, 2, 3, bias=False)
        self.norm0 = HipBatchNorm2d(num_init_features)
        nf = num_init_features
        self.num_blocks = len(block_config)
        for i, n in enumerate(block_config):
            self.add_module(f"denseblock{i + 1}", DenseBlockModule(n, nf, growth_rate, bn_size))
            nf += n * growth_rate
            if i + 1 < len(block_config):
                if nf % 16:
                    raise NotImplementedError(f"transition{i + 1} would halve {nf} channels to a width that is no multiple of 8")
                self.add_module(f"transition{i + 1}", Transition(nf, nf // 2))
                nf //= 2
        self.norm5 = HipBatchNorm2d(nf)
        self.num_features = nf
        for m in self.modules():
            if isinstance(m, HipConv2d):
                nn.init.kaiming_normal_(m.weight)


class DenseNetEncoder(nn.Module):
    """The reference's `encoder` wrapper for a DenseNet: ``base_model`` = the features module; forward returns the five maps it picks by name
    (relu0, pool0, transition1, transition2, norm5), the last with the ReLU that BTSNet.py:L207 applies to it (the decoder is its only reader)."""

    schedule_family = "resnet"

    def __init__(self, growth_rate=32, block_config=(6, 12, 24, 16), num_init_features=64, bn_size=4):
        super().__init__()
        if len(block_config) != 4:
            raise NotImplementedError("the BTS decoder reads five features: four dense blocks")
        self.base_model = DenseNetFeatures(growth_rate, block_config, num_init_features, bn_size)
        m = self.base_model
        self.feat_out_channels = [num_init_features, num_init_features, m.transition1.conv.out_channels, m.transition2.conv.out_channels, m.num_features]

    def forward(self, x):
        """x: NHWC normalised image (channels padded).  Returns the 5 NHWC feature maps."""
        m = self.base_model
        if torch.is_grad_enabled():
            f0, f0_pool = conv_bn(m.conv0, m.norm0, x, n_out=2)          # decoder skip + max-pool
        else:
            f0 = f0_pool = conv_bn(m.conv0, m.norm0, x)
        feats = [f0]
        x = HN.max_pool_3x3_s2(f0_pool)
        for i in range(1, 4):
            tr = getattr(m, f"transition{i}")
            first, a = getattr(m, f"denseblock{i}")(x, tr.norm)
            feats.append(first)                    # pool0 / transition1 / transition2: the block input, read by the block and by the decoder
            x = HD.avg_pool_2x2(tr.conv(a))
        _, dense = m.denseblock4(x, m.norm5)       # (transition3's output is no feature)
        return feats + [dense]

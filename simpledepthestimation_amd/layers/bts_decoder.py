"""BTS decoder on the HIP path (contract: detectron2/modeling/depth_net/BTSNet.py:L32-275, `bts`).

Module tree and state-dict names are the reference's (``upconv5.conv.weight``, ``daspp_12.atrous_conv.aconv_sequence.4.weight``,
``reduc8x8.reduc.inter_128_64.0.weight`` ...): parameter-free members (nn.ELU / nn.ReLU / nn.Sigmoid) are kept as placeholders so that the
Sequential indices match, and never run.  The arithmetic is the conv engine (every convolution; the dilated ones as space-to-batch around
it) and csrc/bts.hip (up-sampling, concatenations, first_bn statistics, the fused plane head + LPG, the sigmoid heads).
"""
import torch
from torch import nn

from ..hip import bts as HB
from ..hip import nn as HN
from .hip_modules import HipBatchNorm2d, HipConv2d

FOCAL_REF = 715.0873      # bts.forward: final_depth * focal / 715.0873 on KITTI


def _conv(cin, cout, k):
    return HipConv2d(cin, cout, k, 1, k // 2, bias=False, reflect=False)


class AtrousConv(nn.Module):
    """atrous_conv (L39-64): [first_bn] -> ReLU -> 1x1 -> BN -> ReLU -> 3x3 with dilation d (pad d)."""

    def __init__(self, in_channels, out_channels, dilation, apply_bn_first=True):
        super().__init__()
        self.dilation = int(dilation)
        self.atrous_conv = nn.Sequential()
        if apply_bn_first:
            self.atrous_conv.add_module("first_bn", HipBatchNorm2d(in_channels, eps=1.1e-5, momentum=0.01))
        self.atrous_conv.add_module("aconv_sequence", nn.Sequential(nn.ReLU(), _conv(in_channels, out_channels * 2, 1),
                                                                    HipBatchNorm2d(out_channels * 2, eps=1e-5, momentum=0.01), nn.ReLU(),
                                                                    _conv(out_channels * 2, out_channels, 3)))

    def forward(self, x):
        seq = self.atrous_conv.aconv_sequence
        if hasattr(self.atrous_conv, "first_bn"):
            bn = self.atrous_conv.first_bn
            x = bn(x, HB.channel_stats(x) if bn.training else None, relu=True)
        else:
            x = HB.relu(x)
        bn = seq[2]
        if bn.training:
            y, st = seq[1](x, bn_stats=True)
        else:
            y, st = seq[1](x), None
        return HB.dilated_conv3x3(seq[4], bn(y, st, relu=True), self.dilation)


class UpConv(nn.Module):
    """upconv (L67-79): nearest x2 -> 3x3 zero-padded convolution -> ELU."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.elu = nn.ELU()
        self.conv = _conv(in_channels, out_channels, 3)

    def forward(self, x, bn_stats=False):
        return self.conv(HB.upsample2(x), act=HN.ACT_ELU, bn_stats=bn_stats)


class Reduction1x1(nn.Module):
    """reduction_1x1 (L82-123): 1x1 + ELU chain, then a 3-channel `plane_params` convolution or (is_final) a 1-channel one + sigmoid.
    forward returns the last convolution's raw NHWC output; the heads live in hip.bts (lpg / sigmoid_head)."""

    def __init__(self, num_in_filters, num_out_filters, max_depth, is_final=False):
        super().__init__()
        self.max_depth, self.is_final = max_depth, is_final
        self.sigmoid = nn.Sigmoid()
        self.reduc = nn.Sequential()
        self.chain = []
        while num_out_filters >= 4:
            if num_out_filters < 8:
                if is_final:
                    self.reduc.add_module("final", nn.Sequential(_conv(num_in_filters, 1, 1), nn.Sigmoid()))
                else:
                    self.reduc.add_module("plane_params", _conv(num_in_filters, 3, 1))
                break
            self.reduc.add_module("inter_{}_{}".format(num_in_filters, num_out_filters), nn.Sequential(_conv(num_in_filters, num_out_filters, 1), nn.ELU()))
            num_in_filters = num_out_filters
            num_out_filters = num_out_filters // 2
        if not (hasattr(self.reduc, "final") or hasattr(self.reduc, "plane_params")):
            raise NotImplementedError("reduction_1x1 without a head layer (BTS_SIZE below 128) builds a decoder the reference cannot run")

    def forward(self, x):
        for name, m in self.reduc.named_children():
            if name.startswith("inter_"):
                x = m[0](x, act=HN.ACT_ELU)
            elif name == "final":
                x = m[0](x)
            else:
                x = m(x)
        return x


class BtsDecoder(nn.Module):
    def __init__(self, dataset, max_depth, feat_out_channels, num_features=512):
        super().__init__()
        self.dataset, self.max_depth = dataset, float(max_depth)
        nf, fc = int(num_features), [int(c) for c in feat_out_channels]
        self.nf, self.fc = nf, fc

        def bn(c):
            return HipBatchNorm2d(c, eps=1.1e-5, momentum=0.01)

        self.upconv5 = UpConv(fc[4], nf)
        self.bn5 = bn(nf)
        self.conv5 = nn.Sequential(_conv(nf + fc[3], nf, 3), nn.ELU())
        self.upconv4 = UpConv(nf, nf // 2)
        self.bn4 = bn(nf // 2)
        self.conv4 = nn.Sequential(_conv(nf // 2 + fc[2], nf // 2, 3), nn.ELU())
        self.bn4_2 = bn(nf // 2)
        self.daspp_3 = AtrousConv(nf // 2, nf // 4, 3, apply_bn_first=False)
        self.daspp_6 = AtrousConv(nf // 2 + nf // 4 + fc[2], nf // 4, 6)
        self.daspp_12 = AtrousConv(nf + fc[2], nf // 4, 12)
        self.daspp_18 = AtrousConv(nf + nf // 4 + fc[2], nf // 4, 18)
        self.daspp_24 = AtrousConv(nf + nf // 2 + fc[2], nf // 4, 24)
        self.daspp_conv = nn.Sequential(_conv(nf + nf // 2 + nf // 4, nf // 4, 3), nn.ELU())
        self.reduc8x8 = Reduction1x1(nf // 4, nf // 4, self.max_depth)
        self.upconv3 = UpConv(nf // 4, nf // 4)
        self.bn3 = bn(nf // 4)
        self.conv3 = nn.Sequential(_conv(nf // 4 + fc[1] + 1, nf // 4, 3), nn.ELU())
        self.reduc4x4 = Reduction1x1(nf // 4, nf // 8, self.max_depth)
        self.upconv2 = UpConv(nf // 4, nf // 8)
        self.bn2 = bn(nf // 8)
        self.conv2 = nn.Sequential(_conv(nf // 8 + fc[0] + 1, nf // 8, 3), nn.ELU())
        self.reduc2x2 = Reduction1x1(nf // 8, nf // 16, self.max_depth)
        self.upconv1 = UpConv(nf // 8, nf // 16)
        self.reduc1x1 = Reduction1x1(nf // 16, nf // 32, self.max_depth, is_final=True)
        self.conv1 = nn.Sequential(_conv(nf // 16 + 4, nf // 16, 3), nn.ELU())
        self.get_depth = nn.Sequential(_conv(nf // 16, 1, 3), nn.Sigmoid())
        for m in self.modules():          # weights_init_xavier (L32-36); no decoder convolution has a bias
            if isinstance(m, HipConv2d):
                nn.init.xavier_uniform_(m.weight)

    @staticmethod
    def _upconv_bn(up, bn, x):
        if bn.training:
            y, st = up(x, bn_stats=True)
        else:
            y, st = up(x), None
        return bn(y, st, relu=False)

    def forward(self, features, focal, flip=False):
        """features: the encoder's five NHWC maps; focal: [B] fp32 (used only when dataset == 'kitti').
        Returns (depth_8x8, depth_4x4, depth_2x2, reduc1x1, final_depth) as [B,1,H,W] fp32 (final_depth mirrored when flip)."""
        nf, fc, md = self.nf, self.fc, self.max_depth
        skip0, skip1, skip2, skip3, dense = features      # dense = layer4's output: already ReLU'd, torch.nn.ReLU() of L207 is the identity
        upconv5 = self._upconv_bn(self.upconv5, self.bn5, dense)
        iconv5 = self.conv5[0](HB.cat([(upconv5, nf), (skip3, fc[3])]), act=HN.ACT_ELU)
        upconv4 = self._upconv_bn(self.upconv4, self.bn4, iconv5)
        concat4 = HB.cat([(upconv4, nf // 2), (skip2, fc[2])])
        if self.bn4_2.training:
            y, st = self.conv4[0](concat4, act=HN.ACT_ELU, bn_stats=True)
        else:
            y, st = self.conv4[0](concat4, act=HN.ACT_ELU), None
        iconv4 = self.bn4_2(y, st, relu=False)
        q = nf // 4
        daspp_3 = self.daspp_3(iconv4)
        c4_2 = HB.cat([(concat4, nf // 2 + fc[2]), (daspp_3, q)])
        daspp_6 = self.daspp_6(c4_2)
        c4_3 = HB.cat([(c4_2, nf // 2 + fc[2] + q), (daspp_6, q)])
        daspp_12 = self.daspp_12(c4_3)
        c4_4 = HB.cat([(c4_3, nf + fc[2]), (daspp_12, q)])
        daspp_18 = self.daspp_18(c4_4)
        c4_5 = HB.cat([(c4_4, nf + fc[2] + q), (daspp_18, q)])
        daspp_24 = self.daspp_24(c4_5)
        daspp_feat = self.daspp_conv[0](HB.cat([(iconv4, nf // 2), (daspp_3, q), (daspp_6, q), (daspp_12, q), (daspp_18, q), (daspp_24, q)]),
                                        act=HN.ACT_ELU)
        depth_8x8, depth_8x8_ds = HB.lpg(self.reduc8x8(daspp_feat), 8, md, ds=4)
        upconv3 = self._upconv_bn(self.upconv3, self.bn3, daspp_feat)
        iconv3 = self.conv3[0](HB.cat([(upconv3, q), (skip1, fc[1]), (depth_8x8_ds, 1)]), act=HN.ACT_ELU)
        depth_4x4, depth_4x4_ds = HB.lpg(self.reduc4x4(iconv3), 4, md, ds=2)
        upconv2 = self._upconv_bn(self.upconv2, self.bn2, iconv3)
        iconv2 = self.conv2[0](HB.cat([(upconv2, nf // 8), (skip0, fc[0]), (depth_4x4_ds, 1)]), act=HN.ACT_ELU)
        depth_2x2 = HB.lpg(self.reduc2x2(iconv2), 2, md)
        upconv1 = self.upconv1(iconv2)
        reduc1x1 = HB.sigmoid_head(self.reduc1x1(upconv1))
        iconv1 = self.conv1[0](HB.cat([(upconv1, nf // 16), (reduc1x1, 1), (depth_2x2, 1), (depth_4x4, 1), (depth_8x8, 1)]), act=HN.ACT_ELU)
        kitti = self.dataset == "kitti"
        final = HB.sigmoid_head(self.get_depth[0](iconv1), md, focal if kitti else None, FOCAL_REF if kitti else 1.0, flip)
        return depth_8x8, depth_4x4, depth_2x2, reduc1x1, final

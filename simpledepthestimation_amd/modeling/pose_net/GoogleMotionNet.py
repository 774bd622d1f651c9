"""GooglePoseNet and GoogleMotionNet on the HIP kernels (contract of detectron2/modeling/pose_net/GooglePoseNet.py:L31-208).

Both read batch["pose_net_input"] ([N, 8 or 6, H, W] fp32 NCHW; N = 2B in MotionLearning, both frame orders) and add ``pose_pred``, ONE tensor
[N,4,4]; GoogleMotionNet also adds ``motion_pred`` [N,3,H,W] fp32, already multiplied by ``motion_weight``.  Gradients reach every parameter
and, when it requires grad, pose_net_input (its depth channels come from the depth net).

State-dict keys and shapes equal the reference's: ``convN.0.{weight,bias}`` (+ ``convN.1.*`` = GroupNorm with GROUP_NORM; the ReLU has no
parameters), ``pose_pred.weight`` (+ ``.bias`` in GooglePoseNet), ``conv8.*``, ``refinerK.{conv1,conv21,conv22}.0.*`` (``.1.*`` with
GROUP_NORM, never in refiner0), ``refinerK.conv3.weight``, and the 0-dim ``rot_scale`` / ``trans_scale`` first with LEARN_SCALE.  Refiner
weights keep the reference's input-channel order (motion field first, then the skip): hip.motion.resize_cat lays its output out that way.
"""
import torch
import torch.nn.functional as F
from torch import nn

from ...hip import bts as HB
from ...hip import motion as HM
from ...hip import photometric as HP
from ...layers.hip_modules import HipConv2d, HipGroupNorm
from ..depth_net.DepthResNet import compute_dtype
from .build import POSE_NET_REGISTRY

_POSE_STAGES = ((16, 7), (32, 5), (64, 3), (128, 3), (256, 3), (256, 3), (256, 3))         # (output channels, kernel size), all stride 2
_MOTION_STAGES = tuple((c, 3) for c in (16, 32, 64, 128, 256, 512, 1024))
SCALE_CONSTRAINS = ("clip", "clip_ste", "softplus")


def conv_gn_relu(in_planes, out_planes, kernel_size=3, stride=2, group_norm=True):
    """GooglePoseNet.py:L11-20: index 0 the convolution, index 1 the GroupNorm when present (the ReLU is fused into the GroupNorm kernel, or a
    pass of its own without one)."""
    layers = [HipConv2d(in_planes, out_planes, kernel_size, stride=stride, padding=(kernel_size - 1) // 2, bias=True)]
    if group_norm:
        layers.append(HipGroupNorm(16, out_planes))
    return nn.Sequential(*layers)


def run_conv_gn_relu(seq, x):
    y = seq[0](x)
    return seq[1](y, relu=True) if len(seq) > 1 else HB.relu(y)


def _init_convs(module):
    for m in module.modules():
        if isinstance(m, HipConv2d):
            nn.init.xavier_uniform_(m.weight.data)
            if m.bias is not None:
                m.bias.data.zero_()


def _compute_dtype(cfg, name):
    dtype = compute_dtype(cfg)
    if dtype not in (torch.float32, torch.bfloat16):
        raise NotImplementedError(f"{name} runs in fp32 or bf16 (MODEL.COMPUTE_DTYPE); fp16 / AMP is not on its HIP path")
    return dtype


def _get(node, key, default):
    return node.get(key, default) if hasattr(node, "get") else getattr(node, key, default)


def burn_in_weight(step, burn_in_iters):
    """projects/MotionLearning/train.py:L111-114: the weight of the motion field at global step `step` (counted from 1) -- 0 over the first half of
    the burn-in, then a linear ramp that reaches 1 at BURN_IN_ITERS."""
    return min(max(2.0 * step / burn_in_iters - 1.0, 0.0), 1.0)


def _head_vector(head, feat):
    """The 1x1 pose head on the spatial mean of the last feature map: [N,h,w,C] -> [N,6] fp32 (the mean is tiny: torch glue, as in PoseNet)."""
    mean = feat.float().mean(dim=(1, 2)).to(feat.dtype).view(feat.shape[0], 1, 1, feat.shape[3])
    return head(mean)


@POSE_NET_REGISTRY.register()
class GooglePoseNet(nn.Module):
    def __init__(self, cfg, **kwargs):
        super().__init__()
        pn = cfg.MODEL.POSE_NET
        group_norm = bool(pn.GROUP_NORM)
        self.learn_scale = bool(pn.LEARN_SCALE)
        self.dtype = _compute_dtype(cfg, "GooglePoseNet")
        if self.learn_scale:
            self.rot_scale = nn.Parameter(torch.tensor(0.01))
            self.trans_scale = nn.Parameter(torch.tensor(0.01))
        width = self.in_channels = 4 * 2 if pn.USE_DEPTH else 3 * 2
        for idx, (out_ch, k) in enumerate(_POSE_STAGES, start=1):
            setattr(self, f"conv{idx}", conv_gn_relu(width, out_ch, kernel_size=k, group_norm=group_norm))
            width = out_ch
        self.pose_pred = HipConv2d(width, 6, 1, stride=1, padding=0, bias=True)
        _init_convs(self)

    def forward(self, batch):
        x = batch["pose_net_input"]
        if x.shape[1] != self.in_channels:
            raise ValueError(f"GooglePoseNet expects {self.in_channels} input channels (MODEL.POSE_NET.USE_DEPTH), got {x.shape[1]}")
        feat, _ = HM.prep_input_grad(x, self.dtype)
        for idx in range(1, len(_POSE_STAGES) + 1):
            feat = run_conv_gn_relu(getattr(self, f"conv{idx}"), feat)
        pose = _head_vector(self.pose_pred, feat)[:, 0, 0, :6].float()
        trans, rot = pose[:, :3], pose[:, 3:]                                              # L72
        if self.learn_scale:
            rot_scale = torch.relu(self.rot_scale - 0.001) + 0.001
            trans_scale = torch.relu(self.trans_scale - 0.001) + 0.001
            pose = torch.cat([trans * trans_scale, rot * rot_scale], -1)
        else:
            pose = torch.cat([trans * 0.01, rot * 0.01], -1)
        batch["pose_pred"] = HP.pose_vec2mat(pose.contiguous())
        return batch


class MotionRefiner(nn.Module):
    """GooglePoseNet.py:L79-100 on an fp32 [N,h,w,4] motion field and an NHWC skip."""

    def __init__(self, channel_out, channel_mid, group_norm):
        super().__init__()
        assert channel_out == 3
        self.channel_mid = int(channel_mid)
        self.conv1 = conv_gn_relu(channel_out + channel_mid, channel_mid, kernel_size=3, group_norm=group_norm, stride=1)
        self.conv21 = conv_gn_relu(channel_out + channel_mid, channel_mid, kernel_size=3, group_norm=group_norm, stride=1)
        self.conv22 = conv_gn_relu(channel_mid, channel_mid, kernel_size=3, group_norm=group_norm, stride=1)
        self.conv3 = HipConv2d(channel_mid * 2, channel_out, 1, stride=1, padding=0, bias=False)

    def forward(self, field, skip):
        xa, xb, up = HM.resize_cat(field, skip, self.channel_mid)          # one alias of the refiner input per branch
        out1 = run_conv_gn_relu(self.conv1, xa)
        out2 = run_conv_gn_relu(self.conv22, run_conv_gn_relu(self.conv21, xb))
        return HM.refiner_tail(out1, out2, self.conv3.weight, up)


@POSE_NET_REGISTRY.register()
class GoogleMotionNet(nn.Module):
    def __init__(self, cfg, **kwargs):
        super().__init__()
        pn = cfg.MODEL.POSE_NET
        group_norm = bool(pn.GROUP_NORM)
        self.learn_scale = bool(pn.LEARN_SCALE)
        self.mask_motion = bool(pn.MASK_MOTION)
        self.scale_constrain = _get(pn, "SCALE_CONSTRAIN", "clip")
        if self.learn_scale and self.scale_constrain not in SCALE_CONSTRAINS:
            raise NotImplementedError(f"MODEL.POSE_NET.SCALE_CONSTRAIN must be one of {SCALE_CONSTRAINS}, got {self.scale_constrain!r}")
        self.burn_in_iters = int(_get(pn, "BURN_IN_ITERS", 20000))
        self.dtype = _compute_dtype(cfg, "GoogleMotionNet")
        if self.learn_scale:
            init = 0.4 if self.scale_constrain == "softplus" else 0.01
            self.rot_scale = nn.Parameter(torch.tensor(init))
            self.trans_scale = nn.Parameter(torch.tensor(init))
        width = self.in_channels = 4 * 2 if pn.USE_DEPTH else 3 * 2
        channels = [c for c, _ in _MOTION_STAGES]
        for idx, (out_ch, k) in enumerate(_MOTION_STAGES, start=1):
            setattr(self, f"conv{idx}", conv_gn_relu(width, out_ch, kernel_size=k, group_norm=group_norm))
            width = out_ch
        self.pose_pred = HipConv2d(channels[6], 6, 1, stride=1, padding=0, bias=False)
        self.conv8 = HipConv2d(6, 3, 1, stride=1, padding=0, bias=True)
        for idx in range(7, 0, -1):
            setattr(self, f"refiner{idx}", MotionRefiner(3, channels[idx - 1], group_norm))
        self.refiner0 = MotionRefiner(3, self.in_channels, False)
        # device scalars the head kernels read: a training loop changes them between steps without a rebuild or a re-capture
        self.register_buffer("_motion_weight", torch.ones(1), persistent=False)
        self.register_buffer("_const_scale", torch.full((1,), 0.01), persistent=False)
        self._weight = 1.0
        _init_convs(self)

    @property
    def motion_weight(self):
        return self._weight

    @motion_weight.setter
    def motion_weight(self, value):
        self._weight = float(value)
        self._motion_weight.fill_(self._weight)

    def _scales(self):
        """(trans_scale, rot_scale) as the reference constrains them (L175-186): scalars, torch glue."""
        if not self.learn_scale:
            return self._const_scale, self._const_scale
        t, r = self.trans_scale, self.rot_scale
        if self.scale_constrain == "clip_ste":
            return (torch.clamp_min(t, 0.001) - t).detach() + t, (torch.clamp_min(r, 0.001) - r).detach() + r
        if self.scale_constrain == "clip":
            return torch.relu(t - 0.001) + 0.001, torch.relu(r - 0.001) + 0.001
        return F.softplus(t) * 0.01 + 0.001, F.softplus(r) * 0.01 + 0.001

    def forward(self, batch):
        x = batch["pose_net_input"]
        if x.shape[1] != self.in_channels:
            raise ValueError(f"GoogleMotionNet expects {self.in_channels} input channels (MODEL.POSE_NET.USE_DEPTH), got {x.shape[1]}")
        N = x.shape[0]
        x_conv, x_skip = HM.prep_input_grad(x, self.dtype)
        feats, feat = [], x_conv
        for idx in range(1, len(_MOTION_STAGES) + 1):
            feat = run_conv_gn_relu(getattr(self, f"conv{idx}"), feat)
            feats.append(feat)
        pose = _head_vector(self.pose_pred, feats[-1])                                     # [N,1,1,8]: 6 real channels
        field = self.conv8(pose)[..., :4].float().contiguous()                             # [N,1,1,4] fp32: the motion trunk, channel 3 zero
        pose = pose[:, 0, 0, :6].float()
        rot, trans = pose[:, :3], pose[:, 3:]                                              # L155
        for idx in range(7, 0, -1):
            field = getattr(self, f"refiner{idx}")(field, feats[idx - 1])
        field = self.refiner0(field, x_skip)
        trans_scale, rot_scale = self._scales()
        pose = torch.cat([trans * trans_scale, rot * rot_scale], -1)
        batch["pose_pred"] = HP.pose_vec2mat(pose.contiguous())
        batch["motion_pred"] = HM.motion_head(field, trans_scale, self._motion_weight, self.mask_motion)
        return batch

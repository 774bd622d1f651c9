"""Parameter-holding building blocks whose forward runs on libsde_hip.so (NHWC activations).

Parameter names/layouts equal torch's (``weight`` OIHW fp32, ``bias``, BatchNorm ``running_mean`` ...), so the reference's
checkpoints load with ``load_state_dict`` unchanged.
"""
import math

import torch
import torch.nn as nn

from ..hip import google as HG
from ..hip import nn as HN


class HipConv2d(nn.Module):
    """nn.Conv2d stand-in (weights only); the arithmetic is sde_conv_fwd / sde_conv_wgrad (include/sde_hip.h)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, reflect=False):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = int(in_channels), int(out_channels), int(kernel_size)
        self.stride, self.padding, self.reflect = int(stride), int(padding), bool(reflect)
        self.weight = nn.Parameter(torch.empty(self.out_channels, self.in_channels, self.kernel_size, self.kernel_size))
        self.bias = nn.Parameter(torch.empty(self.out_channels)) if bias else None
        self._packed = None        # (forward operand, dgrad operand) maintained by hip.nn.WeightPacker, else packed per call
        self._pack_shapes = None
        self.reset_parameters()

    def reset_parameters(self):   # torch.nn.Conv2d default initialisation
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1.0 / math.sqrt(self.in_channels * self.kernel_size ** 2)
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x, skip=None, upsample=False, act=HN.ACT_NONE, bn_stats=False, n_out=1):
        return HN.conv2d(x, self.weight, self.bias, self.stride, self.padding, self.reflect, act, skip, upsample, bn_stats, owner=self, n_out=n_out)

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}, k={self.kernel_size}, s={self.stride}, p={self.padding}, reflect={self.reflect}"


class HipConvTranspose2d(nn.Module):
    """nn.ConvTranspose2d(Cin, Cout, 3, stride=2, padding=1, output_padding=1) stand-in: ``weight`` [Cin,Cout,3,3] and ``bias`` [Cout] as torch's; the
    arithmetic is sde_deconv3x3s2_fwd and, in backward, the convolution engine on the adjoint Conv2d(Cout -> Cin, 3, stride 2, padding 1), whose OIHW
    weight this weight is.  ``_pack_shapes`` / ``_packed`` are therefore that adjoint's: hip.nn.WeightPacker packs the layer with the convolutions."""

    SUPPORTED = "kernel_size=3, stride=2, padding=1, output_padding=1"
    FORWARD_READS_DGRAD_OPERAND = True      # _packed[1] is this layer's FORWARD operand: hip.nn.WeightPacker must have it ready before the forward pass starts

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=2, padding=1, output_padding=1, bias=True):
        super().__init__()
        if (int(kernel_size), int(stride), int(padding), int(output_padding)) != (3, 2, 1, 1):
            raise NotImplementedError(f"HipConvTranspose2d supports {self.SUPPORTED} only, got kernel_size={kernel_size}, stride={stride}, "
                                      f"padding={padding}, output_padding={output_padding}")
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.weight = nn.Parameter(torch.empty(self.in_channels, self.out_channels, 3, 3))
        self.bias = nn.Parameter(torch.empty(self.out_channels)) if bias else None
        self._packed = None        # (adjoint forward operand = this layer's data-gradient operand, adjoint dgrad operand = this layer's forward operand)
        self._pack_shapes = None
        self.reset_parameters()

    def reset_parameters(self):   # torch.nn.ConvTranspose2d default initialisation (fan_in is computed from dim 1: out_channels * 9)
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1.0 / math.sqrt(self.out_channels * 9)
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x, act=HN.ACT_NONE):
        return HN.conv_transpose2d(x, self.weight, self.bias, act, owner=self)

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}, {self.SUPPORTED}"


class HipGroupedConv2d(nn.Module):
    """nn.Conv2d(channels, channels, 3, stride, padding=1, groups=groups, bias=False) stand-in, the 3x3 of a ResNeXt bottleneck: ``weight``
    [C, C/groups, 3, 3] as torch's; the arithmetic is sde_gconv3x3_fwd / _dgrad / _wgrad, which read the fp32 weight itself (no packed operands, so
    hip.nn.WeightPacker passes the layer by).  Same forward contract as HipConv2d towards conv_bn / conv_norm."""

    SUPPORTED = f"channels a multiple of 16, channels / groups in {HN.GCONV_CG}, stride 1 or 2"

    def __init__(self, channels, groups, stride=1):
        super().__init__()
        channels, groups, stride = int(channels), int(groups), int(stride)
        if groups <= 0 or channels % groups or channels % 16 or channels // groups not in HN.GCONV_CG or stride not in (1, 2):
            raise NotImplementedError(f"HipGroupedConv2d supports {self.SUPPORTED}; got channels={channels}, groups={groups}, stride={stride}")
        self.in_channels = self.out_channels = channels
        self.groups, self.stride, self.kernel_size, self.padding = groups, stride, 3, 1
        self.weight = nn.Parameter(torch.empty(channels, channels // groups, 3, 3))
        self.bias = None
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))       # torch.nn.Conv2d default initialisation

    def forward(self, x, bn_stats=False, n_out=1):
        return HN.grouped_conv3x3(x, self.weight, self.groups, self.stride, bn_stats, n_out)

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}, k=3, s={self.stride}, p=1, groups={self.groups}"


class HipBatchNorm2d(nn.Module):
    """nn.BatchNorm2d stand-in: batch statistics come from the producing convolution's epilogue (stats slab)."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1):
        super().__init__()
        self.num_features, self.eps, self.momentum = int(num_features), eps, momentum
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
        self._pending_batches = 0     # counted on the host, folded into the buffer when the state dict is read (no per-layer kernel)

    def flush_counters(self):
        if self._pending_batches:
            self.num_batches_tracked += self._pending_batches
            self._pending_batches = 0

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        self.flush_counters()
        super()._save_to_state_dict(destination, prefix, keep_vars)

    def _load_from_state_dict(self, *args, **kwargs):
        self._pending_batches = 0                  # the loaded num_batches_tracked is the whole count
        super()._load_from_state_dict(*args, **kwargs)

    def forward(self, y, stats, residual=None, relu=True, n_out=1):
        if self.training:
            self._pending_batches += 1
        return HN.batch_norm_act(y, stats, self.weight, self.bias, self.running_mean, self.running_var, residual, relu, self.momentum, self.eps,
                                 self.training, n_out)


class HipGroupNorm(nn.Module):
    """nn.GroupNorm stand-in fused with the following activation: ReLU (PoseNet.py:L13-20), "elu" (layers01.py:L33-40) or none."""

    def __init__(self, num_groups, num_channels, eps=1e-5):
        super().__init__()
        self.num_groups, self.num_channels, self.eps = num_groups, num_channels, eps
        self.weight = nn.Parameter(torch.ones(num_channels))
        self.bias = nn.Parameter(torch.zeros(num_channels))

    def forward(self, x, relu=True, residual=None):
        return HN.group_norm_relu(x, self.weight, self.bias, self.num_groups, self.eps, relu, residual)


def conv_bn(conv, bn, x, residual=None, relu=True, n_out=1):
    """conv -> training-mode BatchNorm [-> + residual] [-> ReLU]; in eval mode BN uses its running statistics.
    n_out > 1: that many aliases of the result, one per consumer (see hip.nn._BatchNormAct)."""
    if bn.training:
        y, stats = conv(x, bn_stats=True)
    else:
        y, stats = conv(x), None
    return bn(y, stats, residual, relu, n_out)


def conv_norm(conv, norm, x, residual=None, relu=True, n_out=1):
    """conv -> norm [-> + residual] [-> ReLU] for either norm layer of the ResNet blocks: BatchNorm takes its statistics from the convolution's
    epilogue (conv_bn), RandLayerNorm runs on the plain convolution output."""
    if isinstance(norm, HipBatchNorm2d):
        return conv_bn(conv, norm, x, residual, relu, n_out)
    return norm(conv(x), residual, relu, n_out)


class HipRandLayerNorm(nn.Module):
    """RandLayerNorm (detectron2/layers/layer_norm.py:L7-33) on NHWC activations: per-sample statistics, noise-scaled in training.

    Same forward contract as HipBatchNorm2d minus the statistics slab: norm(y, residual, relu, n_out).  ``stddev`` lives in a one-element
    device buffer (not in the state dict, which holds weight and bias only, as the reference's) that the kernel reads, so a captured graph
    follows later set_stddev values.  z: [2,B,C] draws (mean, variance) for the next training forward -- the owning network hands each norm a
    slice of one draw per forward (``_z``); ``inject_z`` overrides them for one forward (tests)."""

    def __init__(self, num_channels, eps=1e-3):
        super().__init__()
        self.num_channels, self.eps = int(num_channels), eps
        self.weight = nn.Parameter(torch.ones(num_channels))
        self.bias = nn.Parameter(torch.zeros(num_channels))
        self.register_buffer("noise_stddev", torch.full((1,), 0.5), persistent=False)
        self._stddev = 0.5
        self._z = None
        self._injected = None

    @property
    def stddev(self):
        return self._stddev

    @stddev.setter
    def stddev(self, value):
        self._stddev = float(value)
        self.noise_stddev.fill_(self._stddev)

    def inject_z(self, z_mean, z_var):
        """Use these [B,C] draws (the reference's randn_like(mean) and randn_like(var)) in the next training forward."""
        self._injected = torch.stack([torch.as_tensor(z_mean).reshape(-1), torch.as_tensor(z_var).reshape(-1)])

    def forward(self, y, residual=None, relu=True, n_out=1):
        z = None
        if self.training:
            B, C = y.shape[0], self.num_channels
            if self._injected is not None:
                z, self._injected = self._injected.to(device=y.device, dtype=torch.float32).reshape(2, B, C), None
            elif self._z is not None:
                z, self._z = self._z, None
            else:
                z = torch.randn(2, B, C, device=y.device)
        return HG.rand_layer_norm(y, self.weight, self.bias, z, self.noise_stddev, self.eps, self.training, residual, relu, n_out)

    def extra_repr(self):
        return f"{self.num_channels}, eps={self.eps}, stddev={self._stddev}"

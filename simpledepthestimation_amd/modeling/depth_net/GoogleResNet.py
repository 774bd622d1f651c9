"""GoogleResNet = ResNetTF encoder + bilinear up-sampling decoder + softplus (reference: detectron2/modeling/depth_net/GoogleResNet.py:L126-171).

The depth net of the MotionLearning project; it returns depth_pred = [depth] (one full-resolution map), so SupDepthModel trains it as it does
BtsModel.  State-dict keys equal the reference's (``encoder.encoder.layer1.0.bn1.weight``, ``decoder.scale``, ``decoder.blocks.4.iconv.weight``,
``decoder.out_conv.bias``), so its checkpoints load with ``strict=True``.  NORM: randLN (RandLayerNorm, layers/hip_modules.py), BN or None (BN).
"""
import torch
import torch.nn as nn

from ...hip import nn as HN
from ...layers.google_resnet import NORMS, GoogleDepthDecoder, GoogleResnetEncoder
from ...layers.hip_modules import HipRandLayerNorm
from .build import DEPTH_NET_REGISTRY
from .DepthResNet import compute_dtype


def noise_ramp(noise_stddev, rampup_iters, step):
    """projects/MotionLearning/train.py:L101-105: the RandLayerNorm noise at global step `step` (counted from 1)."""
    return noise_stddev * min(step / float(rampup_iters), 1.0) ** 2


class GoogleDepthNet(nn.Module):
    """What GoogleResNet and GoogleResNetv2 share: the NORM / compute-dtype keys, the RandLayerNorm noise (set_stddev, one pooled draw per forward,
    inject_z) and the forward pass around ``self.encoder`` / ``self.decoder`` (flip folded into prep_input and the softplus head)."""

    def _configure(self, cfg):
        """Reads NORM and the compute dtype; returns the norm layer class."""
        dn = cfg.MODEL.DEPTH_NET
        norm = dn.get("NORM", "randLN") if hasattr(dn, "get") else getattr(dn, "NORM", "randLN")
        norm = None if norm in (None, "", "None") else norm
        if norm not in NORMS:
            raise ValueError(f"MODEL.DEPTH_NET.NORM must be one of 'randLN', 'BN' or None, got {norm!r}")
        self.dtype = compute_dtype(cfg)
        if self.dtype not in (torch.float32, torch.bfloat16):
            raise NotImplementedError(f"{type(self).__name__} runs in fp32 or bf16 (MODEL.COMPUTE_DTYPE); fp16 / AMP is not on its HIP path")
        self.norm = norm
        self.upsample_depth = dn.UPSAMPLE_DEPTH
        return NORMS[norm]

    def _collect_norms(self):
        self._rand_norms = [(n, m) for n, m in self.named_modules() if isinstance(m, HipRandLayerNorm)]

    def set_stddev(self, stddev):
        """GoogleResNet.py:L149-155: the noise scale of every RandLayerNorm (written to their device buffers; captured graphs follow it)."""
        for _, m in self._rand_norms:
            m.stddev = stddev

    def inject_z(self, draws):
        """Test hook: {norm module name: (z_mean [B,C], z_var [B,C])} replaces those modules' draws in the next training forward."""
        mods = dict(self._rand_norms)
        for name, (zm, zv) in draws.items():
            mods[name].inject_z(zm, zv)

    def _draw_noise(self, B, device):
        """One N(0,1) draw per forward for all RandLayerNorms together (under graph replay every replay draws anew)."""
        sizes = [2 * B * m.num_channels for _, m in self._rand_norms]
        pool = torch.randn(sum(sizes), device=device)
        off = 0
        for (_, m), n in zip(self._rand_norms, sizes):
            m._z = pool[off:off + n].view(2, B, m.num_channels)
            off += n

    def forward(self, batch):
        """Adds depth_pred = [depth] ([B,1,H,W] fp32), GoogleResNet.py:L157-171."""
        flip = bool(batch.get("flip", False))
        x = batch.get("depth_net_input_nhwc")
        if x is None:
            x = HN.prep_input(batch["depth_net_input"], None, None, self.dtype, flip)   # flip folded into the layout change
        B, H, W = x.shape[:3]
        if H % 32 or W % 32:
            raise ValueError(f"{type(self).__name__} needs H and W divisible by 32 (the decoder's skips would not line up), got {H}x{W}")
        if self._rand_norms and (H // 32) * (W // 32) < 2:
            raise ValueError(f"{type(self).__name__} with RandLayerNorm needs at least 2 pixels in layer4's map (H x W / 1024 >= 2), got {H}x{W}: "
                             "the unbiased variance of one pixel is NaN")
        if self.training and self._rand_norms:
            self._draw_noise(B, x.device)
        depth = self.decoder(self.encoder(x), flip)                    # the output flip is folded into the softplus head
        batch["depth_pred"] = [depth]
        return batch


@DEPTH_NET_REGISTRY.register()
class GoogleResNet(GoogleDepthNet):
    def __init__(self, cfg, **kwargs):
        super().__init__()
        dn = cfg.MODEL.DEPTH_NET
        version = dn.ENCODER_NAME
        assert version is not None, "DispResNet needs a version"
        num_layers = int(version[:2])
        if version[2:] == "pt":
            raise RuntimeError("ImageNet weights cannot be downloaded here; load them from a local checkpoint with load_state_dict "
                               "(use ENCODER_NAME '18'/'50' instead of '18pt'/'50pt')")
        assert num_layers in [18, 34, 50], "ResNet version {} not available".format(num_layers)
        norm_layer = self._configure(cfg)
        self.encoder = GoogleResnetEncoder(num_layers, norm_layer)
        self.decoder = GoogleDepthDecoder(self.encoder.num_ch_enc, learn_scale=bool(dn.LEARN_SCALE))
        self._collect_norms()

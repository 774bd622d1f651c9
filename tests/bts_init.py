"""Seeded BtsModel weights shared by scripts/gen_golden_bts.py (reference run, CPU) and the BTS tests (no conftest: a plain helper module).

Encoder: oracle.models.init_state_dict(50, seed) (torchvision ResNet-50 initialisers) renamed to ``encoder.base_model.*``; decoder:
xavier-uniform convolution weights drawn from a torch.Generator in state-dict order, BatchNorm gamma=1 beta=0 (weights_init_xavier, BTSNet.py:L32-36).
"""
import math

import torch


def bts_state_dict(ref_names_shapes, seed=0):
    """ref_names_shapes: [(name, shape)] of the BtsModel state dict (as the golden file lists it) -> {name: tensor}."""
    from oracle import models as OM
    enc = OM.init_state_dict(50, seed=seed)
    pre = "depth_net.encoder.encoder."
    sd = {}
    g = torch.Generator().manual_seed(seed + 1000)
    for name, shape in ref_names_shapes:
        shape = tuple(int(s) for s in shape)
        if name.startswith("encoder.base_model."):
            sd[name] = enc[pre + name[len("encoder.base_model."):]].clone().reshape(shape)
        elif name.endswith("num_batches_tracked"):
            sd[name] = torch.zeros((), dtype=torch.long)
        elif name.endswith("running_mean") or name.endswith(".bias"):
            sd[name] = torch.zeros(shape)
        elif name.endswith("running_var"):
            sd[name] = torch.ones(shape)
        elif len(shape) == 4:
            fan_in, fan_out = shape[1] * shape[2] * shape[3], shape[0] * shape[2] * shape[3]
            bound = math.sqrt(6.0 / (fan_in + fan_out))
            sd[name] = (torch.rand(shape, generator=g) * 2 - 1) * bound
        else:
            sd[name] = torch.ones(shape)        # BatchNorm gamma
    return sd


def bts_batch(B, H, W, seed=0):
    """Normalised-image input, ground truth and KITTI-like intrinsics (focal differs per sample)."""
    g = torch.Generator().manual_seed(seed + 7)
    img = torch.rand(B, 3, H, W, generator=g)
    depth = torch.rand(B, 1, H, W, generator=g) * 60 + 0.5        # some pixels below the gt > 1 mask
    K = torch.zeros(B, 3, 3)
    for b in range(B):
        f = 720.0 + 15.0 * b
        K[b] = torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]])
    return {"img": img, "depth": depth, "intrinsics": K}


PIXEL_MEAN = (0.485, 0.456, 0.406)
PIXEL_STD = (0.229, 0.224, 0.225)

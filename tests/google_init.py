"""Seeded GoogleResNet weights and batches shared by scripts/gen_golden_google.py (reference run, CPU) and the GoogleResNet tests (no conftest:
a plain helper module).

Convolutions: kaiming-normal (fan_out) in the encoder, xavier-uniform in the decoder (GoogleResNet.py:L92-96), drawn from a torch.Generator
in state-dict order.  Norm gammas / betas and decoder biases get small random offsets (the reference's ones / zeros would leave the affine
and bias paths untested); BatchNorm running buffers start at 0 / 1.
"""
import math

import torch


def google_state_dict(ref_names_shapes, seed=0):
    """ref_names_shapes: [(name, shape)] of the GoogleResNet state dict (as the golden file lists it) -> {name: tensor}."""
    g = torch.Generator().manual_seed(seed + 2000)
    sd = {}
    for name, shape in ref_names_shapes:
        shape = tuple(int(s) for s in shape)
        if name.endswith("num_batches_tracked"):
            sd[name] = torch.zeros((), dtype=torch.long)
        elif name.endswith("running_mean"):
            sd[name] = torch.zeros(shape)
        elif name.endswith("running_var"):
            sd[name] = torch.ones(shape)
        elif name == "decoder.scale":
            sd[name] = torch.ones(shape)
        elif len(shape) == 4 and name.startswith("encoder."):
            sd[name] = torch.randn(shape, generator=g) * math.sqrt(2.0 / (shape[0] * shape[2] * shape[3]))
        elif len(shape) == 4:
            fan_in, fan_out = shape[1] * shape[2] * shape[3], shape[0] * shape[2] * shape[3]
            sd[name] = (torch.rand(shape, generator=g) * 2 - 1) * math.sqrt(6.0 / (fan_in + fan_out))
        elif ".fc." in name:
            bound = 1.0 / math.sqrt(shape[-1]) if len(shape) == 2 else 0.01
            sd[name] = (torch.rand(shape, generator=g) * 2 - 1) * bound
        elif name.endswith(".weight"):          # norm gamma
            sd[name] = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:                                   # norm beta, convolution bias
            sd[name] = 0.05 * torch.randn(shape, generator=g)
    return sd


def google_batch(B, H, W, seed=0):
    """Image input in [0, 1] and a ground-truth depth map (some pixels below the gt > 1 mask)."""
    g = torch.Generator().manual_seed(seed + 11)
    img = torch.rand(B, 3, H, W, generator=g)
    depth = torch.rand(B, 1, H, W, generator=g) * 60 + 0.5
    return {"img": img, "depth": depth}


PIXEL_MEAN = (0.485, 0.456, 0.406)
PIXEL_STD = (0.229, 0.224, 0.225)

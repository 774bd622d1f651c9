"""Seeded GoogleResNetv2 weights and batches shared by scripts/gen_golden_google_v2.py (reference run, CPU) and the GoogleResNetv2 tests (no conftest:
a plain helper module).

Convolutions: kaiming-normal (fan_out) in the encoder, xavier-uniform in the decoder -- transposed convolutions [Cin,Cout,3,3] included
(GoogleResNetv2.py:L98-103, L159-163) -- drawn from a torch.Generator in state-dict order.  Norm gammas / betas and decoder biases get small random
offsets (the reference's ones / zeros would leave the affine and bias paths untested); BatchNorm running buffers start at 0 / 1.
"""
import math

import torch

from google_init import PIXEL_MEAN, PIXEL_STD, google_batch  # noqa: F401  (the same images and ground truth as the GoogleResNet tests)


def google_v2_state_dict(ref_names_shapes, seed=0):
    """ref_names_shapes: [(name, shape)] of the GoogleResNetv2 state dict (as the golden file lists it) -> {name: tensor}."""
    g = torch.Generator().manual_seed(seed + 4000)
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
        elif len(shape) == 4:                   # Conv2d [Cout,Cin,3,3] and ConvTranspose2d [Cin,Cout,3,3]: the bound is symmetric in the two
            sd[name] = (torch.rand(shape, generator=g) * 2 - 1) * math.sqrt(6.0 / ((shape[0] + shape[1]) * shape[2] * shape[3]))
        elif name.endswith(".weight"):          # norm gamma
            sd[name] = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:                                   # norm beta, convolution bias
            sd[name] = 0.05 * torch.randn(shape, generator=g)
    return sd

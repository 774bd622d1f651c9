"""Seeded GoogleMotionNet / GooglePoseNet weights, inputs and loss weights shared by scripts/gen_golden_motion.py (reference run, CPU) and the
pose-network tests (no conftest: a plain helper module).

Convolution weights: xavier-uniform (GooglePoseNet.py:L56-61, L142-146), drawn from a torch.Generator in state-dict order.  GroupNorm gammas /
betas and convolution biases get small random offsets (the reference's ones / zeros would leave the affine and bias paths untested); the two
scales move off their initial value so that their gradients differ.
"""
import math

import torch

# (network, GROUP_NORM, SCALE_CONSTRAIN, MASK_MOTION, LEARN_SCALE, USE_DEPTH, N, H, W); gradients are compared on the mask-off cases
CASES = [
    ("GoogleMotionNet", False, "clip_ste", True, True, True, 2, 40, 104),      # widths 52, 26, 13, 7, 4, 2, 1
    ("GoogleMotionNet", True, "clip", False, True, True, 2, 32, 96),           # reaches 1x1 early and keeps convolving it
    ("GoogleMotionNet", False, "softplus", False, True, False, 2, 24, 104),
    ("GoogleMotionNet", False, "clip", True, False, True, 2, 32, 96),
    ("GooglePoseNet", True, "clip", False, True, True, 2, 24, 40),
    ("GooglePoseNet", False, "clip", False, False, True, 2, 24, 56),
]
FULL_GRADS = ("rot_scale", "trans_scale", "conv8.weight", "conv8.bias", "refiner0.conv3.weight", "pose_pred.weight")


def case_cfg(cfg, case, compute_dtype="fp32"):
    """Fill a config node (get_cfg()) for one golden case."""
    name, gn, sc, mask, learn, use_depth = case[:6]
    pn = cfg.MODEL.POSE_NET
    pn.NAME, pn.GROUP_NORM, pn.SCALE_CONSTRAIN, pn.MASK_MOTION, pn.LEARN_SCALE, pn.USE_DEPTH = name, gn, sc, mask, learn, use_depth
    cfg.MODEL.COMPUTE_DTYPE = compute_dtype
    return cfg


def motion_state_dict(ref_names_shapes, seed=0):
    """ref_names_shapes: [(name, shape)] of the reference's state dict (as the golden file lists it) -> {name: tensor}."""
    g = torch.Generator().manual_seed(seed + 3000)
    sd = {}
    for name, shape in ref_names_shapes:
        shape = tuple(int(s) for s in shape)
        if name in ("rot_scale", "trans_scale"):
            sd[name] = None                     # filled by scaled_init: depends on the constraint
        elif len(shape) == 4:
            fan_in, fan_out = shape[1] * shape[2] * shape[3], shape[0] * shape[2] * shape[3]
            sd[name] = (torch.rand(shape, generator=g) * 2 - 1) * math.sqrt(6.0 / (fan_in + fan_out))
        elif name.endswith(".1.weight"):        # GroupNorm gamma
            sd[name] = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:                                   # GroupNorm beta, convolution bias
            sd[name] = 0.05 * torch.randn(shape, generator=g)
    return sd


def scaled_init(sd, constrain):
    base = 0.4 if constrain == "softplus" else 0.01
    if "rot_scale" in sd:
        sd["rot_scale"] = torch.tensor(base * 1.3)
        sd["trans_scale"] = torch.tensor(base * 0.8)
    return sd


def motion_input(N, C, H, W, seed=0):
    """pose_net_input: two frames of RGB in [0, 1] (+ a depth channel each, 0.5 .. 4.5, when C == 8)."""
    g = torch.Generator().manual_seed(seed + 31)
    x = torch.rand(N, C, H, W, generator=g)
    if C == 8:
        x[:, 3] = x[:, 3] * 4 + 0.5
        x[:, 7] = x[:, 7] * 4 + 0.5
    return x


def loss_weights(N, H, W, seed=0):
    """(Wm [N,3,H,W], Wp [N,4,4]) of the linear loss sum(motion_pred * Wm) + sum(pose_pred * Wp)."""
    g = torch.Generator().manual_seed(seed + 77)
    return torch.randn(N, 3, H, W, generator=g), torch.randn(N, 4, 4, generator=g)

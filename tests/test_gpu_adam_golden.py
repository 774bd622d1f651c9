"""GPU: sde_adam_step and sde_adam_step_twin against recorded bits (tests/golden/adam.npz).

adam_update (csrc/nn.hip) states the update with contraction off and the fused operations spelled out, so that its bits do not depend on what a compiler
chooses to fuse.  The fixture holds p, m, v after three steps as the library built BEFORE that restatement produced them (one-element kernel, compiler's
own contraction), for AdamW, Adam + L2, AdamW under loss scaling and Adam + L2 with a clip coefficient, together with the inputs: 1027 elements (a
4-wide body and a 3-element tail), two segments with a boundary inside a group of four, gradients over ten orders of magnitude with exact zeros.  A
compiler upgrade or an edit that changes one rounding anywhere in either kernel fails here."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adam.npz")
N, SEG_END, SEG_LR, SEG_WD, EPS, STEPS = 1027, [501, 1027], [1e-2, 3e-3], [1e-2, 0.05], 1e-6, 3
VARIANTS = {"adamw": dict(decoupled_wd=True), "l2": dict(decoupled_wd=False),
            "adamw_scale": dict(decoupled_wd=True, scale=[512.0, 0.0, 0.0, 5.0]), "l2_clip": dict(decoupled_wd=False, clip=[3.0, 0.37])}


def run_variant(NN, arrays, name, twin_dtype=None):
    """Three steps from the fixture's inputs; returns (p, m, v[, twin]) as device tensors."""
    kw = dict(VARIANTS[name])
    scale, clip = kw.pop("scale", None), kw.pop("clip", None)
    if scale is not None:
        kw["scale_state"] = torch.tensor(scale, device=DEV)
    if clip is not None:
        kw["clip_state"] = torch.tensor(clip, device=DEV)
    p, m, v = (torch.from_numpy(arrays[k].copy()).to(DEV) for k in ("p0", "m0", "v0"))
    twin = torch.zeros(N, device=DEV, dtype=twin_dtype) if twin_dtype is not None else None
    for t in range(1, STEPS + 1):
        g = torch.from_numpy(arrays[f"g{t}"].copy()).to(DEV)
        NN.adam_step(p, g, m, v, SEG_END, SEG_LR, SEG_WD, (1 - 0.9 ** t, 1 - 0.999 ** t), eps=EPS, **kw, **({"twin": twin} if twin is not None else {}))
    torch.cuda.synchronize()
    return (p, m, v) + ((twin,) if twin is not None else ())


@pytest.fixture(scope="module")
def NN():
    from simpledepthestimation_amd.hip import nn
    return nn


@pytest.fixture(scope="module")
def arrays():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("kernel", ["plain", "twin_bf16", "twin_fp16"])
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_adam_bits_equal_the_recorded_ones(NN, arrays, name, kernel):
    dt = {"plain": None, "twin_bf16": torch.bfloat16, "twin_fp16": torch.float16}[kernel]
    out = run_variant(NN, arrays, name, dt)
    for key, got in zip("pmv", out):
        want = arrays[f"{name}.{key}"]
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), f"{name} {kernel}: {key} differs from the recorded bits"
        assert np.isfinite(want).all() and not np.array_equal(want, arrays[f"{key}0"])
    if dt is not None:
        assert torch.equal(out[3].view(torch.int16), out[0].to(dt).view(torch.int16))       # the twin is the round-to-nearest-even cast of the stored p

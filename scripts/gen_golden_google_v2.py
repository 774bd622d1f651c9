"""Writes tests/golden/google_v2.npz from the reference's own GoogleResNetv2.py (run on the CPU, unmodified).

Usage: python scripts/gen_golden_google_v2.py   (needs the reference checkout named by oracle.ref_harness; not used on the GPU machine)

In this process only: torch.randn_like (RandLayerNorm's noise) draws values that are exactly representable in fp16, recorded per module so the GPU
tests can inject the same draws.  Weights come from tests/google_v2_init.py.
Contents (arrays and name lists only):
  case{k}_names / case{k}_shapes   the state dict of each case
  case{k}_depth, _loss             the training-mode depth map and its SILog loss
  case{k}_grad_names / _grad_norms the gradient norm of every parameter that receives one
  case{k}_z_{step}_{module}        the noise draws [2,B,C] (mean, variance) of every RandLayerNorm, step 0 = the forward above
  case0_eval / case0_flip          eval-mode outputs (no noise), plain and flipped
  case0_adam_loss / _adam_norms    3 AdamW steps as supervised_trainer builds them (projects/Supervised/train.py:L77-81), steps 1..3
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness  # noqa: E402
import google_v2_init  # noqa: E402

# (norm, learn_scale, B, H, W)
CASES = [("randLN", False, 2, 64, 192), ("BN", False, 2, 64, 192), ("randLN", True, 2, 64, 192)]
ADAM_STEPS = 3
LR = 2e-4
TRACK = ["encoder.conv1.weight", "encoder.layer1.0.bn1.weight", "encoder.layer4.1.conv2.weight", "encoder.layer2.0.downsample.weight",
         "decoder.blocks.0.upconv.weight", "decoder.blocks.4.upconv.bias", "decoder.out_conv.weight", "decoder.out_conv.bias"]
DRAWS = []          # the draws of the running forward, in call order


def load_ref():
    ref = ref_harness.load()
    dn = sys.modules["detectron2.modeling.depth_net"]
    dn.DEPTH_NET_REGISTRY = sys.modules["detectron2.modeling.depth_net.build"].DEPTH_NET_REGISTRY
    G = importlib.import_module("detectron2.modeling.depth_net.GoogleResNetv2")
    LN = importlib.import_module("detectron2.layers.layer_norm")
    gen = torch.Generator().manual_seed(4321)

    def randn_like(t):
        z = torch.randn(t.shape, generator=gen).half().float()        # exactly representable in fp16
        DRAWS.append(z)
        return z

    torch.randn_like = randn_like            # (this process only) RandLayerNorm.forward is the one caller
    return ref, G, LN


class Cfg:
    def __init__(self, norm, learn_scale):
        dn = type("DN", (), dict(ENCODER_NAME="18??", NORM=norm, LEARN_SCALE=learn_scale, UPSAMPLE_DEPTH=False))
        self.MODEL = type("M", (), dict(DEPTH_NET=dn))


def model_input(batch, flip=False):
    mean = torch.tensor(google_v2_init.PIXEL_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(google_v2_init.PIXEL_STD).view(1, 3, 1, 1)
    d = {"depth_net_input": (batch["img"] - mean) / std}
    if flip:
        d["flip"] = True
    return d


def run(model, LN, batch, out, key):
    """One forward; records every RandLayerNorm's (mean, variance) draws under out[key + module name]."""
    names = [n for n, m in model.named_modules() if isinstance(m, LN.RandLayerNorm)]
    DRAWS.clear()
    res = model(model_input(batch))
    if model.training and names:
        # modules run in registration order: the blocks' norms follow their convolutions, the shortcut has none
        assert len(DRAWS) == 2 * len(names)
        for i, n in enumerate(names):
            zm, zv = DRAWS[2 * i], DRAWS[2 * i + 1]
            out[key + n] = torch.stack([zm.reshape(zm.shape[0], -1), zv.reshape(zv.shape[0], -1)]).numpy().astype(np.float16)
    return res


def main():
    ref, G, LN = load_ref()
    silog = ref.losses.silog_loss(0.85)
    out = {}
    for ci, (norm, ls, B, H, W) in enumerate(CASES):
        p = f"case{ci}_"
        torch.manual_seed(0)
        model = G.GoogleResNetv2(Cfg(norm, ls))
        sd = model.state_dict()
        out[p + "names"] = np.array(list(sd))
        out[p + "shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
        init = google_v2_init.google_v2_state_dict([(n, tuple(v.shape)) for n, v in sd.items()], seed=ci)
        model.load_state_dict(init, strict=True)
        model.train()
        batch = google_v2_init.google_batch(B, H, W, seed=ci)
        res = run(model, LN, batch, out, p + "z_0_")
        loss = silog(res["depth_pred"][0], batch["depth"])
        loss.backward()
        out[p + "depth"] = res["depth_pred"][0].detach().numpy()
        out[p + "loss"] = np.float64(loss.item())
        gn = [(n, q.grad.double().norm().item()) for n, q in model.named_parameters() if q.grad is not None]
        out[p + "grad_names"] = np.array([n for n, _ in gn])
        out[p + "grad_norms"] = np.array([v for _, v in gn])
        if ci:
            continue
        with torch.no_grad():
            model.eval()
            out[p + "eval"] = model(model_input(batch))["depth_pred"][0].numpy()
            out[p + "flip"] = model(model_input(batch, flip=True))["depth_pred"][0].numpy()
        model.load_state_dict(init, strict=True)
        model.train()
        opt = torch.optim.AdamW([{"params": model.encoder.parameters(), "weight_decay": 1e-2},
                                 {"params": model.decoder.parameters(), "weight_decay": 0}], lr=LR, eps=1e-6)
        losses, norms = [], []
        for k in range(ADAM_STEPS):
            opt.zero_grad()
            res = run(model, LN, batch, out, p + f"z_{k + 1}_")
            loss = silog(res["depth_pred"][0], batch["depth"])
            loss.backward()
            opt.step()
            losses.append(loss.item())
            norms.append([dict(model.named_parameters())[n].detach().double().norm().item() for n in TRACK])
        out[p + "adam_loss"] = np.array(losses)
        out[p + "adam_norms"] = np.array(norms)
    out["adam_track"] = np.array(TRACK)
    path = os.path.join(ROOT, "tests", "golden", "google_v2.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

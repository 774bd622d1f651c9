"""Writes tests/golden/motion.npz from the reference's own GooglePoseNet.py (run on the CPU, unmodified).

Usage: python scripts/gen_golden_motion.py   (needs the reference checkout named by oracle.ref_harness; not used on the GPU machine)

Every case of tests/motion_init.py CASES runs twice, in fp32 (the golden values) and in fp64 (their error bars), with the weights, input and
loss weights of tests/motion_init.py; the loss is sum(motion_pred * Wm) + sum(pose_pred * Wp).  Contents (arrays and name lists only):
  case{k}_names / _shapes          the state dict
  case{k}_pose, _motion, _loss     fp32 outputs (motion: GoogleMotionNet only)
  case{k}_grad_names / _grad_norms / _grad_norms64   gradient norm of every parameter, fp32 and fp64 run
  case{k}_full_{name}              full fp32 gradients of the small parameters motion_init.FULL_GRADS
  case{k}_xgrad                    d loss / d pose_net_input (mask-off cases and GooglePoseNet)
  case{k}_d_{pose,motion,loss,xgrad}, _d_grad_norms, _d_full_{name}   relative difference fp32 vs fp64 of each compared quantity
                                   (tensors: max |a - b| / max |b|; norms and the loss: |a - b| / |b|)
  case{k}_band                     mask-on cases: np.packbits of the pixels [N,H,W] whose norm lies within 1e-3 * mean of the mask threshold
                                   in the fp64 run (left out of the motion_pred comparison; at most 1 % of the pixels, asserted here)
"""
import copy
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness  # noqa: E402
import motion_init  # noqa: E402


class CN(dict):
    __getattr__ = dict.__getitem__


def ref_cfg(case):
    _, gn, sc, mask, learn, use_depth = case[:6]
    return CN(MODEL=CN(POSE_NET=CN(GROUP_NORM=gn, LEARN_SCALE=learn, MASK_MOTION=mask, SCALE_CONSTRAIN=sc, USE_DEPTH=use_depth)))


def rel_t(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


def run(net, x, wm, wp, dt):
    n = copy.deepcopy(net).to(dt).train()
    xi = x.detach().clone().to(dt).requires_grad_(True)
    o = n({"pose_net_input": xi})
    loss = (o["pose_pred"] * wp.to(dt)).sum()
    if "motion_pred" in o:
        loss = loss + (o["motion_pred"] * wm.to(dt)).sum()
    loss.backward()
    grads = {k: p.grad.detach() for k, p in n.named_parameters() if p.grad is not None}
    return dict(pose=o["pose_pred"].detach(), motion=o["motion_pred"].detach() if "motion_pred" in o else None, loss=loss.detach(),
                xgrad=xi.grad.detach(), grads=grads)


def main():
    ref_harness.load()
    G = importlib.import_module("detectron2.modeling.pose_net.GooglePoseNet")
    out = {}
    for ci, case in enumerate(motion_init.CASES):
        name, gn, sc, mask, learn, use_depth, N, H, W = case
        p = f"case{ci}_"
        torch.manual_seed(0)
        net = getattr(G, name)(ref_cfg(case))
        sd = net.state_dict()
        out[p + "names"] = np.array(list(sd))
        out[p + "shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
        init = motion_init.scaled_init(motion_init.motion_state_dict([(n, tuple(v.shape)) for n, v in sd.items()], seed=ci), sc)
        net.load_state_dict(init, strict=True)
        x = motion_init.motion_input(N, 8 if use_depth else 6, H, W, seed=ci)
        wm, wp = motion_init.loss_weights(N, H, W, seed=ci)
        a, b = run(net, x, wm, wp, torch.float32), run(net, x, wm, wp, torch.float64)
        out[p + "pose"] = a["pose"].numpy()
        out[p + "d_pose"] = np.float64(rel_t(a["pose"], b["pose"]))
        out[p + "loss"] = np.float64(a["loss"].item())
        out[p + "d_loss"] = np.float64(abs(a["loss"].item() - b["loss"].item()) / abs(b["loss"].item()))
        sel = None
        if name == "GoogleMotionNet" and mask:
            net64 = copy.deepcopy(net).double().train()
            net64.mask_motion = False
            r = net64({"pose_net_input": x.double()})["motion_pred"].detach()
            nrm = torch.sqrt((r ** 2).sum(1))
            mean = nrm.mean()
            band = (nrm - mean).abs() <= 1e-3 * mean
            frac = band.double().mean().item()
            assert frac <= 0.01, (ci, frac)
            out[p + "band"] = np.packbits(band.numpy().astype(np.uint8).reshape(-1))
            sel = (~band).unsqueeze(1).expand_as(r)
            print(f"case {ci}: {100 * frac:.3f} % of the pixels in the threshold band, {100 * (nrm > mean).double().mean().item():.1f} % pass the mask")
        if a["motion"] is not None:
            out[p + "motion"] = a["motion"].numpy()
            ma, mb = (a["motion"], b["motion"]) if sel is None else (a["motion"][sel], b["motion"][sel])
            out[p + "d_motion"] = np.float64(rel_t(ma, mb))
        names = list(a["grads"])
        n32 = np.array([a["grads"][k].double().norm().item() for k in names])
        n64 = np.array([b["grads"][k].double().norm().item() for k in names])
        out[p + "grad_names"], out[p + "grad_norms"], out[p + "grad_norms64"] = np.array(names), n32, n64
        out[p + "d_grad_norms"] = np.abs(n32 - n64) / np.maximum(n64, 1e-300)
        for k in motion_init.FULL_GRADS:
            if k in a["grads"]:
                out[p + "full_" + k] = a["grads"][k].numpy()
                out[p + "d_full_" + k] = np.float64(rel_t(a["grads"][k], b["grads"][k]))
        if not (name == "GoogleMotionNet" and mask):
            out[p + "xgrad"] = a["xgrad"].numpy()
            out[p + "d_xgrad"] = np.float64(rel_t(a["xgrad"], b["xgrad"]))
        print(f"case {ci} {name}: d_pose {out[p + 'd_pose']:.2e} d_motion {float(out.get(p + 'd_motion', 0)):.2e} d_loss {out[p + 'd_loss']:.2e} "
              f"d_xgrad {float(out.get(p + 'd_xgrad', 0)):.2e} max d_grad_norm {out[p + 'd_grad_norms'].max():.2e} "
              f"max d_full {max(float(v) for k, v in out.items() if k.startswith(p + 'd_full_')):.2e}")
    path = os.path.join(ROOT, "tests", "golden", "motion.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

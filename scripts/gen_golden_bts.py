"""Writes tests/golden/bts.npz from the reference's own BTSNet.py (run on the CPU, fp32/fp64-free, unmodified).

Usage: python scripts/gen_golden_bts.py   (needs the reference checkout named by oracle.ref_harness; not used on the GPU machine)

In this process only: torchvision.models.resnet50 accepts pretrained=True and initialises randomly (no download), Tensor.cuda is the
identity (local_planar_guidance moves its grids with .cuda()).  Weights come from tests/bts_init.py, shared with the tests.
Contents (arrays and name lists only):
  names / shapes                 the BtsModel state dict (BTS_SIZE 512)
  trainable_{none,conv,convs}    names of parameters left trainable by set_misc for FIX_1ST_CONV / FIX_1ST_CONVS
  case{0,1}_*                    two cases (BTS_SIZE 512 at bs 2, 64x128; BTS_SIZE 128 at bs 2, 96x320), each: the five outputs, the SILog
                                 loss, the grad norm of every trainable parameter, the running statistics of bn5, daspp_12's first_bn and the
                                 encoder's frozen bn1 after one train forward, (case 0:) the other four outputs, the flip output, the eval output after that train forward,
                                 and the loss and parameter norms over 3 AdamW steps built as in projects/Supervised/train.py:L77-81
BTS_SIZE 64 is not a case: its reduc1x1 has no layer at all and the reference's conv1 then receives 11 instead of 8 channels.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness  # noqa: E402
import bts_init  # noqa: E402

CASES = [(512, 2, 64, 128), (128, 2, 96, 320)]
MAX_DEPTH = 80.0
ADAM_STEPS = 3
LR = 2e-4
TRACK = ["encoder.base_model.conv1.weight", "encoder.base_model.layer1.0.conv1.weight", "encoder.base_model.layer4.2.conv3.weight",
         "encoder.base_model.fc.weight", "decoder.upconv5.conv.weight", "decoder.daspp_24.atrous_conv.aconv_sequence.4.weight",
         "decoder.get_depth.0.weight", "decoder.bn5.weight"]
RUNNING = ["decoder.bn5", "decoder.daspp_12.atrous_conv.first_bn", "encoder.base_model.bn1"]


def load_ref():
    ref = ref_harness.load()
    tvm = sys.modules["torchvision.models"]
    base = tvm.resnet50
    tvm.resnet50 = lambda pretrained=False, **kw: base(**kw)
    torch.Tensor.cuda = lambda self, *a, **k: self
    dn = sys.modules["detectron2.modeling.depth_net"]
    dn.DEPTH_NET_REGISTRY = sys.modules["detectron2.modeling.depth_net.build"].DEPTH_NET_REGISTRY
    import importlib
    return ref, importlib.import_module("detectron2.modeling.depth_net.BTSNet")


class Cfg:
    def __init__(self, bts_size, fix1=False, fix2=False):
        dn = type("DN", (), dict(ENCODER_NAME="resnet50_bts", BTS_SIZE=bts_size, BN_NO_TRACK=False, FIX_1ST_CONV=fix1, FIX_1ST_CONVS=fix2))
        self.MODEL = type("M", (), dict(DEPTH_NET=dn, DATASET="kitti", MAX_DEPTH=MAX_DEPTH))


def model_input(batch):
    mean = torch.tensor(bts_init.PIXEL_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(bts_init.PIXEL_STD).view(1, 3, 1, 1)
    return {"depth_net_input": (batch["img"] - mean) / std, "intrinsics": batch["intrinsics"]}


def main():
    ref, BT = load_ref()
    silog = ref.losses.silog_loss(0.85)
    out = {}
    torch.manual_seed(0)
    m512 = BT.BtsModel(Cfg(512))
    names = list(m512.state_dict().keys())
    out["names"] = np.array(names)
    out["shapes"] = np.array([",".join(str(s) for s in v.shape) for v in m512.state_dict().values()])
    for tag, f1, f2 in (("none", False, False), ("conv", True, False), ("convs", False, True)):
        m = BT.BtsModel(Cfg(128, f1, f2))
        out["trainable_" + tag] = np.array([n for n, p in m.named_parameters() if p.requires_grad])
    for ci, (size, B, H, W) in enumerate(CASES):
        p = f"case{ci}_"
        torch.manual_seed(0)
        model = BT.BtsModel(Cfg(size))
        sd = model.state_dict()
        init = bts_init.bts_state_dict([(n, tuple(v.shape)) for n, v in sd.items()], seed=ci)
        model.load_state_dict(init, strict=True)
        model.train()
        batch = bts_init.bts_batch(B, H, W, seed=ci)
        res = model(model_input(batch))
        loss = silog(res["depth_pred"][0], batch["depth"])
        loss.backward()
        for k in (("depth_8x8", "depth_4x4", "depth_2x2", "reduc_1x1") if ci == 0 else ()):     # (size limit: case 1 keeps the final map)
            out[p + k] = res[k].detach().numpy()
        out[p + "final"] = res["depth_pred"][0].detach().numpy()
        out[p + "loss"] = np.float64(loss.item())
        gn = [(n, q.grad.double().norm().item()) for n, q in model.named_parameters() if q.requires_grad and q.grad is not None]
        out[p + "grad_names"] = np.array([n for n, _ in gn])
        out[p + "grad_norms"] = np.array([v for _, v in gn])
        out[p + "no_grad"] = np.array([n for n, q in model.named_parameters() if q.grad is None])
        sd1 = model.state_dict()
        for r in RUNNING:
            out[p + "rm_" + r] = sd1[r + ".running_mean"].clone().numpy()
            out[p + "rv_" + r] = sd1[r + ".running_var"].clone().numpy()
        with torch.no_grad():
            model.eval()
            out[p + "eval_final"] = model(model_input(batch))["depth_pred"][0].numpy()
            fb = model_input(batch)
            fb["flip"] = True
            out[p + "flip_final"] = model(fb)["depth_pred"][0].numpy()
        if ci:      # (size limit: case 1 keeps neither)
            del out[p + "eval_final"], out[p + "flip_final"]
        # 3 AdamW steps as do_train builds them, from the initial weights
        model.load_state_dict(init, strict=True)
        model.train()
        opt = torch.optim.AdamW([{"params": model.encoder.parameters(), "weight_decay": 1e-2},
                                 {"params": model.decoder.parameters(), "weight_decay": 0}], lr=LR, eps=1e-6)
        losses, norms = [], []
        for _ in range(ADAM_STEPS):
            opt.zero_grad()
            res = model(model_input(batch))
            loss = silog(res["depth_pred"][0], batch["depth"])
            loss.backward()
            opt.step()
            losses.append(loss.item())
            norms.append([dict(model.named_parameters())[n].detach().double().norm().item() for n in TRACK])
        out[p + "adam_loss"] = np.array(losses)
        out[p + "adam_norms"] = np.array(norms)
    out["adam_track"] = np.array(TRACK)
    out["running_names"] = np.array(RUNNING)
    path = os.path.join(ROOT, "tests", "golden", "bts.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

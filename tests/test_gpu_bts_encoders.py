"""GPU: the ResNet-101 / ResNeXt encoders against the torch restatement of torchvision's network (tests/resnext_ref.py), and BtsModel on
resnext101_bts through one captured training step.

Tolerance of the network comparisons, relative to the maximum (`rel` of tests/test_gpu_bts.py): 4 x the deviation between the restatement run in float32
and in float64 on the same inputs -- measured on the CPU here and printed, separately over the five features and over the parameter gradients -- with
the project's fp32 tolerance 2e-5 as the floor.  The margin of 4 covers a different but equally valid fp32 summation order through ~100 layers; the
bound never derives from the code under test.  The comparison itself is against the float64 run.
Measured deviations of the restatement (float32 vs float64): one-block ResNeXt 4.3e-6 (features) / 8.2e-6 (gradients); the full 101-layer encoders at
2 x 96 x 160 4.9e-4 / 4.7e-4 on the features but 0.43 / 0.26 on the worst parameter gradient -- at that size the gradients are ill-conditioned, so the
full-depth gradient check only bounds gross errors and the one-block network carries the tight one (MI355X: 4.7e-6 / 9.6e-6 there).
"""
import functools
import math

import pytest
import torch

import bts_init
import resnext_ref

pytestmark = pytest.mark.gpu
dev = "cuda:0"
FLOOR = 2e-5


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


NETS = {  # name: (restatement, encoder factory)
    "resnext_1111_32x4d": (lambda: resnext_ref.ResNet([1, 1, 1, 1], 32, 4), (2, 64, 96)),
    "resnext101_bts": (resnext_ref.resnext101_32x8d, (2, 96, 160)),
    "resnet101_bts": (resnext_ref.resnet101, (2, 96, 160)),
}


def make_encoder(name):
    from simpledepthestimation_amd.layers.resnet_encoder import ResnetEncoder
    from simpledepthestimation_amd.modeling.depth_net.BTSNet import BtsEncoder
    if name == "resnext_1111_32x4d":
        return ResnetEncoder(101, groups=32, width_per_group=4, layers=[1, 1, 1, 1])
    return BtsEncoder(name)


def run_ref(net, x, cots, dtype):
    net = net.to(dtype).train()
    for p in net.parameters():
        p.grad = None
    feats = net.features(x.to(dtype))
    torch.autograd.backward(feats, [c.to(dtype) for c in cots])
    return [f.detach() for f in feats], {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's weights, the input, the cotangents, its float64 features and gradients, and the two float32-vs-float64 deviations: computed
    once per network, shared, never modified."""
    make, (B, H, W) = NETS[name]
    torch.manual_seed(len(name))
    net = make()
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, 3, H, W, generator=g)
    with torch.no_grad():
        shapes = [f.shape for f in net.eval().features(x)]
    cots = [torch.randn(s, generator=g) / math.sqrt(s[1] * s[2] * s[3]) for s in shapes]
    f32, g32 = run_ref(net, x, cots, torch.float32)
    net.load_state_dict(sd)                       # (the training-mode run moved the running statistics)
    f64, g64 = run_ref(net, x, cots, torch.float64)
    dev_f = max(rel(a, b) for a, b in zip(f32, f64))
    dev_g = max(rel(g32[n], g64[n]) for n in g64)
    print(f"  {name}: restatement float32 vs float64: features {dev_f:.2e}, gradients {dev_g:.2e}")
    return dict(sd=sd, x=x, cots=cots, feats=f64, grads=g64, tol_f=max(4 * dev_f, FLOOR), tol_g=max(4 * dev_g, FLOOR))


def run_device(name, direct):
    from simpledepthestimation_amd.hip import nn as HN
    ref = reference(name)
    old = HN.GCONV_DIRECT
    HN.GCONV_DIRECT = direct
    try:
        enc = make_encoder(name)
        enc.encoder.load_state_dict(ref["sd"], strict=True)
        enc = enc.to(dev).train()
        x = HN.prep_input(ref["x"].to(dev), None, None, torch.float32)
        feats = enc(x)
        torch.autograd.backward(feats, [c.permute(0, 2, 3, 1).contiguous().to(dev) for c in ref["cots"]])
        torch.cuda.synchronize()
    finally:
        HN.GCONV_DIRECT = old
    return [f.detach().permute(0, 3, 1, 2) for f in feats], {n: p.grad for n, p in enc.encoder.named_parameters() if p.grad is not None}


def check(name, direct):
    ref = reference(name)
    feats, grads = run_device(name, direct)
    ef = [rel(a, b) for a, b in zip(feats, ref["feats"])]
    assert set(grads) == set(ref["grads"])
    eg = {n: rel(grads[n], ref["grads"][n]) for n in grads}
    worst = max(eg, key=eg.get)
    print(f"  {name} direct={direct}: features {max(ef):.2e} (bound {ref['tol_f']:.2e}), gradients {eg[worst]:.2e} at {worst} (bound {ref['tol_g']:.2e})")
    assert max(ef) <= ref["tol_f"], f"features: {ef}"
    assert eg[worst] <= ref["tol_g"], f"gradient of {worst}: {eg[worst]:.3e}"


@pytest.mark.parametrize("direct", [True, False], ids=["kernels", "composed"])
def test_small_resnext_encoder_matches_the_restatement(direct):
    check("resnext_1111_32x4d", direct)


@pytest.mark.parametrize("name", ["resnext101_bts", "resnet101_bts"])
def test_bts_encoder_matches_the_restatement(name):
    check(name, True)


def build_model(dtype, encoder="resnext101_bts"):
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.modeling import build_model as build
    cfg = get_cfg()
    cfg.MODEL.META_ARCHITECTURE, cfg.MODEL.DEVICE, cfg.MODEL.DATASET, cfg.MODEL.COMPUTE_DTYPE = "SupDepthModel", dev, "kitti", dtype
    cfg.MODEL.DEPTH_NET.NAME, cfg.MODEL.DEPTH_NET.ENCODER_NAME, cfg.MODEL.DEPTH_NET.BTS_SIZE = "BtsModel", encoder, 128
    cfg.SOLVER.DEPTH_LR = 2e-4
    torch.manual_seed(1)
    return build(cfg), cfg


def test_resnext101_bts_model_trains_under_graph_capture_and_evaluates():
    from simpledepthestimation_amd.engine.trainer import supervised_trainer
    from simpledepthestimation_amd.layers.hip_modules import HipGroupedConv2d
    model, cfg = build_model("bf16")
    model.train()
    tr = supervised_trainer(model, cfg, use_graph=True)
    conv = model.depth_net.encoder.base_model.layer3[5].conv2
    assert isinstance(conv, HipGroupedConv2d)
    batch = {k: v.to(dev) for k, v in bts_init.bts_batch(2, 96, 160, seed=2).items()}
    before = [conv.weight.detach().clone(), model.depth_net.decoder.get_depth[0].weight.detach().clone()]
    losses = []
    for _ in range(3):                            # eager first step, then capture and replay
        out = tr.step(dict(batch))
        losses.append(float(out["silog_loss"].detach()))
    torch.cuda.synchronize()
    assert all(math.isfinite(v) for v in losses), losses
    assert torch.isfinite(tr.pflat).all()
    assert not torch.equal(conv.weight.detach(), before[0]) and not torch.equal(model.depth_net.decoder.get_depth[0].weight.detach(), before[1])
    model.eval()
    with torch.no_grad():
        ev = model(dict(batch))["depth_pred"]
    ev = ev[0] if isinstance(ev, (list, tuple)) else ev
    assert tuple(ev.shape) == (2, 1, 96, 160) and torch.isfinite(ev).all()


@pytest.mark.parametrize("encoder", ["resnext101_bts", "resnet101_bts"])
def test_do_train_runs_with_the_new_encoders(encoder, tmp_path):
    """bts_r50.yaml's model with another MODEL.DEPTH_NET.ENCODER_NAME through engine.loops.do_train: two logged iterations with finite losses."""
    from simpledepthestimation_amd.engine.loops import do_train
    model, cfg = build_model("bf16", encoder)
    cfg.OUTPUT_DIR = str(tmp_path)
    cfg.LOG_PERIOD, cfg.SOLVER.MAX_EPOCHS, cfg.TEST.EVAL_PERIOD = 1, 1, 0
    loader = [bts_init.bts_batch(2, 96, 160, seed=30 + i) for i in range(2)]
    rec = do_train(cfg, model, loader, None)
    assert [r["iteration"] for r in rec] == [1, 2]
    assert all(math.isfinite(r["total_loss"]) for r in rec)

"""GPU: the DenseNet encoder against the torch restatement of torchvision's network (tests/densenet_ref.py) on both routes of
hip.dense.DENSE_DIRECT, its launch structure, and BtsModel on densenet121_bts through captured training steps.

Tolerance of the network comparisons (the rule of tests/test_gpu_bts_encoders.py), relative to the maximum: 4 x the deviation between the
restatement run in float32 and in float64 on the same inputs -- measured on the CPU here and printed, separately over the five features and over
the parameter gradients -- with the project's fp32 tolerance 2e-5 as the floor.  The bound never derives from the code under test; the comparison
itself is against the float64 run.  The small network carries the tight gradient check; at full depth the gradients are ill-conditioned and the
bound only catches gross errors.
"""
import functools
import math

import pytest
import torch

import bts_init
import densenet_ref

pytestmark = pytest.mark.gpu
dev = "cuda:0"
FLOOR = 2e-5
SMALL = dict(growth_rate=16, block_config=(2, 2, 2, 2), num_init_features=32)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


NETS = {  # name: (restatement, input size, whether the input is chosen clear of the ReLU kinks: see reference())
    "densenet_2222": (lambda: densenet_ref.DenseNetFeatures(**SMALL), (2, 64, 96), True),
    "densenet121_bts": (densenet_ref.densenet121, (2, 96, 160), False),
}


def make_encoder(name):
    from simpledepthestimation_amd.layers.densenet_encoder import DenseNetEncoder
    from simpledepthestimation_amd.modeling.depth_net.BTSNet import build_encoder
    return DenseNetEncoder(**SMALL) if name == "densenet_2222" else build_encoder(name)


def run_ref(net, x, cots, dtype):
    """(features, parameter gradients, BatchNorm outputs = every ReLU's input) of the restatement in `dtype`."""
    net = net.to(dtype).train()
    for p in net.parameters():
        p.grad = None
    pre = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: pre.append(out.detach())) for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    feats = net.features(x.to(dtype))
    for h in hooks:
        h.remove()
    torch.autograd.backward(feats, [c.to(dtype) for c in cots])
    return [f.detach() for f in feats], {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}, pre


KINK_MARGIN = 2       # a ReLU input counts as clear of the kink when it is this many times its layer's LARGEST float32-vs-float64 deviation away from zero
                      # (the typical deviation of an element is a tenth of the largest; about one input seed in seven qualifies)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's weights, the input, the cotangents, its float64 features and gradients, and the two float32-vs-float64 deviations: computed
    once per network, shared, never modified.

    A ReLU input within float32 rounding of zero makes the gradient of its channel a coin toss between two equally valid float32 evaluations (one
    pixel of a 2 x 2 x 3 map is a twelfth of a channel's gradient), which no tolerance derived from rounding covers.  For the network that carries
    the tight gradient check the input seed is therefore the first one for which every BatchNorm output of the float64 run lies at least
    KINK_MARGIN x (that layer's largest float32-vs-float64 deviation, both measured on the restatement) away from zero.  Decided by the restatement alone."""
    make, (B, H, W), clear_of_kinks = NETS[name]
    torch.manual_seed(len(name))
    net = make()
    with torch.no_grad():       # BatchNorm parameters off their 1 / 0 initialisation, so that a wrong gamma / beta gradient or channel offset shows
        for n, p in net.named_parameters():
            if "norm" in n:
                p.add_(0.2 * torch.randn(p.shape))
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    for seed in range(11, 43):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(B, 3, H, W, generator=g)
        net.load_state_dict(sd)
        with torch.no_grad():
            shapes = [f.shape for f in net.float().eval().features(x)]
        cots = [torch.randn(s, generator=g) / math.sqrt(s[1] * s[2] * s[3]) for s in shapes]
        f32, g32, z32 = run_ref(net, x, cots, torch.float32)
        net.load_state_dict(sd)                       # (the training-mode run moved the running statistics)
        f64, g64, z64 = run_ref(net, x, cots, torch.float64)
        clearance = min(float(b.abs().min() / (a.double() - b).abs().max().clamp_min(1e-12)) for a, b in zip(z32, z64))
        if not clear_of_kinks or clearance >= KINK_MARGIN:
            break
    else:
        raise AssertionError(f"{name}: no input seed keeps every ReLU input {KINK_MARGIN} x the layer's deviation away from zero")
    dev_f = max(rel(a, b) for a, b in zip(f32, f64))
    dev_g = max(rel(g32[n], g64[n]) for n in g64)
    print(f"  {name}: input seed {seed}, nearest ReLU input {clearance:.1f} x its layer's deviation from zero; restatement float32 vs float64: features {dev_f:.2e}, "
          f"gradients {dev_g:.2e}")
    return dict(sd=sd, x=x, cots=cots, feats=f64, grads=g64, tol_f=max(4 * dev_f, FLOOR), tol_g=max(4 * dev_g, FLOOR))


def run_device(name, direct, count=None):
    from simpledepthestimation_amd.hip import bts as HB
    from simpledepthestimation_amd.hip import dense as HD
    from simpledepthestimation_amd.hip import nn as HN
    ref = reference(name)
    old = HD.DENSE_DIRECT, HB.cat, HB.channel_stats
    HD.DENSE_DIRECT = direct
    if count is not None:
        def counted(key, fn):
            def call(*a, **k):
                count[key] = count.get(key, 0) + 1
                return fn(*a, **k)
            return call
        HB.cat, HB.channel_stats = counted("cat", HB.cat), counted("channel_stats", HB.channel_stats)
    try:
        enc = make_encoder(name)
        enc.base_model.load_state_dict(ref["sd"], strict=True)
        enc = enc.to(dev).train()
        x = HN.prep_input(ref["x"].to(dev), None, None, torch.float32)
        feats = enc(x)
        torch.autograd.backward(feats, [c.permute(0, 2, 3, 1).contiguous().to(dev) for c in ref["cots"]])
        torch.cuda.synchronize()
    finally:
        HD.DENSE_DIRECT, HB.cat, HB.channel_stats = old
    return [f.detach().permute(0, 3, 1, 2) for f in feats], {n: p.grad for n, p in enc.base_model.named_parameters() if p.grad is not None}


def check(name, direct):
    ref = reference(name)
    feats, grads = run_device(name, direct)
    assert [tuple(f.shape) for f in feats] == [tuple(f.shape) for f in ref["feats"]]
    ef = [rel(a, b) for a, b in zip(feats, ref["feats"])]
    assert set(grads) == set(ref["grads"])
    eg = {n: rel(grads[n], ref["grads"][n]) for n in grads}
    worst = max(eg, key=eg.get)
    print(f"  {name} direct={direct}: features {max(ef):.2e} (bound {ref['tol_f']:.2e}), gradients {eg[worst]:.2e} at {worst} (bound {ref['tol_g']:.2e})")
    assert max(ef) <= ref["tol_f"], f"features: {ef}"
    assert eg[worst] <= ref["tol_g"], f"gradient of {worst}: {eg[worst]:.3e}"


@pytest.mark.parametrize("direct", [True, False], ids=["kernels", "composed"])
def test_small_densenet_encoder_matches_the_restatement(direct):
    check("densenet_2222", direct)


def test_densenet121_encoder_matches_the_restatement():
    check("densenet121_bts", True)


def test_direct_route_never_concatenates_and_reduces_each_block_input_once():
    count = {}
    run_device("densenet_2222", True, count)
    assert count.get("cat", 0) == 0 and count.get("channel_stats", 0) <= 4, count
    composed = {}
    run_device("densenet_2222", False, composed)        # the counters do count: the composed route concatenates and reduces per norm
    assert composed["cat"] == 8 and composed["channel_stats"] == 12, composed


def build_model(dtype, encoder="densenet121_bts"):
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.modeling import build_model as build
    cfg = get_cfg()
    cfg.MODEL.META_ARCHITECTURE, cfg.MODEL.DEVICE, cfg.MODEL.DATASET, cfg.MODEL.COMPUTE_DTYPE = "SupDepthModel", dev, "kitti", dtype
    cfg.MODEL.DEPTH_NET.NAME, cfg.MODEL.DEPTH_NET.ENCODER_NAME, cfg.MODEL.DEPTH_NET.BTS_SIZE = "BtsModel", encoder, 128
    cfg.SOLVER.DEPTH_LR = 2e-4
    torch.manual_seed(1)
    return build(cfg), cfg


def test_densenet121_bts_model_trains_under_graph_capture_and_evaluates():
    from simpledepthestimation_amd.engine.trainer import supervised_trainer
    model, cfg = build_model("bf16")
    model.train()
    tr = supervised_trainer(model, cfg, use_graph=True)
    conv = model.depth_net.encoder.base_model.denseblock3.denselayer24.conv2
    norm = model.depth_net.encoder.base_model.denseblock3.denselayer24.norm1
    batch = {k: v.to(dev) for k, v in bts_init.bts_batch(2, 96, 160, seed=2).items()}
    before = [conv.weight.detach().clone(), model.depth_net.decoder.get_depth[0].weight.detach().clone(), norm.running_mean.detach().clone()]
    losses = []
    for _ in range(3):                            # eager first step, then capture and replay
        out = tr.step(dict(batch))
        losses.append(float(out["silog_loss"].detach()))
    torch.cuda.synchronize()
    assert all(math.isfinite(v) for v in losses), losses
    assert torch.isfinite(tr.pflat).all()
    assert not torch.equal(conv.weight.detach(), before[0]) and not torch.equal(model.depth_net.decoder.get_depth[0].weight.detach(), before[1])
    assert not torch.equal(norm.running_mean, before[2]) and torch.isfinite(norm.running_var).all()
    model.eval()
    with torch.no_grad():
        ev = model(dict(batch))["depth_pred"]
    ev = ev[0] if isinstance(ev, (list, tuple)) else ev
    assert tuple(ev.shape) == (2, 1, 96, 160) and torch.isfinite(ev).all()


def test_do_train_runs_with_densenet121(tmp_path):
    """bts_r50.yaml's model with MODEL.DEPTH_NET.ENCODER_NAME densenet121_bts through engine.loops.do_train: two logged iterations with finite losses."""
    from simpledepthestimation_amd.engine.loops import do_train
    model, cfg = build_model("bf16")
    cfg.OUTPUT_DIR = str(tmp_path)
    cfg.LOG_PERIOD, cfg.SOLVER.MAX_EPOCHS, cfg.TEST.EVAL_PERIOD = 1, 1, 0
    loader = [bts_init.bts_batch(2, 96, 160, seed=30 + i) for i in range(2)]
    rec = do_train(cfg, model, loader, None)
    assert [r["iteration"] for r in rec] == [1, 2]
    assert all(math.isfinite(r["total_loss"]) for r in rec)

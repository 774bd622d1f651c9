"""GPU: GoogleResNet's operators against float64 torch restatements, and the model against the reference's golden run (tests/golden/google.npz)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import google_init

pytestmark = pytest.mark.gpu
dev = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "google.npz"))
CASES = [("18", "randLN", False, 2, 64, 192), ("18", "BN", False, 2, 64, 192), ("50", "randLN", True, 2, 64, 128)]
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
TOL = {"fp32": 2e-5, "bf16": 2e-2}


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def nhwc(x, c_pad, dt):
    B, C, H, W = x.shape
    out = torch.zeros(B, H, W, c_pad, dtype=dt)
    out[..., :C] = x.permute(0, 2, 3, 1).to(dt)
    return out.to(dev).contiguous()


def nchw(x, C):
    return x[..., :C].permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------------------------------------------------------
def rln_torch(y, gamma, beta, zm, zv, s, train, res, relu, eps=1e-3):
    """float64 restatement of RandLayerNorm (layer_norm.py:L24-33) + residual + ReLU; s == 0 means factor 1."""
    var, mean = torch.var_mean(y, dim=[2, 3], keepdim=True)
    if train and s != 0:
        mean = mean * (1.0 + torch.fmod(zm.view_as(mean) * s, s * 2))
        var = var * (1.0 + torch.fmod(zv.view_as(var) * s, s * 2))
    out = (y - mean.detach()) * torch.rsqrt(var + eps).detach()
    out = gamma.view(1, -1, 1, 1) * out + beta.view(1, -1, 1, 1)
    if res is not None:
        out = out + res
    return F.relu(out) if relu else out


VARIANTS = [  # (train, residual, n_out, s, relu)
    (True, False, 1, 0.5, True), (True, True, 2, 0.5, True), (True, True, 3, 0.0, True), (True, False, 2, 0.5, False), (False, True, 1, 0.5, True)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("variant", range(len(VARIANTS)))
@pytest.mark.parametrize("shape", [(2, 4, 13, 512), (2, 5, 7, 96), (3, 64, 208, 64)])
def test_randln_fwd_bwd(dtype, variant, shape):
    from simpledepthestimation_amd.layers.hip_modules import HipRandLayerNorm
    train, has_res, n_out, s, relu = VARIANTS[variant]
    B, H, W, C = shape
    dt = DT[dtype]
    g = torch.Generator().manual_seed(C + H + variant)
    y = (torch.randn(B, C, H, W, generator=g) * 2 + torch.randn(1, C, 1, 1, generator=g) * 3).to(dt).float()
    res = torch.randn(B, C, H, W, generator=g).to(dt).float() if has_res else None
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    zm, zv = torch.randn(B, C, generator=g), torch.randn(B, C, generator=g)
    gos = [torch.randn(B, C, H, W, generator=g).to(dt).float() for _ in range(n_out)]
    yd = y.double().requires_grad_(True)
    rd = res.double().requires_grad_(True) if has_res else None
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ref = rln_torch(yd, gd, bd, zm.double(), zv.double(), s, train, rd, relu)
    ref.backward(sum(go.double() for go in gos))

    m = HipRandLayerNorm(C).to(dev)
    with torch.no_grad():
        m.weight.copy_(gamma); m.bias.copy_(beta)
    m.stddev = s
    m.train(train)
    m.inject_z(zm, zv)
    yh = nhwc(y, C, dt).requires_grad_(True)
    rh = nhwc(res, C, dt).requires_grad_(True) if has_res else None
    outs = m(yh, rh, relu, n_out)
    outs = outs if isinstance(outs, tuple) else (outs,)
    sum((o.float() * nhwc(go, C, torch.float32)).sum() for o, go in zip(outs, gos)).backward()
    torch.cuda.synchronize()
    tol = TOL[dtype]
    assert rel(nchw(outs[0], C), ref) < tol
    assert rel(nchw(yh.grad, C), yd.grad) < tol
    if has_res:
        assert rel(nchw(rh.grad, C), rd.grad) < tol
    assert rel(m.weight.grad, gd.grad) < (tol if dtype == "fp32" else 3e-2)
    assert rel(m.bias.grad, bd.grad) < (tol if dtype == "fp32" else 3e-2)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_randln_pad_channels_are_zero(dtype):
    from simpledepthestimation_amd.hip import google as HG
    dt = DT[dtype]
    B, H, W, C, ld = 2, 6, 10, 90, 96
    g = torch.Generator().manual_seed(3)
    y = torch.randn(B, H, W, ld, generator=g).to(dt).to(dev).requires_grad_(True)      # garbage in the pad channels
    gamma, beta = torch.ones(C, device=dev, requires_grad=True), torch.full((C,), 0.5, device=dev, requires_grad=True)
    z = torch.randn(2, B, C, device=dev)
    out = HG.rand_layer_norm(y, gamma, beta, z, torch.full((1,), 0.5, device=dev), relu=False)
    out.backward(torch.randn(out.shape, generator=g).to(dt).to(dev))
    torch.cuda.synchronize()
    out = out.detach()
    assert float(out[..., C:].abs().max()) == 0.0 and float(out[..., :C].abs().max()) > 0
    assert float(y.grad[..., C:].abs().max()) == 0.0


def test_randln_default_noise_factors_lie_in_range():
    """Injection off: every (n, c) mean / variance factor 1 + fmod(z s, 2s) lies in (1 - 2s, 1 + 2s); two forwards draw differently."""
    from simpledepthestimation_amd.layers.hip_modules import HipRandLayerNorm
    B, C, HW = 4, 64, 256
    s = 0.5
    g = torch.Generator().manual_seed(9)
    base = torch.randn(B, C, HW, generator=g, dtype=torch.float64)
    mean0 = 5.0 + torch.rand(B, C, 1, generator=g, dtype=torch.float64)
    y = (base + mean0).float()
    var, mean = torch.var_mean(y.double(), dim=2, keepdim=True)
    m = HipRandLayerNorm(C).to(dev).train()
    m.stddev = s
    x = y.permute(0, 2, 1).reshape(B, 16, 16, C).contiguous().to(dev)
    facs = []
    with torch.no_grad():
        for _ in range(2):
            o = m(x, relu=False).double().cpu().reshape(B, HW, C).permute(0, 2, 1)        # o = (y - m~) r~
            yd = y.double()
            r = (o[..., 1] - o[..., 0]) / (yd[..., 1] - yd[..., 0])
            mt = yd[..., 0] - o[..., 0] / r
            fm = mt / mean[..., 0]
            fv = (1.0 / r ** 2 - 1e-3) / var[..., 0]
            facs.append((fm, fv))
    for fm, fv in facs:
        assert float(fm.min()) > 1 - 2 * s - 1e-3 and float(fm.max()) < 1 + 2 * s + 1e-3
        assert float(fv.min()) > 1 - 2 * s - 1e-3 and float(fv.max()) < 1 + 2 * s + 1e-3
        assert float(fm.std()) > 0.05 and float(fv.std()) > 0.05
    assert float((facs[0][0] - facs[1][0]).abs().max()) > 0.05


# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 5, 7, 16), (1, 1, 9, 8), (2, 3, 1, 24), (2, 2, 13, 512), (1, 1, 1, 8)])
def test_bilinear2_align_corners(dtype, shape):
    from simpledepthestimation_amd.hip import google as HG
    B, H, W, C = shape
    dt = DT[dtype]
    g = torch.Generator().manual_seed(H * 31 + W)
    x = torch.randn(B, C, H, W, generator=g).to(dt).float()
    xd = x.double().requires_grad_(True)
    ref = F.interpolate(xd, scale_factor=2, mode="bilinear", align_corners=True)
    go = torch.randn(ref.shape, generator=g).to(dt).float()
    ref.backward(go.double())
    xh = nhwc(x, C, dt).requires_grad_(True)
    out = HG.bilinear2(xh)
    goh = nhwc(go, C, dt)
    out.backward(goh)
    torch.cuda.synchronize()
    assert rel(nchw(out, C), ref) < TOL[dtype]
    assert rel(nchw(xh.grad, C), xd.grad) < TOL[dtype]
    # gather-form backward: identical bits on a second run
    xh2 = xh.detach().clone().requires_grad_(True)
    HG.bilinear2(xh2).backward(goh)
    torch.cuda.synchronize()
    assert torch.equal(xh2.grad, xh.grad)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("flip", [False, True])
def test_softplus_head(dtype, flip):
    from simpledepthestimation_amd.hip import google as HG
    dt = DT[dtype]
    B, H, W = 2, 8, 12
    g = torch.Generator().manual_seed(4)
    z = torch.randn(B, 1, H, W, generator=g) * 10
    z[0, 0, :2] = 25.0 + torch.rand(2, W, generator=g)           # above the threshold
    z = z.to(dt).float()
    zd = z.double().requires_grad_(True)
    ref = F.softplus(zd)
    if flip:
        ref = torch.flip(ref, [3])
    go = torch.randn(ref.shape, generator=g)
    ref.backward(go.double())
    ld = 4 if dt == torch.float32 else 8
    y = nhwc(z, ld, dt)
    y[..., 1:] = 7.0
    y.requires_grad_(True)
    out = HG.softplus_head(y, flip)
    out.backward(go.to(dev))
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, 1, H, W)
    assert rel(out, ref.detach()) < 1e-6
    assert rel(nchw(y.grad, 1), zd.grad) < (1e-6 if dt == torch.float32 else 1e-2)
    assert float(y.grad[..., 1:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------
def build(ci, dtype="fp32"):
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.modeling import build_model
    enc, norm, ls = CASES[ci][:3]
    cfg = get_cfg()
    cfg.MODEL.META_ARCHITECTURE, cfg.MODEL.DEVICE, cfg.MODEL.COMPUTE_DTYPE = "SupDepthModel", dev, dtype
    cfg.MODEL.DEPTH_NET.NAME, cfg.MODEL.DEPTH_NET.ENCODER_NAME = "GoogleResNet", enc
    cfg.MODEL.DEPTH_NET.NORM, cfg.MODEL.DEPTH_NET.LEARN_SCALE = norm, ls
    cfg.SOLVER.DEPTH_LR = 2e-4
    model = build_model(cfg)
    dn = model.depth_net
    sd = google_init.google_state_dict([(n, tuple(v.shape)) for n, v in dn.state_dict().items()], seed=ci)
    dn.load_state_dict(sd, strict=True)
    return model.train(), cfg


def dbatch(ci):
    B, H, W = CASES[ci][3:]
    return {k: v.to(dev) for k, v in google_init.google_batch(B, H, W, seed=ci).items()}


def inject(model, ci, step):
    pre = f"case{ci}_z_{step}_"
    draws = {k[len(pre):]: torch.from_numpy(GOLD[k].astype(np.float32)) for k in GOLD.files if k.startswith(pre)}
    if CASES[ci][1] == "randLN":
        assert len(draws) == len(model.depth_net._rand_norms)
    model.depth_net.inject_z({n: (z[0], z[1]) for n, z in draws.items()})


@pytest.mark.parametrize("ci", [0, 1, 2])
def test_model_matches_reference_fp32(ci):
    p = f"case{ci}_"
    model, _ = build(ci)
    inject(model, ci, 0)
    out = model(dbatch(ci))
    out["silog_loss"].backward()
    torch.cuda.synchronize()
    assert rel(out["depth_pred"][0], torch.from_numpy(GOLD[p + "depth"])) < 1e-4
    assert abs(out["silog_loss"].item() - float(GOLD[p + "loss"])) < 1e-4 * abs(float(GOLD[p + "loss"]))
    params = dict(model.depth_net.named_parameters())
    for n, v in zip(GOLD[p + "grad_names"], GOLD[p + "grad_norms"]):
        gn = params[n].grad.double().norm().item()
        assert abs(gn - v) <= 3e-3 * v + 1e-7, (n, gn, v)
    if ci == 0:
        model.eval()
        with torch.no_grad():
            ev = model(dbatch(0))["depth_pred"]
            b = dbatch(0)
            b["flip"] = True
            fl = model(b)["depth_pred"]
        assert rel(ev, torch.from_numpy(GOLD[p + "eval"])) < 1e-4
        assert rel(fl, torch.from_numpy(GOLD[p + "flip"])) < 1e-4


def test_adamw_steps_track_the_reference():
    from simpledepthestimation_amd.engine.trainer import supervised_trainer
    model, cfg = build(0)
    tr = supervised_trainer(model, cfg)
    losses = []
    for k in range(3):
        inject(model, 0, k + 1)
        losses.append(float(tr.step(dbatch(0))["silog_loss"].detach()))
    torch.cuda.synchronize()
    np.testing.assert_allclose(losses, GOLD["case0_adam_loss"], rtol=2e-4)
    params = dict(model.depth_net.named_parameters())
    for n, v in zip(GOLD["adam_track"], GOLD["case0_adam_norms"][-1]):
        assert abs(params[n].detach().double().norm().item() - v) <= 1e-4 * v, n


def test_learn_scale_parameter_stays_one():
    from simpledepthestimation_amd.engine.trainer import supervised_trainer
    model, cfg = build(2)
    tr = supervised_trainer(model, cfg)
    for _ in range(2):
        out = tr.step(dbatch(2))
    torch.cuda.synchronize()
    assert math.isfinite(float(out["silog_loss"]))
    assert float(model.depth_net.decoder.scale.detach()) == 1.0


def test_graph_replay_equals_eager_step_at_zero_noise():
    from simpledepthestimation_amd.engine.trainer import supervised_trainer
    res = []
    for graph in (False, True):
        model, cfg = build(0)
        model.depth_net.set_stddev(0.0)
        tr = supervised_trainer(model, cfg, use_graph=graph)
        for _ in range(3):
            out = tr.step(dbatch(0))
        torch.cuda.synchronize()
        res.append((float(out["silog_loss"].detach()), tr.pflat.clone()))
    assert abs(res[0][0] - res[1][0]) <= 1e-5 * abs(res[0][0])
    assert float((res[1][1] - res[0][1]).abs().max()) <= 3 * 2 * cfg.SOLVER.DEPTH_LR


def test_graph_follows_set_stddev_and_redraws():
    """A forward captured at s = 0.5 replays at s = 0 after set_stddev(0) (the kernels read s from device memory) and equals the eager s = 0
    forward; two replays at s = 0.5 draw different noise."""
    model, _ = build(0)
    dn = model.depth_net
    b = dbatch(0)
    dn.set_stddev(0.5)
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                model(dict(b))
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static = model(dict(b))["depth_pred"][0]
        dn.set_stddev(0.0)
        graph.replay()
        replay0 = static.clone()
        eager0 = model(dict(b))["depth_pred"][0]
        dn.set_stddev(0.5)
        graph.replay()
        r1 = static.clone()
        graph.replay()
        r2 = static.clone()
    torch.cuda.synchronize()
    assert rel(replay0, eager0) < 1e-6
    assert float((r1 - r2).abs().max()) > 1e-3 * float(r1.abs().max())
    assert float((r1 - eager0).abs().max()) > 1e-3 * float(r1.abs().max())


def test_bf16_is_finite_and_close_to_fp32():
    outs = []
    for dtype in ("fp32", "bf16"):
        model, _ = build(0, dtype)
        inject(model, 0, 0)
        out = model(dbatch(0))
        out["silog_loss"].backward()
        outs.append((out["silog_loss"].item(), out["depth_pred"][0].detach(), model.depth_net.decoder.out_conv.weight.grad.clone()))
    torch.cuda.synchronize()
    (l32, d32, g32), (l16, d16, g16) = outs
    assert math.isfinite(l16) and torch.isfinite(d16).all() and torch.isfinite(g16).all()
    assert abs(l16 - l32) < 3e-2 * abs(l32)


def test_full_size_bf16_step_and_eval():
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.modeling import build_model
    cfg = get_cfg()
    cfg.MODEL.META_ARCHITECTURE, cfg.MODEL.DEVICE, cfg.MODEL.COMPUTE_DTYPE = "SupDepthModel", dev, "bf16"
    cfg.MODEL.DEPTH_NET.NAME, cfg.MODEL.DEPTH_NET.ENCODER_NAME = "GoogleResNet", "18"
    model = build_model(cfg).train()
    b = {k: v.to(dev) for k, v in google_init.google_batch(16, 128, 416, seed=3).items()}
    out = model(dict(b))
    out["silog_loss"].backward()
    torch.cuda.synchronize()
    assert math.isfinite(out["silog_loss"].item())
    assert torch.isfinite(model.depth_net.encoder.encoder.conv1.weight.grad).all()
    assert torch.isfinite(model.depth_net.encoder.encoder.layer4[1].bn2.weight.grad).all()
    model.depth_net.set_stddev(0.0)
    model.eval()
    with torch.no_grad():
        ev = model(dict(b))["depth_pred"]
    assert tuple(ev.shape) == (16, 1, 128, 416) and torch.isfinite(ev).all()


def test_do_train_ramps_the_noise(tmp_path):
    from simpledepthestimation_amd.engine.loops import do_train
    model, cfg = build(0)
    cfg.OUTPUT_DIR = str(tmp_path)
    cfg.LOG_PERIOD, cfg.SOLVER.MAX_EPOCHS, cfg.TEST.EVAL_PERIOD = 1, 1, 0
    cfg.MODEL.DEPTH_NET.RAMPUP_ITERS, cfg.MODEL.DEPTH_NET.NOISE_STDDEV = 4, 0.5
    loader = [google_init.google_batch(2, 64, 192, seed=20 + i) for i in range(2)]
    rec = do_train(cfg, model, loader, None)
    assert [r["iteration"] for r in rec] == [1, 2]
    assert [r["noise_stddev"] for r in rec] == [0.5 * (1 / 4) ** 2, 0.5 * (2 / 4) ** 2]
    assert all(math.isfinite(r["total_loss"]) for r in rec)
    assert model.depth_net.encoder.encoder.bn1.stddev == 0.125

"""GPU: the BTS decoder's operators and BtsModel against float64 torch restatements and the reference's golden run (tests/golden/bts.npz)."""
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bts_init
import conv_bounds as CB

pytestmark = pytest.mark.gpu
dev = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "bts.npz"))
CASES = [(512, 2, 64, 128), (128, 2, 96, 320)]
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
REF_DT = dict(DT, fp16=torch.float16)       # the references also in fp16, for the CPU self-test of their bounds (tests/test_conv_bounds.py)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def nhwc(x, c_pad, dt):
    B, C, H, W = x.shape
    out = torch.zeros(B, H, W, c_pad, dtype=dt)
    out[..., :C] = x.permute(0, 2, 3, 1).to(dt)
    return out.to(dev).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------------
BOUNDED_DILATED = {(2, 5, 7, 37, 21), (2, 13, 19, 40, 24)}     # shapes whose fp64 adjoints take a fraction of a second on the CPU


@functools.lru_cache(maxsize=None)
def dilated_reference(dtype, d, shape):
    """Operands (rounded to the storage type), the fp64 result and, for the small shapes, the per-element bounds of tests/conv_bounds.py: computed
    once per case, never modified."""
    B, H, W, Cin, Cout = shape
    dt = REF_DT[dtype]
    g = torch.Generator().manual_seed(d * 7 + Cin)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    w[:, :, 0, 2] *= 3.0          # asymmetric taps: a flipped or transposed operand shows
    gy = torch.randn(B, Cout, H, W, generator=g)
    if dt != torch.float32:       # compare against the rounded operands
        x, w, gy = x.to(dt).float(), w.to(dt).float(), gy.to(dt).float()
    xd = x.double().requires_grad_(True)
    wd = w.double().requires_grad_(True)
    yr = F.conv2d(xd, wd, padding=d, dilation=d)
    yr.backward(gy.double())
    case = bw = None
    if shape in BOUNDED_DILATED:
        case = CB.Conv3x3Case(x, w, dt, dilation=d)
        bw = case.backward(gy)
    return dict(x=x, w=w, gy=gy, y=yr.detach(), dx=xd.grad, dw=wd.grad, case=case, bw=bw)


def dilated_conv_case(dtype, d, shape):
    from simpledepthestimation_amd.hip import bts as HB
    from simpledepthestimation_amd.hip import nn as HN
    from simpledepthestimation_amd.layers.hip_modules import HipConv2d
    B, H, W, Cin, Cout = shape
    dt = REF_DT[dtype]
    # (the large shape's reference is used once: not kept)
    ref = dilated_reference(dtype, d, shape) if shape in BOUNDED_DILATED else dilated_reference.__wrapped__(dtype, d, shape)
    x, w, gy = ref["x"], ref["w"], ref["gy"]
    conv = HipConv2d(Cin, Cout, 3, 1, 1, bias=False).to(dev)
    with torch.no_grad():
        conv.weight.copy_(w)
    V = HN.vec_of(dt)
    xh = nhwc(x, HN.pad_to(Cin, V), dt).requires_grad_(True)
    y = HB.dilated_conv3x3(conv, xh, d)
    gyh = nhwc(gy, y.shape[3], dt)
    y.backward(gyh)
    torch.cuda.synchronize()
    tol = {"fp32": 2e-5, "bf16": 2e-2, "fp16": 2e-2 * 2.0 ** -3}[dtype]      # fp16: the bf16 value scaled by the ratio of the unit roundoffs
    yo = y[..., :Cout].permute(0, 3, 1, 2)
    assert rel(yo, ref["y"]) < tol
    assert rel(xh.grad[..., :Cin].permute(0, 3, 1, 2), ref["dx"]) < tol
    assert float(xh.grad[..., Cin:].abs().max() if xh.grad.shape[3] > Cin else 0) == 0.0
    assert rel(conv.weight.grad, ref["dw"]) < tol
    if ref["case"] is not None:       # every element against its a-priori limit (split and merge move data: the dilated convolution is the reference)
        CB.assert_within(yo.detach().float().cpu(), ref["case"].y, dt, f"{dtype} dilated y", l2_tol=float("inf"))
        CB.assert_within(xh.grad[..., :Cin].permute(0, 3, 1, 2).float().cpu(), ref["bw"]["dX"], dt, f"{dtype} dilated dX", l2_tol=float("inf"))
        CB.assert_within(conv.weight.grad.cpu(), ref["bw"]["dW"], torch.float32, f"{dtype} dilated dW", l2_tol=float("inf"))


# (one list with explicit ids -- "<shape>-<d>-<dtype>", what the stacked decorators produced -- so that fp16 can join for small_odd alone)
DILATED = [pytest.param(shape, d, dtype, id=f"{sid}-{d}-{dtype}") for dtype in ("fp32", "bf16", "fp16") for d in (1, 3, 6, 12, 18, 24)
           for sid, shape in (("44x88_256to128", (2, 44, 88, 256, 128)), ("small_odd", (2, 5, 7, 37, 21))) if dtype != "fp16" or sid == "small_odd"]


@pytest.mark.parametrize("shape,d,dtype", DILATED)
def test_dilated_conv_fwd_dgrad_wgrad(dtype, d, shape):
    """small_odd: also element by element (tests/conv_bounds.py), and in fp16.  The 44 x 88 shape keeps the whole-tensor assertion alone: its fp64
    adjoints take too long on the CPU."""
    dilated_conv_case(dtype, d, shape)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("d", [3, 6])
def test_dilated_conv_unequal_subgrids(dtype, d):
    """d smaller than H and W and dividing neither: sub-grids of unequal size, the last row and column of some of them missing."""
    dilated_conv_case(dtype, d, (2, 13, 19, 40, 24))


# ---------------------------------------------------------------------------------------------------------------------------------------
def lpg_torch(a, r, max_depth, ds):
    """float64 restatement of reduction_1x1's plane head + normalize + local_planar_guidance + / max_depth (+ nearest 1/ds copy)."""
    theta = torch.sigmoid(a[:, 0]) * math.pi / 3
    phi = torch.sigmoid(a[:, 1]) * math.pi * 2
    dist = torch.sigmoid(a[:, 2]) * max_depth
    n = torch.stack([torch.sin(theta) * torch.cos(phi), torch.sin(theta) * torch.sin(phi), torch.cos(theta)], 1)
    n = F.normalize(n, 2, 1)
    pe = torch.cat([n, dist.unsqueeze(1)], 1)
    pe = torch.repeat_interleave(torch.repeat_interleave(pe, r, 2), r, 3)
    B, _, H, W = pe.shape
    u = ((torch.arange(W, dtype=a.dtype) % r) - (r - 1) * 0.5) / r
    v = ((torch.arange(H, dtype=a.dtype) % r) - (r - 1) * 0.5) / r
    depth = pe[:, 3] / (pe[:, 0] * u.view(1, 1, W) + pe[:, 1] * v.view(1, H, 1) + pe[:, 2])
    full = depth.unsqueeze(1) / max_depth
    return full, (F.interpolate(full, scale_factor=1.0 / ds, mode="nearest") if ds else None)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("r,ds", [(8, 4), (4, 2), (2, 0)])
def test_lpg_head_fwd_bwd(dtype, r, ds):
    from simpledepthestimation_amd.hip import bts as HB
    dt = REF_DT[dtype]
    B, h, w, md = 2, 6, 10, 80.0
    g = torch.Generator().manual_seed(r)
    a = (torch.randn(B, 3, h, w, generator=g) * 1.5).to(dt).float()
    ad = a.double().requires_grad_(True)
    full_r, down_r = lpg_torch(ad, r, md, ds)
    gf = torch.randn(full_r.shape, generator=g)
    loss = (full_r * gf.double()).sum()
    if ds:
        gd = torch.randn(down_r.shape, generator=g)
        loss = loss + (down_r * gd.double()).sum()
    loss.backward()
    y = nhwc(a, 8, dt).requires_grad_(True)
    out = HB.lpg(y, r, md, ds)
    full, down = (out if ds else (out, None))
    hl = (full * gf.to(dev)).sum() + ((down * gd.to(dev)).sum() if ds else 0)
    hl.backward()
    torch.cuda.synchronize()
    # fp32 against float64: the plane denominator (no clamp, as in the reference) amplifies the rounding of the normal near its zero
    assert rel(full, full_r.detach()) < 1e-4
    if ds:
        assert rel(down, down_r.detach()) < 1e-4
    # bf16: the stored logit gradient; fp16: the bf16 value scaled by the ratio of the unit roundoffs, not below the fp32 one
    assert rel(y.grad[..., :3].permute(0, 3, 1, 2), ad.grad) < {"fp32": 1e-3, "bf16": 1e-2, "fp16": max(1e-3, 1e-2 * 2.0 ** -3)}[dtype]
    assert float(y.grad[..., 3:].abs().max()) == 0.0


@pytest.mark.parametrize("flip", [False, True])
def test_sigmoid_heads_with_per_sample_focal(flip):
    from simpledepthestimation_amd.hip import bts as HB
    B, H, W = 3, 8, 12
    g = torch.Generator().manual_seed(5)
    z = torch.randn(B, 1, H, W, generator=g)
    focal = torch.tensor([700.0, 720.5, 760.25])
    zd = z.double().requires_grad_(True)
    ref = torch.sigmoid(zd) * 80.0 * focal.double().view(-1, 1, 1, 1) / 715.0873
    if flip:
        ref = torch.flip(ref, [3])
    go = torch.randn(ref.shape, generator=g)
    ref.backward(go.double())
    y = nhwc(z, 4, torch.float32).requires_grad_(True)
    out = HB.sigmoid_head(y, 80.0, focal.to(dev), 715.0873, flip)
    out.backward(go.to(dev))
    torch.cuda.synchronize()
    assert rel(out, ref.detach()) < 1e-6
    assert rel(y.grad[..., :1].permute(0, 3, 1, 2), zd.grad) < 1e-5
    r1 = HB.sigmoid_head(y)
    assert rel(r1, torch.sigmoid(z)) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------------------------
def build(size, dtype="fp32"):
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.modeling import build_model
    cfg = get_cfg()
    cfg.MODEL.META_ARCHITECTURE, cfg.MODEL.DEVICE, cfg.MODEL.DATASET, cfg.MODEL.COMPUTE_DTYPE = "SupDepthModel", dev, "kitti", dtype
    cfg.MODEL.DEPTH_NET.NAME, cfg.MODEL.DEPTH_NET.ENCODER_NAME, cfg.MODEL.DEPTH_NET.BTS_SIZE = "BtsModel", "resnet50_bts", size
    cfg.SOLVER.DEPTH_LR = 2e-4
    model = build_model(cfg)
    dn = model.depth_net
    sd = bts_init.bts_state_dict([(n, tuple(v.shape)) for n, v in dn.state_dict().items()], seed=CASES.index(next(c for c in CASES if c[0] == size)))
    dn.load_state_dict(sd, strict=True)
    return model.train(), cfg, sd


def dbatch(ci):
    _, B, H, W = CASES[ci]
    return {k: v.to(dev) for k, v in bts_init.bts_batch(B, H, W, seed=ci).items()}


@pytest.mark.parametrize("ci", [0, 1])
def test_model_matches_reference_fp32(ci):
    p = f"case{ci}_"
    model, _, _ = build(CASES[ci][0])
    out = model(dbatch(ci))
    out["silog_loss"].backward()
    torch.cuda.synchronize()
    assert rel(out["depth_pred"][0], torch.from_numpy(GOLD[p + "final"])) < 1e-4
    for k in ("depth_8x8", "depth_4x4", "depth_2x2", "reduc_1x1"):
        if p + k in GOLD.files:
            assert rel(out[k], torch.from_numpy(GOLD[p + k])) < 1e-4, k
    assert abs(out["silog_loss"].item() - float(GOLD[p + "loss"])) < 1e-4 * abs(float(GOLD[p + "loss"]))
    params = dict(model.depth_net.named_parameters())
    for n, v in zip(GOLD[p + "grad_names"], GOLD[p + "grad_norms"]):
        gn = params[n].grad.double().norm().item()
        assert abs(gn - v) <= 3e-3 * v + 1e-7, (n, gn, v)
    for n in GOLD[p + "no_grad"]:
        assert params[n].grad is None, n
    bufs = dict(model.depth_net.named_buffers())
    for r in GOLD["running_names"]:
        assert rel(bufs[r + ".running_mean"], torch.from_numpy(GOLD[p + "rm_" + r])) < 1e-4, r
        assert rel(bufs[r + ".running_var"], torch.from_numpy(GOLD[p + "rv_" + r])) < 1e-4, r
    if ci == 0:
        model.eval()
        with torch.no_grad():
            ev = model(dbatch(0))["depth_pred"]
            b = dbatch(0)
            b["flip"] = True
            fl = model(b)["depth_pred"]
        assert rel(ev, torch.from_numpy(GOLD[p + "eval_final"])) < 1e-4
        assert rel(fl, torch.from_numpy(GOLD[p + "flip_final"])) < 1e-4


def test_missing_intrinsics_raises():
    model, _, _ = build(128)
    b = dbatch(1)
    del b["intrinsics"]
    with pytest.raises(KeyError, match="intrinsics"):
        model(b)


@pytest.mark.parametrize("ci", [0, 1])
def test_adamw_steps_track_the_reference(ci):
    from simpledepthestimation_amd.engine.trainer import supervised_trainer
    p = f"case{ci}_"
    model, cfg, sd = build(CASES[ci][0])
    tr = supervised_trainer(model, cfg)
    frozen = {n: q.detach().clone() for n, q in model.depth_net.named_parameters() if not q.requires_grad or ".fc." in n}
    losses = []
    for _ in range(3):
        out = tr.step(dbatch(ci))
        losses.append(float(out["silog_loss"].detach()))
    torch.cuda.synchronize()
    np.testing.assert_allclose(losses, GOLD[p + "adam_loss"], rtol=2e-4)
    params = dict(model.depth_net.named_parameters())
    for n, v in zip(GOLD["adam_track"], GOLD[p + "adam_norms"][-1]):
        assert abs(params[n].detach().double().norm().item() - v) <= 1e-4 * v, n
    for n, t in frozen.items():
        assert torch.equal(params[n].detach(), t), n


def test_graph_replay_equals_eager_step():
    from simpledepthestimation_amd.engine.trainer import supervised_trainer
    res = []
    for graph in (False, True):
        model, cfg, _ = build(128)
        tr = supervised_trainer(model, cfg, use_graph=graph)
        for _ in range(3):
            out = tr.step(dbatch(1))
        torch.cuda.synchronize()
        res.append((float(out["silog_loss"].detach()), tr.pflat.clone()))
    # not bit-identical: the two runs' gradients differ in the last fp32 bits, and AdamW turns that into up to one step (lr) on parameters whose
    # gradient is near zero -- hence an absolute bound of two steps per step on the parameters, and a tight one on the loss
    assert abs(res[0][0] - res[1][0]) <= 1e-5 * abs(res[0][0])
    assert float((res[1][1] - res[0][1]).abs().max()) <= 3 * 2 * cfg.SOLVER.DEPTH_LR


def test_bf16_is_finite_and_close_to_fp32():
    outs = []
    for dtype in ("fp32", "bf16"):
        model, _, _ = build(128, dtype)
        out = model(dbatch(1))
        out["silog_loss"].backward()
        dec = model.depth_net.decoder
        outs.append((out["silog_loss"].item(), out["depth_pred"][0].detach(), dec.get_depth[0].weight.grad.clone(), dec.upconv5.conv.weight.grad.clone()))
    torch.cuda.synchronize()
    (l32, d32, g32, u32), (l16, d16, g16, u16) = outs
    assert math.isfinite(l16) and torch.isfinite(d16).all() and torch.isfinite(g16).all() and torch.isfinite(u16).all()
    assert abs(l16 - l32) < 3e-2 * abs(l32)
    assert float((d16 - d32).norm() / d32.norm()) < 3e-2      # bf16 activations through ~70 layers: relative L2 of the depth map
    assert float((g16.flatten() @ g32.flatten()) / (g16.norm() * g32.norm())) > 0.9        # the head's weight gradient
    # the deepest decoder layer's gradient has come back through ~40 bf16 layers and four BatchNorms over 240-pixel maps: its direction is
    # noise-dominated at this size (cosine ~0.6 measured), its magnitude is not
    assert abs(float(u16.norm() / u32.norm()) - 1) < 0.1


def test_full_size_bf16_step_and_eval():
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.modeling import build_model
    cfg = get_cfg()
    cfg.MODEL.META_ARCHITECTURE, cfg.MODEL.DEVICE, cfg.MODEL.DATASET, cfg.MODEL.COMPUTE_DTYPE = "SupDepthModel", dev, "kitti", "bf16"
    cfg.MODEL.DEPTH_NET.NAME, cfg.MODEL.DEPTH_NET.ENCODER_NAME = "BtsModel", "resnet50_bts"
    model = build_model(cfg).train()
    b = {k: v.to(dev) for k, v in bts_init.bts_batch(8, 352, 704, seed=3).items()}
    out = model(dict(b))
    out["silog_loss"].backward()
    torch.cuda.synchronize()
    assert math.isfinite(out["silog_loss"].item())
    assert torch.isfinite(model.depth_net.decoder.daspp_24.atrous_conv.aconv_sequence[4].weight.grad).all()
    model.eval()
    with torch.no_grad():
        ev = model(dict(b))["depth_pred"]
    assert tuple(ev.shape) == (8, 1, 352, 704) and torch.isfinite(ev).all()

"""GPU: the GoogleMotionNet / GooglePoseNet operators against float64 torch restatements, and both networks against the reference's golden run
(tests/golden/motion.npz, written by scripts/gen_golden_motion.py).

Model-level bounds: the project's fp32 parity precedent (outputs 1e-4, gradients 3e-3, relative) or 8 x the reference's own fp32-vs-fp64
difference `d` of that quantity (stored in the golden file), whichever is larger.  The factor 8 covers a different summation order over
K <= 9 * 1027 and eight chained refiners.  Tensors are compared as max |a - b| / max |b|, norms and the loss as |a - b| / |b|.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import motion_init

pytestmark = pytest.mark.gpu
dev = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "motion.npz"))
CASES = motion_init.CASES
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
TOL = {"fp32": 2e-5, "bf16": 2e-2}          # the elementwise-kernel tolerances of tests/test_gpu_google_resnet.py
OUT_TOL, GRAD_TOL, D_FACTOR = 1e-4, 3e-3, 8.0


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


def pad_to(c, dt):
    v = 4 if dt == torch.float32 else 8
    return (c + v - 1) // v * v


# ---------------------------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------------------------
# (h, w) -> (H, W), real skip channels: 1-pixel sources, odd ratios, the same size, and skip widths that are not a multiple of the vector width
RESIZE_CASES = [((1, 1), (1, 4), 16), ((1, 4), (2, 7), 16), ((4, 13), (8, 26), 32), ((3, 5), (3, 5), 13), ((2, 7), (3, 13), 6), ((1, 1), (1, 1), 8),
                ((5, 3), (20, 11), 8)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", RESIZE_CASES)
def test_resize_cat(case, dtype):
    from simpledepthestimation_amd.hip import motion as HM
    (h, w), (H, W), Cr = case
    dt = DT[dtype]
    g = torch.Generator().manual_seed(h * 100 + W)
    B = 2
    Cs, Cx = pad_to(Cr, dt), pad_to(Cr + 3, dt)
    field = torch.randn(B, 3, h, w, generator=g)
    skip = torch.randn(B, Cr, H, W, generator=g).to(dt).float()
    wa, wb = (torch.randn(B, Cr + 3, H, W, generator=g).to(dt).float() for _ in range(2))
    wu = torch.randn(B, 3, H, W, generator=g)
    fh = nhwc(field, 4, torch.float32).requires_grad_(True)
    sh = nhwc(skip, Cs, dt).requires_grad_(True)
    xa, xb, up = HM.resize_cat(fh, sh, Cr)
    assert xa.shape == (B, H, W, Cx) and xa.dtype == dt and up.shape == (B, H, W, 4) and up.dtype == torch.float32
    (xa.float() * nhwc(wa, Cx, torch.float32)).sum().backward(retain_graph=True)
    ga = (fh.grad.clone(), sh.grad.clone())
    fh.grad = sh.grad = None
    ((xa.float() * nhwc(wa, Cx, torch.float32)).sum() + (xb.float() * nhwc(wb, Cx, torch.float32)).sum() + (up * nhwc(wu, 4, torch.float32)).sum()).backward()
    fd, sd = field.double().requires_grad_(True), skip.double().requires_grad_(True)
    r = F.interpolate(fd, size=(H, W), mode="bilinear", align_corners=True)
    X = torch.cat([r, sd], 1)
    (X * wa.double()).sum().backward(retain_graph=True)
    gda = (fd.grad.clone(), sd.grad.clone())
    fd.grad = sd.grad = None
    ((X * (wa + wb).double()).sum() + (r * wu.double()).sum()).backward()
    tol = TOL[dtype]
    print(f"resize_cat {case} {dtype}: X {rel(nchw(xa, Cr + 3), X):.2e} up {rel(nchw(up, 3), r):.2e} dfield {rel(nchw(fh.grad, 3), fd.grad):.2e} "
          f"dskip {rel(nchw(sh.grad, Cr), sd.grad):.2e}")
    assert rel(nchw(xa, Cr + 3), X) < tol and torch.equal(xa, xb)
    assert rel(nchw(up, 3), r) < TOL["fp32"]                                  # the trunk is fp32 in both modes
    if Cx > Cr + 3:
        assert float(xa[..., Cr + 3:].detach().float().abs().max()) == 0.0
    assert float(up[..., 3].abs().max()) == 0.0
    assert rel(nchw(ga[0], 3), gda[0]) < tol and rel(nchw(ga[1], Cr), gda[1]) < tol      # one consumer only
    assert rel(nchw(fh.grad, 3), fd.grad) < tol and rel(nchw(sh.grad, Cr), sd.grad) < tol
    assert float(fh.grad[..., 3].abs().max()) == 0.0
    if Cs > Cr:
        assert float(sh.grad[..., Cr:].float().abs().max()) == 0.0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 9, 13, 8), (2, 5, 7, 6), (2, 6, 5, 64), (2, 1, 4, 1024), (3, 2, 7, 512), (1, 33, 31, 16)])
def test_refiner_tail(shape, dtype):
    from simpledepthestimation_amd.hip import motion as HM
    B, H, W, mid = shape
    dt = DT[dtype]
    g = torch.Generator().manual_seed(mid + H)
    ld = pad_to(mid, dt)
    o1, o2 = (torch.randn(B, mid, H, W, generator=g).to(dt).float() for _ in range(2))
    w3 = torch.randn(3, 2 * mid, 1, 1, generator=g) / (2 * mid) ** 0.5
    up = torch.randn(B, 3, H, W, generator=g)
    wo = torch.randn(B, 3, H, W, generator=g)
    h1, h2 = nhwc(o1, ld, dt).requires_grad_(True), nhwc(o2, ld, dt).requires_grad_(True)
    hw, hu = w3.to(dev).requires_grad_(True), nhwc(up, 4, torch.float32).requires_grad_(True)
    out = HM.refiner_tail(h1, h2, hw, hu)
    (out * nhwc(wo, 4, torch.float32)).sum().backward()
    d1, d2, dw, du = o1.double().requires_grad_(True), o2.double().requires_grad_(True), w3.double().requires_grad_(True), up.double().requires_grad_(True)
    ref = du + F.conv2d(torch.cat([d1, d2], 1), dw)
    (ref * wo.double()).sum().backward()
    tol = TOL[dtype]
    print(f"tail {shape} {dtype}: out {rel(nchw(out, 3), ref):.2e} do1 {rel(nchw(h1.grad, mid), d1.grad):.2e} do2 {rel(nchw(h2.grad, mid), d2.grad):.2e} "
          f"dw3 {rel(hw.grad, dw.grad):.2e} dup {rel(nchw(hu.grad, 3), du.grad):.2e}")
    assert out.dtype == torch.float32 and rel(nchw(out, 3), ref) < TOL["fp32"]           # fp32 accumulation of exactly representable inputs
    assert rel(nchw(h1.grad, mid), d1.grad) < tol and rel(nchw(h2.grad, mid), d2.grad) < tol
    assert rel(hw.grad, dw.grad) < TOL["fp32"] and rel(nchw(hu.grad, 3), du.grad) < TOL["fp32"]
    if ld > mid:
        assert float(h1.grad[..., mid:].float().abs().max()) == 0.0 and float(h2.grad[..., mid:].float().abs().max()) == 0.0


def constrain(t, kind):
    """GooglePoseNet.py:L175-183."""
    if kind == "clip_ste":
        return (torch.clamp_min(t, 0.001) - t).detach() + t
    if kind == "clip":
        return torch.relu(t - 0.001) + 0.001
    return F.softplus(t) * 0.01 + 0.001


@pytest.mark.parametrize("mask", [True, False])
@pytest.mark.parametrize("kind,t0", [("clip", 0.013), ("clip", 0.0004), ("clip_ste", 0.0004), ("clip_ste", 0.008), ("softplus", 0.4)])
def test_motion_head(kind, t0, mask):
    from simpledepthestimation_amd.hip import motion as HM
    B, H, W = 2, 19, 37
    g = torch.Generator().manual_seed(5)
    m = torch.randn(B, 3, H, W, generator=g) * torch.rand(B, 1, H, W, generator=g) * 3
    wo = torch.randn(B, 3, H, W, generator=g)
    weight = torch.full((1,), 0.75, device=dev)
    th = torch.tensor(t0, device=dev, requires_grad=True)
    mh = nhwc(m, 4, torch.float32).requires_grad_(True)
    out = HM.motion_head(mh, constrain(th, kind), weight, mask)
    (out * wo.to(dev)).sum().backward()
    td, md = torch.tensor(t0, dtype=torch.float64, requires_grad=True), m.double().requires_grad_(True)
    r = md * constrain(td, kind)
    keep = torch.ones(B, 1, H, W, dtype=torch.bool)
    clear = keep.clone()
    if mask:
        n = torch.sqrt((r ** 2).sum(1, keepdim=True))
        keep = (n > n.mean()).detach()
        clear = ((n - n.mean()).abs() > 1e-5 * n.mean()).detach()          # fp32 rounding may flip a pixel that sits on the threshold
        assert clear.double().mean() > 0.99 and 0.2 < keep.double().mean() < 0.8
        r = r * keep
    ref = r * 0.75
    (ref * wo.double()).sum().backward()
    sel3 = clear.expand(B, 3, H, W)
    print(f"head {kind} t={t0} mask={mask}: out {rel(out.cpu()[sel3], ref[sel3]):.2e} dfield {rel(nchw(mh.grad, 3).cpu()[sel3], md.grad[sel3]):.2e} "
          f"dscale {abs(th.grad.item() - td.grad.item()) / max(abs(td.grad.item()), 1e-12):.2e}")
    assert out.shape == (B, 3, H, W) and out.dtype == torch.float32
    assert rel(out.cpu()[sel3], ref[sel3]) < TOL["fp32"]
    assert torch.equal((out.cpu() != 0)[sel3], keep.expand(B, 3, H, W)[sel3] & (ref != 0)[sel3])          # outside the band the mask agrees exactly
    assert rel(nchw(mh.grad, 3).cpu()[sel3], md.grad[sel3]) < TOL["fp32"]
    if clear.all():
        if kind == "clip" and t0 < 0.001:
            assert th.grad.item() == 0.0 and td.grad.item() == 0.0
        else:
            assert abs(th.grad.item() - td.grad.item()) <= TOL["fp32"] * abs(td.grad.item())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [8, 6])
def test_prep_input_gradient(C, dtype):
    from simpledepthestimation_amd.hip import motion as HM
    from simpledepthestimation_amd.hip import nn as HN
    dt = DT[dtype]
    B, H, W = 2, 7, 13
    g = torch.Generator().manual_seed(C)
    x = torch.rand(B, C, H, W, generator=g).to(dev).requires_grad_(True)
    wa, wb = (torch.randn(B, C, H, W, generator=g).to(dt).float() for _ in range(2))
    xa, xb = HM.prep_input_grad(x, dt)
    assert torch.equal(xa, HN.prep_input(x.detach(), None, None, dt)) and torch.equal(xa, xb)
    (xa.float() * nhwc(wa, 8, torch.float32)).sum().backward(retain_graph=True)
    assert rel(x.grad, wa) < TOL[dtype]
    x.grad = None
    ((xa.float() * nhwc(wa, 8, torch.float32)).sum() + (xb.float() * nhwc(wb, 8, torch.float32)).sum()).backward()
    assert rel(x.grad, wa + wb) < TOL[dtype] and x.grad.shape == x.shape and x.grad.dtype == torch.float32
    ya, yb = HM.prep_input_grad(x.detach(), dt)
    assert not ya.requires_grad and torch.equal(ya, xa)


# ---------------------------------------------------------------------------------------------------------------------------------------
# models against the reference
# ---------------------------------------------------------------------------------------------------------------------------------------
def build(ci, dtype="fp32"):
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.modeling.pose_net import build_pose_net
    net = build_pose_net(motion_init.case_cfg(get_cfg(), CASES[ci], dtype))
    names = [(str(n), tuple(int(s) for s in str(v).split(",") if s)) for n, v in zip(GOLD[f"case{ci}_names"], GOLD[f"case{ci}_shapes"])]
    net.load_state_dict(motion_init.scaled_init(motion_init.motion_state_dict(names, seed=ci), CASES[ci][2]), strict=True)
    return net.to(dev).train()


def data(ci, requires_grad=True):
    N, H, W = CASES[ci][6:]
    x = motion_init.motion_input(N, 8 if CASES[ci][5] else 6, H, W, seed=ci).to(dev).requires_grad_(requires_grad)
    wm, wp = motion_init.loss_weights(N, H, W, seed=ci)
    return x, wm.to(dev), wp.to(dev)


def run(net, x, wm, wp, motion_only=False):
    out = net({"pose_net_input": x})
    loss = 0.0 if motion_only else (out["pose_pred"] * wp).sum()
    if "motion_pred" in out:
        loss = loss + (out["motion_pred"] * wm).sum()
    loss.backward()
    return out, loss


def bound(precedent, key):
    d = float(GOLD[key])
    return max(precedent, D_FACTOR * d), d


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_model_matches_reference_fp32(ci):
    p = f"case{ci}_"
    name, gn, sc, mask, learn, use_depth, N, H, W = CASES[ci]
    net = build(ci)
    x, wm, wp = data(ci)
    out, loss = run(net, x, wm, wp)
    torch.cuda.synchronize()
    assert out["pose_pred"].shape == (N, 4, 4)
    b, d = bound(OUT_TOL, p + "d_pose")
    e = rel(out["pose_pred"], torch.from_numpy(GOLD[p + "pose"]))
    print(f"case {ci} pose_pred: {e:.2e} (d {d:.2e}, bound {b:.2e})")
    assert e < b
    masked = name == "GoogleMotionNet" and mask
    if name == "GoogleMotionNet":
        gold = torch.from_numpy(GOLD[p + "motion"])
        mp = out["motion_pred"].detach().cpu()
        assert mp.shape == (N, 3, H, W) and mp.dtype == torch.float32
        sel = torch.ones(N, 1, H, W, dtype=torch.bool)
        if masked:
            band = torch.from_numpy(np.unpackbits(GOLD[p + "band"])[:N * H * W].astype(bool)).view(N, 1, H, W)
            assert band.double().mean() <= 0.01
            sel = ~band
            zero = (gold == 0).all(1, keepdim=True)
            assert 0.2 < zero.double().mean() < 0.8
            assert torch.equal((mp == 0).all(1, keepdim=True)[sel], zero[sel])              # outside the band the mask agrees exactly
        sel = sel.expand(N, 3, H, W)
        b, d = bound(OUT_TOL, p + "d_motion")
        e = rel(mp[sel], gold[sel])
        print(f"case {ci} motion_pred: {e:.2e} (d {d:.2e}, bound {b:.2e})")
        assert e < b
    if masked:
        return                      # gradient parity uses the mask-off cases; the mask's backward is covered at kernel level
    b, d = bound(OUT_TOL, p + "d_loss")
    e = abs(loss.item() - float(GOLD[p + "loss"])) / abs(float(GOLD[p + "loss"]))
    print(f"case {ci} loss: {e:.2e} (d {d:.2e}, bound {b:.2e})")
    assert e < b
    params = dict(net.named_parameters())
    names = [str(n) for n in GOLD[p + "grad_names"]]
    assert set(names) == set(params)
    n64 = dict(zip(names, GOLD[p + "grad_norms64"]))
    worst = (0.0, None)
    for n, v, dn in zip(names, GOLD[p + "grad_norms"], GOLD[p + "d_grad_norms"]):
        assert params[n].grad is not None, n
        gnorm = params[n].grad.double().norm().item()
        wname = n[:-len("bias")] + "weight"
        if n.endswith(".bias") and n64[n] < 1e-6 * n64[wname]:
            # an exactly zero true gradient (a GroupNorm with one channel per group removes the bias): the reference returns rounding noise, so
            # only the size is compared, against the gradient tolerance applied to the layer's weight gradient
            print(f"case {ci} {n}: zero gradient, |g| {gnorm:.2e} against |g_weight| {n64[wname]:.2e}")
            assert gnorm <= GRAD_TOL * n64[wname], (n, gnorm)
            continue
        b = max(GRAD_TOL, D_FACTOR * float(dn))
        e = abs(gnorm - v) / v
        worst = max(worst, (e / b, n, e, float(dn)))
        assert e <= b, (n, gnorm, v, b)
    print(f"case {ci} gradient norms: worst {worst[1]} {worst[2]:.2e} (d {worst[3]:.2e})")
    for k in motion_init.FULL_GRADS:
        if p + "full_" + k in GOLD.files:
            b, d = bound(GRAD_TOL, p + "d_full_" + k)
            e = rel(params[k].grad, torch.from_numpy(GOLD[p + "full_" + k]))
            print(f"case {ci} full gradient {k}: {e:.2e} (d {d:.2e}, bound {b:.2e})")
            assert e < b, k
    b, d = bound(GRAD_TOL, p + "d_xgrad")
    e = rel(x.grad, torch.from_numpy(GOLD[p + "xgrad"]))
    print(f"case {ci} input gradient: {e:.2e} (d {d:.2e}, bound {b:.2e})")
    assert x.grad.shape == x.shape and e < b


@pytest.mark.parametrize("ci", [1, 2])
def test_model_bf16_against_reference(ci):
    """bf16 activations through up to 40 layers on a mask-off case: relative L2 of the outputs, the bound tests/test_gpu_bts.py uses."""
    p = f"case{ci}_"
    net = build(ci, "bf16")
    x, wm, wp = data(ci)
    out, _ = run(net, x, wm, wp)
    torch.cuda.synchronize()
    assert torch.isfinite(out["motion_pred"]).all() and torch.isfinite(out["pose_pred"]).all() and torch.isfinite(x.grad).all()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in net.parameters())
    for key, t in (("motion", out["motion_pred"]), ("pose", out["pose_pred"])):
        gold = torch.from_numpy(GOLD[p + key]).double()
        e = float((t.detach().double().cpu() - gold).norm() / gold.norm())
        print(f"case {ci} bf16 {key}_pred relative L2: {e:.2e}")
        assert e < 3e-2


@pytest.mark.parametrize("ci", [0, 4])
def test_no_host_synchronisation(ci):
    net = build(ci, "bf16")
    x, wm, wp = data(ci)
    run(net, x, wm, wp)                      # warm: library load, first allocations
    net.zero_grad(set_to_none=True)
    x.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        run(net, x, wm, wp)
        if ci == 0:
            net.motion_weight = 0.5
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


def test_motion_weight_is_a_device_scalar():
    net = build(2)
    x, wm, wp = data(2)
    out1, _ = run(net, x, wm, wp, motion_only=True)
    m1, g1 = out1["motion_pred"].detach().clone(), net.refiner0.conv3.weight.grad.clone()
    net.zero_grad(set_to_none=True)
    net.motion_weight = 0.25
    assert net.motion_weight == 0.25
    out2, _ = run(net, x, wm, wp, motion_only=True)
    assert torch.equal(out2["motion_pred"], 0.25 * m1) and float(m1.abs().max()) > 0
    assert torch.equal(net.refiner0.conv3.weight.grad, 0.25 * g1) and float(g1.abs().max()) > 0


@pytest.mark.parametrize("ci,dtype", [(0, "fp32"), (1, "bf16"), (4, "fp32")])
def test_repeated_runs_give_identical_bits(ci, dtype):
    net = build(ci, dtype)
    res = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        x, wm, wp = data(ci)
        out, _ = run(net, x, wm, wp)
        res.append(([out["pose_pred"].detach().clone()] + ([out["motion_pred"].detach().clone()] if "motion_pred" in out else []) + [x.grad.clone()],
                    {n: q.grad.clone() for n, q in net.named_parameters()}))
    assert all(torch.equal(a, b) for a, b in zip(res[0][0], res[1][0]))
    bad = [n for n in res[0][1] if not torch.equal(res[0][1][n], res[1][1][n])]
    assert not bad, bad


@pytest.mark.parametrize("ci", [2, 5])
def test_input_without_grad(ci):
    net = build(ci)
    x, wm, wp = data(ci)
    out1, _ = run(net, x, wm, wp)
    g1 = {n: q.grad.clone() for n, q in net.named_parameters()}
    net.zero_grad(set_to_none=True)
    x2, _, _ = data(ci, requires_grad=False)
    out2, _ = run(net, x2, wm, wp)
    assert x.grad is not None and x2.grad is None
    assert torch.equal(out1["pose_pred"], out2["pose_pred"])
    if "motion_pred" in out1:
        assert torch.equal(out1["motion_pred"], out2["motion_pred"])
    bad = [n for n, q in net.named_parameters() if not torch.equal(q.grad, g1[n])]
    assert not bad, bad


def test_full_size_bf16():
    """The reference setting: batch 16 in both frame orders (N = 32) at 128 x 416, bf16, GROUP_NORM off."""
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.modeling.pose_net import build_pose_net
    torch.manual_seed(0)
    net = build_pose_net(motion_init.case_cfg(get_cfg(), ("GoogleMotionNet", False, "clip_ste", True, True, True), "bf16")).to(dev).train()
    x = motion_init.motion_input(32, 8, 128, 416, seed=9).to(dev).requires_grad_(True)
    torch.cuda.reset_peak_memory_stats()
    out = net({"pose_net_input": x})
    (out["motion_pred"].sum() + out["pose_pred"].sum()).backward()
    torch.cuda.synchronize()
    print(f"full size: peak memory {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB")
    assert out["motion_pred"].shape == (32, 3, 128, 416) and out["pose_pred"].shape == (32, 4, 4)
    assert torch.isfinite(out["motion_pred"]).all() and torch.isfinite(out["pose_pred"]).all() and torch.isfinite(x.grad).all()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in net.parameters())

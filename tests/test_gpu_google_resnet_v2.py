"""GPU: GoogleResNetv2 against the reference's golden run (tests/golden/google_v2.npz), at the tolerances of tests/test_gpu_google_resnet.py, and
MotionLearningModel with the v2 depth net from the embedded Waymo config under motion_learning_trainer."""
import math
import os

import numpy as np
import pytest
import torch

import google_v2_init

pytestmark = pytest.mark.gpu
dev = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "google_v2.npz"))
CASES = [("randLN", False, 2, 64, 192), ("BN", False, 2, 64, 192), ("randLN", True, 2, 64, 192)]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def build(ci, dtype="fp32"):
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.modeling import build_model
    norm, ls = CASES[ci][:2]
    cfg = get_cfg()
    cfg.MODEL.META_ARCHITECTURE, cfg.MODEL.DEVICE, cfg.MODEL.COMPUTE_DTYPE = "SupDepthModel", dev, dtype
    cfg.MODEL.DEPTH_NET.NAME, cfg.MODEL.DEPTH_NET.ENCODER_NAME = "GoogleResNetv2", "18??"
    cfg.MODEL.DEPTH_NET.NORM, cfg.MODEL.DEPTH_NET.LEARN_SCALE = norm, ls
    cfg.SOLVER.DEPTH_LR = 2e-4
    model = build_model(cfg)
    dn = model.depth_net
    sd = google_v2_init.google_v2_state_dict([(n, tuple(v.shape)) for n, v in dn.state_dict().items()], seed=ci)
    dn.load_state_dict(sd, strict=True)
    return model.train(), cfg


def dbatch(ci):
    B, H, W = CASES[ci][2:]
    return {k: v.to(dev) for k, v in google_v2_init.google_batch(B, H, W, seed=ci).items()}


def inject(model, ci, step):
    pre = f"case{ci}_z_{step}_"
    draws = {k[len(pre):]: torch.from_numpy(GOLD[k].astype(np.float32)) for k in GOLD.files if k.startswith(pre)}
    if CASES[ci][0] == "randLN":
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
    e = rel(out["depth_pred"][0], torch.from_numpy(GOLD[p + "depth"]))
    print(f"  case {ci}: depth {e:.2e}, loss {out['silog_loss'].item():.7g} golden {float(GOLD[p + 'loss']):.7g}")
    assert e < 1e-4
    assert abs(out["silog_loss"].item() - float(GOLD[p + "loss"])) < 1e-4 * abs(float(GOLD[p + "loss"]))
    sd = model.depth_net.state_dict(keep_vars=True)          # the reference's names
    assert len(GOLD[p + "grad_names"]) == sum(1 for q in model.depth_net.parameters() if q.grad is not None)
    for n, v in zip(GOLD[p + "grad_names"], GOLD[p + "grad_norms"]):
        gn = sd[n].grad.double().norm().item()
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
    print("  losses", losses, "golden", GOLD["case0_adam_loss"])
    np.testing.assert_allclose(losses, GOLD["case0_adam_loss"], rtol=2e-4)
    sd = model.depth_net.state_dict()
    for n, v in zip(GOLD["adam_track"], GOLD["case0_adam_norms"][-1]):
        assert abs(sd[n].detach().double().norm().item() - v) <= 1e-4 * v, n
    assert model.depth_net.decoder.blocks[0].upconv._packed is not None, "the batched weight pack did not pick the transposed convolutions up"


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


def test_graph_follows_set_stddev():
    """A forward captured at s = 0.5 replays at s = 0 after set_stddev(0) (the kernels read s from device memory) and equals the eager s = 0 forward."""
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
    torch.cuda.synchronize()
    assert rel(replay0, eager0) < 1e-6
    assert float((r1 - eager0).abs().max()) > 1e-3 * float(r1.abs().max())


def test_bf16_is_finite_and_close_to_fp32():
    outs = []
    for dtype in ("fp32", "bf16"):
        model, _ = build(0, dtype)
        inject(model, 0, 0)
        out = model(dbatch(0))
        out["silog_loss"].backward()
        outs.append((out["silog_loss"].item(), out["depth_pred"][0].detach(), model.depth_net.decoder.blocks[4].upconv.weight.grad.clone()))
    torch.cuda.synchronize()
    (l32, d32, g32), (l16, d16, g16) = outs
    print(f"  loss fp32 {l32:.6g} bf16 {l16:.6g}")
    assert math.isfinite(l16) and torch.isfinite(d16).all() and torch.isfinite(g16).all()
    assert abs(l16 - l32) < 3e-2 * abs(l32)          # the bound of tests/test_gpu_google_resnet.py's same check


# ---------------------------------------------------------------------------------------------------------------------------------------
# MotionLearningModel with the v2 depth net, from the embedded Waymo config (2 x 64 x 192 with masks: the smallest size the randLN check allows)
# ---------------------------------------------------------------------------------------------------------------------------------------
B_ML, H_ML, W_ML = 2, 64, 192


def waymo_cfg():
    from simpledepthestimation_amd.config import get_project_cfg
    cfg = get_project_cfg("MotionLearningWaymo")
    cfg.MODEL.DEVICE, cfg.MODEL.COMPUTE_DTYPE = dev, "fp32"
    return cfg


def waymo_model(cfg, seed=0):
    from simpledepthestimation_amd.modeling import build_model
    torch.manual_seed(seed)
    return build_model(cfg).train()


def waymo_batch(seed=9):
    import motion_loss_init as MI
    v = MI.inputs(B_ML, H_ML, W_ML, seed=seed)
    mask = torch.zeros(B_ML, 1, H_ML, W_ML)
    mask[:, :, 20:44, 60:120] = 1.0
    ctx_mask = torch.zeros(B_ML, 1, H_ML, W_ML)
    ctx_mask[:, :, 22:46, 70:130] = 1.0
    return {"img": v["frame1"].to(dev), "ctx_img": [v["frame2"].to(dev)], "intrinsics": v["K"].to(dev), "mask": mask.to(dev), "ctx_mask": [ctx_mask.to(dev)]}


def total(out):
    terms = [v for k, v in out.items() if "loss" in k]
    return sum(terms[1:], terms[0])


def test_motion_learning_builds_and_steps_with_the_v2_depth_net():
    from simpledepthestimation_amd.engine.trainer import motion_learning_trainer
    from simpledepthestimation_amd.modeling.depth_net.GoogleResNetv2 import GoogleResNetv2
    cfg = waymo_cfg()
    model = waymo_model(cfg)
    assert isinstance(model.depth_net, GoogleResNetv2) and model.with_mask and model.num_scales == 1
    model.pose_net.motion_weight = 1.0          # past the burn-in: the motion field, and with it the masks, are in the loss
    tr = motion_learning_trainer(model, cfg)
    assert tr.clip_grad == 10.0
    out = tr.step(waymo_batch())
    torch.cuda.synchronize()
    t = float(total(out).detach())
    print(f"  total loss {t:.6g}, grad norm {float(tr.grad_norm()):.6g}")
    assert math.isfinite(t) and all(math.isfinite(float(v.detach())) for k, v in out.items() if "loss" in k)
    for n, p in model.depth_net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, n


def test_motion_learning_graph_replay_equals_eager_at_zero_noise():
    from simpledepthestimation_amd.engine.trainer import motion_learning_trainer
    res = []
    for graph in (False, True):
        cfg = waymo_cfg()
        model = waymo_model(cfg)
        model.depth_net.set_stddev(0.0)
        model.pose_net.motion_weight = 1.0
        tr = motion_learning_trainer(model, cfg, use_graph=graph)
        for k in range(3):
            out = tr.step(waymo_batch())
        torch.cuda.synchronize()
        res.append((float(total(out).detach()), tr.pflat.clone()))
    print(f"  eager {res[0][0]:.7g} graph {res[1][0]:.7g}")
    assert math.isfinite(res[0][0]) and abs(res[0][0] - res[1][0]) <= 1e-4 * abs(res[0][0])      # OUT_TOL of tests/test_gpu_motion_model.py's replay check
    lr = max(cfg.SOLVER.DEPTH_LR, cfg.SOLVER.POSE_LR)
    assert float((res[1][1] - res[0][1]).abs().max()) <= 3 * 2 * lr

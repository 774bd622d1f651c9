"""GPU: sde_motion_prep_fwd / _bwd and sde_mask_dilate against plain torch, MotionLearningModel from stub predictions against the reference's golden run
(tests/golden/motion_model.npz) on the fused and on the composed path, and the model end to end with its real networks, eagerly and as a captured graph.

Bounds: outputs / losses 1e-4, gradients 3e-3 (relative to the largest reference element), or 8 x the reference's own fp32-vs-fp64 difference where the
golden file carries one; at most 0.1 % of the occlusion pixels may flip and at most 0.1 % of a gradient map's elements may be off-bound."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import motion_model_ref as MM  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "motion_model.npz"))
DEV = "cuda:0"
OUT_TOL, GRAD_TOL = 1e-4, 3e-3


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ---------------------------------------------------------------------------------------------------------------------------------------
# pair_prep
# ---------------------------------------------------------------------------------------------------------------------------------------
# (N, H0, W0, h, w): identity with an odd width; uneven windows and two column blocks (70 > 64) at two ratios; four samples, two column blocks, identity
PREP_SHAPES = [(2, 7, 13, 7, 13), (2, 30, 70, 15, 35), (2, 30, 70, 7, 17), (4, 9, 70, 9, 70)]
# (motion, scale_normalize, mask)
PREP_MODES = [(True, False, False), (True, True, False), (False, False, False), (False, True, False), (True, False, True), (True, True, True)]
OUTS = ("depth_r", "depth_n", "t", "m_norm", "t_sw")


def prep_inputs(shape, motion, mask):
    N, H0, W0, h, w = shape
    g = torch.Generator().manual_seed(N * 1000 + H0 * 10 + h)
    v = {"depth": torch.rand(N, 1, H0, W0, generator=g) * 30 + 2, "t_pose": torch.randn(N, 3, generator=g) * 0.3,
         "motion": torch.randn(N, 3, H0, W0, generator=g) * 0.2 if motion else None,
         "mask": (torch.rand(N, 1, H0, W0, generator=g) > 0.4).float() if mask else None}
    cot = {k: torch.randn(N, 1 if k.startswith("depth") else 3, h, w, generator=g) for k in OUTS}      # one cotangent per differentiable output
    return v, cot


def run_prep(fn, v, cot, size, normalize, dtype, dev):
    c = lambda x: None if x is None else x.detach().clone().to(device=dev, dtype=dtype)
    depth, t_pose, motion, mask = c(v["depth"]).requires_grad_(True), c(v["t_pose"]).requires_grad_(True), c(v["motion"]), c(v["mask"])
    if motion is not None:
        motion.requires_grad_(True)
    o = fn(depth, motion, t_pose, mask, size, normalize)
    sum((o[k] * c(cot[k])).sum() for k in OUTS if o[k] is not None).backward()
    grads = {"depth": depth.grad, "t_pose": t_pose.grad}
    if motion is not None:
        grads["motion"] = motion.grad
    return o, grads


@pytest.mark.parametrize("mode", PREP_MODES, ids=lambda m: "motion%d-norm%d-mask%d" % tuple(int(x) for x in m))
@pytest.mark.parametrize("shape", PREP_SHAPES, ids=lambda s: "N%d-%dx%d-to-%dx%d" % s)
def test_pair_prep(shape, mode):
    from simpledepthestimation_amd.hip import motion_loss as HM
    motion, normalize, mask = mode
    N, H0, W0, h, w = shape
    v, cot = prep_inputs(shape, motion, mask)
    ref, gref = run_prep(MM.pair_prep, v, cot, (h, w), normalize, torch.float64, "cpu")
    o, g = run_prep(HM.pair_prep, v, cot, (h, w), normalize, torch.float32, DEV)
    o2, g2 = run_prep(HM.pair_prep, v, cot, (h, w), normalize, torch.float32, DEV)
    torch.cuda.synchronize()
    bad = []
    for k in OUTS + ("depth_n_sw", "overall_motion"):
        if ref[k] is None:
            assert o[k] is None, k
            continue
        e = rel(o[k], ref[k])
        print(f"  {k}: {e:.2e}")
        if not e <= OUT_TOL:
            bad.append(f"{k}: {e:.2e} > {OUT_TOL}")
        assert torch.equal(o[k], o2[k]), k + " does not repeat bit for bit"
    for k in gref:
        e = rel(g[k], gref[k])
        print(f"  d {k}: {e:.2e}")
        if not e <= GRAD_TOL:
            bad.append(f"d {k}: {e:.2e} > {GRAD_TOL}")
        assert torch.equal(g[k], g2[k]), "d " + k + " does not repeat bit for bit"
    assert set(g) == set(gref)
    assert not bad, "\n".join(bad)
    assert not o["depth_n_sw"].requires_grad and not o["overall_motion"].requires_grad
    if not normalize:
        assert o["depth_n"] is o["depth_r"]
    if (h, w) == (H0, W0) and not mask and not normalize:
        depth, t_pose = v["depth"].to(DEV), v["t_pose"].to(DEV)
        assert torch.equal(o["depth_r"], depth)
        t = t_pose[:, :, None, None] + v["motion"].to(DEV) if motion else t_pose[:, :, None, None].expand(-1, -1, h, w)
        assert torch.equal(o["t"], t)


def test_pair_prep_refuses_bad_arguments():
    from simpledepthestimation_amd.hip import lib as L
    from simpledepthestimation_amd.hip import motion_loss as HM
    d, t = torch.ones(3, 1, 4, 6, device=DEV), torch.zeros(3, 3, device=DEV)
    with pytest.raises(L.SdeHipError):
        HM.pair_prep(d, None, t, None, (4, 6))                                   # an odd batch cannot hold both directions
    with pytest.raises(L.SdeHipError):
        HM.pair_prep(d[:2], None, t[:2], torch.ones(2, 1, 4, 6, device=DEV), (4, 6))     # a mask without a motion field


# ---------------------------------------------------------------------------------------------------------------------------------------
# dilate_mask
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 8])
@pytest.mark.parametrize("size", [(7, 13), (20, 70)])
def test_dilate_mask(size, d):
    from simpledepthestimation_amd.hip import motion_loss as HM
    g = torch.Generator().manual_seed(d)
    m = (torch.rand(3, 1, *size, generator=g) > 0.93).float() * torch.randint(1, 4, (3, 1, *size), generator=g)     # sparse, values 1..3, and negatives below
    m[0, 0, 0, 0], m[1, 0, -1, -1], m[2, 0, 3, 5] = 2.0, 1.0, -1.0
    ref = F.max_pool2d((m > 0).float(), 2 * d + 1, stride=1, padding=d)
    out = HM.dilate_mask(m.to(DEV), d)
    assert torch.equal(out.cpu(), ref)
    assert torch.equal(HM.dilate_mask(m.to(DEV), 0).cpu(), (m > 0).float())


# ---------------------------------------------------------------------------------------------------------------------------------------
# the model from stub predictions against the golden file
# ---------------------------------------------------------------------------------------------------------------------------------------
def hip_fn(name, fused):
    from simpledepthestimation_amd.modeling.losses.losses import silog_loss
    from simpledepthestimation_amd.modeling.losses.ssim_loss import WeightedSSIM
    from simpledepthestimation_amd.modeling.meta_arch import MotionLearning as ML
    s = MM.settings(name)

    def fn(batch, depth_net, pose_net, record):
        model = MM.make_instance(ML.MotionLearningModel, s, depth_net, pose_net, WeightedSSIM(s["C1"], s["C2"]), silog_loss(s["variance_focus"]), torch.float32, DEV)
        real, flag = ML.rgbd_consistency_loss, ML.FUSED_PREP

        def recording(*a, **k):
            out = real(*a, **k)
            record.append(out["occlusion_mask"].detach())
            return out
        ML.rgbd_consistency_loss, ML.FUSED_PREP = recording, fused
        try:
            return model(batch)
        finally:
            ML.rgbd_consistency_loss, ML.FUSED_PREP = real, flag
    return fn


_RUNS = {}


def model_run(name, fused):
    if (name, fused) not in _RUNS:
        _RUNS[(name, fused)] = MM.run_case(name, hip_fn(name, fused), torch.float32, DEV)
        torch.cuda.synchronize()
    return _RUNS[(name, fused)]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("name", list(MM.CASES))
def test_model_from_stub_predictions(name, fused):
    bad = MM.compare_with_golden(model_run(name, fused), GOLD, name)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", list(MM.CASES))
def test_fused_and_composed_paths_agree(name):
    a, b = model_run(name, True), model_run(name, False)
    assert sorted(a["losses"]) == sorted(b["losses"])
    for k in a["losses"]:
        e = abs(float(a["losses"][k]) - float(b["losses"][k])) / abs(float(b["losses"][k]))
        print(f"  {name} {k}: {e:.2e}")
        assert e <= OUT_TOL, (k, e)
    for k in a["grads"]:
        e = rel(a["grads"][k], b["grads"][k])
        print(f"  {name} d {k}: {e:.2e}")
        assert e <= GRAD_TOL, (k, e)


# ---------------------------------------------------------------------------------------------------------------------------------------
# end to end with the real networks
# ---------------------------------------------------------------------------------------------------------------------------------------
B_E2E, H_E2E, W_E2E = 1, 32, 96          # the smallest size of tests/test_gpu_motion_net.py that GoogleResNet accepts (multiples of 32, two pixels in layer4)
E2E_KEYS = ("rgb_l1_loss", "ssim_loss", "rot_loss", "trans_loss", "motion_smooth_loss", "motion_sparsity_loss", "smooth_loss")


def real_model(seed=0):
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.modeling import build_model
    cfg = get_cfg()
    cfg.merge_from_other_cfg({"MODEL": {"META_ARCHITECTURE": "MotionLearningModel", "DEVICE": DEV, "COMPUTE_DTYPE": "fp32",
                                        "DEPTH_NET": {"NAME": "GoogleResNet", "NORM": "randLN"},
                                        "POSE_NET": {"NAME": "GoogleMotionNet", "USE_DEPTH": True, "SCALE_CONSTRAIN": "clip_ste"}},
                              "LOSS": {"NUM_SCALES": 1, "SSIM_WEIGHT": 3.0, "C1": "inf", "C2": 9e-6, "DEPTH_L1_WEIGHT": 0.0, "MOTION_SMOOTHNESS_WEIGHT": 1.0,
                                       "MOTION_SPARSITY_WEIGHT": 0.2, "ROT_CYCLE_WEIGHT": 1e-3, "TRANS_CYCLE_WEIGHT": 5e-2, "SCALE_NORMALIZE": False}})
    cfg.MODEL.DEPTH_NET.ENCODER_NAME = "18"        # set directly: merging would read the string as a number
    torch.manual_seed(seed)
    return build_model(cfg)


def real_batch():
    import motion_loss_init as MI
    v = MI.inputs(B_E2E, H_E2E, W_E2E, seed=9)
    return {"img": v["frame1"].to(DEV), "ctx_img": [v["frame2"].to(DEV)], "intrinsics": v["K"].to(DEV)}


def total(out):
    return sum(v for k, v in out.items() if "loss" in k)


def test_end_to_end_with_real_networks():
    model = real_model().train()
    torch.manual_seed(1)
    out = model(real_batch())
    for k in E2E_KEYS:
        assert k in out and out[k].dim() == 0 and torch.isfinite(out[k]), k
    assert not any(k in out for k in ("depth_l1_loss", "sup_loss", "var_loss"))
    assert len(out["overall_motion"]) == len(out["depth_proximity_weight"]) == 1
    assert out["overall_motion"][0][0].shape == (B_E2E, 3, H_E2E, W_E2E) and out["depth_proximity_weight"][0][1].shape == (B_E2E, 1, H_E2E, W_E2E)
    total(out).backward()
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        if ".encoder.fc." in n:          # torchvision's classifier head: part of the reference's state dict, read by neither forward pass
            assert p.grad is None, n
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    g_with = model.depth_net.decoder.parameters().__next__().grad.clone()
    # the same step with the depth channels of pose_net_input detached: the depth net's gradient must change
    from simpledepthestimation_amd.modeling.meta_arch import MotionLearning as ML
    model.zero_grad(set_to_none=True)
    real_cat = torch.cat

    class DetachDepth(torch.nn.Module):
        def __init__(self, net):
            super().__init__()
            self.net = net

        def forward(self, batch):
            x = batch["pose_net_input"]
            batch["pose_net_input"] = real_cat([x[:, :3], x[:, 3:4].detach(), x[:, 4:7], x[:, 7:8].detach()], 1)
            return self.net(batch)
    pose_net = model.pose_net
    model.pose_net = DetachDepth(pose_net)
    torch.manual_seed(1)
    out2 = model(real_batch())
    total(out2).backward()
    torch.cuda.synchronize()
    model.pose_net = pose_net
    g_without = model.depth_net.decoder.parameters().__next__().grad
    assert abs(float(total(out)) - float(total(out2))) <= 1e-6 * abs(float(total(out)))
    assert rel(g_with, g_without) > 1e-6, "USE_DEPTH sends no gradient into the depth net"
    assert ML.FUSED_PREP
    model.eval()
    with torch.no_grad():
        pred = model({"img": real_batch()["img"]})
    assert set(pred) == {"depth_pred"} and pred["depth_pred"].shape == (B_E2E, 1, H_E2E, W_E2E)


def test_forward_and_backward_capture_as_a_graph():
    import motion_loss_init as MI
    model = real_model().train()
    model.depth_net.set_stddev(0.0)          # RandLayerNorm's factor is exactly 1: an eager step and a replay on the same inputs compute the same losses
    static = real_batch()
    inputs = []
    for seed in (11, 12):
        v = MI.inputs(B_E2E, H_E2E, W_E2E, seed=seed)
        inputs.append((v["frame1"].to(DEV), v["frame2"].to(DEV), v["K"].to(DEV)))

    def load(i):
        static["img"].copy_(inputs[i][0]); static["ctx_img"][0].copy_(inputs[i][1]); static["intrinsics"].copy_(inputs[i][2])

    def step():
        model.zero_grad(set_to_none=False)
        out = model({"img": static["img"], "ctx_img": [static["ctx_img"][0]], "intrinsics": static["intrinsics"]})
        total(out).backward()
        return {k: out[k] for k in E2E_KEYS}

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    eager = []
    with torch.cuda.stream(side):
        step()                                       # warm-up: caches (ticket, weight vectors, workspaces) are built outside the capture
        for i in range(2):
            load(i)
            eager.append({k: float(v.detach()) for k, v in step().items()})
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    grad = next(model.depth_net.parameters()).grad
    for i in range(2):
        load(i)
        graph.replay()
        torch.cuda.synchronize()
        for k in E2E_KEYS:
            e = abs(float(captured[k]) - eager[i][k]) / abs(eager[i][k])
            print(f"  replay {i} {k}: {float(captured[k]):.6g} eager {eager[i][k]:.6g} ({e:.1e})")
            assert e <= OUT_TOL, (i, k, e)           # only the t_B2A scatter of motion consistency has no fixed order
        assert torch.isfinite(grad).all() and float(grad.abs().sum()) > 0

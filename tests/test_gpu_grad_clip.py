"""GPU: sde_grad_norm (global L2 norm of the flat gradient + torch's clip coefficient, on the device) and sde_adam_step's clip_state against torch's
nn.utils.clip_grad_norm_ + torch.optim.Adam; the pair inside a captured graph; MotionLearningModel trained by motion_learning_trainer against a twin
stepped by torch; engine.loops.do_train on MotionLearningModel (burn-in, noise ramp, per-epoch LR, logged scalars, resume).

Bounds
  total_norm: relative difference to the float64 sum at most 4 x the difference torch's own fp32 clip_grad_norm_ total shows to float64 on the same
      data (floor 1e-6); the coefficient follows from the kernel's own total by torch's formula (1 fp32 rounding per operation: 1e-6 relative).
  Adam with clip: p, m, v within 1e-6 absolute of the CPU run, the bound of tests/test_gpu_nn.py::test_adam_step.
  trajectory: grad_norm per step within 3e-3 relative (the gradient bound of the model tests), parameters after three steps within 3 * 2 * lr
      (every Adam step moves a parameter by at most ~lr; a gradient element near zero may take the other sign in the twin), as
      tests/test_gpu_google_resnet.py::test_graph_replay_equals_eager_step_at_zero_noise."""
import functools
import math
import os
import sys

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def NN():
    from simpledepthestimation_amd.hip import nn
    return nn


# ---------------------------------------------------------------------------------------------------------------------------------------
# the norm kernel
# ---------------------------------------------------------------------------------------------------------------------------------------
# one element; one 0-dim parameter's slot; a ragged tail inside one workgroup's worth; more than one grid-stride round at the workgroup cap + a tail
NORM_SIZES = [1, 4, 1777, 4 * 256 * 1024 + 23]


@functools.lru_cache(maxsize=None)
def norm_case(n):
    """(gradient fp32 on the CPU, ||g|| in float64, torch's fp32 clip_grad_norm_ total of it), computed once per size."""
    g = torch.randn(n, generator=torch.Generator().manual_seed(n % 1000 + 7))
    ref64 = float(g.double().square().sum().sqrt())
    p = torch.zeros(n, requires_grad=True)
    p.grad = g.clone()
    torch32 = float(nn.utils.clip_grad_norm_([p], float("inf")))
    return g, ref64, torch32


@pytest.mark.parametrize("above", [False, True], ids=["clipped", "coef1"])
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("n", NORM_SIZES)
def test_grad_norm_against_float64(NN, n, grad_scale, above):
    g, ref64, torch32 = norm_case(n)
    ref, own = ref64 * grad_scale, abs(torch32 - ref64) / ref64            # (the scale is a power of two: torch's relative error does not change)
    bound = max(4 * own, 1e-6)
    max_norm = ref * (2.0 if above else 0.5)
    gd = g.to(DEV)
    before = gd.clone()
    state, state2 = torch.full((2,), -1.0, device=DEV), torch.full((2,), -1.0, device=DEV)
    out = NN.grad_norm(gd, state, max_norm, grad_scale)
    assert out is state
    NN.grad_norm(gd, state2, max_norm, grad_scale, work=torch.full((NN.GRAD_NORM_WORK,), float("nan"), device=DEV))      # the workspace needs no initial value
    torch.cuda.synchronize()
    total, coef = (float(x) for x in state)
    err = abs(total - ref) / ref
    print(f"  n={n} scale={grad_scale} max_norm={max_norm:.6g}: total {total:.9g} float64 {ref:.9g} rel {err:.2e} (torch fp32 {own:.2e}, bound {bound:.2e}) coef {coef:.9g}")
    assert err <= bound, (err, bound)
    if above:
        assert coef == 1.0
    else:
        want = torch.tensor(max_norm, dtype=torch.float32) / (state[0].cpu() + torch.tensor(1e-6, dtype=torch.float32))
        assert coef < 1.0 and abs(coef - float(want)) <= 1e-6 * float(want), (coef, float(want))
    assert torch.equal(state, state2), "a second run gives other bits"
    assert torch.equal(gd, before), "the gradient was rescaled in memory"


def test_grad_norm_refuses_bad_arguments(NN):
    from simpledepthestimation_amd.hip.lib import SdeHipError
    g, state = torch.ones(8, device=DEV), torch.zeros(2, device=DEV)
    with pytest.raises(SdeHipError):
        NN.grad_norm(g, state, 0.0)                                     # max_norm must be positive
    with pytest.raises(SdeHipError):
        NN.grad_norm(g, torch.zeros(1, device=DEV), 1.0)                # clip_state holds two floats
    with pytest.raises(SdeHipError):
        NN.grad_norm(g, state, 1.0, work=torch.zeros(16, device=DEV))   # a workspace shorter than GRAD_NORM_WORK
    with pytest.raises(SdeHipError):
        NN.grad_norm(g[1:], state, 1.0)                                 # not 16-byte aligned


# ---------------------------------------------------------------------------------------------------------------------------------------
# Adam with the clip coefficient
# ---------------------------------------------------------------------------------------------------------------------------------------
N1, N2 = 1000, 777
SEG_END, SEG_LR, SEG_WD = [N1, N1 + N2], [2e-4, 1e-4], [0.0, 0.0]
ADAM_MAX_NORM = 10.0


def adam_inputs():
    g = torch.Generator().manual_seed(4)
    p, gr = torch.randn(N1 + N2, generator=g), torch.randn(N1 + N2, generator=g)
    gr = gr / gr.norm()
    grads = [gr * (4 * ADAM_MAX_NORM), gr * (0.5 * ADAM_MAX_NORM), gr.flip(0) * (4 * ADAM_MAX_NORM)]      # norm 4 x max_norm, below it, 4 x again
    return p, grads


def torch_clipped_adam(p, grads):
    pa, pb = p[:N1].clone().requires_grad_(True), p[N1:].clone().requires_grad_(True)
    opt = torch.optim.Adam([{"params": [pa], "lr": SEG_LR[0]}, {"params": [pb], "lr": SEG_LR[1]}], weight_decay=0.0, eps=1e-7)
    totals = []
    for gt in grads:
        pa.grad, pb.grad = gt[:N1].clone(), gt[N1:].clone()
        totals.append(float(nn.utils.clip_grad_norm_([pa, pb], ADAM_MAX_NORM)))
        opt.step()
    cat = lambda key: torch.cat([opt.state[pa][key], opt.state[pb][key]])
    return torch.cat([pa.detach(), pb.detach()]), cat("exp_avg"), cat("exp_avg_sq"), totals


def hip_clipped_adam(NN, p, grads, clip=True):
    pd, m, v = p.clone().to(DEV), torch.zeros(N1 + N2, device=DEV), torch.zeros(N1 + N2, device=DEV)
    state, work = torch.zeros(2, device=DEV), torch.zeros(NN.GRAD_NORM_WORK, device=DEV)
    states = []
    for t, gt in enumerate(grads, start=1):
        gd = gt.to(DEV)
        if clip:
            NN.grad_norm(gd, state, ADAM_MAX_NORM, 1.0, work)
        NN.adam_step(pd, gd, m, v, SEG_END, SEG_LR, SEG_WD, (1 - 0.9 ** t, 1 - 0.999 ** t), eps=1e-7, clip_state=state if clip else None)
        states.append(state.clone())
    torch.cuda.synchronize()
    return pd, m, v, states


def test_adam_with_clip_matches_torch(NN):
    p, grads = adam_inputs()
    ref_p, ref_m, ref_v, totals = torch_clipped_adam(p, grads)
    pd, m, v, states = hip_clipped_adam(NN, p, grads)
    coefs = [float(s[1]) for s in states]
    print(f"  totals {[float(s[0]) for s in states]} (torch {totals}) coefs {coefs}")
    assert coefs[0] < 0.26 and coefs[1] == 1.0 and coefs[2] < 0.26
    for name, a, b in (("p", pd, ref_p), ("m", m, ref_m), ("v", v, ref_v)):
        e = float((a.cpu() - b).abs().max())
        print(f"  {name}: max abs difference {e:.2e}")
        assert e < 1e-6, (name, e)
    # the clip is what makes them agree: without it the first update is the same (Adam's first step does not see the gradient's scale) but m and v are not
    _, m_free, _, _ = hip_clipped_adam(NN, p, grads, clip=False)
    assert float((m_free.cpu() - ref_m).abs().max()) > 1e-3


def test_adam_without_clip_state_is_the_plain_kernel(NN):
    """clip_state=None is the update without the field: bit for bit what a coefficient of exactly 1.0 gives (g * 1.0f is g), and the existing
    tests/test_gpu_nn.py::test_adam_step keeps holding that path to torch."""
    p, grads = adam_inputs()
    plain = hip_clipped_adam(NN, p, grads, clip=False)
    pd, m, v = p.clone().to(DEV), torch.zeros(N1 + N2, device=DEV), torch.zeros(N1 + N2, device=DEV)
    one = torch.tensor([123.0, 1.0], device=DEV)
    for t, gt in enumerate(grads, start=1):
        NN.adam_step(pd, gt.to(DEV), m, v, SEG_END, SEG_LR, SEG_WD, (1 - 0.9 ** t, 1 - 0.999 ** t), eps=1e-7, clip_state=one)
    torch.cuda.synchronize()
    assert torch.equal(pd, plain[0]) and torch.equal(m, plain[1]) and torch.equal(v, plain[2])


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_gradient_poisons_the_update_as_in_torch(NN, bad):
    """torch: a NaN element makes total_norm NaN, clamp(NaN, max=1) stays NaN and every gradient -- so every parameter -- becomes NaN.  An infinite
    element makes total_norm inf and the coefficient max_norm / inf = 0: inf * 0 = NaN at that element, 0 elsewhere."""
    p, grads = adam_inputs()
    g = grads[1].clone()
    g[5] = bad
    ref_p, _, _, totals = torch_clipped_adam(p, [g])
    pd, m, v, states = hip_clipped_adam(NN, p, [g])
    total, coef = float(states[0][0]), float(states[0][1])
    print(f"  total {total} (torch {totals[0]}) coef {coef}")
    if math.isnan(bad):
        assert math.isnan(total) and math.isnan(coef) and math.isnan(totals[0])
        assert torch.isnan(pd).all() and torch.isnan(ref_p).all()
    else:
        assert total == float("inf") and totals[0] == float("inf") and coef == 0.0
        assert torch.equal(torch.isnan(pd).cpu(), torch.isnan(ref_p)) and int(torch.isnan(pd).sum()) == 1 and bool(torch.isnan(pd[5]))
        keep = ~torch.isnan(ref_p)
        assert float((pd.cpu()[keep] - ref_p[keep]).abs().max()) < 1e-6


def test_norm_and_adam_capture_into_a_graph(NN):
    p, grads = adam_inputs()
    eager = hip_clipped_adam(NN, p, grads[:1])
    pd, m, v = p.clone().to(DEV), torch.zeros(N1 + N2, device=DEV), torch.zeros(N1 + N2, device=DEV)
    gd, state, work = grads[0].to(DEV), torch.zeros(2, device=DEV), torch.zeros(NN.GRAD_NORM_WORK, device=DEV)

    def pair():
        NN.grad_norm(gd, state, ADAM_MAX_NORM, 1.0, work)
        NN.adam_step(pd, gd, m, v, SEG_END, SEG_LR, SEG_WD, (1 - 0.9, 1 - 0.999), eps=1e-7, clip_state=state)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                  # a host sync inside either call would fail the capture
        pair()
    torch.cuda.synchronize()
    assert torch.equal(pd.cpu(), p) and float(state[1]) == 0.0, "the capture ran the kernels"
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(state, eager[3][0]) and torch.equal(pd, eager[0]) and torch.equal(m, eager[1]) and torch.equal(v, eager[2])


# ---------------------------------------------------------------------------------------------------------------------------------------
# MotionLearningModel under the trainer: the 1 x 32 x 96 fp32 model of tests/test_gpu_motion_model.py
# ---------------------------------------------------------------------------------------------------------------------------------------
B_E2E, H_E2E, W_E2E = 1, 32, 96


def real_cfg():
    from simpledepthestimation_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_other_cfg({"MODEL": {"META_ARCHITECTURE": "MotionLearningModel", "DEVICE": DEV, "COMPUTE_DTYPE": "fp32",
                                        "DEPTH_NET": {"NAME": "GoogleResNet", "NORM": "randLN"},
                                        "POSE_NET": {"NAME": "GoogleMotionNet", "USE_DEPTH": True, "SCALE_CONSTRAIN": "clip_ste"}},
                              "LOSS": {"NUM_SCALES": 1, "SSIM_WEIGHT": 3.0, "C1": "inf", "C2": 9e-6, "DEPTH_L1_WEIGHT": 0.0, "MOTION_SMOOTHNESS_WEIGHT": 1.0,
                                       "MOTION_SPARSITY_WEIGHT": 0.2, "ROT_CYCLE_WEIGHT": 1e-3, "TRANS_CYCLE_WEIGHT": 5e-2, "SCALE_NORMALIZE": False}})
    cfg.MODEL.DEPTH_NET.ENCODER_NAME = "18"        # set directly: merging would read the string as a number
    cfg.SOLVER.DEPTH_LR, cfg.SOLVER.POSE_LR = 1e-4, 2e-4
    return cfg


def real_model(cfg, seed=0):
    from simpledepthestimation_amd.modeling import build_model
    torch.manual_seed(seed)
    return build_model(cfg).train()


def real_batch(seed=9):
    import motion_loss_init as MI
    v = MI.inputs(B_E2E, H_E2E, W_E2E, seed=seed)
    return {"img": v["frame1"].to(DEV), "ctx_img": [v["frame2"].to(DEV)], "intrinsics": v["K"].to(DEV)}


def total(out):
    terms = [v for k, v in out.items() if "loss" in k]
    return sum(terms[1:], terms[0])


@functools.lru_cache(maxsize=None)
def twin_run():
    """The same model stepped three times by torch.optim.Adam(eps=1e-7) + clip_grad_norm_ at half its own first gradient norm.  Computed once."""
    cfg = real_cfg()
    probe = real_model(cfg)
    probe.depth_net.set_stddev(0.0)
    total(probe(real_batch())).backward()
    max_norm = 0.5 * float(nn.utils.clip_grad_norm_(probe.parameters(), float("inf")))
    del probe
    twin = real_model(cfg)
    twin.depth_net.set_stddev(0.0)
    opt = torch.optim.Adam([{"params": twin.depth_net.parameters(), "lr": cfg.SOLVER.DEPTH_LR}, {"params": twin.pose_net.parameters(), "lr": cfg.SOLVER.POSE_LR}],
                           weight_decay=0.0, eps=1e-7)
    totals = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        total(twin(real_batch())).backward()
        totals.append(float(nn.utils.clip_grad_norm_(twin.parameters(), max_norm)))
        opt.step()
    torch.cuda.synchronize()
    return max_norm, totals, {n: p.detach().clone() for n, p in twin.named_parameters()}


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_trainer_follows_the_torch_twin(use_graph):
    from simpledepthestimation_amd.engine.trainer import motion_learning_trainer
    max_norm, totals, twin_params = twin_run()
    cfg = real_cfg()
    cfg.SOLVER.CLIP_GRAD = max_norm
    model = real_model(cfg)
    model.depth_net.set_stddev(0.0)
    tr = motion_learning_trainer(model, cfg, use_graph=use_graph)
    assert tr.clip_grad == max_norm and tr.eps == 1e-7 and not tr.adamw
    for k in range(3):
        out = tr.step(real_batch())
        gn = tr.grad_norm()
        assert gn.is_cuda and gn.dim() == 0
        e = abs(float(gn) - totals[k]) / totals[k]
        print(f"  step {k + 1}: grad_norm {float(gn):.6g} twin {totals[k]:.6g} ({e:.1e}), max_norm {max_norm:.6g}, coef {float(tr.clip_state[1]):.4f}")
        assert e <= 3e-3, (k, e)
        assert all(math.isfinite(float(v.detach())) for v in out.values())
    assert totals[0] > max_norm and float(tr.clip_state[1]) <= 1.0
    worst = max((float((p.detach() - twin_params[n]).abs().max()), n) for n, p in model.named_parameters() if ".encoder.fc." not in n)
    lr = max(cfg.SOLVER.DEPTH_LR, cfg.SOLVER.POSE_LR)
    print(f"  max |dp| after 3 steps: {worst[0]:.3e} at {worst[1]} (bound {3 * 2 * lr:.1e})")
    for n, p in model.named_parameters():
        if ".encoder.fc." in n:
            continue
        lr_n = cfg.SOLVER.POSE_LR if n.startswith("pose_net") else cfg.SOLVER.DEPTH_LR
        assert float((p.detach() - twin_params[n]).abs().max()) <= 3 * 2 * lr_n, n


def test_do_train_motion_learning(tmp_path):
    from simpledepthestimation_amd.engine.loops import do_train
    cfg = real_cfg()
    cfg.OUTPUT_DIR = str(tmp_path)
    cfg.LOG_PERIOD, cfg.SOLVER.MAX_EPOCHS, cfg.TEST.EVAL_PERIOD, cfg.SOLVER.CHECKPOINT_PERIOD = 1, 2, 0, 1
    cfg.MODEL.POSE_NET.BURN_IN_ITERS, cfg.MODEL.DEPTH_NET.RAMPUP_ITERS, cfg.MODEL.DEPTH_NET.NOISE_STDDEV = 4, 4, 0.5
    cfg.SOLVER.LR_STEPS, cfg.SOLVER.GAMMA, cfg.SOLVER.CLIP_GRAD = (1,), 0.5, 10.0
    loader = [real_batch(seed=20 + i) for i in range(2)]
    model = real_model(cfg)
    rec = do_train(cfg, model, loader, None)
    print("\n".join(str(r) for r in rec))
    assert [r["iteration"] for r in rec] == [1, 2, 3, 4]
    assert [r["motion_weight"] for r in rec] == [0.0, 0.0, 0.5, 1.0]
    assert [r["noise_stddev"] for r in rec] == [0.5 * (k / 4) ** 2 for k in (1, 2, 3, 4)]
    assert [r["lr"] for r in rec] == [cfg.SOLVER.DEPTH_LR] * 2 + [cfg.SOLVER.DEPTH_LR * 0.5] * 2
    for r in rec:
        assert math.isfinite(r["grad_norm"]) and r["grad_norm"] > 0 and math.isfinite(r["total_loss"])
        assert 0 < r["trans_scale"] < 0.1 and 0 < r["rot_scale"] < 0.1
    assert float(model.pose_net._motion_weight) == 1.0 and model.pose_net.motion_weight == 1.0
    # one more epoch on a resumed run (a fresh model and trainer): both schedules continue from step 4
    cfg.SOLVER.MAX_EPOCHS = 3
    model2 = real_model(cfg, seed=5)
    rec2 = do_train(cfg, model2, loader, None, resume=True)
    print("\n".join(str(r) for r in rec2))
    assert [r["iteration"] for r in rec2] == [5, 6] and [r["epoch"] for r in rec2] == [2, 2]
    assert [r["motion_weight"] for r in rec2] == [1.0, 1.0] and [r["noise_stddev"] for r in rec2] == [0.5, 0.5]
    assert [r["lr"] for r in rec2] == [cfg.SOLVER.DEPTH_LR * 0.5] * 2
    assert all(math.isfinite(r["grad_norm"]) and r["grad_norm"] > 0 for r in rec2)
    assert abs(rec2[0]["trans_scale"] - rec[-1]["trans_scale"]) <= 2 * cfg.SOLVER.POSE_LR      # the resumed parameters, one step further

"""CPU: the control path of MotionLearning training -- gradient-norm clipping in HipTrainer (clip_fn / adam_fn torch restatements stand in for
sde_grad_norm / sde_adam_step), the burn-in schedule and motion_learning_trainer's optimizer state.

Reference: projects/MotionLearning/train.py:L69-73 (Adam, eps 1e-7), L111-114 (burn-in), L157 (clip_grad_norm_)."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from test_dp_gloo import Tiny, _data, _free_port, torch_adam

MAX_NORM = 0.3          # below the gradient norm of Tiny on _data() at its initial weights (checked in the tests): the clip is active


def torch_clip(g, clip_state, max_norm, grad_scale, work):
    """sde_grad_norm restated: {grad_scale * ||g||, clamp(max_norm / (total + 1e-6), max=1)}."""
    total = g.norm() * grad_scale
    clip_state[0] = total
    clip_state[1] = torch.clamp(max_norm / (total + 1e-6), max=1.0)


def torch_adam_clip(p, g, m, v, seg_end, seg_lr, seg_wd, bias_corr, b1, b2, eps, grad_scale, decoupled, clip_state=None):
    """sde_adam_step restated: the clip coefficient multiplies grad_scale, nothing else changes."""
    if clip_state is not None:
        grad_scale = grad_scale * float(clip_state[1])
    torch_adam(p, g, m, v, seg_end, seg_lr, seg_wd, bias_corr, b1, b2, eps, grad_scale, decoupled)


def _make(seed):
    torch.manual_seed(seed)
    return Tiny()


def _groups(model):
    from simpledepthestimation_amd.engine.trainer import ParamGroup
    return [ParamGroup("a", model.a.named_parameters(prefix="a"), 1e-2, 0.0), ParamGroup("b", model.b.named_parameters(prefix="b"), 5e-3, 0.0)]


def _trainer(model, clip_grad=MAX_NORM, **kw):
    from simpledepthestimation_amd.engine.trainer import HipTrainer
    return HipTrainer(model, _groups(model), adamw=False, eps=1e-7, bucket_mb=1e-5, adam_fn=torch_adam_clip, clip_fn=torch_clip, clip_grad=clip_grad, **kw)


def test_without_clip_grad_the_optimizer_call_is_unchanged():
    from simpledepthestimation_amd.engine.trainer import HipTrainer
    calls, clips = [], []

    def spy(*a, **k):
        calls.append((a, k))
        torch_adam(*a, **k)
    model = _make(3)
    for clip in (None, 0):
        tr = HipTrainer(model, _groups(model), adamw=False, eps=1e-7, adam_fn=spy, clip_fn=lambda *a: clips.append(a), clip_grad=clip)
        assert tr.clip_grad is None and tr.clip_state is None
        x, t = _data(8)
        tr.step({"x": x, "t": t})
        with pytest.raises(RuntimeError):
            tr.grad_norm()
        a, k = calls.pop()
        assert not calls and not clips
        assert k == {} and len(a) == 13          # (p, g, m, v, seg_end, lrs, wds, bias_corr, b1, b2, eps, 1 / world, adamw): positional, no clip_state
        assert a[0] is tr.pflat and a[1] is tr.gflat and a[4] == tr.seg_end and a[10] == 1e-7 and a[11] == 1.0 and a[12] is False


def test_three_clipped_steps_match_torch():
    model, ref = _make(3), _make(3)
    tr = _trainer(model)
    opt = torch.optim.Adam([{"params": ref.a.parameters(), "lr": 1e-2}, {"params": ref.b.parameters(), "lr": 5e-3}], weight_decay=0.0, eps=1e-7)
    x, t = _data(8)
    coefs = []
    for _ in range(3):
        tr.step({"x": x, "t": t})
        opt.zero_grad(); ref({"x": x, "t": t})["mse_loss"].backward()
        total = nn.utils.clip_grad_norm_(ref.parameters(), MAX_NORM)
        opt.step()
        assert abs(float(tr.grad_norm()) - float(total)) <= 1e-6 * float(total)
        assert tr.grad_norm().data_ptr() == tr.clip_state.data_ptr()        # a view of the device state, not a copy
        coefs.append(float(tr.clip_state[1]))
    assert min(coefs) < 1.0, coefs                                          # the clip was active
    for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        assert torch.allclose(p, q, rtol=1e-5, atol=1e-7), n
    # and it matters: the unclipped trajectory is a different one
    free = _make(3)
    tr_free = _trainer(free, clip_grad=None)
    for _ in range(3):
        tr_free.step({"x": x, "t": t})
    assert not torch.allclose(tr_free.pflat, tr.pflat, rtol=1e-5, atol=1e-7)


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        tr = _trainer(_make(10 + rank))
        x, t = _data(8)
        half = slice(rank * 4, rank * 4 + 4)
        states = []
        for _ in range(3):
            tr.step({"x": x[half], "t": t[half]})
            states.append(tr.clip_state.clone())
        out[rank] = (torch.stack(states), tr.pflat.clone())
    finally:
        dist.destroy_process_group()


def test_two_ranks_clip_by_the_norm_of_the_averaged_gradient():
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        out = mgr.dict()
        port = _free_port()
        procs = [ctx.Process(target=_worker, args=(r, 2, port, out)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(120)
            assert p.exitcode == 0
        (s0, p0), (s1, p1) = out[0], out[1]
    assert torch.equal(s0, s1) and torch.equal(p0, p1), "ranks diverged"
    tr = _trainer(_make(10))
    x, t = _data(8)
    single = []
    for _ in range(3):
        tr.step({"x": x, "t": t})
        single.append(tr.clip_state.clone())
    single = torch.stack(single)
    assert float(single[:, 1].min()) < 1.0
    assert torch.allclose(s0, single, rtol=1e-5, atol=0)          # {total_norm, clip_coef} per step: the concatenated batch's
    assert torch.allclose(tr.pflat, p0, rtol=1e-5, atol=1e-7)


def test_amp_with_clip_grad_raises():
    with pytest.raises(ValueError, match="clip_grad"):
        _trainer(_make(0), amp=True)
    with pytest.raises(ValueError):
        _trainer(_make(0), clip_grad=-1.0)


def test_burn_in_weight_is_the_reference_closed_form():
    from simpledepthestimation_amd.engine.loops import burn_in_weight
    for B in (4, 20000):
        for step in (0, B // 2, 3 * B // 4, B, 2 * B):
            assert burn_in_weight(step, B) == float(np.clip(2 * step / B - 1, 0.0, 1.0)), (step, B)      # train.py:L113
        assert [burn_in_weight(s, B) for s in (0, B // 2, 3 * B // 4, B, 2 * B)] == [0.0, 0.0, 0.5, 1.0, 1.0]


class TinyMotion(nn.Module):
    """depth_net / pose_net with a 0-dim parameter, as GoogleMotionNet's trans_scale: the two groups of motion_learning_trainer."""

    def __init__(self):
        super().__init__()
        self.depth_net = nn.Linear(6, 5)
        self.pose_net = nn.Linear(5, 1)
        self.pose_net.trans_scale = nn.Parameter(torch.tensor(0.5))

    def forward(self, batch):
        y = self.pose_net(torch.tanh(self.depth_net(batch["x"]))).squeeze(-1) * self.pose_net.trans_scale
        return {"mse_loss": ((y - batch["t"]) ** 2).mean()}


def _motion(seed=5):
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.engine.trainer import motion_learning_trainer
    cfg = get_cfg()
    assert cfg.SOLVER.CLIP_GRAD == 0                                    # the default: off
    cfg.SOLVER.DEPTH_LR, cfg.SOLVER.POSE_LR, cfg.SOLVER.CLIP_GRAD = 1e-2, 5e-3, MAX_NORM
    torch.manual_seed(seed)
    model = TinyMotion()
    return model, motion_learning_trainer(model, cfg, adam_fn=torch_adam_clip, clip_fn=torch_clip), cfg


def _torch_motion(model, cfg):
    return torch.optim.Adam([{"params": model.depth_net.parameters(), "lr": cfg.SOLVER.DEPTH_LR}, {"params": model.pose_net.parameters(), "lr": cfg.SOLVER.POSE_LR}],
                            weight_decay=0.0, eps=1e-7)


def test_motion_learning_trainer_state_round_trips_through_torch_adam():
    model, tr, cfg = _motion()
    assert [g.name for g in tr.groups] == ["Depth", "Pose"] and not tr.adamw and tr.eps == 1e-7 and tr.clip_grad == MAX_NORM
    x, t = _data(8)
    for _ in range(2):
        tr.step({"x": x, "t": t})
    sd = tr.state_dict()
    assert [g["eps"] for g in sd["param_groups"]] == [1e-7, 1e-7]
    # trainer -> torch.optim.Adam(eps=1e-7) over the same groups: one more clipped step on both sides
    ref, _, _ = _motion()
    ref.load_state_dict(model.state_dict())
    opt = _torch_motion(ref, cfg)
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["eps"] == 1e-7 and opt.param_groups[1]["lr"] == 5e-3
    tr.step({"x": x, "t": t})
    opt.zero_grad(); ref({"x": x, "t": t})["mse_loss"].backward()
    nn.utils.clip_grad_norm_(ref.parameters(), MAX_NORM); opt.step()
    for (k, a), (_, b) in zip(model.state_dict().items(), ref.state_dict().items()):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6, msg=k)
    # and back: torch's state into a fresh trainer, one more step on both
    model2, tr2, _ = _motion(seed=6)
    model2.load_state_dict(ref.state_dict())
    tr2.load_state_dict(opt.state_dict())
    assert tr2.t == 3
    tr2.step({"x": x, "t": t})
    tr.step({"x": x, "t": t})
    for (k, a), (_, b) in zip(model.state_dict().items(), model2.state_dict().items()):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6, msg=k)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the weight-gradient schedule family the trainer applies (hip.lib.SCHEDULES): declared by the networks, not read off class names
# ---------------------------------------------------------------------------------------------------------------------------------------
def _depth_net(name, enc="18", norm="randLN"):
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.modeling.depth_net import build_depth_net
    cfg = get_cfg()
    cfg.MODEL.DEPTH_NET.NAME, cfg.MODEL.DEPTH_NET.ENCODER_NAME, cfg.MODEL.DEPTH_NET.NORM = name, enc, norm
    return build_depth_net(cfg)


def _motion_learning_model():
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.modeling import build_model
    cfg = get_cfg()
    cfg.merge_from_other_cfg({"MODEL": {"META_ARCHITECTURE": "MotionLearningModel", "DEVICE": "cpu", "DEPTH_NET": {"NAME": "GoogleResNet", "NORM": "randLN"},
                                        "POSE_NET": {"NAME": "GoogleMotionNet", "USE_DEPTH": True, "SCALE_CONSTRAIN": "clip_ste"}},
                              "LOSS": {"NUM_SCALES": 1, "SSIM_WEIGHT": 3.0, "C1": "inf", "C2": 9e-6, "DEPTH_L1_WEIGHT": 0.0, "MOTION_SMOOTHNESS_WEIGHT": 1.0,
                                       "MOTION_SPARSITY_WEIGHT": 0.2, "ROT_CYCLE_WEIGHT": 1e-3, "TRANS_CYCLE_WEIGHT": 5e-2, "SCALE_NORMALIZE": False}})
    cfg.MODEL.DEPTH_NET.ENCODER_NAME = "18"        # set directly: merging would read the string as a number
    return build_model(cfg)


FAMILY_TABLE = [("DepthResNet-18", lambda: _depth_net("DepthResNet", "18"), "resnet_basic"),
                ("DepthResNet-50", lambda: _depth_net("DepthResNet", "50"), "resnet"),
                ("GoogleResNet-18-randLN", lambda: _depth_net("GoogleResNet", "18", "randLN"), "resnet"),
                ("GoogleResNet-50-BN", lambda: _depth_net("GoogleResNet", "50", "BN"), "resnet"),
                ("PackNet01", lambda: _depth_net("PackNet01"), "packnet"),
                ("MotionLearningModel", _motion_learning_model, "resnet"),
                ("Linear", lambda: nn.Linear(3, 2), "resnet")]


@pytest.mark.parametrize("make,family", [c[1:] for c in FAMILY_TABLE], ids=[c[0] for c in FAMILY_TABLE])
def test_schedule_family_table(make, family):
    from simpledepthestimation_amd.engine.trainer import HipTrainer, ParamGroup, schedule_family
    from simpledepthestimation_amd.hip import lib as L
    model = make()
    assert schedule_family(model) == family
    before = (L.JOIN_LAG, L.WGRAD_GROUP, L.FIRST_GROUP)
    try:
        L.apply_schedule("packnet" if family != "packnet" else "resnet")      # something else, so that the trainer has to set it
        HipTrainer(model, [ParamGroup("all", model.named_parameters(), 1e-3, 0.0)], adam_fn=torch_adam)
        assert (L.JOIN_LAG, L.WGRAD_GROUP, L.FIRST_GROUP) == L.SCHEDULES[family]
    finally:
        L.JOIN_LAG, L.WGRAD_GROUP, L.FIRST_GROUP = before

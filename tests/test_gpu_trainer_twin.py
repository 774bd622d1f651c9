"""GPU: HipTrainer(twin_operands=True) -- forward operands as views of the Adam kernel's 16-bit twin, data-gradient operands transposed from it --
against twin_operands=False (per-step full pack from fp32 + sde_adam_step), bit for bit: losses, parameters, gradients and both moments after each
of four steps, eager and captured, in bf16 and in fp16 with loss scaling and one overflow step; a load_state_dict in the middle; a foreign write to a
parameter followed by refresh_operands(); a net with a transposed convolution, whose forward pass reads the "data-gradient" operand.  The net has one layer of each kind: three that share the twin (1x1 64->64 + BN, 3x3 64->128 stride 2 + BN,
3x3 128->64 with bias + ELU) and a one-channel 3x3 head that stays on the per-step pack."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda"


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        from simpledepthestimation_amd.layers.hip_modules import HipBatchNorm2d, HipConv2d
        self.c1, self.b1 = HipConv2d(64, 64, 1, bias=False), HipBatchNorm2d(64)
        self.c2, self.b2 = HipConv2d(64, 128, 3, stride=2, padding=1, bias=False), HipBatchNorm2d(128)
        self.c3 = HipConv2d(128, 64, 3, padding=1, bias=True)
        self.head = HipConv2d(64, 1, 3, padding=1, bias=True)

    def forward(self, batch):
        from simpledepthestimation_amd.hip import nn as HN
        from simpledepthestimation_amd.layers.hip_modules import conv_bn
        x = conv_bn(self.c1, self.b1, batch["x"])
        x = conv_bn(self.c2, self.b2, x)
        x = self.c3(x, act=HN.ACT_ELU)
        y = self.head(x)[..., 0].float()
        return {"sq_loss": ((y - batch["t"]) ** 2).mean()}


def make(dt, twin, graph, amp=False):
    from simpledepthestimation_amd.engine.trainer import HipTrainer, ParamGroup
    torch.manual_seed(4)
    model = Net().to(DEV).train()
    groups = [ParamGroup("early", [(n, p) for n, p in model.named_parameters() if n[:2] in ("c1", "b1", "c2", "b2")], 1e-3, 1e-2),
              ParamGroup("late", [(n, p) for n, p in model.named_parameters() if n[:2] not in ("c1", "b1", "c2", "b2")], 3e-3, 0.0)]
    tr = HipTrainer(model, groups, adamw=True, eps=1e-6, use_graph=graph, amp=amp, init_scale=256.0, twin_operands=twin)
    return model, tr


def batches(dt, n, bad=None):
    g = torch.Generator().manual_seed(8)
    out = []
    for i in range(n):
        x = torch.randn(2, 16, 32, 64, generator=g)
        if i == bad:
            x[0, 3, 5, 7] = float("inf")             # forced overflow: non-finite gradients, the step is skipped and the scale backs off
        out.append({"x": x.to(DEV, dt), "t": torch.randn(2, 8, 16, generator=g).to(DEV)})
    return out


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def state(tr, loss):
    return [bits(next(iter(loss.values())).float().reshape(1).clone()), bits(tr.pflat.clone()), bits(tr.gflat.clone()), bits(tr.m.clone()), bits(tr.v.clone())]


def run(dt, twin, graph, amp=False, bad=None, steps=4, mid=None):
    model, tr = make(dt, twin, graph, amp)
    out = []
    for i, b in enumerate(batches(dt, steps, bad)):
        if mid is not None and i == 2:
            mid(model, tr)
        out.append(state(tr, tr.step(b)))
    torch.cuda.synchronize()
    return out, tr


def assert_same(a, b):
    for i, (sa, sb) in enumerate(zip(a, b)):
        for name, x, y in zip(("loss", "pflat", "gflat", "m", "v"), sa, sb):
            assert torch.equal(x, y), f"step {i}: {name} differs"


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_twin_operands_change_no_bit_bf16(graph):
    ref, tr0 = run(torch.bfloat16, False, graph)
    new, tr1 = run(torch.bfloat16, True, graph)
    assert tr0.twin is None and tr0._packer.n_shared == 0 and tr0._packer.n == 4
    assert tr1.twin is not None and tr1._packer.n_shared == 3 and tr1._packer.n == 1
    assert_same(ref, new)
    assert not torch.equal(ref[0][1], ref[3][1])          # (the parameters did move)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_twin_operands_change_no_bit_fp16_amp_with_an_overflow_step(graph):
    ref, tr0 = run(torch.float16, False, graph, amp=True, bad=1)
    new, tr1 = run(torch.float16, True, graph, amp=True, bad=1)
    assert tr1._packer.n_shared == 3
    assert_same(ref, new)
    assert torch.equal(ref[0][1], ref[1][1]) and not torch.equal(ref[1][1], ref[2][1])      # step 1 was skipped, step 2 applied
    assert tr1.applied_steps() == 3 and float(tr1.scale_state[0]) == 128.0


def test_no_refresh_in_ordinary_steps():
    """The version check of step() must not see the trainer's own work as a foreign write: one refresh, at the packer's construction."""
    model, tr = make(torch.bfloat16, True, True)
    bs = batches(torch.bfloat16, 4)
    tr.step(bs[0])
    calls = []
    inner = tr._packer.refresh
    tr._packer.refresh = lambda: (calls.append(1), inner())
    for b in bs[1:]:
        tr.step(b)
    torch.cuda.synchronize()
    assert calls == []


def test_load_state_dict_in_the_middle():
    def mid(model, tr):
        sd = tr.state_dict()
        for ent in sd["state"].values():
            ent["exp_avg"].mul_(0.5)
        tr.load_state_dict(sd)
    ref, _ = run(torch.bfloat16, False, True, mid=mid)
    new, _ = run(torch.bfloat16, True, True, mid=mid)
    assert_same(ref, new)


@pytest.mark.parametrize("how", ["data", "inplace"])
def test_foreign_write_then_refresh(how):
    """A write to a parameter that did not come from the Adam kernel: through .data (invisible: refresh_operands() is the caller's duty) or in place
    through the parameter (step() notices the version bump and refreshes by itself)."""
    def mid(model, tr):
        with torch.no_grad():
            if how == "data":
                model.c2.weight.data.mul_(0.5)
                model.head.weight.data.mul_(2.0)
                tr.refresh_operands()
            else:
                model.c2.weight.mul_(0.5)
                model.head.weight.mul_(2.0)
    ref, _ = run(torch.bfloat16, False, True, mid=mid)
    new, _ = run(torch.bfloat16, True, True, mid=mid)
    assert_same(ref, new)
    plain, _ = run(torch.bfloat16, False, True)
    assert not torch.equal(plain[2][0], ref[2][0])         # (the write did change the step)


class UpNet(nn.Module):
    """1x1 64->64 + BN, then a transposed convolution 64->32 (+ReLU) whose FORWARD operand is WeightPacker's data-gradient operand of the adjoint
    convolution, then the one-channel head."""

    def __init__(self):
        super().__init__()
        from simpledepthestimation_amd.layers.hip_modules import HipBatchNorm2d, HipConv2d, HipConvTranspose2d
        self.c1, self.b1 = HipConv2d(64, 64, 1, bias=False), HipBatchNorm2d(64)
        self.up = HipConvTranspose2d(64, 32)
        self.head = HipConv2d(32, 1, 3, padding=1, bias=True)

    def forward(self, batch):
        from simpledepthestimation_amd.hip import nn as HN
        from simpledepthestimation_amd.layers.hip_modules import conv_bn
        x = conv_bn(self.c1, self.b1, batch["x"])
        x = self.up(x, act=HN.ACT_RELU)
        y = self.head(x)[..., 0].float()
        return {"sq_loss": ((y - batch["t"]) ** 2).mean()}


def run_up(twin, graph, steps=4):
    from simpledepthestimation_amd.engine.trainer import HipTrainer, ParamGroup
    torch.manual_seed(6)
    model = UpNet().to(DEV).train()
    tr = HipTrainer(model, [ParamGroup("all", list(model.named_parameters()), 3e-3, 1e-2)], adamw=True, eps=1e-6, use_graph=graph, twin_operands=twin)
    g = torch.Generator().manual_seed(9)
    out = []
    for _ in range(steps):
        b = {"x": torch.randn(2, 8, 16, 64, generator=g).to(DEV, torch.bfloat16), "t": torch.randn(2, 16, 32, generator=g).to(DEV)}
        out.append(state(tr, tr.step(b)))
    torch.cuda.synchronize()
    return out, tr, model


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_transposed_convolution_shares_the_twin_and_is_packed_before_forward(graph):
    from simpledepthestimation_amd.hip import nn as HN
    ref, tr0, _ = run_up(False, graph)
    new, tr1, model = run_up(True, graph)
    pk = tr1._packer
    # c1 and up share the twin; only c1's data-gradient operand may run beside the forward pass: up's is read BY the forward pass and rides with the head's
    assert pk.n_shared == 2 and pk.n_dgrad == 1 and pk.n == 2
    assert_same(ref, new)
    assert not torch.equal(ref[0][1], ref[3][1])
    dt, cin_pad, ldy = model.up._pack_shapes
    model.up._packed[1].view(torch.int16).fill_(0x7f7f)
    pk.run()                                   # the head-of-step launch alone must leave up's forward operand ready
    torch.cuda.synchronize()
    want = HN.pack_weight(model.up.weight, dt, cin_pad, ldy, for_dgrad=True)
    assert torch.equal(model.up._packed[1].view(torch.int16), want.view(torch.int16))

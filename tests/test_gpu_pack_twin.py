"""GPU: the weight pack's 16-bit twin source (SDE_W_TWIN16).

Six convolutions live channels-last in one flat fp32 buffer, as HipTrainer keeps them, with a 16-bit twin of that buffer.  The four that need no
padding (64->64 1x1, 64->128 3x3, 128->64 3x3, 192->64 3x3) take their forward operand as a view of the twin and their data-gradient operand from it;
the stem-like 3->64 7x7 and the one-channel head 64->1 3x3 stay on the fp32 kind.  Every operand must equal the per-layer fp32 pack bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(64, 64, 1), (64, 128, 3), (3, 64, 7), (128, 64, 3), (64, 1, 3), (192, 64, 3)]      # (Cin, Cout, k); the 3rd and 5th are not eligible
ELIGIBLE = [True, True, False, True, False, True]


@pytest.fixture(scope="module")
def NN():
    from simpledepthestimation_amd.hip import nn
    return nn


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def setup(request, NN):
    from simpledepthestimation_amd.engine.trainer import flat_view
    from simpledepthestimation_amd.layers.hip_modules import HipConv2d
    dt = request.param
    torch.manual_seed(11)
    net = torch.nn.ModuleList([HipConv2d(ci, co, k, padding=k // 2, bias=False) for ci, co, k in SHAPES]).to(DEV)
    sizes = [(m.weight.numel() + 7) & ~7 for m in net]            # 8-element slots: every slot of the twin starts on 16 bytes
    flat = torch.zeros(sum(sizes), device=DEV)
    offs, off = {}, 0
    for m, n in zip(net, sizes):
        flat_view(flat, off, m.weight).copy_(m.weight.data)
        m.weight.data = flat_view(flat, off, m.weight)
        offs[id(m.weight)] = off
        off += n
    for m, (ci, co, k) in zip(net, SHAPES):
        m(torch.zeros(1, 8, 8, (ci + 7) // 8 * 8, device=DEV, dtype=dt))          # records the padded operand shapes
    twin = torch.zeros(flat.numel(), device=DEV, dtype=dt)
    packer = NN.WeightPacker(net, twin, lambda w: offs.get(id(w)))
    ref = [(NN.pack_weight(m.weight, dt, m._pack_shapes[1], m._pack_shapes[2], for_dgrad=False),
            NN.pack_weight(m.weight, dt, m._pack_shapes[1], m._pack_shapes[2], for_dgrad=True)) for m in net]
    return net, flat, twin, packer, ref, dt


def poison(net):
    for m in net:
        m._packed[1].view(torch.int16).fill_(0x7f7f)


def test_eligible_layers_share_the_twin(setup):
    net, flat, twin, packer, ref, dt = setup
    assert packer.n_shared == 4 and packer.n == 2 and packer.n_dgrad == 4
    lo, hi = twin.data_ptr(), twin.data_ptr() + twin.numel() * 2
    for m, ok in zip(net, ELIGIBLE):
        inside = lo <= m._packed[0].data_ptr() < hi
        assert inside == ok, (m, ok)
        assert m._packed[0].data_ptr() % 16 == 0 and m._packed[1].data_ptr() % 16 == 0


def test_refresh_then_per_step_tables_equal_the_fp32_pack(setup):
    net, flat, twin, packer, ref, dt = setup
    packer.refresh()
    for m, (wp, wd) in zip(net, ref):
        assert torch.equal(bits(m._packed[0]), bits(wp)) and torch.equal(bits(m._packed[1]), bits(wd)), f"refresh: {m}"
    poison(net)
    packer.run()            # fp32 kind: the two layers that do not share the twin, both operands
    packer.run_dgrad()      # twin kind: the four that do, data-gradient operand only
    for m, (wp, wd) in zip(net, ref):
        assert torch.equal(bits(m._packed[0]), bits(wp)), f"forward operand {m}"
        assert torch.equal(bits(m._packed[1]), bits(wd)), f"data-gradient operand {m}"


def test_sources_twin_for_eligible_fp32_for_the_rest(setup, NN):
    """Moving the fp32 masters without the twin changes only the non-eligible layers' operands; moving the twin changes the eligible ones'."""
    net, flat, twin, packer, ref, dt = setup
    packer.refresh()
    kept = flat.clone()
    try:
        flat.mul_(2.0)
        new = [(NN.pack_weight(m.weight, dt, m._pack_shapes[1], m._pack_shapes[2], for_dgrad=False),
                NN.pack_weight(m.weight, dt, m._pack_shapes[1], m._pack_shapes[2], for_dgrad=True)) for m in net]
        poison(net)
        packer.run()
        packer.run_dgrad()
        for m, ok, (wp, wd), (wp2, wd2) in zip(net, ELIGIBLE, ref, new):
            assert torch.equal(bits(m._packed[1]), bits(wd if ok else wd2)), f"{m}: eligible {ok}"
            if not ok:
                assert torch.equal(bits(m._packed[0]), bits(wp2)) and not torch.equal(bits(wd), bits(wd2))
        twin.mul_(2.0)                           # doubling a 16-bit value is exact: the twin's operands are now 2 x the old ones
        packer.run_dgrad()
        for m, ok, (wp, wd), (wp2, wd2) in zip(net, ELIGIBLE, ref, new):
            assert torch.equal(bits(m._packed[1]), bits((wd.float() * 2.0).to(dt) if ok else wd2)), f"{m} after the twin moved"
    finally:
        flat.copy_(kept)
        packer.refresh()

"""CPU: hip.nn.aliases / hip.nn.fan_in, the fan-out of one kernel output to n consumers and the fan-in of their gradients to a backward kernel's slots."""
import pytest
import torch

from simpledepthestimation_amd.hip.nn import aliases, fan_in


def _grads(n):
    g = torch.Generator().manual_seed(n)
    return [torch.randn(3, 5, generator=g) for _ in range(n)]


def test_aliases_share_storage():
    out = torch.zeros(2, 3, 4, 8)
    assert aliases(out, 1) is out
    a = aliases(out, 3)
    assert isinstance(a, tuple) and len(a) == 3 and a[0] is out
    assert all(t.data_ptr() == out.data_ptr() and t.shape == out.shape and t.stride() == out.stride() for t in a)
    assert a[1] is not out and a[2] is not a[1]          # distinct tensors: autograd hands backward one gradient per alias


@pytest.mark.parametrize("slots", [2, 3])
def test_fan_in_drops_folds_and_pads(slots):
    assert not fan_in((), slots) and not fan_in((None,), slots) and not fan_in((None, None, None, None), slots)
    (g,) = _grads(1)
    for douts in ((g,), (None, g), (g, None, None), (None, None, g, None)):
        r = fan_in(douts, slots)
        assert len(r) == slots and r[0] is g and all(x is None for x in r[1:])
    gs = _grads(slots)
    r = fan_in([None] + gs[:1] + [None, None] + gs[1:], slots)
    assert len(r) == slots and all(a is b for a, b in zip(r, gs))          # exactly as many as the kernel takes: no add, no copy
    gs = _grads(slots + 1)
    r = fan_in(gs[:1] + [None] + gs[1:] + [None], slots)
    assert len(r) == slots and all(a is b for a, b in zip(r[:-1], gs)) and torch.equal(r[-1], gs[slots - 1] + gs[slots])
    gs = _grads(slots + 2)
    r = fan_in([None, None] + gs[:2] + [None] + gs[2:], slots)
    assert len(r) == slots and all(a is b for a, b in zip(r[:-1], gs))
    assert torch.equal(r[-1], (gs[slots - 1] + gs[slots]) + gs[slots + 1])      # the left fold into the last slot
    assert all(torch.equal(a, b) for a, b in zip(gs, _grads(slots + 2)))        # the arriving gradients are left as they were

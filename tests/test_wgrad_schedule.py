"""Weight-gradient schedule of a backward phase (hip.nn.wgrad_group_rule, WGradReducer.phase) on the CPU.

The rule is replayed over hand-built layer sequences the way WGradReducer applies it: which layers' weight-gradient GEMMs share one fork of the
side stream ("group"), which fork on their own ("alone") and which stay on the main stream ("inline"), in launch order.  A sequence runs in
backward order and ends with the stem, the one layer without a data gradient."""
import pytest
import torch

from simpledepthestimation_amd.hip import lib as L
from simpledepthestimation_amd.hip import nn as HN

MB = 1 << 20


def schedule(layers, first_group, group, early_tail=True):
    """layers: operand bytes of each layer; None marks a layer without a data gradient (it cannot fork).  Returns [(place, layer indices)]."""
    out, queue, queued_bytes, done = [], [], 0, 0

    def run_queue():
        nonlocal queue, queued_bytes, done
        if queue:
            out.append(("group", tuple(queue)))
            queue, queued_bytes, done = [], 0, done + 1

    for i, nbytes in enumerate(layers):
        need_dx = nbytes is not None
        run_first, place, close = HN.wgrad_group_rule(len(queue), queued_bytes, done, nbytes or MB, need_dx, need_dx, first_group, group,
                                                      L.GROUP_MAX_BYTES, L.GROUP_BUDGET_BYTES, early_tail)
        if run_first:
            run_queue()
        if place == "group":
            queue.append(i)
            queued_bytes += nbytes
            if close:
                run_queue()
        else:
            out.append((place, (i,)))
    run_queue()                 # the phase's flush
    return out


def small(n):
    return [10 * MB] * n


def test_resnet_schedule():
    _, group, first = L.SCHEDULES["resnet"]
    assert (group, first) == (6, 0)
    assert schedule(small(14) + [None], first, group) == [
        ("group", (0, 1, 2, 3, 4, 5)), ("group", (6, 7, 8, 9, 10, 11)), ("group", (12, 13)), ("inline", (14,))]


def test_resnet_basic_schedule_has_a_short_first_group():
    _, group, first = L.SCHEDULES["resnet_basic"]
    assert (group, first) == (6, 3)
    assert schedule(small(13) + [None], first, group) == [
        ("group", (0, 1, 2)), ("group", (3, 4, 5, 6, 7, 8)), ("group", (9, 10, 11, 12)), ("inline", (13,))]


def test_packnet_schedule_forks_full_resolution_layers_alone():
    _, group, first = L.SCHEDULES["packnet"]
    assert (group, first) == (3, 0)
    big = 190 * MB
    assert big > L.GROUP_MAX_BYTES
    # the layer over GROUP_MAX_BYTES forks the open group first (it closes early and counts as a group), then itself
    assert schedule(small(4) + [big] + small(2) + [big, None], first, group) == [
        ("group", (0, 1, 2)), ("group", (3,)), ("alone", (4,)), ("group", (5, 6)), ("alone", (7,)), ("inline", (8,))]


def test_two_digit_first_group():
    assert schedule(small(13) + [None], 33, 6) == [
        ("group", (0, 1, 2)), ("group", (3, 4, 5)), ("group", (6, 7, 8, 9, 10, 11)), ("group", (12,)), ("inline", (13,))]


def test_early_closed_group_counts_towards_the_first_group_digits():
    big = L.GROUP_MAX_BYTES + 1
    assert schedule([10 * MB, big] + small(5), 33, 6) == [
        ("group", (0,)), ("alone", (1,)), ("group", (2, 3, 4)), ("group", (5, 6))]


def test_layer_over_group_max_bytes_in_the_middle_of_a_group():
    big = L.GROUP_MAX_BYTES + 1
    assert schedule(small(3) + [big] + small(6), 0, 6) == [
        ("group", (0, 1, 2)), ("alone", (3,)), ("group", (4, 5, 6, 7, 8, 9))]
    # exactly GROUP_MAX_BYTES still groups
    assert schedule([L.GROUP_MAX_BYTES] + small(1), 0, 6) == [("group", (0, 1))]


def test_byte_budget_closes_a_group_early():
    per = 100 * MB                    # four of them reach the 384 MB budget before the sixth layer
    assert per <= L.GROUP_MAX_BYTES and 3 * per < L.GROUP_BUDGET_BYTES <= 4 * per
    assert schedule([per] * 9, 0, 6) == [("group", (0, 1, 2, 3)), ("group", (4, 5, 6, 7)), ("group", (8,))]


@pytest.mark.parametrize("early_tail", [True, False])
def test_early_tail_at_the_stem(early_tail):
    got = schedule(small(8) + [None], 0, 6, early_tail=early_tail)
    if early_tail:      # the open group goes to the side stream underneath the stem's weight gradient
        assert got == [("group", (0, 1, 2, 3, 4, 5)), ("group", (6, 7)), ("inline", (8,))]
    else:               # ... or after it, at the phase's flush
        assert got == [("group", (0, 1, 2, 3, 4, 5)), ("inline", (8,)), ("group", (6, 7))]


def test_no_grouping():
    assert schedule(small(3) + [None], 0, 1) == [("alone", (0,)), ("alone", (1,)), ("alone", (2,)), ("inline", (3,))]


@pytest.mark.parametrize("defer", [True, False])
def test_phase_installs_the_reducer_and_always_restores(defer):
    r = HN.WGradReducer(defer=defer)
    outside = HN.WGRAD_DEFER
    with r.phase(torch.device("cpu"), phase_b=True):
        assert HN.WGRAD_DEFER is r and HN.MAIN_STREAM is None and r.first_group == L.FIRST_GROUP_B
    assert HN.WGRAD_DEFER is outside and r.first_group is None
    with pytest.raises(ValueError):
        with r.phase(torch.device("cpu")):
            raise ValueError("backward raised")
    assert HN.WGRAD_DEFER is outside and HN.MAIN_STREAM is None

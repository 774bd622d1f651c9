"""CPU: the convolution dispatcher answers every query over the grid of tests/conv_route_sweep.py as recorded in tests/golden/conv_routes.json.

The file was recorded (scripts/record_conv_routes.py) from the commit before the dispatcher's rules moved into route_fwd / route_wgrad; a rule
that changes in the launch changes in every query with it, and this test says on the CPU which option set and storage type moved.  The compute-unit
count falls back to 256 without a device and is 256 on an MI355X, so the digests hold on both."""
import ctypes
import json
import os

import pytest

import conv_route_sweep as S


@pytest.fixture(scope="module")
def lib():
    from simpledepthestimation_amd.hip import lib as L
    return S.bind(L.lib())


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_routes.json")) as f:
        return json.load(f)


def test_every_answer_of_the_grid_is_the_recorded_one(lib, golden):
    got, defaults = S.digests(lib)
    assert set(got) == set(golden["digests"]) == {name for name, _, _ in S.OPTION_SETS}
    moved = [(name, dt) for name in got for dt in got[name] if got[name][dt] != golden["digests"][name].get(dt)]
    assert not moved, f"answers moved for (option set, dtype) {moved}: scripts/record_conv_routes.py --against OLD_LIBRARY names the descriptors"
    assert S.histogram(defaults) == golden["histogram"]


def test_recorded_grid_exercises_every_kernel_and_rule(golden):
    h = golden["histogram"]
    assert h["refused"] == 0 and h["descriptors"] > 0
    short = {name: h[name] for name in S.COVER if h[name] < S.MIN_COVER}
    assert not short, f"fewer than {S.MIN_COVER} descriptors of the grid take {short}"


def _refused_descriptors():
    ok = dict(dtype=S.BF16, mode=0, B=2, H0=16, W0=16, C0=64, C1=0, IH=16, IW=16, k=3, stride=1, pad=1, reflect=0)
    no_source = S.make_desc(**ok)
    no_source.x0 = None
    bad_dtype = S.make_desc(**dict(ok, dtype=7))
    ragged_channels = S.make_desc(**dict(ok, C0=60))
    wrong_extent = S.make_desc(**dict(ok, IH=17))
    return {"null": None, "no source": no_source, "bad dtype": bad_dtype, "channels off the 16-byte group": ragged_channels,
            "plain source of another size": wrong_extent}


@pytest.mark.parametrize("case", list(_refused_descriptors()))
def test_queries_answer_zero_with_a_reason_for_a_descriptor_the_launch_refuses(lib, case):
    d = _refused_descriptors()[case]
    r = ctypes.byref(d) if d is not None else None
    calls = {"sde_conv_fwd_variant": (r, 64), "sde_conv_fwd_tiles_m": (r, 64), "sde_conv_fwd_ws_bytes": (r, 64), "sde_conv_dgrad_bnbwd_rows": (r, 64, 64),
             "sde_conv_dgrad_bnbwd_res_rows": (r, 64, 64), "sde_conv_wgrad_variant": (r, 64, 64), "sde_conv_wgrad_splits": (r, 64)}
    assert set(calls) == set(S.QUERIES)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == 0, name
        reason = lib.sde_last_error().decode()       # (the last error is never cleared: the reason has to be this query's own)
        assert reason.startswith(name + ":"), f"{name} left {reason!r}"

"""GPU: sde_depth_warp_fuse.  Every case is compared bit for bit with the host twin (hip/temporal.py: warp_fuse_host) and, outside the pixels an
undecided source can reach, with the float64 restatement of temporal_ref.py within its per-element bounds; every destination sits between
guard bytes."""
import functools

import numpy as np
import pytest
import torch

import temporal_ref as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5
GUARD = 64


@functools.lru_cache(maxsize=None)
def reference(name):
    """Inputs, restatement and the twin's result of one case: computed once, shared, never modified."""
    from simpledepthestimation_amd.hip.temporal import warp_fuse_host
    inp = TR.case_inputs(name)
    return inp, TR.restate(**inp), warp_fuse_host(**inp)


def on_device(inp):
    return {k: (torch.from_numpy(v).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in inp.items()}


def guarded(shape, dtype):
    """A destination with guard bytes on both sides, everything filled with FILL: (the whole buffer, the destination view)."""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD:GUARD + nbytes].view(dtype).view(shape)


def run(inp, want_state=True, want_warped=True, alias=None):
    """-> (fused, state, warped) host arrays (None when not asked for); the guards of every destination are checked.  alias: "prev" or "cur",
    the input that is also the destination of `fused`."""
    from simpledepthestimation_amd.hip.temporal import warp_fuse
    d = on_device(inp)
    shape = tuple(inp["prev"].shape)
    bufs = [guarded(shape, t) for t in (torch.float32, torch.uint8, torch.float32, torch.int32)]
    if alias is not None:
        bufs[0][1].copy_(d[alias])
        d[alias] = bufs[0][1]
    fused, state, warped = warp_fuse(d["prev"], d["cur"], d["K"], d["T"], motion=d["motion"], alpha=inp["alpha"], tol=inp["tol"], out=bufs[0][1],
                                     want_state=want_state, want_warped=want_warped, zbuf=bufs[3][1], state=bufs[1][1] if want_state else None,
                                     warped=bufs[2][1] if want_warped else None)
    torch.cuda.synchronize()
    res = []
    for (buf, view), o, w in zip(bufs[:3], (fused, state, warped), (True, want_state, want_warped)):
        raw = buf.cpu().numpy()
        assert bool((raw[:GUARD] == FILL).all() and (raw[-GUARD:] == FILL).all()), "bytes outside a destination were written"
        if w:
            assert o.data_ptr() == view.data_ptr()
            res.append(view.cpu().numpy())
        else:
            assert o is None and bool((raw == FILL).all()), "an output that was not asked for was written"
            res.append(None)
    raw = bufs[3][0].cpu().numpy()
    assert bool((raw[:GUARD] == FILL).all() and (raw[-GUARD:] == FILL).all()), "bytes outside the z-buffer were written"
    return res


def same_bits(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("name", TR.CASES)
def test_warp_fuse(name):
    inp, want, twin = reference(name)
    got = run(inp)
    TR.compare(got, want, inp["cur"], name)
    for g, t, what in zip(got, twin, ("fused", "state", "warped")):
        differing = int((np.ascontiguousarray(g).view(np.uint8) != np.ascontiguousarray(t).view(np.uint8)).sum())
        print(f"  {what}: {differing} bytes differ from the host twin")
        assert g.tobytes() == t.tobytes(), what
    if name == "several_workgroups":
        assert inp["prev"].size > 4 * 256 and inp["prev"].shape[1] * inp["prev"].shape[2] % 256 != 0          # more than one workgroup, a ragged last one
    if name == "two_poses":
        assert not inp["motion"][0].any() and inp["motion"][1].any() and not np.array_equal(inp["T"][0], inp["T"][1])


def test_grid_stride():
    """600 x 900 pixels are more than the 2048 workgroups of 256 that a launch is capped at: every kernel walks its grid-stride loop."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "simpledepthestimation_amd", "csrc", "temporal.hip")).read()
    tile, cap = (int(re.search(r"constexpr int %s = (\d+);" % k, src).group(1)) for k in ("TILE", "MAX_BLOCKS"))
    inp, want, twin = reference("grid_stride")
    assert inp["prev"].size > tile * cap
    got = run(inp)
    TR.compare(got, want, inp["cur"], "grid_stride")
    assert same_bits(got, twin)


def test_fused_may_alias_either_input():
    inp, _, twin = reference("several_workgroups")
    for alias in ("prev", "cur"):
        assert same_bits(run(inp, alias=alias), twin), alias


def test_two_runs_give_equal_bytes_and_unrequested_outputs_stay_untouched():
    inp, _, twin = reference("two_poses")
    a, b = run(inp), run(inp)
    assert same_bits(a, b) and same_bits(a, twin)
    for want_state, want_warped in ((False, False), (True, False), (False, True)):
        got = run(inp, want_state=want_state, want_warped=want_warped)            # run() checks the sentinels of what was left out
        assert got[0].tobytes() == a[0].tobytes()
        assert (got[1] is None) == (not want_state) and (got[1] is None or got[1].tobytes() == a[1].tobytes())
        assert (got[2] is None) == (not want_warped) and (got[2] is None or got[2].tobytes() == a[2].tobytes())


def test_capturable_with_state_in_place():
    """A graph of the call with fused = prev, replayed twice, equals two eager calls: the state moves on with every replay."""
    from simpledepthestimation_amd.hip.temporal import warp_fuse, warp_fuse_host
    inp, _, _ = reference("several_workgroups")
    d = on_device(inp)
    kw = dict(motion=d["motion"], alpha=inp["alpha"], tol=inp["tol"])
    eager = d["prev"].clone()
    states = []
    for _ in range(2):
        _, st, _ = warp_fuse(eager, d["cur"], d["K"], d["T"], out=eager, **kw)
        states.append(st.clone())
    state = d["prev"].clone()
    zbuf, st_g = torch.empty(state.shape, dtype=torch.int32, device=DEV), torch.empty(state.shape, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        warp_fuse(state, d["cur"], d["K"], d["T"], out=state, zbuf=zbuf, state=st_g, **kw)
    for k in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(st_g, states[k]), k
    assert torch.equal(state, eager)
    once = warp_fuse_host(**inp)
    twice = warp_fuse_host(once[0], inp["cur"], inp["K"], inp["T"], inp["motion"], inp["alpha"], inp["tol"])
    assert state.cpu().numpy().tobytes() == twice[0].tobytes() and states[1].cpu().numpy().tobytes() == twice[1].tobytes()


def test_binding_refuses_what_the_library_would():
    from simpledepthestimation_amd.hip import lib as L
    from simpledepthestimation_amd.hip.temporal import warp_fuse
    inp, _, _ = reference("odd_sizes")
    d = on_device(inp)
    with pytest.raises(ValueError):
        warp_fuse(d["prev"], d["cur"], d["K"], d["T"], alpha=1.0)
    with pytest.raises(ValueError):
        warp_fuse(d["prev"], d["cur"], d["K"], d["T"], tol=0.0)
    with pytest.raises(L.SdeHipError):
        warp_fuse(d["prev"], d["cur"], d["K"], d["T"][:, :3])
    with pytest.raises(L.SdeHipError):
        warp_fuse(d["prev"], d["cur"][:, :, :-1].contiguous(), d["K"], d["T"])

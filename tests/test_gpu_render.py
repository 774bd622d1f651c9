"""GPU: sde_tsdf_render.  Every case of render_ref.py is compared bit for bit with the host twin (hip/volume.py: render_host, the full march) and,
outside the pixels whose outcome hangs on a rounding, with the float64 restatement within its a-priori bounds; the destinations and the
volume's arrays sit between guard bytes, and the destinations are pre-filled so that a miss has to be written."""
import functools

import numpy as np
import pytest
import torch

import render_ref as RR
from test_gpu_volume import DEV, FILL, guarded, guards_intact, make_volume, read_back

pytestmark = pytest.mark.gpu


def volume_of(inp):
    nz, ny, nx = inp["tsdf"].shape
    vol = dict(dims=(nx, ny, nz), voxel=float(inp["voxel"]), origin=tuple(float(o) for o in inp["origin"]))
    colour = inp["rgba"] is not None
    return make_volume(vol, colour, state=(inp["tsdf"], inp["weight"], inp["rgba"]))


def render(inp, v, normals=True, picture=None, out=None):
    """One launch into guarded, pre-filled destinations -> (depth, normal or None, picture or None) host arrays; the destinations' guards checked."""
    H, W = inp["size"]
    picture = (inp["rgba"] is not None) if picture is None else picture
    bufs = [guarded((H, W), torch.float32), guarded((H, W, 3), torch.float32) if normals else (None, None),
            guarded((H, W, 4), torch.uint8) if picture else (None, None)]
    K, C = torch.from_numpy(inp["K"]).to(DEV), torch.from_numpy(inp["C"]).to(DEV)
    far = float(inp["near"]) + (inp["n"] - 0.5) * float(inp["step"])                 # ceil((far - near) / step) = n
    got = v.render(K, C, inp["size"], near=inp["near"], far=far, step=inp["step"], min_weight=inp["min_weight"], normals=normals, picture=picture,
                   out=tuple(d for _, d in bufs))
    torch.cuda.synchronize()
    assert all(g is d or (g is None and d is None) for g, (_, d) in zip(got, bufs))
    assert all(b is None or guards_intact(b) for b, _ in bufs), "bytes outside a destination were written"
    return tuple(None if g is None else g.cpu().numpy() for g in got)


@functools.lru_cache(maxsize=None)
def reference(name):
    """Inputs, restatement and the twin's result of one case: computed once, shared, never modified."""
    from simpledepthestimation_amd.hip.volume import render_host
    inp = RR.case_inputs(name)
    twin = render_host(inp["tsdf"], inp["weight"], inp["rgba"], inp["K"], inp["C"], inp["size"], inp["origin"], inp["voxel"], inp["near"], inp["step"],
                       inp["n"], inp["min_weight"])
    return inp, RR.restate(inp), twin


def same_bits(a, b):
    return all((x is None and y is None) or (x is not None and y is not None and x.tobytes() == y.tobytes()) for x, y in zip(a, b))


@pytest.mark.parametrize("name", RR.CASES)
def test_render(name):
    from simpledepthestimation_amd.hip.volume import check_render
    inp, want, twin = reference(name)
    v, vbufs = volume_of(inp)
    state = read_back(v, vbufs)
    got = render(inp, v)
    RR.compare(got, want, name)
    for g, t, what in zip(got, twin, ("depth", "normal", "picture")):
        if g is not None:
            print(f"  {what}: {int((g.view(np.uint8) != t.view(np.uint8)).sum())} bytes differ from the host twin")
            assert g.tobytes() == t.tobytes(), what
    assert got[2] is not None or inp["rgba"] is None
    assert same_bits(read_back(v, vbufs), state)                                      # the volume is read only, and nothing was written around it
    miss = got[0] == 0
    assert not got[1][miss].any() and (got[2] is None or not got[2][miss].any())      # the 0xA5 fill is gone from every miss
    hits = int((~miss).sum())
    if name in ("all_miss", "flat_dims") or name in RR.BAD_POSE:
        assert hits == 0
    elif name == "camera_inside":
        assert hits == miss.size
    else:
        assert 0 < hits < miss.size
    if name == "zero_sample":                                                         # t == 0 hits, at one whole step behind the sample in front; a flat cell: no normal
        assert bool((got[0][~miss] == got[0][~miss][0]).all()) and not got[1].any()
    if name == "beyond_far":
        assert inp["n"] == 3 and int((want["index"] == 1).sum()) > 0


@pytest.mark.parametrize("name", ["oblique_plane", "holes"])
def test_optional_outputs_absent(name):
    inp, _, twin = reference(name)
    v, _ = volume_of(inp)
    for normals, picture in ((False, False), (True, False), (False, True)):
        got = render(inp, v, normals=normals, picture=picture)
        assert (got[1] is None) == (not normals) and (got[2] is None) == (not picture)
        assert same_bits(got, (twin[0], twin[1] if normals else None, twin[2] if picture else None))


def test_second_call_and_graph_replays_give_the_same_bytes():
    inp, _, twin = reference("integrated")
    v, vbufs = volume_of(inp)
    H, W = inp["size"]
    first, second = render(inp, v), render(inp, v)
    assert same_bits(first, twin) and same_bits(second, twin)
    K, C = torch.from_numpy(inp["K"]).to(DEV), torch.from_numpy(inp["C"]).to(DEV)
    out = (torch.empty((H, W), dtype=torch.float32, device=DEV), torch.empty((H, W, 3), dtype=torch.float32, device=DEV),
           torch.empty((H, W, 4), dtype=torch.uint8, device=DEV))
    far = float(inp["near"]) + (inp["n"] - 0.5) * float(inp["step"])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        v.render(K, C, inp["size"], near=inp["near"], far=far, step=inp["step"], min_weight=inp["min_weight"], out=out)
    for _ in range(2):
        for o in out:
            o.fill_(FILL)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(tuple(o.cpu().numpy() for o in out), twin)
    read_back(v, vbufs)


def test_points_before_and_after_a_render_agree():
    inp, _, _ = reference("holes")
    v, vbufs = volume_of(inp)
    before = [x.cpu().numpy().copy() for x in v.points()]
    render(inp, v)
    after = [x.cpu().numpy() for x in v.points()]
    assert int(before[1][0]) > 0 and all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    read_back(v, vbufs)


def test_binding_refuses_what_the_library_would():
    from simpledepthestimation_amd.hip import lib as L
    inp, _, _ = reference("no_colour")
    v, _ = volume_of(inp)
    K, C = torch.from_numpy(inp["K"]).to(DEV), torch.from_numpy(inp["C"]).to(DEV)
    with pytest.raises(ValueError):
        v.render(K, C, inp["size"])                                                   # picture=True on a volume without colour
    with pytest.raises(ValueError):
        v.render(K, C, inp["size"], picture=False, near=0.0, far=1.0, step=1e-6)       # 10^6 samples
    with pytest.raises(ValueError):
        v.render(K, C, inp["size"], picture=False, min_weight=0)
    with pytest.raises(L.SdeHipError):
        v.render(K, C[:3], inp["size"], picture=False)
    with pytest.raises(L.SdeHipError):
        v.render(K.cpu(), C, inp["size"], picture=False)
    with pytest.raises(L.SdeHipError):
        v.render(K, C, inp["size"], picture=False, out=(torch.empty((3, 3), dtype=torch.float32, device=DEV), None, None))
    lib = L.lib()
    H, W = inp["size"]
    depth = torch.empty((H, W), dtype=torch.float32, device=DEV)
    nx, ny, nz = v.dims
    call = lambda n, step, near, pic: lib.sde_tsdf_render(L.ptr(v.tsdf), L.ptr(v.weight), None, nx, ny, nz, v._origin, v.voxel, 1.0, L.ptr(K), L.ptr(C), H, W, near,
                                                          step, n, L.ptr(depth), None, pic, L.stream())
    assert call(10, 0.1, 0.5, None) == 0
    for bad in ((0, 0.1, 0.5, None), (65537, 0.1, 0.5, None), (10, 0.0, 0.5, None), (10, float("nan"), 0.5, None), (10, 0.1, float("inf"), None),
                (10, 0.1, 0.5, L.ptr(depth))):
        assert call(*bad) != 0, bad
    torch.cuda.synchronize()

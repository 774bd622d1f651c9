"""GPU: sde_tsdf_mesh.  Every case is compared bit for bit with the host twin (hip/volume.py: mesh_host), which tests/test_mesh.py holds against
the float64 restatement of mesh_ref.py; the small cases meet that restatement here too.  Every destination and the workspace sit between guard
bytes, and the slots behind the written entries keep their fill."""
import functools
import re

import numpy as np
import pytest
import torch

import mesh_ref as MR
import volume_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5
GUARD = 64


def guarded(shape, dtype):
    """A destination with guard bytes on both sides, everything filled with FILL: (the whole buffer, the destination view)."""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD:GUARD + nbytes].view(dtype).view(shape)


def guards_intact(buf):
    raw = buf.cpu().numpy()
    return bool((raw[:GUARD] == FILL).all() and (raw[-GUARD:] == FILL).all())


def make_volume(inp, colour=True):
    """A TsdfVolume holding the case's arrays between guard bytes -> (volume, the guarded buffers)."""
    from simpledepthestimation_amd.hip.volume import TsdfVolume
    nz, ny, nx = inp["tsdf"].shape
    v = TsdfVolume((nx, ny, nz), float(inp["voxel"]), origin=tuple(float(o) for o in inp["origin"]), colour=colour, device=DEV)
    bufs = [guarded((nz, ny, nx), torch.float32), guarded((nz, ny, nx), torch.float32)] + ([guarded((nz, ny, nx, 4), torch.uint8)] if colour else [])
    v.tsdf, v.weight = bufs[0][1], bufs[1][1]
    v.tsdf.copy_(torch.from_numpy(inp["tsdf"]))
    v.weight.copy_(torch.from_numpy(inp["weight"]))
    if colour:
        v.rgba = bufs[2][1]
        v.rgba.copy_(torch.from_numpy(inp["rgba"]))
    return v, [b for b, _ in bufs]


@functools.lru_cache(maxsize=None)
def twin(name, colour=True):
    """Inputs and the twin's full result of one case: computed once, shared, never modified."""
    from simpledepthestimation_amd.hip.volume import mesh_host
    inp = MR.mesh_inputs(name)
    return inp, mesh_host(inp["tsdf"], inp["weight"], inp["rgba"] if colour else None, inp["origin"], inp["voxel"], inp["min_weight"])


def run_mesh(inp, room, colour=True, ws_byte=None, volume=None):
    """One call with room = (vertices, faces) -> (vertex records, faces, count as a list, raw vertices [room,16], raw faces [room,3]); the
    volume's arrays, the three destinations and the workspace lie between guard bytes, which are checked."""
    from simpledepthestimation_amd.hip.cloud import as_records
    v, bufs = volume if volume is not None else make_volume(inp, colour)
    before = [b.clone() for b in bufs]
    vbuf, vertices = guarded((room[0], 16), torch.uint8)
    fbuf, faces = guarded((room[1], 3), torch.int32)
    cbuf, count = guarded((2,), torch.int32)
    wbuf, ws = guarded((v.mesh_workspace_numel(),), torch.int32)
    if ws_byte is not None:
        ws.view(torch.uint8).fill_(ws_byte)
    out = v.mesh(min_weight=inp["min_weight"], cap_vertices=room[0], cap_faces=room[1], out=(vertices, faces, count), workspace=ws)
    torch.cuda.synchronize()
    assert [o.data_ptr() for o in out] == [vertices.data_ptr(), faces.data_ptr(), count.data_ptr()]
    assert all(guards_intact(b) for b in (vbuf, fbuf, cbuf, wbuf)), "bytes outside a destination or the workspace were written"
    assert all(torch.equal(a, b) for a, b in zip(before, bufs)), "the volume was written"
    n = [int(c) for c in count.cpu()]
    raw_v, raw_f = vertices.cpu().numpy(), faces.cpu().numpy()
    return as_records(raw_v, min(n[0], room[0])), raw_f[:min(n[1], room[1])], n, raw_v, raw_f


def untouched_behind(raw, n):
    return bool((raw[n:].view(np.uint8) == FILL).all())


@pytest.mark.parametrize("name", MR.CASES)
def test_mesh(name):
    inp, (rec_t, faces_t, count_t) = twin(name)
    nv, nf = (int(c) for c in count_t)
    rec, faces, count, raw_v, raw_f = run_mesh(inp, (nv + 3, nf + 3))
    MR.compare_mesh(rec, faces, count, MR.restate_mesh(**inp), label=name)
    assert count == [nv, nf] and rec.tobytes() == rec_t.tobytes() and faces.tobytes() == faces_t.tobytes()
    assert untouched_behind(raw_v, nv) and untouched_behind(raw_f, nf)
    if name == "dim_of_one":
        assert count == [0, 0]
    if name == "three_tiles":
        tile, _ = VR.launch_limits()
        assert -(-inp["tsdf"].size // tile) == 3 and inp["tsdf"].size % tile != 0


@pytest.mark.parametrize("name", ["random", "three_tiles"])
def test_the_workspace_contents_do_not_matter(name):
    inp, (rec_t, faces_t, count_t) = twin(name)
    room = (int(count_t[0]) + 2, int(count_t[1]) + 2)
    for byte in (0x00, 0xFF):
        rec, faces, count, raw_v, raw_f = run_mesh(inp, room, ws_byte=byte)
        assert count == count_t.tolist() and rec.tobytes() == rec_t.tobytes() and faces.tobytes() == faces_t.tobytes(), hex(byte)
        assert untouched_behind(raw_v, count[0]) and untouched_behind(raw_f, count[1])


def test_grid_stride_and_the_scan_carry():
    """More voxels than TILE * MAX_BLOCKS and more tiles than one chunk of the scan; the wavy surface crosses many tile borders."""
    tile, blocks = VR.launch_limits()
    inp, (rec_t, faces_t, count_t) = twin("grid_stride")
    rows = int(re.search(r"constexpr int SCAN_ROWS = (\d+);", open(VR._SRC).read()).group(1))
    assert inp["tsdf"].size > tile * blocks and inp["tsdf"].size // tile > rows * tile
    nv, nf = (int(c) for c in count_t)
    assert nv > 10000 and nf > 20000
    rec, faces, count, raw_v, raw_f = run_mesh(inp, (nv + 5, nf + 5))
    assert count == [nv, nf] and rec.tobytes() == rec_t.tobytes() and faces.tobytes() == faces_t.tobytes()
    assert untouched_behind(raw_v, nv) and untouched_behind(raw_f, nf)
    from simpledepthestimation_amd.hip.volume import crossings_np
    with_crossing = np.flatnonzero(crossings_np(inp["tsdf"], inp["weight"], inp["min_weight"]).any(-1))
    assert np.unique(with_crossing // tile).size > blocks // 8 and with_crossing.max() > tile * blocks          # many tiles, also in the second trip


def test_overflow_of_both_lists_no_colour_and_two_runs():
    inp, (rec_t, faces_t, count_t) = twin("three_tiles")
    nv, nf = (int(c) for c in count_t)
    for cv, cf in ((nv // 3, nf // 3), (nv + 2, nf // 2 + 1), (1, nf + 2), (nv // 2, 1)):     # an odd face cap cuts a quad in two
        rec, faces, count, raw_v, raw_f = run_mesh(inp, (cv, cf))                      # the guards sit right behind the cap-th entries
        assert count == [nv, nf], (cv, cf)
        assert rec.tobytes() == rec_t[:cv].tobytes() and faces.tobytes() == faces_t[:cf].tobytes(), (cv, cf)
    assert int(faces_t.max()) > nv // 2                                                # the run with room for one vertex wrote the true numbers of all
    plain_inp, (rec_p, faces_p, count_p) = twin("three_tiles", colour=False)
    rec, faces, count, _, _ = run_mesh(inp, (nv, nf), colour=False)
    assert count == [nv, nf] and rec.tobytes() == rec_p.tobytes() and faces.tobytes() == faces_t.tobytes()
    assert not rec["red"].any() and not rec["green"].any() and not rec["blue"].any() and bool((rec["alpha"] == 255).all())
    a, b = run_mesh(inp, (nv, nf)), run_mesh(inp, (nv, nf))
    assert a[2] == b[2] and a[3].tobytes() == b[3].tobytes() and a[4].tobytes() == b[4].tobytes() and a[0].tobytes() == rec_t.tobytes()


def test_points_are_the_same_before_and_after_the_mesh():
    from simpledepthestimation_amd.hip.volume import points_host
    inp, (rec_t, faces_t, count_t) = twin("random")
    want, total = points_host(**inp)
    vol = make_volume(inp)
    v = vol[0]
    p0, c0 = v.points(min_weight=inp["min_weight"], cap=total + 2)
    run_mesh(inp, (int(count_t[0]), int(count_t[1])), volume=vol)
    p1, c1 = v.points(min_weight=inp["min_weight"], cap=total + 2)
    torch.cuda.synchronize()
    assert int(c0.item()) == int(c1.item()) == total and p0[:total].cpu().numpy().tobytes() == p1[:total].cpu().numpy().tobytes() == want.tobytes()


def test_capturable():
    """integrate + mesh in one graph, replayed twice, equal two eager rounds: the volume moves on with every replay and the mesh follows."""
    vol, frames = VR.case_inputs("two_frames")
    from simpledepthestimation_amd.hip import present as HP
    from simpledepthestimation_amd.hip.volume import TsdfVolume
    fr = frames[1]
    d = {k: torch.from_numpy(fr[k]).to(DEV) for k in ("pred", "K", "C", "frame")}
    results = []
    for use_graph in (False, True):
        v = TsdfVolume(vol["dims"], vol["voxel"], origin=vol["origin"], trunc=vol["trunc"], max_weight=vol["max_weight"], min_depth=vol["min_depth"],
                       max_depth=vol["max_depth"], device=DEV)
        ymap, xmap = torch.from_numpy(fr["ymap"]).to(DEV), torch.from_numpy(fr["xmap"]).to(DEV)
        cv, cf = v.default_mesh_caps()
        out = (torch.zeros((cv, 16), dtype=torch.uint8, device=DEV), torch.zeros((cf, 3), dtype=torch.int32, device=DEV),
               torch.zeros(2, dtype=torch.int32, device=DEV))
        ws = torch.empty(v.mesh_workspace_numel(), dtype=torch.int32, device=DEV)

        def chain():
            v.integrate(d["pred"], ymap, xmap, d["K"], d["C"], frame=d["frame"])
            v.mesh(out=out, workspace=ws)
        if use_graph:
            HP.ensure_checked(ymap, xmap, *fr["pred"].shape, torch.device(DEV))         # the one validation of a device pair, outside the capture
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                chain()
            g.replay()
            g.replay()
        else:
            chain()
            chain()
        torch.cuda.synchronize()
        results.append([t.cpu().numpy() for t in (v.tsdf, v.weight, v.rgba) + out])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(*results))
    assert int(results[0][5][0]) > 0 and int(results[0][5][1]) > 0 and float(results[0][1].max()) == 2


def test_binding_refuses_what_the_library_would():
    from simpledepthestimation_amd.hip import lib as L
    inp, _ = twin("one_cell")
    v, _ = make_volume(inp)
    for kw in (dict(min_weight=0), dict(min_weight=float("nan")), dict(cap_vertices=0), dict(cap_faces=0), dict(cap_vertices=1 << 31), dict(cap_faces=1 << 31)):
        with pytest.raises(ValueError):
            v.mesh(**kw)
    ok = lambda: (torch.empty((4, 16), dtype=torch.uint8, device=DEV), torch.empty((4, 3), dtype=torch.int32, device=DEV),
                  torch.empty(2, dtype=torch.int32, device=DEV))
    v.mesh(cap_vertices=4, cap_faces=4, out=ok())
    for at, bad in ((0, torch.empty((4, 8), dtype=torch.uint8, device=DEV)), (0, torch.empty((4, 16), dtype=torch.uint8)),
                    (1, torch.empty((4, 3), dtype=torch.int64, device=DEV)), (1, torch.empty((3, 4), dtype=torch.int32, device=DEV)),
                    (2, torch.empty(1, dtype=torch.int32, device=DEV))):
        out = list(ok())
        out[at] = bad
        with pytest.raises(L.SdeHipError):
            v.mesh(cap_vertices=4, cap_faces=4, out=tuple(out))
    for ws in (torch.empty(v.mesh_workspace_numel() - 1, dtype=torch.int32, device=DEV), torch.empty(64, dtype=torch.float32, device=DEV),
               torch.empty(64, dtype=torch.int32), np.zeros(64, np.int32)):
        with pytest.raises(L.SdeHipError):
            v.mesh(cap_vertices=4, cap_faces=4, workspace=ws)
    torch.cuda.synchronize()


def test_save_mesh_runs_again_with_the_counted_room(tmp_path):
    from simpledepthestimation_amd.hip.volume import read_mesh_ply
    inp, (rec_t, faces_t, count_t) = twin("sphere8")
    v, _ = make_volume(inp)
    nv, nf = (int(c) for c in count_t)
    for caps in ((None, None), (nv // 2, None), (None, nf // 2), (1, 1)):
        path = str(tmp_path / "mesh.ply")
        assert v.save_mesh(path, min_weight=inp["min_weight"], cap_vertices=caps[0], cap_faces=caps[1]) == (nv, nf)
        rec, faces = read_mesh_ply(path)
        assert rec.tobytes() == rec_t.tobytes() and faces.tobytes() == faces_t.tobytes(), caps


def test_demo_tool_mesh(tmp_path):
    """The tool end to end with --pairs --volume --save-mesh on six generated frames: volume_mesh.ply read back is the device's mesh of the
    volume the same stream fills, and volume.ply is written as before."""
    import yaml
    from PIL import Image
    from test_gpu_temporal_stream import K_SRC, NET_H, NET_W, sequence
    from test_gpu_volume_stream import DIMS, volume_params
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.engine.predictor import PairPredictor
    from simpledepthestimation_amd.hip.cloud import as_records
    from simpledepthestimation_amd.hip.volume import TsdfVolume, mesh_host, read_mesh_ply
    from simpledepthestimation_amd.tools import demo
    src, dst = tmp_path / "frames", tmp_path / "out"
    src.mkdir()
    frames = sequence(6, seed=8)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(src / f"f{i:02d}.png")
    conf = {"MODEL": {"META_ARCHITECTURE": "MonoDepth2Model", "DEVICE": DEV, "POSE_NET": {"NAME": "PoseNet", "NUM_CONTEXTS": 2}},
            "DATASETS": {"TEST": {"PREPROCESS": [{"NAME": "LoadImg"}, {"NAME": "Resize", "IMG_H": NET_H, "IMG_W": NET_W}, {"NAME": "ToTensor"}]}}}
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(conf))
    cfg = get_cfg()
    cfg.set_new_allowed(True)
    cfg.merge_from_file(str(tmp_path / "config.yaml"))
    torch.manual_seed(7)
    pp = PairPredictor(cfg)
    p = volume_params(pp, frames)
    k = [str(v) for v in (K_SRC[0, 0], K_SRC[1, 1], K_SRC[0, 2], K_SRC[1, 2])]
    torch.manual_seed(7)
    assert demo.main(["--cfg", str(tmp_path / "config.yaml"), "--input", str(src), "--output", str(dst), "--pairs", "--intrinsics"] + k +
                     ["--volume"] + [str(n) for n in DIMS] + ["--voxel", repr(p["voxel"]), "--volume-origin"] + [repr(float(o)) for o in p["origin"]] +
                     ["--min-weight", "2", "--save-mesh"]) == 0
    assert sorted(q.name for q in dst.iterdir()) == sorted([f"f{i:02d}.png" for i in range(1, 5)] + ["volume.ply", "volume_mesh.ply"])
    v = TsdfVolume(DIMS, p["voxel"], origin=p["origin"], min_depth=float(cfg.MODEL.get("MIN_DEPTH", 0.0)), max_depth=float(cfg.MODEL.MAX_DEPTH), device=DEV)
    assert len(list(pp.stream(iter(frames), K_SRC, volume=v))) == 4
    v.save_ply(str(tmp_path / "want.ply"), min_weight=2)
    assert (dst / "volume.ply").read_bytes() == (tmp_path / "want.ply").read_bytes()
    vertices, faces, count = v.mesh(min_weight=2)
    nv, nf = (int(c) for c in count.cpu())
    assert nv > 0 and nf > 0 and nv <= vertices.shape[0] and nf <= faces.shape[0]
    rec, tri = read_mesh_ply(str(dst / "volume_mesh.ply"))
    assert rec.tobytes() == as_records(vertices, nv).tobytes() and tri.tobytes() == faces[:nf].cpu().numpy().tobytes()
    host = mesh_host(v.tsdf.cpu().numpy(), v.weight.cpu().numpy(), v.rgba.cpu().numpy(), v.origin, v.voxel, min_weight=2)
    assert host[2].tolist() == [nv, nf] and host[0].tobytes() == rec.tobytes() and host[1].tobytes() == tri.tobytes()

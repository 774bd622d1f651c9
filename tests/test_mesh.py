"""CPU: the host twin of the triangle mesh (hip/volume.py: mesh_host) against the float64 restatement of mesh_ref.py -- positions within its
a-priori bounds; counts, numbering, indices and colours exactly --, the topology of closed and open surfaces, the cross-check with points_host,
caps, the argument refusals of the C side and of the host, the PLY round trip and save_mesh's second run.  No GPU."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mesh_ref as MR
import volume_ref as VR
from simpledepthestimation_amd.hip import volume as HV
from simpledepthestimation_amd.hip.cloud import RECORD


@functools.lru_cache(maxsize=None)
def reference(name):
    """Inputs, restatement and the twin's result of one case: computed once, shared, never modified."""
    inp = MR.mesh_inputs(name)
    return inp, MR.restate_mesh(**inp), HV.mesh_host(**inp)


@pytest.mark.parametrize("name", MR.CASES)
def test_twin_against_the_restatement(name):
    inp, want, (rec, faces, count) = reference(name)
    MR.compare_mesh(rec, faces, count, want, label=name)
    assert count.dtype == np.int32 and rec.dtype == RECORD
    nv = rec.size
    assert faces.size == 0 or (0 <= int(faces.min()) and int(faces.max()) < nv)
    nz, ny, nx = inp["tsdf"].shape
    if name == "dim_of_one":                                # no cells at all
        assert min(nx, ny, nz) == 1 and count.tolist() == [0, 0]
    if name == "one_cell":                                  # at most a vertex, never a face
        assert count[0] <= 1 and count[1] == 0
    if name == "three_tiles":                               # rows that are no multiple of the wave, three tiles
        tile, _ = VR.launch_limits()
        assert nx % 64 != 0 and -(-inp["tsdf"].size // tile) == 3 and count[0] > 0 and count[1] > 0
    if name == "random":
        assert count[0] > 100 and count[1] > 100 and bool((inp["tsdf"] == 0).any()) and bool((inp["weight"] < inp["min_weight"]).any())


@pytest.mark.parametrize("name", sorted(MR.SPHERES))
def test_a_sphere_is_closed_oriented_and_near_the_analytic_one(name):
    inp, want, (rec, faces, count) = reference(name)
    _, r, c = MR.SPHERES[name]
    und, dirs = MR.undirected_edges(faces), MR.directed_edges(faces)
    xyz = MR.positions(rec)
    vol = MR.signed_volume(xyz, faces)
    centre = np.array([MR.world(c[a], a) for a in range(3)])
    off = np.abs(np.linalg.norm(xyz - centre, axis=1) - r * float(MR.VOXEL)) / float(MR.VOXEL)
    print(f"{name}: {rec.size} vertices, {faces.shape[0]} triangles, {len(und)} edges, signed volume {vol:.6g} "
          f"(the ball's {4 / 3 * np.pi * (r * float(MR.VOXEL)) ** 3:.6g}), largest distance from the sphere {off.max():.3f} voxels")
    assert rec.size > 0 and faces.shape[0] > 0
    assert set(und.values()) == {2}                          # every undirected edge lies in exactly two triangles
    assert set(dirs.values()) == {1}                         # every directed edge appears once: consistently oriented
    assert MR.euler(rec.size, faces) == 2
    assert np.unique(faces).size == rec.size                 # no vertex without a triangle
    assert vol > 0
    assert bool(np.all(off <= 1.0))                          # a vertex lies inside its cell, and the cell holds a crossing


def test_a_plane_is_flat_and_faces_up():
    inp, want, (rec, faces, count) = reference("plane")
    nz, ny, nx = inp["tsdf"].shape
    assert count.tolist() == [(nx - 1) * (ny - 1), 2 * (nx - 2) * (ny - 2)]
    z = MR.world(MR.PLANE_Z0, 2)
    assert bool(np.all(np.abs(rec["z"].astype(np.float64) - z) <= want["bound"][:, 2]))
    assert bool(np.all(want["xyz"][:, 2] == want["xyz"][0, 2])) and abs(want["xyz"][0, 2] - z) < 1e-12          # the restatement lies ON the plane: f = 0.25 exactly
    n = MR.normals(MR.positions(rec), faces)
    assert bool(np.all(n[:, 2] > 0)) and bool(np.all(np.abs(n[:, :2]) <= 1e-6 * n[:, 2:3]))       # from negative to positive tsdf: +z


def crossing_edges(inp):
    """[(i, j, k, a)] of the crossings in the order of sde_tsdf_points, by loops."""
    nz, ny, nx = inp["tsdf"].shape
    valid, neg = inp["weight"] >= np.float32(inp["min_weight"]), inp["tsdf"] < 0
    out = []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                for a, (kn, jn, inn) in enumerate(((k, j, i + 1), (k, j + 1, i), (k + 1, j, i))):
                    if kn < nz and jn < ny and inn < nx and valid[k, j, i] and valid[kn, jn, inn] and neg[k, j, i] != neg[kn, jn, inn]:
                        out.append((i, j, k, a))
    return out


@pytest.mark.parametrize("name", ["sphere8", "random", "three_tiles"])
def test_the_mesh_connects_the_records_of_points_host(name):
    inp, want, (rec, faces, count) = reference(name)
    points, total = HV.points_host(**inp)
    edges = crossing_edges(inp)
    assert total == len(edges) == points.size
    nz, ny, nx = inp["tsdf"].shape
    dims = (nx, ny, nz)
    inner = [e for e in edges if all(1 <= e[b] <= dims[b] - 2 for b in MR.AXES[e[3]])]
    assert inner == want["quads"] and int(count[1]) == 2 * len(inner) == faces.shape[0]
    number = {tuple(c): n for n, c in enumerate(want["cells"].tolist())}
    # every face names the four cells around its edge
    for n, (i, j, k, a) in enumerate(inner):
        b, c = MR.AXES[a]
        around = set()
        for db, dc in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
            w = [i, j, k]
            w[b] += db
            w[c] += dc
            around.add(number[tuple(w)])
        assert set(faces[2 * n].tolist()) | set(faces[2 * n + 1].tolist()) == around and len(around) == 4
        assert faces[2 * n][0] == faces[2 * n + 1][0] and faces[2 * n][2] == faces[2 * n + 1][1]
    # every vertex is the mean of the points_host records on its cell's edges
    at = {e: n for n, e in enumerate(edges)}
    xyz = MR.positions(points)
    got = MR.positions(rec)
    for n, (i, j, k) in enumerate(want["cells"].tolist()):
        mine = [at[(i + d[0], j + d[1], k + d[2], a)] for a, d in MR.cell_edges() if (i + d[0], j + d[1], k + d[2], a) in at]
        assert mine, "a vertex in a cell without a crossing"
        assert bool(np.all(np.abs(xyz[mine].mean(0) - got[n]) <= 2 * want["bound"][n]))      # the records' own rounding is within the bound once more
        col = np.stack([points[ch][mine].astype(np.int64) for ch in ("red", "green", "blue")], 1).sum(0)
        assert [(2 * int(t) + len(mine)) // (2 * len(mine)) for t in col] == [int(rec[ch][n]) for ch in ("red", "green", "blue")]
    cells_without = (nx - 1) * (ny - 1) * (nz - 1) - len(number)
    print(f"{name}: {total} crossings, {len(inner)} with four cells around them, {len(number)} cells with a vertex, {cells_without} without")


def test_caps_below_the_totals():
    inp, want, (rec, faces, count) = reference("sphere8")
    nv, nf = (int(c) for c in count)
    for cv, cf in ((nv // 3, nf // 3), (1, 1), (nv, nf - 1), (nv + 5, nf // 2 + 1), (nv - 1, nf + 7)):
        r, f, c = HV.mesh_host(cap_vertices=cv, cap_faces=cf, **inp)
        MR.compare_mesh(r, f, c, want, cap_vertices=cv, cap_faces=cf, label=f"caps {cv}, {cf}")
        assert c.tolist() == [nv, nf] and r.size == min(cv, nv) and f.shape[0] == min(cf, nf)
        assert r.tobytes() == rec[:cv].tobytes() and f.tobytes() == faces[:cf].tobytes()      # the prefixes, with the true vertex numbers
    assert int(HV.mesh_host(cap_vertices=2, cap_faces=nf, **inp)[1].max()) == nv - 1


def test_without_colour():
    inp, want, (rec, faces, count) = reference("sphere8")
    r, f, c = HV.mesh_host(inp["tsdf"], inp["weight"], None, inp["origin"], inp["voxel"], inp["min_weight"])
    assert c.tolist() == count.tolist() and f.tobytes() == faces.tobytes()
    assert not r["red"].any() and not r["green"].any() and not r["blue"].any() and bool((r["alpha"] == 255).all())
    for ch in "xyz":
        assert r[ch].tobytes() == rec[ch].tobytes()


def test_workspace_query():
    from simpledepthestimation_amd.hip import lib as L
    lib = L.lib()
    tile, _ = VR.launch_limits()
    for dims in ((1, 1, 1), (5, 3, 2), (37, 5, 3), (256, 256, 128)):
        n = dims[0] * dims[1] * dims[2]
        assert lib.sde_tsdf_mesh_ws_bytes(*dims) == 4 * (2 * -(-n // tile) + n), dims
    for dims in ((0, 3, 2), (5, -1, 2), (1025, 1, 1), (1024, 1024, 1025)):
        assert lib.sde_tsdf_mesh_ws_bytes(*dims) == 0, dims


def test_refusals_precede_any_device_call():
    """Every refusal returns SDE_ERR_ARG with a message; the pointers are never followed (they point into host memory, and this runs without a GPU)."""
    from simpledepthestimation_amd.hip import lib as L
    lib = L.lib()
    host = (ctypes.c_float * 64)()
    base = ctypes.addressof(host)
    assert base % 16 == 0
    p = ctypes.c_void_p(base)
    origin = (ctypes.c_float * 3)(0, 0, 0)
    nan = float("nan")
    need = lib.sde_tsdf_mesh_ws_bytes(2, 2, 2)
    assert need == 4 * (2 + 8)

    def mesh(**kw):
        a = dict(tsdf=p, weight=p, rgba=None, nx=2, ny=2, nz=2, origin=origin, voxel=0.1, min_weight=1.0, ws=p, ws_bytes=need, vertices=p, cap_v=8, faces=p,
                 cap_f=8, count=p)
        a.update(kw)
        return lib.sde_tsdf_mesh(a["tsdf"], a["weight"], a["rgba"], a["nx"], a["ny"], a["nz"], a["origin"], a["voxel"], a["min_weight"], a["ws"], a["ws_bytes"],
                                 a["vertices"], a["cap_v"], a["faces"], a["cap_f"], a["count"], None)
    for kw in (dict(nx=0), dict(nz=2000), dict(nx=1024, ny=1024, nz=1025), dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=nan), dict(min_weight=0.5),
               dict(min_weight=nan), dict(cap_v=0), dict(cap_v=1 << 31), dict(cap_f=0), dict(cap_f=1 << 31), dict(tsdf=None), dict(weight=None),
               dict(origin=None), dict(vertices=None), dict(faces=None), dict(count=None), dict(ws=None), dict(ws_bytes=need - 1),
               dict(ws=ctypes.c_void_p(base + 2)), dict(vertices=ctypes.c_void_p(base + 8)), dict(faces=ctypes.c_void_p(base + 2)),
               dict(rgba=ctypes.c_void_p(base + 1))):
        assert mesh(**kw) == -1, kw
        assert b"sde_tsdf_mesh" in lib.sde_last_error(), kw
    assert not any(host)


def test_the_host_refuses():
    one = np.ones((2, 2, 2), np.float32)
    for bad in (0, 0.5, -1, float("nan")):
        with pytest.raises(ValueError):
            HV.mesh_host(one, one, None, (0, 0, 0), 0.1, min_weight=bad)
    rec = np.zeros(3, RECORD)
    tri = np.array([[0, 1, 2]], np.int32)
    for v, f in ((rec.view(np.uint8), tri), (rec.reshape(3, 1), tri), (rec, tri.astype(np.int64)), (rec, tri.reshape(-1)), (rec, tri + 1), (rec, tri - 1)):
        with pytest.raises(ValueError):
            HV.write_mesh_ply("/nonexistent/never-opened.ply", v, f)
    from simpledepthestimation_amd.tools import demo
    base = ["--cfg", "c.yaml", "--input", "frames", "--pairs", "--intrinsics", "1", "2", "3", "4"]
    assert demo.parse_args(base + ["--volume", "8", "8", "8", "--voxel", "0.1", "--save-mesh"]).save_mesh
    assert not demo.parse_args(base + ["--volume", "8", "8", "8", "--voxel", "0.1"]).save_mesh
    with pytest.raises(SystemExit):
        demo.parse_args(base + ["--save-mesh"])                                 # needs --volume


def test_ply_round_trip(tmp_path):
    inp, want, (rec, faces, count) = reference("sphere8")
    path = str(tmp_path / "mesh.ply")
    HV.write_mesh_ply(path, rec, faces)
    raw = open(path, "rb").read()
    head = raw[:raw.index(b"end_header\n")].decode("ascii").rstrip("\n").split("\n")
    assert head[:3] == ["ply", "format binary_little_endian 1.0", f"element vertex {rec.size}"]
    assert head[-2:] == [f"element face {faces.shape[0]}", "property list uchar int vertex_indices"]
    assert len(raw) == raw.index(b"end_header\n") + 11 + 16 * rec.size + 13 * faces.shape[0]
    v, f = HV.read_mesh_ply(path)
    assert v.dtype == RECORD and v.tobytes() == rec.tobytes() and f.dtype == np.int32 and f.tobytes() == faces.tobytes()
    HV.write_mesh_ply(path, rec[:0], faces[:0])                                 # an empty mesh is a legal file
    v, f = HV.read_mesh_ply(path)
    assert v.size == 0 and f.shape == (0, 3)
    open(path, "ab").write(b"\0")
    with pytest.raises(ValueError):
        HV.read_mesh_ply(path)


class HostVolume:
    """Stands in for a TsdfVolume whose `mesh` is the host twin: what save_mesh does with the counts needs no GPU."""
    save_mesh = HV.TsdfVolume.save_mesh

    def __init__(self, inp, caps):
        self.inp, self.caps, self.calls = inp, caps, []

    def mesh(self, min_weight=1, cap_vertices=None, cap_faces=None):
        cv, cf = self.caps[0] if cap_vertices is None else cap_vertices, self.caps[1] if cap_faces is None else cap_faces
        self.calls.append((cv, cf))
        rec, faces, count = HV.mesh_host(cap_vertices=cv, cap_faces=cf, **dict(self.inp, min_weight=min_weight))
        v, f = np.full((cv, 16), 0xA5, np.uint8), np.full((cf, 3), -7, np.int32)
        v[:rec.size], f[:faces.shape[0]] = rec.view(np.uint8).reshape(-1, 16), faces
        return torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(count)


def test_save_mesh_runs_again_instead_of_truncating(tmp_path):
    inp, want, (rec, faces, count) = reference("sphere8")
    nv, nf = (int(c) for c in count)
    path = str(tmp_path / "mesh.ply")
    for caps, calls in (((nv + 3, nf + 3), 1), ((nv, nf), 1), ((nv - 1, nf + 3), 2), ((nv + 3, nf - 1), 2), ((1, 1), 2)):
        vol = HostVolume(inp, caps)
        assert vol.save_mesh(path, min_weight=inp["min_weight"]) == (nv, nf)
        assert vol.calls == [caps, (nv, nf)][:calls], (caps, vol.calls)                     # the second run has exactly the counted room
        v, f = HV.read_mesh_ply(path)
        assert v.tobytes() == rec.tobytes() and f.tobytes() == faces.tobytes()
    empty = HostVolume(MR.mesh_inputs("dim_of_one"), (4, 4))
    assert empty.save_mesh(path) == (0, 0) and empty.calls == [(4, 4)]
    v, f = HV.read_mesh_ply(path)
    assert v.size == 0 and f.shape == (0, 3)

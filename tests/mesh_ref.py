"""Helper (no tests): float64 restatement of sde_tsdf_mesh as include/sde_hip.h defines it, written with plain loops over voxels, cells and edges
(nothing shared with the vectorised twin hip.volume.mesh_host), the inputs of the cases the CPU and the GPU tests share, a-priori bounds on the
float32 vertex positions, and topology helpers.  EPS = 2^-24, all inputs are float32 values and enter the restatement exactly.

Decisions.  Validity is weight >= min_weight and the crossing test compares (tsdf < 0) of two stored values: no decision hangs on a rounding, so
nothing is excluded -- the number of vertices and of triangles, the numbering, every index and both counts must match exactly.

Positions.  A crossing point is volume_ref's: the centre w = o + (i + 0.5) voxel with E_w = EPS |(i + 0.5) voxel| + EPS |w|, f = tv / (tv - tn)
with E_f = 2 EPS |f| (a difference and a division), and along the edge's axis p = w + f voxel with
    E_p = E_w + (E_f voxel + EPS |f voxel|) + EPS |p|;       the other two coordinates are the centre's, E_p = E_w.
The vertex coordinate is s / m with s = ((0 + p_1) + p_2) + ... + p_m in edge order, m <= 12: the first addition is exact, each of the others
rounds its partial sum, which is at most A_t = |p_1| + ... + |p_t| (+ the errors so far, second order: SLACK):
    E_s = sum_e E_p_e + EPS sum_{t = 2..m} A_t;         E_vertex = E_s / m + EPS |s / m|       (m is exact, one division).

Colours.  A channel is stored as (uint8)((float)t / (float)m + 0.5f) with integers t <= 12 * 255 and m <= 12.  t / m + 0.5 = (2 t + m) / (2 m)
reaches an integer n only where t / m = n - 0.5, a float32 number that the correctly rounded division returns exactly; everywhere else it stays
at least 1 / (2 m) >= 1 / 24 away from an integer, far beyond the rounding of the division (255 * 2^-23).  So the stored byte is
floor((2 t + m) / (2 m)) in integers, never hangs on a rounding, and colours must match exactly.  WHICH bytes are summed is a decision of
sde_tsdf_points (f < 0.5f): volume_ref leaves a crossing's colour undecided where |f - 0.5| <= E_f, and a vertex fed by such a crossing is the
only thing this file does not compare (colour only; `colour_decided`)."""
from collections import Counter

import numpy as np

import volume_ref as VR

EPS, SLACK = VR.EPS, VR.SLACK
AXES = ((1, 2), (0, 2), (0, 1))                            # b < c, the other two axes of x, y, z


def cell_edges():
    """The 12 edges of a cell in the header's order: (axis, (di, dj, dk) of the corner the edge starts at)."""
    out = []
    for a in range(3):
        for db, dc in ((0, 0), (1, 0), (0, 1), (1, 1)):
            d = [0, 0, 0]
            d[AXES[a][0]], d[AXES[a][1]] = db, dc
            out.append((a, tuple(d)))
    return out


def restate_mesh(tsdf, weight, rgba, origin, voxel, min_weight=1):
    """-> dict(xyz float64 [nv,3], bound [nv,3], colour uint8 [nv,3], colour_decided bool [nv], cells int [nv,3] (i, j, k), faces int [nf,3],
    quads: the list of (i, j, k, a) of the crossing edges that give faces, in order)."""
    nz, ny, nx = tsdf.shape
    dims = (nx, ny, nz)
    voxel = float(np.float32(voxel))
    valid, neg = weight >= np.float32(min_weight), tsdf < 0
    cen = [VR._centres(n, o, voxel) for n, o in zip(dims, origin)]

    def crossing(i, j, k, a):
        n = [i, j, k]
        n[a] += 1
        if n[a] >= dims[a] or not valid[k, j, i] or not valid[n[2], n[1], n[0]] or neg[k, j, i] == neg[n[2], n[1], n[0]]:
            return None
        tv, tn = float(tsdf[k, j, i]), float(tsdf[n[2], n[1], n[0]])
        f = tv / (tv - tn)
        Ef = SLACK * 2 * EPS * abs(f)
        p = [cen[0][0][i], cen[1][0][j], cen[2][0][k]]
        E = [cen[0][1][i], cen[1][1][j], cen[2][1][k]]
        p[a] = p[a] + f * voxel
        E[a] = SLACK * (E[a] + Ef * voxel + EPS * abs(f * voxel) + EPS * abs(p[a]))
        src = (k, j, i) if f < 0.5 else (n[2], n[1], n[0])
        col = [int(c) for c in rgba[src][:3]] if rgba is not None else [0, 0, 0]
        return p, E, col, abs(f - 0.5) > Ef

    xyz, bound, colour, decided, cells, number = [], [], [], [], [], {}
    edges = cell_edges()
    for k in range(nz - 1):
        for j in range(ny - 1):
            for i in range(nx - 1):
                found = [c for c in (crossing(i + d[0], j + d[1], k + d[2], a) for a, d in edges) if c is not None]
                m = len(found)
                if m == 0:
                    continue
                pos, err = [], []
                for b in range(3):
                    s, A, Es = 0.0, 0.0, 0.0
                    for t, (p, E, _, _) in enumerate(found):
                        s += p[b]
                        A += abs(p[b])
                        Es += E[b] + (EPS * A if t > 0 else 0.0)
                    pos.append(s / m)
                    err.append(SLACK * (Es / m + EPS * abs(s / m)))
                tot = [sum(c[2][ch] for c in found) for ch in range(3)]
                number[(i, j, k)] = len(xyz)
                xyz.append(pos)
                bound.append(err)
                colour.append([(2 * t + m) // (2 * m) for t in tot])
                decided.append(all(c[3] for c in found))
                cells.append((i, j, k))
    faces, quads = [], []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                for a in range(3):
                    if crossing(i, j, k, a) is None:
                        continue
                    b, c = AXES[a]
                    v = (i, j, k)
                    if not (1 <= v[b] <= dims[b] - 2 and 1 <= v[c] <= dims[c] - 2):
                        continue

                    def q(db, dc):
                        w = list(v)
                        w[b] += db
                        w[c] += dc
                        return number[tuple(w)]                    # a KeyError here: a cell around a crossing edge without a vertex
                    q0, q1, q2, q3 = q(-1, -1), q(0, -1), q(0, 0), q(-1, 0)
                    p = (q0, q1, q2, q3) if bool(neg[k, j, i]) != (a == 1) else (q0, q3, q2, q1)
                    faces += [(p[0], p[1], p[2]), (p[0], p[2], p[3])]
                    quads.append((i, j, k, a))
    nv = len(xyz)
    return dict(xyz=np.array(xyz, np.float64).reshape(nv, 3), bound=np.array(bound, np.float64).reshape(nv, 3),
                colour=np.array(colour, np.uint8).reshape(nv, 3), colour_decided=np.array(decided, bool).reshape(nv),
                cells=np.array(cells, np.int64).reshape(nv, 3), faces=np.array(faces, np.int64).reshape(len(faces), 3), quads=quads)


def positions(rec):
    return np.stack([rec["x"], rec["y"], rec["z"]], 1).astype(np.float64)


def compare_mesh(rec, faces, count, want, cap_vertices=None, cap_faces=None, label=""):
    """rec: the structured vertex records (the first min(count[0], cap_vertices)), faces int32 [n,3] (the first min(count[1], cap_faces)), count:
    the two reported totals, against `want` of restate_mesh.  Prints the figures before it asserts."""
    nv, nf = want["xyz"].shape[0], want["faces"].shape[0]
    mv, mf = nv if cap_vertices is None else min(nv, cap_vertices), nf if cap_faces is None else min(nf, cap_faces)
    assert rec.shape == (mv,) and faces.shape == (mf, 3) and faces.dtype == np.int32, (rec.shape, faces.shape, faces.dtype, mv, mf)
    err, b = np.abs(positions(rec) - want["xyz"][:mv]), want["bound"][:mv]
    ok = want["colour_decided"][:mv]
    print(f"{label}: {nv} vertices, {nf} triangles, {mv} / {mf} compared, largest position error / bound "
          f"{float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0:.3f}, {int((~ok).sum())} colours undecided")
    assert [int(c) for c in count] == [nv, nf]
    assert bool(np.all(err <= b))
    col = np.stack([rec["red"], rec["green"], rec["blue"]], 1)
    assert np.array_equal(col[ok], want["colour"][:mv][ok]) and bool(np.all(rec["alpha"] == 255))
    assert np.array_equal(faces.astype(np.int64), want["faces"][:mf])


# ---- topology -------------------------------------------------------------------------------------------------------------------------------------
def directed_edges(faces):
    """Counter of the directed edges (p, q) of all triangles."""
    f = np.asarray(faces, dtype=np.int64)
    return Counter((int(p), int(q)) for t in f for p, q in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])))


def undirected_edges(faces):
    c = Counter()
    for (p, q), n in directed_edges(faces).items():
        c[(min(p, q), max(p, q))] += n
    return c


def euler(nv, faces):
    """V - E + F."""
    return int(nv) - len(undirected_edges(faces)) + int(np.asarray(faces).shape[0])


def signed_volume(xyz, faces):
    """sum over the triangles of det(p0, p1, p2) / 6: positive for a closed surface whose triangles are counter-clockwise seen from outside."""
    p = np.asarray(xyz, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    return float(np.einsum("ni,ni->n", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def normals(xyz, faces):
    p = np.asarray(xyz, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])


# ---- the inputs of the shared cases ------------------------------------------------------------------------------------------------------------
SPHERES = {"sphere16": ((16, 16, 16), 5.3, (8.13, 7.9, 8.31)), "sphere8": ((8, 8, 8), 2.3, (4.1, 3.9, 4.2))}       # dims, radius, centre, in voxel indices
PLANE_Z0, PLANE_TRUNC = 3.25, 4.0                          # in voxel indices: tsdf = (k - 3.25) / 4 is exact in float32, and so is f = 0.25
CASES = ("sphere16", "sphere8", "plane", "random", "dim_of_one", "one_cell", "three_tiles")
ORIGIN, VOXEL = (np.float32(-0.4), np.float32(0.3), np.float32(1.1)), np.float32(0.05)


def world(idx, axis):
    """The world coordinate (float64) of the voxel-index coordinate idx along an axis: index i is the centre of voxel i."""
    return float(ORIGIN[axis]) + (np.asarray(idx, dtype=np.float64) + 0.5) * float(VOXEL)


def mesh_inputs(name):
    """-> dict(tsdf, weight, rgba, origin, voxel, min_weight): a synthetic volume."""
    rng = np.random.default_rng(sum(map(ord, name)) + 29)
    dims = {"plane": (9, 8, 7), "random": (13, 11, 9), "dim_of_one": (1, 7, 5), "one_cell": (2, 2, 2), "three_tiles": (37, 5, 3),
            "grid_stride": (128, 96, 48)}.get(name) or SPHERES[name][0]
    nx, ny, nz = dims
    k, j, i = np.mgrid[0:nz, 0:ny, 0:nx].astype(np.float64)
    weight = np.ones((nz, ny, nx), np.float32)
    rgba = rng.integers(0, 256, (nz, ny, nx, 4)).astype(np.uint8)
    min_weight = 1
    if name in SPHERES:                                    # negative inside: the normals point outwards
        _, r, c = SPHERES[name]
        tsdf = np.clip((np.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2) - r) / 3.0, -1, 1).astype(np.float32)
    elif name == "plane":
        tsdf = ((k - PLANE_Z0) / PLANE_TRUNC).astype(np.float32)
    elif name == "grid_stride":                            # not in CASES: more voxels than TILE * MAX_BLOCKS, a wavy surface across many tile borders, for the GPU
        tsdf = np.clip((np.sin(i / 9.0) * 6 + np.cos(j / 7.0) * 5 + 34 - k) / 4, -1, 1).astype(np.float32)
        weight = (rng.random((nz, ny, nx)) < 0.98).astype(np.float32) * 2
        min_weight = 2
    else:                                                  # noise: random signs, exact zeros of both signs, holes in the weights
        tsdf = rng.uniform(-1, 1, (nz, ny, nx)).astype(np.float32)
        flat = tsdf.reshape(-1)
        at = rng.choice(flat.size, max(flat.size // 10, 2), replace=False)
        flat[at[0::2]], flat[at[1::2]] = np.float32(0.0), np.float32(-0.0)
        weight = rng.integers(0, 5, (nz, ny, nx)).astype(np.float32)
        min_weight = 2
    return dict(tsdf=tsdf, weight=weight, rgba=rgba, origin=ORIGIN, voxel=VOXEL, min_weight=min_weight)

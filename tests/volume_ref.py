"""Helper (no tests): numpy float64 restatement of sde_tsdf_integrate and sde_tsdf_points as include/sde_hip.h defines them, the inputs of the
cases the CPU and the GPU tests share, and per-element bounds on the kernels' float32 results.  Every bound is a first-order count of the
roundings in the documented order of operations, times SLACK for the second-order terms; nothing is measured from the kernel.
EPS = 2^-24 is the unit roundoff, all inputs are float32 values and enter the float64 restatement exactly.

Integrate.  With the centre w = o + (i + 0.5) voxel (a product and a sum: E_w = EPS |(i + 0.5) voxel| + EPS |w|):
    q_r = ((C_r0 wx + C_r1 wy) + C_r2 wz) + C_r3:   E_q = sum_k |C_rk| E_wk + 4 EPS S_r,     S_r = sum_k |C_rk w_k| + |C_r3|   (<= 4 roundings per term);
    n = f q + c qz:   E_n = |f| E_q + |c| E_qz + 2 EPS (|f q| + |c qz|);      den = qz + 1e-6:   E_den = E_qz + EPS |den|;
    X = n / den:      E_X = (E_n + |X| E_den) / |den| + EPS |X|.
Decisions.  A voxel is UNDECIDED in a frame, and excluded from every comparison from then on, when a keep / drop decision may fall either way
in float32: |qz| <= E_qz; |frac(X) - 0.5| <= E_X or the same for Y (the landing pixel, and with it inside / outside the image, the maps and the
depth that is read); with sdf = d - qz and E_sdf = E_qz + EPS |sdf|: |sdf + trunc| <= E_sdf (the cut) or |sdf - trunc| <= E_sdf (whether the
colour is touched).  The depth range is decided on the stored float32 value of the decided pixel: exact.  `restate_integrate` asserts that the
undecided voxels are at most MAX_EXCLUDED (5 %) of the voxels the case touches.
Values.  t = min(1, sdf / trunc): E_t = E_sdf / trunc + EPS |t|.  The weights are sums of ones cut at max_weight, exact in float32 (asserted), so
    tsdf' = (t0 w0 + t) / (w0 + 1):   E' = (E_t0 w0 + E_t) / (w0 + 1) + EPS (|t0 w0| + |t0 w0 + t|) / (w0 + 1) + EPS |tsdf'|,
carried from frame to frame (a fresh voxel: t0 = 1, w0 = 0, E = 0).  Weights must agree exactly.
Colour.  c = (c0 w0 + f) / m with m = w0 + 1 and integers c0, f (w0 a multiple of 1/2): c + 0.5 = (2 (c0 w0 + f) + m) / (2 m) is either an
integer -- then c is a float32 number and the correctly rounded division returns it -- or at least 1 / (4 m) >= 1e-3 away from one (asserted),
far beyond 3 EPS 255: the stored byte floor(c + 0.5) never hangs on a rounding, and colours must agree exactly.

Points.  The inputs are the volume's float32 arrays: validity and the sign rule are comparisons of stored values, so the number of records and
their order are exact.  f = tv / (tv - tn): a difference and a division, E_f = 2 EPS |f|; the coordinate along the axis
    x = w + f voxel:   E_x = E_w + (E_f voxel + EPS |f voxel|) + EPS |x|;   the other two coordinates are the centre's, E_w.
The colour comes from v iff f < 0.5: where |f - 0.5| <= E_f the record's colour is not compared."""
import os
import re

import numpy as np

import flow_ref as FR

EPS = FR.EPS
SLACK = 1.01
TINY = FR.TINY
MAX_EXCLUDED = 0.05
_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "simpledepthestimation_amd", "csrc", "volume.hip")


def launch_limits():
    """(TILE, MAX_BLOCKS) of csrc/volume.hip."""
    src = open(_SRC).read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % k, src).group(1)) for k in ("TILE", "MAX_BLOCKS"))


def fresh(dims, colour=True):
    nx, ny, nz = dims
    return np.ones((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.float32), (np.zeros((nz, ny, nx, 4), np.uint8) if colour else None)


def _centres(n, o, voxel):
    """float64 centres and E_w along one axis."""
    a = (np.arange(n, dtype=np.float64) + 0.5) * float(voxel)
    w = float(o) + a
    return w, EPS * np.abs(a) + EPS * np.abs(w)


def restate_integrate(vol, frames, colour=True):
    """vol: dict(dims, voxel, origin, trunc, max_weight, min_depth, max_depth) (float32 values); frames: a list of dict(pred, ymap, xmap, K, C,
    frame), integrated in order into a fresh volume.  -> dict(tsdf float64, bound, weight float64, rgba uint8 or None, skip, touched; all
    [nz,ny,nx])."""
    nx, ny, nz = vol["dims"]
    voxel, trunc, wmax = float(np.float32(vol["voxel"])), float(np.float32(vol["trunc"])), float(np.float32(vol["max_weight"]))
    lo, hi = float(np.float32(vol["min_depth"])), float(np.float32(vol["max_depth"]))
    (wx, Ex), (wy, Ey), (wz, Ez) = (_centres(n, o, voxel) for n, o in zip((nx, ny, nz), vol["origin"]))
    w = [wx[None, None, :], wy[None, :, None], wz[:, None, None]]
    Ew = [Ex[None, None, :], Ey[None, :, None], Ez[:, None, None]]
    tsdf, bound, weight = np.ones((nz, ny, nx)), np.zeros((nz, ny, nx)), np.zeros((nz, ny, nx))
    rgb = np.zeros((nz, ny, nx, 4), np.uint8) if colour else None
    skip, touched = np.zeros((nz, ny, nx), bool), np.zeros((nz, ny, nx), bool)
    for fr in frames:
        C, K = fr["C"].astype(np.float64), fr["K"].astype(np.float64)
        pred, ymap, xmap = fr["pred"], fr["ymap"], fr["xmap"]
        H, W = ymap.size, xmap.size
        q, Eq = [], []
        for r in range(3):
            terms = [C[r, k] * w[k] for k in range(3)]
            q.append(terms[0] + terms[1] + terms[2] + C[r, 3])
            S = sum(np.abs(t) for t in terms) + abs(C[r, 3])
            Eq.append(SLACK * (sum(abs(C[r, k]) * Ew[k] for k in range(3)) + 4 * EPS * S))
        qz, Eqz = q[2], Eq[2]
        undecided = np.abs(qz) <= Eqz
        front = (qz > 0) & ~undecided
        with np.errstate(all="ignore"):
            den = qz + TINY
            Eden = Eqz + EPS * np.abs(den)
            XY, EXY = [], []
            for f, c, qq, E in ((K[0, 0], K[0, 2], q[0], Eq[0]), (K[1, 1], K[1, 2], q[1], Eq[1])):
                n = f * qq + c * qz
                En = abs(f) * E + abs(c) * Eqz + 2 * EPS * (np.abs(f * qq) + np.abs(c * qz))
                X = n / den
                XY.append(X)
                EXY.append(SLACK * ((En + np.abs(X) * Eden) / np.abs(den) + EPS * np.abs(X)))
            X, Y = XY
            edge = (np.abs(X - np.floor(X) - 0.5) <= EXY[0]) | (np.abs(Y - np.floor(Y) - 0.5) <= EXY[1])
        undecided |= front & edge
        live = front & ~edge
        rx, ry = np.where(live, np.rint(X), -1), np.where(live, np.rint(Y), -1)
        live &= (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
        ix, iy = np.where(live, rx, 0).astype(np.int64), np.where(live, ry, 0).astype(np.int64)
        my, mx = ymap[iy], xmap[ix]
        live &= (my >= 0) & (mx >= 0)
        d32 = pred[np.where(live, my, 0), np.where(live, mx, 0)]
        with np.errstate(all="ignore"):
            live &= np.isfinite(d32) & (np.float32(lo) < d32) & (d32 <= np.float32(hi))          # the stored values: exact
        d = np.where(live, d32, 0).astype(np.float64)
        sdf = d - qz
        Esdf = SLACK * (Eqz + EPS * np.abs(sdf))
        cut = live & ((np.abs(sdf + trunc) <= Esdf) | (np.abs(sdf - trunc) <= Esdf))
        undecided |= cut
        keep = live & ~cut & (sdf >= -trunc)
        t = np.minimum(1.0, sdf / trunc)
        Et = SLACK * (Esdf / trunc + EPS * np.abs(t))
        w0, t0, E0 = weight[keep], tsdf[keep], bound[keep]
        m = w0 + 1.0
        assert np.array_equal(m.astype(np.float32).astype(np.float64), m) and np.array_equal(w0 * 2, np.rint(w0 * 2)), "the weights are not exact"
        new = (t0 * w0 + t[keep]) / m
        bound[keep] = (E0 * w0 + Et[keep]) / m + SLACK * EPS * ((np.abs(t0 * w0) + np.abs(t0 * w0 + t[keep])) / m + np.abs(new))
        tsdf[keep] = new
        weight[keep] = np.minimum(m, wmax)
        if colour and fr.get("frame") is not None:
            sel = keep & (sdf <= trunc)
            ws = w0[sel[keep]]                                  # the weights before the update, at the voxels whose colour is touched
            ms = ws + 1.0
            c = (rgb[sel][:, :3].astype(np.float64) * ws[:, None] + fr["frame"][iy[sel], ix[sel]].astype(np.float64)) / ms[:, None]
            off = np.abs(c + 0.5 - np.rint(c + 0.5))
            assert bool(np.all((off < 1e-9) | (off > 1e-3))), "a colour sits next to a rounding boundary"
            out = np.full((c.shape[0], 4), 255, np.uint8)
            out[:, :3] = np.floor(c + 0.5 + 1e-6).astype(np.uint8)
            rgb[sel] = out
        skip |= undecided
        touched |= keep | undecided
    n_touched = int(touched.sum())
    assert int(skip.sum()) <= MAX_EXCLUDED * max(n_touched, 1), f"{int(skip.sum())} undecided voxels of {n_touched} touched"
    return dict(tsdf=tsdf, bound=bound, weight=weight, rgba=rgb, skip=skip, touched=touched)


def compare_integrate(got, want, label=""):
    """got = (tsdf, weight, rgba or None) float32 / uint8 arrays of the kernel or the twin against `want` of restate_integrate, outside the
    excluded voxels.  Prints the figures before it asserts."""
    tsdf, weight, rgba = got
    cmp = ~want["skip"]
    err = np.abs(tsdf.astype(np.float64) - want["tsdf"])[cmp]
    b = want["bound"][cmp]
    hit = want["touched"] & cmp
    print(f"{label}: {int(hit.sum())} of {cmp.size} voxels touched, {int(want['skip'].sum())} excluded, largest tsdf error / bound "
          f"{float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0:.3f}, largest weight {float(want['weight'].max())}")
    assert bool(np.all(err <= b))
    assert np.array_equal(weight.astype(np.float64)[cmp], want["weight"][cmp])
    if rgba is not None and want["rgba"] is not None:
        assert np.array_equal(rgba[cmp], want["rgba"][cmp])


def restate_points(tsdf, weight, rgba, origin, voxel, min_weight=1):
    """-> dict(xyz float64 [n,3], bound [n,3], colour uint8 [n,3], colour_decided bool [n]) of all the crossings, in the kernel's order."""
    nz, ny, nx = tsdf.shape
    voxel = float(np.float32(voxel))
    valid, neg = weight >= np.float32(min_weight), tsdf < 0
    cen = [_centres(n, o, voxel) for n, o in zip((nx, ny, nz), origin)]
    xyz, bound, colour, decided = [], [], [], []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                if not valid[k, j, i]:
                    continue
                for a, (kn, jn, inn) in enumerate(((k, j, i + 1), (k, j + 1, i), (k + 1, j, i))):
                    if kn >= nz or jn >= ny or inn >= nx or not valid[kn, jn, inn] or neg[k, j, i] == neg[kn, jn, inn]:
                        continue
                    tv, tn = float(tsdf[k, j, i]), float(tsdf[kn, jn, inn])
                    f = tv / (tv - tn)
                    Ef = SLACK * 2 * EPS * abs(f)
                    p = [cen[0][0][i], cen[1][0][j], cen[2][0][k]]
                    E = [cen[0][1][i], cen[1][1][j], cen[2][1][k]]
                    p[a] = p[a] + f * voxel
                    E[a] = SLACK * (E[a] + Ef * voxel + EPS * abs(f * voxel) + EPS * abs(p[a]))
                    xyz.append(p)
                    bound.append(E)
                    decided.append(abs(f - 0.5) > Ef)
                    colour.append((rgba[k, j, i] if f < 0.5 else rgba[kn, jn, inn])[:3] if rgba is not None else (0, 0, 0))
    n = len(xyz)
    return dict(xyz=np.array(xyz, np.float64).reshape(n, 3), bound=np.array(bound, np.float64).reshape(n, 3),
                colour=np.array(colour, np.uint8).reshape(n, 3), colour_decided=np.array(decided, bool).reshape(n))


def compare_points(rec, count, want, cap=None, label=""):
    """rec: the structured records (the first min(count, cap)), count: the reported total."""
    n = want["xyz"].shape[0]
    m = n if cap is None else min(n, cap)
    print(f"{label}: {n} crossings, {m} records compared, {int((~want['colour_decided']).sum())} colours undecided")
    assert count == n and rec.size == m
    got = np.stack([rec["x"], rec["y"], rec["z"]], 1).astype(np.float64)
    assert bool(np.all(np.abs(got - want["xyz"][:m]) <= want["bound"][:m]))
    col = np.stack([rec["red"], rec["green"], rec["blue"]], 1)
    ok = want["colour_decided"][:m]
    assert np.array_equal(col[ok], want["colour"][:m][ok]) and bool(np.all(rec["alpha"] == 255))


# ---- the inputs of the shared cases ------------------------------------------------------------------------------------------------------------
CASES = ("single_voxel", "odd_dims", "camera_inside", "bad_values", "trunc_edges", "saturation", "two_frames")
MIN_DEPTH, MAX_DEPTH = 0.25, 6.0


def maps_for(H, W, ph, pw, border):
    """Index maps H x W -> ph x pw: nearest source row / column, and with `border` a -1 frame one pixel wide (outside the prediction)."""
    def one(n, m):
        a = np.full(n, -1, np.int32)
        b = 1 if border else 0
        a[b:n - b] = (np.arange(n - 2 * b) * m // (n - 2 * b)).astype(np.int32)
        return a
    return one(H, ph), one(W, pw)


def camera(H, W):
    f = 0.9 * W
    return np.array([[f, 0, W / 2 + 0.37], [0, 0.97 * f, H / 2 - 0.21], [0, 0, 1]], np.float32)


def surface(rng, ph, pw, z0):
    """A depth map around z0: a ramp and some noise."""
    v, u = np.mgrid[0:ph, 0:pw]
    return (z0 + 0.3 * (u / max(pw - 1, 1) - 0.5) - 0.2 * (v / max(ph - 1, 1) - 0.5) + rng.uniform(-0.05, 0.05, (ph, pw))).astype(np.float32)


def case_inputs(name):
    """-> (vol, frames): the volume's parameters and the frames integrated in order (see restate_integrate).  Depths around 1.5, a volume one
    unit wide in front of the first camera."""
    rng = np.random.default_rng(sum(map(ord, name)) + 11)
    dims, voxel, origin, trunc, max_weight = (8, 6, 7), 0.125, None, None, 64.0
    H, W, ph, pw, border = 12, 16, 12, 16, False
    poses, repeat = [np.eye(4, dtype=np.float32)], 1
    if name == "single_voxel":
        dims, voxel, origin = (1, 1, 1), 0.5, (-0.21, -0.27, 1.2)
    elif name == "odd_dims":                              # 30 voxels; a non-identity map
        dims, voxel, origin = (5, 3, 2), 0.25, (-0.61, -0.33, 1.1)
        ph, pw, border = 6, 8, True
        poses = [FR.pose([1.0, -2.0, 0.5], [0.02, -0.01, 0.03])]
    elif name == "grid_stride":                           # not in CASES: more voxels than TILE * MAX_BLOCKS, for the GPU test of the grid-stride loops
        tile, cap = launch_limits()
        n = int(np.ceil((tile * cap + 1) ** (1 / 3))) + 1
        dims, voxel, origin = (n, n, n - 1), 1.0 / n, (-0.5, -0.5, 1.0)
        H, W, ph, pw = 48, 64, 24, 32
        poses = [FR.pose([0.5, 1.0, -0.5], [0.01, 0.02, -0.02])]
        assert dims[0] * dims[1] * dims[2] > tile * cap
    elif name == "camera_inside":                         # the camera sits inside the volume, which is wider than the picture: voxels behind it and outside
        dims, voxel, origin = (9, 7, 8), 0.5, (-2.3, -1.7, -1.1)
        poses = [FR.pose([2.0, -3.0, 1.0], [0.05, 0.02, -0.04])]
    elif name == "bad_values":
        ph, pw, border = 6, 8, True
        poses = [FR.pose([-1.0, 1.5, 0.0], [0.0, 0.03, 0.02])]
    elif name == "trunc_edges":
        dims, voxel, origin, trunc = (8, 8, 8), 0.25, (-1.0, -1.0, 0.0), 0.5
    elif name == "saturation":
        max_weight, repeat = 3.0, 5                        # max_weight + 2 integrations of one frame
        poses = [FR.pose([0.5, 0.5, 0.5], [0.01, 0.0, 0.0])]
    elif name == "two_frames":
        poses = [np.eye(4, dtype=np.float32), FR.pose([1.5, -2.5, 0.5], [0.08, -0.03, -0.1])]
    if origin is None:
        origin = (-dims[0] * voxel / 2 + 0.013, -dims[1] * voxel / 2 - 0.007, 1.0)
    f32 = lambda x: float(np.float32(x))
    vol = dict(dims=dims, voxel=f32(voxel), origin=tuple(f32(o) for o in origin), trunc=f32(4 * voxel if trunc is None else trunc),
               max_weight=f32(max_weight), min_depth=f32(MIN_DEPTH), max_depth=f32(MAX_DEPTH))
    ymap, xmap = maps_for(H, W, ph, pw, border)
    K = camera(H, W)
    frames = []
    for C in poses:
        pred = surface(rng, ph, pw, 1.0 + 0.5 * dims[2] * voxel)
        if name == "bad_values":
            flat = pred.reshape(-1)
            for at, v in zip(rng.choice(flat.size, 12, replace=False), (np.nan, 0.0, -1.5, MIN_DEPTH, MAX_DEPTH, MAX_DEPTH * 1.5, np.inf, -np.inf, np.nan, 0.0,
                                                                       MIN_DEPTH, MAX_DEPTH)):
                flat[at] = np.float32(v)
        if name == "trunc_edges":                         # identity pose: qz is the centre's z exactly, (k + 0.5) / 4
            pred[:] = np.float32(3.0)                     # sdf > trunc everywhere: t = 1, colour untouched ...
            pred[4:8, 4:12] = surface(rng, 4, 8, 1.0)     # ... but for a patch around the surface ...
            pred[4, 6] = np.float32(0.375)                # ... and two pixels the layer k = 3 (z = 0.875) lands on, at exactly -trunc behind its centres
            pred[8, 10] = np.float32(0.375)
        frame = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        frames += [dict(pred=pred, ymap=ymap, xmap=xmap, K=K, C=np.ascontiguousarray(C, dtype=np.float32), frame=frame)] * repeat
    return vol, frames


POINT_CASES = ("three_axes", "sign_rule", "f_sides", "several_workgroups", "two_scan_chunks", "empty")


def point_inputs(name):
    """-> dict(tsdf, weight, rgba, origin, voxel, min_weight): a synthetic volume."""
    rng = np.random.default_rng(sum(map(ord, name)) + 5)
    dims = {"three_axes": (6, 5, 4), "sign_rule": (4, 3, 2), "f_sides": (3, 1, 1), "several_workgroups": (37, 11, 5), "two_scan_chunks": (64, 48, 24),
            "empty": (5, 4, 3)}[name]
    nx, ny, nz = dims
    tsdf = rng.uniform(-1, 1, (nz, ny, nx)).astype(np.float32)
    weight = rng.integers(0, 4, (nz, ny, nx)).astype(np.float32)           # a quarter of the voxels are invalid: crossings next to them give no record
    rgba = rng.integers(0, 256, (nz, ny, nx, 4)).astype(np.uint8)
    min_weight = 1
    if name == "three_axes":
        weight[-1], weight[:, -1], weight[:, :, -1] = 2, 2, 2             # the last faces are valid: their voxels have no neighbour beyond
        tsdf[-1], tsdf[:, -1, :], tsdf[:, :, -1] = -0.6 * tsdf[-2], -0.6 * tsdf[:, -2, :], -0.6 * tsdf[:, :, -2]
    if name == "sign_rule":                                                # 0 and -0 are not below zero
        weight[:] = 1
        tsdf[0, 0] = [0.0, -0.5, -0.0, 0.5]
        tsdf[1, 1] = [-0.25, 0.0, 0.25, -0.0]
    if name == "f_sides":                                                  # f = 0.2 (the colour of v) and f = 0.75 (the neighbour's)
        weight[:] = 2
        tsdf[0, 0] = [-0.2, 0.9, -0.3]
        min_weight = 2
    if name == "two_scan_chunks":                                          # a smooth field: a surface, not noise
        k, j, i = np.mgrid[0:nz, 0:ny, 0:nx]
        tsdf = np.clip((np.sin(i / 7.0) * 4 + np.cos(j / 5.0) * 3 + 10 - k) / 4, -1, 1).astype(np.float32)
        weight[:] = 1
    if name == "empty":
        tsdf[:], weight[:], rgba[:] = 1, 0, 0
    return dict(tsdf=tsdf, weight=weight, rgba=rgba, origin=(np.float32(-0.4), np.float32(0.3), np.float32(1.1)), voxel=np.float32(0.05), min_weight=min_weight)


def compose_chain(n, seed=3):
    """n step poses [n,4,4] float32: rotations up to 2 degrees, translations up to 0.3."""
    rng = np.random.default_rng(seed)
    return np.stack([FR.pose(rng.uniform(-2, 2, 3), rng.uniform(-0.3, 0.3, 3)) for _ in range(n)])


def compose_bounds(T):
    """A-priori bounds (rotation entries, translation entries) on |compose_host chain - inverse of accumulate_poses| after all of T [n,4,4].
    Rounding: a rotation entry of one step is three products and two sums of entries of magnitude <= 1 (+ the defect), |T||C| <= 3 in the
    Frobenius norm: 3 EPS * 3 per step, and the steps before are carried through matrices of norm 1 + g; a translation entry adds T_r3:
    4 EPS (sqrt(3) |c_k| + |t_k|) <= 11 EPS L with L = 1 + the path's length, which bounds every |c_k| and |t_k|.  The reference: accumulate_poses
    inverts each step as [R^T | -R^T t], exact only for an orthonormal R; with g = max_k ||R_k^T R_k - I||_2 of the float32 steps each
    factor is off by a relative g, to first order n g on a rotation entry and n g L on a translation entry (doubled for the second order)."""
    T = T.astype(np.float64)
    n = T.shape[0]
    g = max(float(np.linalg.norm(R.T @ R - np.eye(3), 2)) for R in T[:, :3, :3])
    L = 1.0 + float(np.linalg.norm(T[:, :3, 3], axis=1).sum())
    grow = (1 + g) ** n
    return n * (10 * EPS + 2 * g) * grow, n * (11 * EPS + 2 * g) * L * grow

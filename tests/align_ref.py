"""Helper (no tests): numpy float64 restatement of sde_frame_align as include/sde_hip.h defines it, the scenes the CPU and the GPU tests share,
and bounds on the kernel's float32 results.  Every bound is a first-order count of the roundings in the documented order of operations, times
SLACK for the second-order terms (volume_ref's EPS = 2^-24 and SLACK); nothing is measured from the kernel.  All inputs are float32 values
and enter the float64 restatement exactly.

The per-pixel stage.  d = s d0:  E_d = EPS |d|.  The ray: k00 = 1 / fx and k02 = (-cx) / fx are one rounding each, rx = k00 u + k02:
E_rx = EPS |k00 u| + EPS |k00 u| + EPS |k02| + EPS |rx|.  p_x = d rx:  E_p = E_d |rx| + |d| E_rx + EPS |p_x|  (p_z = d: E_d).
q_r = ((D_r0 p_x + D_r1 p_y) + D_r2 p_z) + D_r3:  E_q = sum_k |D_rk| E_pk + 4 EPS (sum_k |D_rk p_k| + |D_r3|)  (at most four roundings per term).
The projection: n_x = fx q_x + cx q_z:  E_n = fx E_qx + |cx| E_qz + 2 EPS (|fx q_x| + |cx q_z|);  den = q_z + 1e-6f:  E_den = E_qz + EPS |den|;
X = n_x / den:  E_X = (E_n + |X| E_den) / (|den| - E_den) + EPS |X|.
The model point g_x = m rx(ix):  E_g = |m| E_rx + EPS |g_x|  (g_z = m: exact);  e = q - g:  E_e = E_q + E_g + EPS |e|.
r = (n_x e_x + n_y e_y) + n_z e_z:  E_r = sum_k |n_k| E_ek + 3 EPS sum_k |n_k e_k|.   c_x = q_y n_z - q_z n_y:
E_c = |n_z| E_qy + |n_y| E_qz + 2 EPS (|q_y n_z| + |q_z n_y|);  J = (c, n), the normal's entries are stored values.   rho = m / q_z:
E_rho = |rho| E_qz / (|q_z| - E_qz) + EPS |rho|.
Decisions.  A pixel is UNDECIDED when one of its decisions may fall either way in float32: q_z within E_qz of 0; X or Y within E_X of a half
integer (rintf: the pixel of the model, and with it the range test); | |r| - dist_tol m | <= E_r + EPS |dist_tol m| (the pose gate);
| |rho - 1| - scale_tol | <= E_rho + EPS |rho - 1| (the scale gate).  The tests on stored values (the maps, the depth range, m > 0, the normal)
are exact.  Undecided pixels are left out of the per-pixel comparison; `restate_terms` asserts that they are at most MAX_UNDECIDED (1 %) of the
picture.
The terms.  J_i J_j:  |J_i| E_Jj + |J_j| E_Ji + EPS |J_i J_j|;   J_i r:  |J_i| E_r + |r| E_Ji + EPS |J_i r|;   r r:  2 |r| E_r + EPS r^2.
The sums, over a GIVEN set of inliers (the twin's own masks, so that no decision hides in a tolerance): the terms' bounds add up; the float32
tree over a workgroup of 256 pixels is nine additions deep (six in the wave, three over the waves): + 9 EPS sum |term|; the float64 walk over
the slab and its tree: + 2^-53 (rows / 32 + 5) sum |term|.
The solve.  A xi = -b with |dA| <= EA, |db| <= Eb entrywise:  |d xi| <= |A^-1| (Eb + EA |xi|) to first order (entrywise, with the restated A), plus
the LDL^T in float64: 64 cond(A) 2^-53 |xi|.  The update: T = [Cayley(xi) | v] is smooth with derivative of norm <= 1 in omega / 2 ... the entries
of T move by at most |d xi| (rotation: the Cayley map's entries have gradient <= 1 in omega) + EPS (the rounding to float32); D' = T D is three
products and three sums per entry:  E_D' = sum_k E_Trk |D_kc| + E_Tr3 + 4 EPS (sum_k |T_rk D_kc| + |T_r3|)."""
import functools

import numpy as np

import flow_ref as FR
import volume_ref as VR

EPS = VR.EPS
SLACK = VR.SLACK
MAX_UNDECIDED = 0.01
POSE, SCALE = 1, 2


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------
def restate_terms(inp, D, s, dist_tol, scale_tol, cap=True):
    """inp: dict(pred, ymap, xmap, K, model_depth, model_normal, min_depth, max_depth); D [4,4], s: the state on entry (float32 values).  ->
    dict(kept, pose, scale, undecided bool [H,W]; r, rho, E_r, E_rho [H,W]; J, E_J [H,W,6]; ix, iy): float64, bounds included."""
    pred, ymap, xmap = inp["pred"].astype(np.float64), np.asarray(inp["ymap"]), np.asarray(inp["xmap"])
    H, W = ymap.size, xmap.size
    K, D = inp["K"].astype(np.float64), np.asarray(D, np.float32).astype(np.float64)
    md, mn = inp["model_depth"].astype(np.float64), inp["model_normal"].astype(np.float64)
    lo, hi = float(np.float32(inp["min_depth"])), float(np.float32(inp["max_depth"]))
    s, dist_tol, scale_tol = float(np.float32(s)), float(np.float32(dist_tol)), float(np.float32(scale_tol))
    fx, cx, fy, cy = K[0, 0], K[0, 2], K[1, 1], K[1, 2]
    out = {k: np.zeros((H, W), bool) for k in ("kept", "pose", "scale", "undecided")}
    out.update({k: np.zeros((H, W)) for k in ("r", "rho", "E_r", "E_rho")})
    out.update(J=np.zeros((H, W, 6)), E_J=np.zeros((H, W, 6)), ix=np.zeros((H, W), np.int64), iy=np.zeros((H, W), np.int64))

    def ray(f, c, x):
        k0, k2 = 1.0 / f, -c / f
        r = k0 * x + k2
        return r, 2 * EPS * abs(k0 * x) + EPS * abs(k2) + EPS * abs(r)

    for v in range(H):
        for u in range(W):
            my, mx = int(ymap[v]), int(xmap[u])
            if my < 0 or mx < 0:
                continue
            d0 = pred[my, mx]
            if not (np.isfinite(d0) and lo < d0 <= hi):
                continue
            d = s * d0
            Ed = EPS * abs(d)
            (rx, Erx), (ry, Ery) = ray(fx, cx, u), ray(fy, cy, v)
            p = [d * rx, d * ry, d]
            Ep = [Ed * abs(rx) + abs(d) * Erx + EPS * abs(p[0]), Ed * abs(ry) + abs(d) * Ery + EPS * abs(p[1]), Ed]
            q = [D[r, 0] * p[0] + D[r, 1] * p[1] + D[r, 2] * p[2] + D[r, 3] for r in range(3)]
            Eq = [SLACK * (sum(abs(D[r, k]) * Ep[k] for k in range(3)) + 4 * EPS * (sum(abs(D[r, k] * p[k]) for k in range(3)) + abs(D[r, 3])))
                  for r in range(3)]
            if not np.isfinite(q[2]):
                continue
            if abs(q[2]) <= Eq[2]:
                out["undecided"][v, u] = True
            if not q[2] > 0:
                continue
            den = q[2] + FR.TINY
            Eden = Eq[2] + EPS * abs(den)
            XY, edge = [], False
            for f, c, k in ((fx, cx, 0), (fy, cy, 1)):
                n_ = f * q[k] + c * q[2]
                En = f * Eq[k] + abs(c) * Eq[2] + 2 * EPS * (abs(f * q[k]) + abs(c * q[2]))
                X = n_ / den
                EX = SLACK * ((En + abs(X) * Eden) / (abs(den) - Eden) + EPS * abs(X))
                edge = edge or abs(abs(X - np.floor(X)) - 0.5) <= EX
                XY.append(X)
            if edge:
                out["undecided"][v, u] = True
            if not (abs(np.rint(XY[0])) < 1e9 and abs(np.rint(XY[1])) < 1e9):
                continue
            ix, iy = int(np.rint(XY[0])), int(np.rint(XY[1]))
            if not (0 <= ix < W and 0 <= iy < H):
                continue
            m, n = md[iy, ix], mn[iy, ix]
            if not m > 0 or not n.any():
                continue
            out["kept"][v, u], out["ix"][v, u], out["iy"][v, u] = True, ix, iy
            (gx, Egx), (gy, Egy) = ray(fx, cx, ix), ray(fy, cy, iy)
            g = [m * gx, m * gy, m]
            Eg = [m * Egx + EPS * abs(g[0]), m * Egy + EPS * abs(g[1]), 0.0]
            e = [q[k] - g[k] for k in range(3)]
            Ee = [Eq[k] + Eg[k] + EPS * abs(e[k]) for k in range(3)]
            r = n[0] * e[0] + n[1] * e[1] + n[2] * e[2]
            Er = SLACK * (sum(abs(n[k]) * Ee[k] for k in range(3)) + 3 * EPS * sum(abs(n[k] * e[k]) for k in range(3)))
            gate = dist_tol * m
            if abs(abs(r) - gate) <= Er + EPS * gate:
                out["undecided"][v, u] = True
            out["pose"][v, u] = abs(r) <= gate
            J, EJ = list(n) * 2, [0.0] * 6
            for k, (a, b) in enumerate(((1, 2), (2, 0), (0, 1))):
                J[k] = q[a] * n[b] - q[b] * n[a]
                EJ[k] = SLACK * (abs(n[b]) * Eq[a] + abs(n[a]) * Eq[b] + 2 * EPS * (abs(q[a] * n[b]) + abs(q[b] * n[a])))
            rho = m / q[2]
            Erho = SLACK * (abs(rho) * Eq[2] / (abs(q[2]) - Eq[2]) + EPS * abs(rho))
            if abs(abs(rho - 1.0) - scale_tol) <= Erho + EPS * abs(rho - 1.0):
                out["undecided"][v, u] = True
            out["scale"][v, u] = abs(rho - 1.0) <= scale_tol
            out["r"][v, u], out["E_r"][v, u], out["rho"][v, u], out["E_rho"][v, u] = r, Er, rho, Erho
            out["J"][v, u], out["E_J"][v, u] = J, EJ
    if cap:
        n_und = int(out["undecided"].sum())
        assert n_und <= MAX_UNDECIDED * H * W, f"{n_und} undecided pixels of {H * W}"
    return out


def restate_sums(t, pose, scale):
    """The 31 sums of the restated terms over GIVEN inlier masks, and their bounds against the kernel's totals -> (total [32], bound [32])."""
    total, bound = np.zeros(32), np.zeros(32)
    mag = np.zeros(32)
    H, W = pose.shape
    rows = -(-H // 8) * -(-W // 32)
    for v, u in zip(*np.nonzero(pose)):
        J, EJ, r, Er = t["J"][v, u], t["E_J"][v, u], t["r"][v, u], t["E_r"][v, u]
        k = 0
        for i in range(6):
            for j in range(i, 6):
                x = J[i] * J[j]
                total[k] += x
                mag[k] += abs(x)
                bound[k] += abs(J[i]) * EJ[j] + abs(J[j]) * EJ[i] + EPS * abs(x)
                k += 1
        for i in range(6):
            x = J[i] * r
            total[21 + i] += x
            mag[21 + i] += abs(x)
            bound[21 + i] += abs(J[i]) * Er + abs(r) * EJ[i] + EPS * abs(x)
        total[27] += r * r
        mag[27] += r * r
        bound[27] += 2 * abs(r) * Er + EPS * r * r
        total[28] += 1
    for v, u in zip(*np.nonzero(scale)):
        total[29] += t["rho"][v, u]
        mag[29] += abs(t["rho"][v, u])
        bound[29] += t["E_rho"][v, u]
        total[30] += 1
    return total, SLACK * (bound + (9 * EPS + 2.0 ** -53 * (rows / 32 + 5)) * mag)


def matrices(total):
    A, k = np.zeros((6, 6)), 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = total[k]
            k += 1
    return A, total[21:27].copy()


def cayley(omega):
    a = np.asarray(omega, np.float64) / 2
    ax = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return ((1 - a @ a) * np.eye(3) + 2 * np.outer(a, a) + 2 * ax) / (1 + a @ a)


def restate_solve(total, bound, damping):
    """-> (xi [6], E_xi [6]) from numpy.linalg.solve on the damped restated system, or (None, None) when the matrix is not positive definite."""
    A, b = matrices(total)
    EA, Eb = matrices(bound)
    A = A + np.diag(np.diag(A)) * float(np.float32(damping))
    EA = EA + np.diag(np.diag(EA)) * float(np.float32(damping))
    if not np.isfinite(A).all() or np.linalg.eigvalsh(A).min() <= 0:
        return None, None
    xi = np.linalg.solve(A, -b)
    E = np.abs(np.linalg.inv(A)) @ (Eb + EA @ np.abs(xi)) + 64 * np.linalg.cond(A) * 2.0 ** -53 * np.abs(xi)
    return xi, SLACK * E


def restate_iteration(inp, state, mode, dist_tol, scale_tol, min_count, damping, masks=None):
    """One whole iteration in float64.  state = dict(D [4,4], s, float64); masks: (pose, scale) to sum over in place of the restatement's own.
    -> (new state, info = dict(count, scale_count, sumsq, status, xi, E_xi, A, terms))."""
    t = restate_terms(inp, np.asarray(state["D"], np.float32), np.float32(state["s"]), dist_tol, scale_tol, cap=masks is None)
    pose, scale = masks if masks is not None else (t["pose"], t["scale"])
    total, bound = restate_sums(t, pose, scale)
    count, count_s = int(total[28]), int(total[30])
    info = dict(count=count, scale_count=count_s, sumsq=total[27], status=0, xi=None, E_xi=None, A=matrices(total)[0], terms=t, total=total, bound=bound)
    new = dict(D=np.array(state["D"], np.float64), s=float(state["s"]))
    if count < min_count:
        info["status"] = 1
        return new, info
    if mode & POSE:
        xi, E = restate_solve(total, bound, damping)
        if xi is None:
            info["status"] = 2
            return new, info
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = cayley(xi[:3]), xi[3:]
        new["D"] = T @ new["D"]
        info["xi"], info["E_xi"] = xi, E
    if (mode & SCALE) and count_s >= min_count:
        new["s"] = new["s"] * (total[29] / count_s)
    return new, info


def update_bound(xi, E_xi, D):
    """Entrywise bound [3,4] on |D' of the kernel - D' restated| for ONE iteration from the same D, given |d xi| <= E_xi (module docstring)."""
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = cayley(xi[:3]), xi[3:]
    ET = np.zeros((3, 4))
    ET[:, :3] = np.abs(E_xi[:3]).sum() + EPS
    ET[:, 3] = E_xi[3:] + EPS * np.abs(xi[3:])
    D = np.asarray(D, np.float64)
    out = np.zeros((3, 4))
    for r in range(3):
        for c in range(4):
            out[r, c] = sum(ET[r, k] * abs(D[k, c]) for k in range(3)) + 4 * EPS * sum(abs(T[r, k] * D[k, c]) for k in range(3))
            if c == 3:
                out[r, c] += ET[r, 3] + 4 * EPS * abs(T[r, 3])
    return SLACK * out


def pose_error(D, want):
    """(rotation angle in radians, translation distance) between two rigid [4,4]."""
    E = np.asarray(D, np.float64) @ np.linalg.inv(np.asarray(want, np.float64))
    return float(np.arccos(np.clip((np.trace(E[:3, :3]) - 1) / 2, -1, 1))), float(np.linalg.norm(E[:3, 3]))


# ---- the scenes -----------------------------------------------------------------------------------------------------------------------------------
# A room corner: the back wall z = 2.0 (tilted a little), the floor y = 0.55, the left wall x = -0.8, and a sphere of radius 0.3 in front of them.
# Three planes with independent normals and a curved surface: all six degrees of freedom are constrained.
PLANES = (((0.05, -0.04, 1.0), 2.0), ((0.03, 1.0, 0.06), 0.55), ((-1.0, 0.02, 0.05), 0.8))           # n . x = c, n not normalised
SPHERE = ((0.25, 0.05, 1.45), 0.3)
VOLUME = dict(dims=(48, 40, 44), voxel=0.05, origin=(np.float32(-1.2), np.float32(-1.0), np.float32(0.2)), trunc=0.2, max_weight=64.0, min_depth=0.25, max_depth=6.0)
RENDER = dict(near=0.3, step=0.05, far=2.5)
# The perturbation of the convergence test: the frame's true camera against the predicted one is turned by about 1 degree and moved by about a voxel
# (0.05), and its depth is 4 % short: written down here, chosen before any run of the code under test.
PERTURB_DEG, PERTURB_T, PERTURB_SCALE = (0.6, -0.8, 0.5), (0.035, -0.025, 0.04), 1.04


def scene_depth(K, size, C, planes=PLANES, sphere=SPHERE):
    """The z-depth of the scene seen from the world -> camera pose C through K, float64 [H,W]; inf where a ray meets nothing."""
    H, W = size
    K, C = np.asarray(K, np.float64), np.asarray(C, np.float64)
    R, t = C[:3, :3], C[:3, 3]
    o = -R.T @ t
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    ray = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones((H, W))], -1) @ R          # R^T ray, row-wise
    best = np.full((H, W), np.inf)
    with np.errstate(all="ignore"):
        for n, c in planes:
            n = np.asarray(n, np.float64)
            s = (c - n @ o) / (ray @ n)
            best = np.where((s > 1e-3) & (s < best), s, best)
        if sphere is not None:
            cen, rad = np.asarray(sphere[0], np.float64) - o, sphere[1]
            a, b, c = (ray * ray).sum(-1), -2 * (ray @ cen), cen @ cen - rad * rad
            disc = b * b - 4 * a * c
            s = (-b - np.sqrt(disc)) / (2 * a)
            best = np.where((disc > 0) & (s > 1e-3) & (s < best), s, best)
    return best


def camera(H, W):
    f = 0.9 * W
    return np.array([[f, 0, W / 2 + 0.37], [0, 0.97 * f, H / 2 - 0.21], [0, 0, 1]], np.float32)


CASES = ("corner", "corner_8x8", "corner_9x33", "corner_maps", "corner_264", "plane", "empty", "bad_values")
SIZES = {"corner_8x8": (8, 8), "corner_9x33": (9, 33), "corner_264": (264, 264)}


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """-> dict(pred, ymap, xmap, K, model_depth, model_normal, min_depth, max_depth, volume = (tsdf, weight, rgba), vol = VOLUME, C (the predicted
    pose the model was rendered from), D_true [4,4] float64, s_true, size).  Computed once and shared: nobody modifies it."""
    from simpledepthestimation_amd.hip.volume import integrate_host, render_host
    rng = np.random.default_rng(sum(map(ord, name)) + 23)
    f32 = np.float32
    H, W = size = SIZES.get(name, (40, 72))
    K = camera(H, W)
    vol = dict(VOLUME)
    planes, sphere = PLANES, SPHERE
    if name == "plane":                                       # one fronto-parallel wall: three of the six directions are not constrained
        planes, sphere = (((0.0, 0.0, 1.0), 1.75),), None
    tsdf, weight, rgba = VR.fresh(vol["dims"], colour=False)
    C0 = np.eye(4, dtype=f32)
    if name != "empty":
        # the model: two frames at the picture's own size, from the identity pose and from a camera a little to the side.  The plane is seen from
        # the identity alone: every voxel layer then holds ONE value, the rendered normal is (0, 0, -1) exactly, and three rows of the 6 x 6
        # matrix are exactly zero
        for Ci in (C0,) if name == "plane" else (C0, FR.pose((0.0, 2.0, 0.0), (0.06, 0.0, 0.0))):
            d = scene_depth(K, size, Ci, planes, sphere)
            ym, xm = VR.maps_for(H, W, H, W, False)
            integrate_host(tsdf, weight, None, np.where(np.isfinite(d), d, 0).astype(f32), ym, xm, K, Ci, None, vol["origin"], vol["voxel"], vol["trunc"],
                           vol["max_weight"], vol["min_depth"], vol["max_depth"])
    # the PREDICTED pose of the tracked frame: what the model is rendered from
    C = C0 if name == "plane" else FR.pose((0.5, -0.4, 0.3), (0.02, 0.01, -0.015))
    near, step = f32(RENDER["near"]), f32(RENDER["step"])
    n = int(np.ceil((float(f32(RENDER["far"])) - float(near)) / float(step)))
    depth, normal, _ = render_host(tsdf, weight, None, K, C, size, vol["origin"], vol["voxel"], near, step, n, 1)
    # the frame: seen from the TRUE pose, D_true = C C_true^-1 takes its camera coordinates to the render camera's
    P = FR.pose(PERTURB_DEG, PERTURB_T).astype(np.float64)
    C_true = np.linalg.inv(P) @ C.astype(np.float64)
    D_true = C.astype(np.float64) @ np.linalg.inv(C_true)
    ph, pw = H, W
    if name == "corner_maps":                                 # a prediction at another size, behind maps with a -1 border
        ph, pw = 29, 53
    ymap, xmap = VR.maps_for(H, W, ph, pw, name == "corner_maps")
    # the prediction at its own size: the scene seen through the maps' pixel centres is approximated by sampling the full-size depth
    full = scene_depth(K, size, C_true, planes, sphere) / PERTURB_SCALE
    pred = np.zeros((ph, pw), f32)
    for v in range(H):
        for u in range(W):
            if ymap[v] >= 0 and xmap[u] >= 0:
                pred[ymap[v], xmap[u]] = full[v, u] if np.isfinite(full[v, u]) else 0
    if name == "corner_maps":
        pred[5:9, 20:31] = 0                                  # holes: below min_depth
        depth, normal = depth.copy(), normal.copy()
        depth[20:24, 30:40] = 0                               # ... and misses in the model
        normal[20:24, 30:40] = 0
    if name == "bad_values":
        bad = rng.uniform(size=pred.shape)
        pred = np.where(bad < 0.05, np.nan, np.where(bad < 0.1, np.inf, np.where(bad < 0.15, -1.0, np.where(bad < 0.2, 7.0, pred)))).astype(f32)
        pred[0, 0] = vol["max_depth"]                         # the closed end of the range
    return dict(pred=pred, ymap=ymap, xmap=xmap, K=K, model_depth=depth, model_normal=normal, min_depth=vol["min_depth"], max_depth=vol["max_depth"],
                volume=(tsdf, weight, rgba), vol=vol, C=C, D_true=D_true, s_true=PERTURB_SCALE, size=size, render=(near, step, n))

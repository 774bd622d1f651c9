"""Helper (no tests): numpy float64 restatement of sde_depth_warp_fuse's definition in include/sde_hip.h -- warp, fill, fuse --, the inputs of
the cases the CPU and the GPU tests share, and the per-element bounds on the kernel's float32 results.

Restatement.  Built on flow_ref.restate with identity maps, which gives the float64 X, Y, qz of every previous-frame pixel and the first-order
bounds E_X, E_Y on the kernel's float32 coordinates from the documented order of operations (nothing is measured from the kernel); E_qz, which
flow_ref forms but does not hand out, is formed here from the same line of its docstring:
    E_q = |R_r0| E_px + |R_r1| E_py + eps |s_r| + 4 eps S_r,      E_px = 5 eps |d| (|u / fx| + |cx / fx|),      S_r = sum of the terms' magnitudes.
A source is kept iff d is finite and > 0, qz > 0 and X, Y are finite (flow_ref's bit 0; its check_qz asserts that kept sources have qz >= 0.5
and dropped ones qz <= -0.25, so that no decision on qz hangs on a rounding).  It lands at (rint(X), rint(Y)), half to even; the smallest qz
wins the pixel; an empty pixel takes the smallest entry of its up to eight neighbours (FILLED); the fusion rule follows in float64 on the
float32 values of `cur`, with alpha and tol at their float32 values.

Undecided sources.  A source whose |frac(X) - 0.5| <= E_X (or the same for Y) may land on either side in float32.  Both candidate pixels of
such a source, and the 3 x 3 neighbourhood of each (a changed entry changes what its neighbours are filled with), are excluded from the
comparison; `restate` asserts that they are at most 5 % of the map.

Bounds on the compared pixels.  The pixel's float32 entry is the minimum of the float32 qz of the same sources as in float64; each is within
its E_qz, so the minimum is within the largest E_qz among the sources that land there (for a filled pixel: among those of the ring), E_w below:
    |warped - ref| <= E_w + 2^-24 |ref|.
fused = c + alpha * diff with diff = wv - c:  diff carries E_w and one rounding, the product one more, the sum a third:
    |fused - ref| <= alpha (E_w + eps |diff|) + eps alpha |diff| + eps |fused| <= E_w + 2 eps |fused|
because alpha < 1 and 2 alpha |diff| <= 2 tol |fused| < |fused|: the bound of `warped` plus two roundings.  Where the pixel is not consistent,
fused is cur bit for bit.

Threshold.  The inputs keep every |diff| either <= tol / 2 * min(wv, c) or >= 2 tol * min(wv, c) (asserted in `restate`), far beyond any of
the bounds above, so the class of a compared pixel never hangs on a rounding."""
import numpy as np

import flow_ref as FR

EPS = FR.EPS
NEW, FUSED, NEARER, FARTHER, FILLED = 0, 1, 2, 3, 4
MAX_EXCLUDED = 0.05


def qz_bound(prev, K, T, motion):
    """E_qz [N,h,w]: flow_ref's bound on the float32 qz, from the same formula (its E_q for the row r = z)."""
    N, h, w = prev.shape
    d = np.abs(prev.astype(np.float64))
    K, T = K.astype(np.float64), T.astype(np.float64)
    m = motion.astype(np.float64) if motion is not None else np.zeros((N, 3, h, w))
    u = np.arange(w, dtype=np.float64)[None, None, :]
    v = np.arange(h, dtype=np.float64)[None, :, None]
    b = lambda a: a[:, None, None]
    fx, cx, fy, cy = b(K[:, 0, 0]), b(K[:, 0, 2]), b(K[:, 1, 1]), b(K[:, 1, 2])
    with np.errstate(all="ignore"):
        ax, ay = np.abs(u / fx) + np.abs(cx / fx), np.abs(v / fy) + np.abs(cy / fy)
        Epx, Epy = FR.K_PX * EPS * d * ax, FR.K_PX * EPS * d * ay
        s = b(T[:, 2, 3]) + m[:, 2]
        S = np.abs(b(T[:, 2, 0])) * d * ax + np.abs(b(T[:, 2, 1])) * d * ay + np.abs(b(T[:, 2, 2])) * d + np.abs(s)       # |p| <= d * a: an upper count
        return np.abs(b(T[:, 2, 0])) * Epx + np.abs(b(T[:, 2, 1])) * Epy + EPS * np.abs(s) + 4 * EPS * S


def _ring(a, pad, op):
    """op over the up to eight neighbours (the centre excluded) of every element of a [h,w]; outside the image counts as `pad`."""
    h, w = a.shape
    big = np.full((h + 2, w + 2), pad, dtype=a.dtype)
    big[1:-1, 1:-1] = a
    out = np.full((h, w), pad, dtype=a.dtype)
    for dy in range(3):
        for dx in range(3):
            if (dy, dx) != (1, 1):
                out = op(out, big[dy:dy + h, dx:dx + w])
    return out


def warp(prev, K, T, motion=None):
    """The forward warp alone -> dict of [N,h,w] arrays: z (float64, inf where nothing landed), landed (bool, before the fill), wv (float64
    after the fill, 0 in holes), filled, hole, E_w, skip (the excluded pixels)."""
    N, h, w = prev.shape
    r = FR.restate(prev, np.arange(h, dtype=np.int32), np.arange(w, dtype=np.int32), K, T, motion)
    Eq = qz_bound(prev, K, T, motion)
    out = {k: np.zeros((N, h, w), t) for k, t in (("z", np.float64), ("wv", np.float64), ("E_w", np.float64), ("skip", bool), ("filled", bool))}
    for n in range(N):
        keep = r["bit0"][n]
        X, Y, qz = r["X"][n][keep], r["Y"][n][keep], r["qz"][n][keep]
        EX, EY, E = r["EX"][n][keep], r["EY"][n][keep], Eq[n][keep]
        rx, ry = np.rint(X), np.rint(Y)
        ok = (np.abs(rx) < 1e9) & (np.abs(ry) < 1e9)
        ix, iy = rx[ok].astype(np.int64), ry[ok].astype(np.int64)
        inside = (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
        z = np.full(h * w, np.inf)
        Ez = np.zeros(h * w)
        at = iy[inside] * w + ix[inside]
        np.minimum.at(z, at, qz[ok][inside])
        np.maximum.at(Ez, at, E[ok][inside])
        z, Ez = z.reshape(h, w), Ez.reshape(h, w)
        # undecided sources: both candidates on the undecided axis, the one landing pixel on the other
        fX, fY = np.floor(X), np.floor(Y)
        uX, uY = np.abs(X - fX - 0.5) <= EX, np.abs(Y - fY - 0.5) <= EY
        touched = np.zeros((h, w), bool)
        for ax_, ay_ in ((0, 0), (1, 0), (0, 1), (1, 1)):
            sel = (uX | uY) & (uX | (ax_ == 0)) & (uY | (ay_ == 0))
            cx_ = np.where(uX, fX + ax_, rx)[sel]
            cy_ = np.where(uY, fY + ay_, ry)[sel]
            inb = (cx_ >= 0) & (cx_ < w) & (cy_ >= 0) & (cy_ < h)
            touched[cy_[inb].astype(np.int64), cx_[inb].astype(np.int64)] = True
        skip = touched | _ring(touched, False, np.logical_or)
        empty = np.isinf(z)
        near = _ring(z, np.inf, np.minimum)
        out["filled"][n] = empty & ~np.isinf(near)
        out["z"][n] = z
        zf = np.where(empty, near, z)
        out["wv"][n] = np.where(np.isinf(zf), 0.0, zf)
        out["E_w"][n] = np.where(empty, _ring(Ez, 0.0, np.maximum), Ez)
        out["skip"][n] = skip
    out["landed"] = ~np.isinf(out["z"])
    out["hole"] = ~out["landed"] & ~out["filled"]
    assert float(out["skip"].mean()) <= MAX_EXCLUDED and all(float(s.mean()) <= MAX_EXCLUDED for s in out["skip"]), "too many undecided pixels"
    return out


def restate(prev, cur, K, T, motion=None, alpha=0.5, tol=0.05, check_threshold=True):
    """-> dict of [N,h,w] arrays: fused, warped (float64), state uint8, consistent, bound_w, bound_f, skip, landed, filled, hole."""
    a, t = float(np.float32(alpha)), float(np.float32(tol))
    wp = warp(prev, K, T, motion)
    c = cur.astype(np.float64)
    with np.errstate(all="ignore"):
        usable = ~wp["hole"] & np.isfinite(c) & (c > 0)
        wv = wp["wv"]
        diff = wv - c
        low = np.fmin(wv, c)
        consistent = usable & (np.abs(diff) <= t * low)
        if check_threshold:
            far = np.abs(diff)[usable] / low[usable]
            assert bool(np.all((far <= t / 2) | (far >= 2 * t))), "a pixel sits next to the consistency threshold"
        fused = np.where(consistent, c + a * diff, c)
        cls = np.where(~usable, NEW, np.where(consistent, FUSED, np.where(diff < 0, NEARER, FARTHER)))
    state = (cls | np.where(wp["filled"], FILLED, 0)).astype(np.uint8)
    bound_w = wp["E_w"] + EPS * np.abs(wv)
    bound_f = np.where(consistent, bound_w + 2 * EPS * np.abs(fused), 0.0)
    return dict(fused=fused, warped=wv, state=state, consistent=consistent, bound_w=bound_w, bound_f=bound_f, skip=wp["skip"], landed=wp["landed"],
                filled=wp["filled"], hole=wp["hole"])


def compare(got, want, cur, label=""):
    """got = (fused, state, warped) float32 / uint8 arrays of the kernel or the twin against the restatement `want`, outside the excluded pixels:
    the state equal, warped and fused within their bounds, fused == cur bit for bit where the pixel is not consistent.  Prints the figures
    before it asserts."""
    fused, state, warped = got
    cmp = ~want["skip"]
    ew = np.abs(warped.astype(np.float64) - want["warped"])[cmp]
    blend = cmp & want["consistent"]
    ef = np.abs(fused.astype(np.float64) - want["fused"])[blend]
    print(f"{label}: {int(cmp.sum())} of {cmp.size} pixels compared, states {np.bincount(want['state'].ravel(), minlength=8).tolist()}, "
          f"largest warped error / bound {float((ew / np.maximum(want['bound_w'][cmp], 1e-300)).max()) if ew.size else 0.0:.3f}, "
          f"largest fused error / bound {float((ef / want['bound_f'][blend]).max()) if ef.size else 0.0:.3f}")
    assert np.array_equal(state[cmp], want["state"][cmp])
    assert bool(np.all(ew <= want["bound_w"][cmp]))
    assert bool(np.all(ef <= want["bound_f"][blend]))
    keep = cmp & ~want["consistent"]
    assert np.array_equal(fused.view(np.uint32)[keep], np.ascontiguousarray(cur, dtype=np.float32).view(np.uint32)[keep])
    assert bool(np.all(warped[cmp & want["hole"]] == 0))


# ---- the inputs of the shared cases ------------------------------------------------------------------------------------------------------------
CASES = ("single_pixel", "odd_sizes", "two_poses", "several_workgroups", "bad_values")
ALPHA, TOL = 0.5, 0.05
POSES = (FR.pose([1.0, -2.5, 0.5], [0.2, -0.05, -1.0]), FR.pose([-0.5, 3.0, -1.0], [-0.3, 0.1, 0.9]))


def make_cur(rng, prev, K, T, motion, tol=TOL):
    """A current prediction that keeps every pixel off the threshold: the float64 warp times a factor within 1 +- tol / 4 (half of the pixels),
    or beyond 1 + 3 tol either way (a quarter each); random depths in the holes."""
    wp = warp(prev, K, T, motion)
    pick = rng.integers(0, 4, prev.shape)
    near = rng.uniform(1 - tol / 4, 1 + tol / 4, prev.shape)
    factor = np.where(pick < 2, near, np.where(pick == 2, rng.uniform(1 + 3 * tol, 1.5, prev.shape), 1.0 / rng.uniform(1 + 3 * tol, 1.5, prev.shape)))
    return np.where(wp["hole"], rng.uniform(2.0, 60.0, prev.shape), wp["wv"] * factor).astype(np.float32)


def case_inputs(name):
    """-> dict(prev, cur [N,h,w], K [N,3,3], T [N,4,4], motion [N,3,h,w] or None, alpha, tol): depths in [2, 60] m, |t + m| <= 1.5 m, rotations
    <= 3 degrees -- except the last case's second pose, which moves the camera past the near pixels."""
    rng = np.random.default_rng(sum(map(ord, name)) + 7)
    N, h, w = {"single_pixel": (1, 1, 1), "odd_sizes": (1, 5, 7), "two_poses": (2, 13, 9), "several_workgroups": (2, 33, 47), "bad_values": (2, 11, 23),
               "grid_stride": (1, 600, 900)}[name]          # not in CASES: beyond 2048 workgroups of 256 pixels, for the GPU test of the grid-stride loops
    prev = rng.uniform(2.0, 60.0, (N, h, w)).astype(np.float32)
    K = FR.intrinsics(N, h, w)
    T = np.stack(POSES[:N])
    motion = None
    if name == "single_pixel":
        T = np.eye(4, dtype=np.float32)[None]
    if name in ("two_poses", "several_workgroups"):          # a motion field on the second image alone: the batch boundary
        motion = np.zeros((N, 3, h, w), np.float32)
        motion[1] = rng.uniform(-0.23, 0.23, (3, h, w)).astype(np.float32)
    if name == "bad_values":
        prev[:, 3:6] = rng.uniform(2.0, 2.5, (N, 3, w)).astype(np.float32)            # a near band ...
        prev[:, :3] = np.maximum(prev[:, :3], 6.0)
        prev[:, 6:] = np.maximum(prev[:, 6:], 6.0)
        T[1] = FR.pose([0.5, 1.0, 0.0], [0.1, 0.0, -3.5])                              # ... that the camera of image 1 has driven past: qz = d - 3.5 < 0
        prev[0, 0, 4], prev[1, 8, 2] = np.nan, np.nan
        prev[0, 7, 7], prev[1, 0, 0] = 0.0, 0.0
        prev[0, 9, 20] = np.inf
        prev[1, 10, 1] = -4.0
    cur = make_cur(rng, prev, K, T, motion)
    if name == "bad_values":
        cur[0, 2, 3], cur[1, 5, 5] = 0.0, np.nan
        cur[0, 6, 11], cur[1, 9, 17] = np.nan, 0.0
    return dict(prev=prev, cur=cur, K=K, T=T, motion=motion, alpha=ALPHA, tol=TOL)

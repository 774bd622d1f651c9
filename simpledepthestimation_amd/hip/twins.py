"""What the host twins of the geometry operators share (numpy only): the pinhole camera of csrc/pinhole.h and the z-buffer of csrc/zbuf.h, the
same fp32 operations in the same order, so that a twin and its kernel agree bit for bit."""
import numpy as np

EMPTY = np.uint32(0x7f800000)       # +inf: above every depth that is kept


def pinhole_project_np(d, K, T, m=None):
    """One frame.  d [h,w] depth, K [3,3], T [4,4] (p' = R p + t), m [3,h,w] per-pixel translation or None -> (px, py, qz, X, Y) float32 [h,w]:
    pixel (u, v) lifted through the inverse intrinsics to (px, py, d), moved by [R | t + m] to (qx, qy, qz), projected to (X, Y).  fp32, left to
    right: the order of csrc/pinhole.h."""
    f32 = np.float32
    d, K, T = np.asarray(d, dtype=f32), np.asarray(K, dtype=f32), np.asarray(T, dtype=f32)
    h, w = d.shape
    m = np.asarray(m, dtype=f32) if m is not None else np.zeros((3, h, w), f32)
    fu, fv = np.arange(w, dtype=f32)[None, :], np.arange(h, dtype=f32)[:, None]
    with np.errstate(all="ignore"):
        fx, cx, fy, cy = K[0, 0], K[0, 2], K[1, 1], K[1, 2]
        k00, k11, k02, k12 = f32(1) / fx, f32(1) / fy, (f32(-1) * cx) / fx, (f32(-1) * cy) / fy
        px, py, pz = d * (k00 * fu + k02), d * (k11 * fv + k12), d
        q = [T[r, 0] * px + T[r, 1] * py + T[r, 2] * pz + (T[r, 3] + m[r]) for r in range(3)]
        nx, ny = fx * q[0] + cx * q[2], fy * q[1] + cy * q[2]
        den = q[2] + f32(1e-6)
        return px, py, q[2], nx / den, ny / den


def pinhole_move_project_np(K, T, px, py, pz):
    """Camera-frame points (px, py, pz: float32 arrays of one shape) moved by T [4,4] (q = R p + t) and projected through K [3,3] ->
    (qx, qy, qz, X, Y): pinhole_move<4> with s = t, then pinhole_project, the order of csrc/pinhole.h."""
    f32 = np.float32
    K, T = np.asarray(K, dtype=f32), np.asarray(T, dtype=f32)
    with np.errstate(all="ignore"):
        q = [T[r, 0] * px + T[r, 1] * py + T[r, 2] * pz + T[r, 3] for r in range(3)]
        nx, ny = K[0, 0] * q[0] + K[0, 2] * q[2], K[1, 1] * q[1] + K[1, 2] * q[2]
        den = q[2] + f32(1e-6)
        return q[0], q[1], q[2], nx / den, ny / den


def nearest_pixel_np(X, Y):
    """nearest_pixel of csrc/pinhole.h: (ok, ix, iy) with ix = rint(X), iy = rint(Y) (round-half-even) as int64, ok False where a rounding is
    not below 1e9 in magnitude (a NaN is not); ix, iy are 0 there."""
    with np.errstate(all="ignore"):
        rx, ry = np.rint(np.asarray(X, dtype=np.float32)), np.rint(np.asarray(Y, dtype=np.float32))
        ok = (np.abs(rx) < np.float32(1e9)) & (np.abs(ry) < np.float32(1e9))
        return ok, np.where(ok, rx, 0).astype(np.int64), np.where(ok, ry, 0).astype(np.int64)


def zbuffer_min_np(px, py, values, H, W, keep=None, origin=(0, 0)):
    """px, py: float32 coordinates of the candidates, values: their float32 depths, keep: the candidates the caller admits (all of one shape;
    an admitted depth is positive and finite) -> uint32 [H,W], the smallest bit pattern that lands on each pixel, EMPTY where none does.  A
    candidate lands on (rint(px) - origin[0], rint(py) - origin[1]) -- round-half-even, as rintf -- if both roundings are below 1e9 in
    magnitude (a NaN is not) and the pixel lies inside the map.  Positive floats order like their bit patterns."""
    with np.errstate(all="ignore"):
        rx, ry = np.rint(np.asarray(px, dtype=np.float32)), np.rint(np.asarray(py, dtype=np.float32))
        ok = (np.abs(rx) < np.float32(1e9)) & (np.abs(ry) < np.float32(1e9))
    sel = np.nonzero((ok if keep is None else ok & keep).ravel())[0]
    ix, iy = rx.ravel()[sel].astype(np.int64) - int(origin[0]), ry.ravel()[sel].astype(np.int64) - int(origin[1])
    inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    z = np.full(H * W, EMPTY, dtype=np.uint32)
    np.minimum.at(z, iy[inside] * W + ix[inside], np.ascontiguousarray(values, dtype=np.float32).ravel()[sel][inside].view(np.uint32))
    return z.reshape(H, W)

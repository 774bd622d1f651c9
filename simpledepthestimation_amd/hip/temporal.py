"""Temporally fused depth (include/sde_hip.h: sde_depth_warp_fuse, csrc/temporal.hip): `warp_fuse` binds the kernel, `warp_fuse_host` is its
host twin -- the same fp32 operations in the same order in numpy, for machines without a GPU and for the tests, which compare the two bit for
bit.  The previous frame's depth is forward-projected into the current camera (nearest pixel, closest depth wins), one-pixel holes are closed
from the ring around them, and the result is blended with the current prediction where the two agree within `tol`."""
import numpy as np
import torch

from . import lib as L

NEW, FUSED, NEARER, FARTHER, FILLED = 0, 1, 2, 3, 4        # SDE_TEMPORAL_*: the class in bits 0-1 of `state`, FILLED is bit 2
_EMPTY = np.uint32(0x7f800000)                              # +inf: above every depth that is kept
STATE_COLOURS = np.array([[40, 40, 40], [60, 170, 90], [220, 120, 40], [70, 110, 220]], dtype=np.uint8)      # NEW, FUSED, NEARER, FARTHER


def check_params(alpha, tol):
    """(alpha, tol) as the floats the kernel receives; ValueError for alpha outside [0, 1) or tol <= 0 (a NaN fails both)."""
    alpha, tol = float(np.float32(alpha)), float(np.float32(tol))
    if not 0.0 <= alpha < 1.0:
        raise ValueError(f"warp_fuse: alpha must lie in [0, 1), got {alpha!r}")
    if not tol > 0.0:
        raise ValueError(f"warp_fuse: tol must be positive, got {tol!r}")
    return alpha, tol


def warp_fuse(prev, cur, K, T, motion=None, alpha=0.5, tol=0.05, out=None, want_state=True, want_warped=False, zbuf=None, state=None, warped=None):
    """prev, cur [N,h,w] fp32 (the previous frame's fused depth, the current prediction), K [N,3,3] or [3,3] fp32 at THAT size, T [N,4,4] fp32
    (the pose previous -> current, p_cur = R p_prev + t), motion [N,3,h,w] fp32 or None (a per-pixel translation on the previous frame's grid):
    CUDA tensors.  Returns (fused [N,h,w] fp32, state [N,h,w] uint8, warped [N,h,w] fp32), the last two None when not asked for.  out: the
    destination of `fused`; it may be `prev` or `cur` (a state buffer updated in place).  zbuf: an int32 [N,h,w] workspace (allocated when
    None); state / warped: optional destinations.  Three launches on the current stream, no host synchronisation."""
    alpha, tol = check_params(alpha, tol)
    for name, t in (("prev", prev), ("cur", cur)):
        if not torch.is_tensor(t) or t.dim() != 3 or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise L.SdeHipError(f"warp_fuse: {name} must be a contiguous float32 [N,h,w] device tensor")
    N, h, w = prev.shape
    dev = prev.device
    if tuple(cur.shape) != (N, h, w):
        raise L.SdeHipError(f"warp_fuse: prev {tuple(prev.shape)} and cur {tuple(cur.shape)} differ")
    if N <= 0 or h <= 0 or w <= 0:
        raise L.SdeHipError(f"warp_fuse: N, h and w must be positive ({N}, {h}, {w})")
    if K.dim() == 2:
        K = K[None].expand(N, 3, 3)
    for name, t, shape in (("K", K, (N, 3, 3)), ("T", T, (N, 4, 4)), ("motion", motion, (N, 3, h, w))):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shape or t.device != dev):
            raise L.SdeHipError(f"warp_fuse: {name} must be a float32 {list(shape)} tensor on {dev}, got {t.dtype} {tuple(t.shape)}")

    def dst(t, dtype, want, name):
        if not want:
            return None
        if t is None:
            return torch.empty((N, h, w), dtype=dtype, device=dev)
        if t.dtype != dtype or tuple(t.shape) != (N, h, w) or t.device != dev or not t.is_contiguous():
            raise L.SdeHipError(f"warp_fuse: {name} must be a contiguous {dtype} [{N},{h},{w}] tensor on {dev}, got {t.dtype} {tuple(t.shape)}")
        return t
    fused = dst(out, torch.float32, True, "out")
    state = dst(state, torch.uint8, want_state, "state")
    warped = dst(warped, torch.float32, want_warped, "warped")
    zbuf = dst(zbuf, torch.int32, True, "zbuf")
    L.check(L.lib().sde_depth_warp_fuse(L.ptr(prev), L.ptr(cur), L.ptr(K.contiguous()), L.ptr(T.contiguous()),
                                        L.ptr(motion.contiguous() if motion is not None else None), N, h, w, alpha, tol, L.ptr(zbuf), L.ptr(fused),
                                        L.ptr(state), L.ptr(warped), L.stream()), "sde_depth_warp_fuse")
    return fused, state, warped


def warp_fuse_host(prev, cur, K, T, motion=None, alpha=0.5, tol=0.05):
    """The host twin: numpy arrays of the shapes `warp_fuse` takes -> (fused [N,h,w] float32, state [N,h,w] uint8, warped [N,h,w] float32), the
    bits sde_depth_warp_fuse writes."""
    alpha, tol = check_params(alpha, tol)
    f32 = np.float32
    prev, cur = np.asarray(prev, dtype=f32), np.asarray(cur, dtype=f32)
    N, h, w = prev.shape
    K = np.array(np.broadcast_to(np.asarray(K, dtype=f32), (N, 3, 3)))
    T = np.asarray(T, dtype=f32).reshape(N, 4, 4)
    fu, fv = np.arange(w, dtype=f32)[None, :], np.arange(h, dtype=f32)[:, None]
    fused, state, warped = np.empty((N, h, w), f32), np.empty((N, h, w), np.uint8), np.empty((N, h, w), f32)
    with np.errstate(all="ignore"):
        for n in range(N):
            fx, cx, fy, cy = K[n, 0, 0], K[n, 0, 2], K[n, 1, 1], K[n, 1, 2]
            k00, k11, k02, k12 = f32(1) / fx, f32(1) / fy, (f32(-1) * cx) / fx, (f32(-1) * cy) / fy
            d = prev[n]
            m = np.asarray(motion[n], dtype=f32) if motion is not None else np.zeros((3, h, w), f32)
            px, py, pz = d * (k00 * fu + k02), d * (k11 * fv + k12), d
            q = [T[n, r, 0] * px + T[n, r, 1] * py + T[n, r, 2] * pz + (T[n, r, 3] + m[r]) for r in range(3)]        # fp32, left to right: the kernel's order
            nx, ny = fx * q[0] + cx * q[2], fy * q[1] + cy * q[2]
            den = q[2] + f32(1e-6)
            X, Y = nx / den, ny / den
            keep = np.isfinite(d) & (d > 0) & (q[2] > 0) & np.isfinite(q[2]) & np.isfinite(X) & np.isfinite(Y)
            rx, ry = np.rint(X), np.rint(Y)                                                                           # round-half-even, as rintf
            keep &= (np.abs(rx) < f32(1e9)) & (np.abs(ry) < f32(1e9))
            sel = np.nonzero(keep.ravel())[0]
            ix, iy = rx.ravel()[sel].astype(np.int64), ry.ravel()[sel].astype(np.int64)
            inside = (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
            z = np.full(h * w, _EMPTY, dtype=np.uint32)
            np.minimum.at(z, iy[inside] * w + ix[inside], np.ascontiguousarray(q[2], dtype=f32).ravel()[sel][inside].view(np.uint32))
            z = z.reshape(h, w)
            ring = np.full((h + 2, w + 2), _EMPTY, dtype=np.uint32)                                                  # outside the image: empty
            ring[1:-1, 1:-1] = z
            near = np.full((h, w), _EMPTY, dtype=np.uint32)
            for dy in range(3):
                for dx in range(3):
                    if (dy, dx) != (1, 1):
                        near = np.minimum(near, ring[dy:dy + h, dx:dx + w])
            empty = z == _EMPTY
            filled = empty & (near != _EMPTY)
            z = np.where(empty, near, z)
            hole = z == _EMPTY
            wv = np.where(hole, f32(0), z.view(f32)).astype(f32)
            c = cur[n]
            usable = ~hole & np.isfinite(c) & (c > 0)
            diff = wv - c
            lim = f32(tol) * np.fmin(wv, c)
            consistent = usable & (np.abs(diff) <= lim)
            fused[n] = np.where(consistent, c + f32(alpha) * diff, c)
            cls = np.where(~usable, NEW, np.where(consistent, FUSED, np.where(diff < 0, NEARER, np.where(diff > 0, FARTHER, NEW))))
            state[n] = (cls | np.where(filled, FILLED, 0)).astype(np.uint8)
            warped[n] = wv
    return fused, state, warped


def state_picture(state):
    """state [h,w] uint8 -> RGB uint8 [h,w,3]: the class in four fixed colours (NEW dark grey, FUSED green, NEARER orange, FARTHER blue)."""
    return STATE_COLOURS[np.asarray(state) & 3]

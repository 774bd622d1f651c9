"""Temporally fused depth (include/sde_hip.h: sde_depth_warp_fuse, csrc/temporal.hip): `warp_fuse` binds the kernel, `warp_fuse_host` is its
host twin -- the same fp32 operations in the same order in numpy, for machines without a GPU and for the tests, which compare the two bit for
bit.  The previous frame's depth is forward-projected into the current camera (nearest pixel, closest depth wins), one-pixel holes are closed
from the ring around them, and the result is blended with the current prediction where the two agree within `tol`."""
import numpy as np
import torch

from . import args as A
from . import lib as L
from .twins import EMPTY as _EMPTY, pinhole_project_np, zbuffer_min_np

NEW, FUSED, NEARER, FARTHER, FILLED = 0, 1, 2, 3, 4        # SDE_TEMPORAL_*: the class in bits 0-1 of `state`, FILLED is bit 2
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
    # prev and cur are not copied (`out` may be either of them): lib.ptr refuses a non-contiguous one
    dev = prev.device if torch.is_tensor(prev) else None
    N, h, w = A.same_device_tensor("warp_fuse", "prev", prev, torch.float32, (None, None, None), dev).shape
    A.same_device_tensor("warp_fuse", "cur", cur, torch.float32, (N, h, w), dev)
    if N <= 0 or h <= 0 or w <= 0:
        raise L.SdeHipError(f"warp_fuse: N, h and w must be positive ({N}, {h}, {w})")
    K = A.as_K("warp_fuse", K, N, dev)
    T = A.same_device_tensor("warp_fuse", "T", T, torch.float32, (N, 4, 4), dev)
    if motion is not None:
        motion = A.same_device_tensor("warp_fuse", "motion", motion, torch.float32, (N, 3, h, w), dev).contiguous()
    fused = A.dst("warp_fuse", out, (N, h, w), torch.float32, True, dev)
    state = A.dst("warp_fuse", state, (N, h, w), torch.uint8, want_state, dev)
    warped = A.dst("warp_fuse", warped, (N, h, w), torch.float32, want_warped, dev)
    zbuf = A.dst("warp_fuse", zbuf, (N, h, w), torch.int32, True, dev)
    L.check(L.lib().sde_depth_warp_fuse(L.ptr(prev), L.ptr(cur), L.ptr(K), L.ptr(T.contiguous()), L.ptr(motion), N, h, w, alpha, tol, L.ptr(zbuf),
                                        L.ptr(fused), L.ptr(state), L.ptr(warped), L.stream()), "sde_depth_warp_fuse")
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
    fused, state, warped = np.empty((N, h, w), f32), np.empty((N, h, w), np.uint8), np.empty((N, h, w), f32)
    with np.errstate(all="ignore"):
        for n in range(N):
            d = prev[n]
            _, _, qz, X, Y = pinhole_project_np(d, K[n], T[n], motion[n] if motion is not None else None)
            keep = np.isfinite(d) & (d > 0) & (qz > 0) & np.isfinite(qz) & np.isfinite(X) & np.isfinite(Y)
            z = zbuffer_min_np(X, Y, qz, h, w, keep=keep)
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

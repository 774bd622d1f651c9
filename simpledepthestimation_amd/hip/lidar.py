"""Raw LiDAR scans -> sparse depth maps (include/sde_hip.h: sde_lidar_depth, csrc/lidar.hip): `lidar_depth` binds the kernel, `lidar_depth_np` is
its host twin -- the same fp32 operations in the same order in numpy, one scan at a time, for the data loader's workers and for machines without
a GPU.  Both follow generate_depth_map of monodepth2 / packnet-sfm with the one deviation the header documents (w > 0 and d > 0)."""
import numpy as np
import torch

from . import args as A
from . import lib as L
from .twins import EMPTY as _EMPTY, zbuffer_min_np

VEL_DEPTH, FRONT_ONLY = 1, 2        # SDE_LIDAR_VEL_DEPTH, SDE_LIDAR_FRONT_ONLY


def flag_bits(vel_depth=False, front_only=True):
    return (VEL_DEPTH if vel_depth else 0) | (FRONT_ONLY if front_only else 0)


def lidar_depth(points, count, proj, origin, H, W, vel_depth=False, front_only=True, max_depth=None, out=None):
    """points [B,cap,3 or 4] fp32, count [B] int32 (valid rows per scan), proj [B,3,4] fp32 (the scanner-to-image matrix, geometry.camera's
    velo_to_image), origin [B,2] int32 (x0, y0 of the H x W window in full-image pixels): CUDA tensors.  Returns depth [B,1,H,W] fp32 (`out` when
    given): the closest point per pixel, 0 where none lands, min(d, max_depth) with a max_depth > 0.  Three launches on the current stream, no
    host synchronisation."""
    H, W = int(H), int(W)
    dev = points.device if torch.is_tensor(points) else None
    B, cap, stride = A.same_device_tensor("lidar_depth", "points", points, torch.float32, (None, None, None), dev).shape
    if stride not in (3, 4):
        raise L.SdeHipError(f"lidar_depth: points must be [B,cap,3 or 4], got {tuple(points.shape)}")
    for what, t, dtype, shape in (("count", count, torch.int32, (B,)), ("proj", proj, torch.float32, (B, 3, 4)), ("origin", origin, torch.int32, (B, 2))):
        A.same_device_tensor("lidar_depth", what, t, dtype, shape, dev)
    if H <= 0 or W <= 0 or cap <= 0:
        raise L.SdeHipError(f"lidar_depth: H, W and the scan capacity must be positive (H={H}, W={W}, cap={cap})")
    out = A.dst("lidar_depth", out, (B, 1, H, W), torch.float32, True, dev)
    L.check(L.lib().sde_lidar_depth(L.ptr(points.contiguous()), cap, stride, L.ptr(count.contiguous()), B, L.ptr(proj.contiguous()), L.ptr(origin.contiguous()),
                                    H, W, flag_bits(vel_depth, front_only), float(max_depth) if max_depth else 0.0, L.ptr(out), L.stream()), "sde_lidar_depth")
    return out


def lidar_depth_np(points, proj, origin, H, W, vel_depth=False, front_only=True, max_depth=None):
    """The host twin, one scan: points [N,>=3] (x, y, z in the leading columns), proj [3,4], origin (x0, y0) -> depth [H,W] float32, the bits
    sde_lidar_depth writes."""
    pts = np.asarray(points, dtype=np.float32)
    m = np.asarray(proj, dtype=np.float32).reshape(3, 4)
    x, y, z = (np.ascontiguousarray(pts[:, i]) for i in range(3))
    x0, y0 = int(origin[0]), int(origin[1])
    H, W = int(H), int(W)
    with np.errstate(all="ignore"):
        u, v, w = (m[r, 0] * x + m[r, 1] * y + m[r, 2] * z + m[r, 3] for r in range(3))        # fp32, left to right: the kernel's order
        d = x if vel_depth else w
        keep = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (w > 0) & (d > 0) & (d < np.inf)
        if front_only:
            keep &= x >= 0
        # u / w and v / w in place: as two more 0.5 MB temporaries per scan they cost a loader worker 1.5 ms of page faults on a 4 ms call (measured)
        bits = zbuffer_min_np(np.divide(u, w, out=u), np.divide(v, w, out=v), d, H, W, keep=keep, origin=(1 + x0, 1 + y0))      # the routine's 1-based pixel
    bits[bits == _EMPTY] = 0
    depth = bits.view(np.float32)
    if max_depth and max_depth > 0:
        depth = np.minimum(depth, np.float32(max_depth))
    return depth

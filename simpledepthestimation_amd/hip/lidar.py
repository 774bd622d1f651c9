"""Raw LiDAR scans -> sparse depth maps (include/sde_hip.h: sde_lidar_depth, csrc/lidar.hip): `lidar_depth` binds the kernel, `lidar_depth_np` is
its host twin -- the same fp32 operations in the same order in numpy, one scan at a time, for the data loader's workers and for machines without
a GPU.  Both follow generate_depth_map of monodepth2 / packnet-sfm with the one deviation the header documents (w > 0 and d > 0)."""
import numpy as np
import torch

from . import lib as L

VEL_DEPTH, FRONT_ONLY = 1, 2        # SDE_LIDAR_VEL_DEPTH, SDE_LIDAR_FRONT_ONLY
_EMPTY = np.uint32(0x7f800000)      # +inf: above every depth that is kept


def flag_bits(vel_depth=False, front_only=True):
    return (VEL_DEPTH if vel_depth else 0) | (FRONT_ONLY if front_only else 0)


def lidar_depth(points, count, proj, origin, H, W, vel_depth=False, front_only=True, max_depth=None, out=None):
    """points [B,cap,3 or 4] fp32, count [B] int32 (valid rows per scan), proj [B,3,4] fp32 (the scanner-to-image matrix, geometry.camera's
    velo_to_image), origin [B,2] int32 (x0, y0 of the H x W window in full-image pixels): CUDA tensors.  Returns depth [B,1,H,W] fp32 (`out` when
    given): the closest point per pixel, 0 where none lands, min(d, max_depth) with a max_depth > 0.  Three launches on the current stream, no
    host synchronisation."""
    H, W = int(H), int(W)
    if points.dim() != 3 or points.shape[2] not in (3, 4) or points.dtype != torch.float32 or not points.is_cuda:
        raise L.SdeHipError(f"lidar_depth: points must be a float32 [B,cap,3 or 4] device tensor, got {points.dtype} {tuple(points.shape)} on {points.device}")
    B, cap, stride = points.shape
    dev = points.device
    for name, t, dtype, shape in (("count", count, torch.int32, (B,)), ("proj", proj, torch.float32, (B, 3, 4)), ("origin", origin, torch.int32, (B, 2))):
        if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or t.device != dev:
            raise L.SdeHipError(f"lidar_depth: {name} must be a {dtype} {list(shape)} tensor on {dev}, got "
                                f"{(t.dtype, tuple(t.shape), str(t.device)) if torch.is_tensor(t) else type(t).__name__}")
    if H <= 0 or W <= 0 or cap <= 0:
        raise L.SdeHipError(f"lidar_depth: H, W and the scan capacity must be positive (H={H}, W={W}, cap={cap})")
    if out is None:
        out = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, 1, H, W) or out.device != dev or not out.is_contiguous():
        raise L.SdeHipError(f"lidar_depth: out must be a contiguous float32 [{B},1,{H},{W}] tensor on {dev}, got {out.dtype} {tuple(out.shape)}")
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
        ru, rv = np.rint(u / w), np.rint(v / w)                                                   # round-half-even, as rintf
        keep &= (np.abs(ru) < 1e9) & (np.abs(rv) < 1e9)
    sel = np.nonzero(keep)[0]
    px = ru[sel].astype(np.int64) - 1 - x0
    py = rv[sel].astype(np.int64) - 1 - y0
    inside = (px >= 0) & (px < W) & (py >= 0) & (py < H)
    bits = np.full(H * W, _EMPTY, dtype=np.uint32)
    np.minimum.at(bits, py[inside] * W + px[inside], d[sel][inside].view(np.uint32))          # positive floats order like their bit patterns
    bits[bits == _EMPTY] = 0
    depth = bits.view(np.float32).reshape(H, W)
    if max_depth and max_depth > 0:
        depth = np.minimum(depth, np.float32(max_depth))
    return depth

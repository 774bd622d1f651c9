"""Helper (no tests): numpy / torch restatement of the point-cloud kernels' definitions in include/sde_hip.h, written from the formulas, and the
inputs of the GPU cases.

Compacted cloud: the restored depth is read through the index maps (-1 = outside: 0); the keep decision is made on the float32 value (finite and
min_depth < d <= max_depth, both limits as float32); the kept pixels follow in raster order; the coordinates are float64:
x = d (u - cx) / fx, y = d (v - cy) / fy, z = d.

Bound on the kernel's float32 x (y alike), per element, from the documented evaluation order
    Kinv00 = 1 / fx;  Kinv02 = (-1 * cx) / fx;  x = d * (Kinv00 * u + Kinv02)
u and d are exact float32 values, the negation is exact, so the roundings are five: the division 1 / fx, the product Kinv00 * u, the division
cx / fx, the sum, the product with d.  The first term of the sum passes four of them, the second three; to first order
    |x_fp32 - x| <= 2^-24 * |d| * (4 |Kinv00 u| + 3 |Kinv02|) <= 2^-24 * k * |d| * (|Kinv00 u| + |Kinv02|)   with k = 4;
K_BOUND = 5 counts all five roundings, which leaves the second-order terms (products of two 2^-24 errors) and the float64 evaluation of this
restatement inside the bound.  Nothing is measured from the kernel.  z is a copy: bit-exact.

Dense mode: img_to_points in torch, any dtype, differentiated by autograd."""
import numpy as np
import torch

K_BOUND = 5
TILE = 256            # candidates per workgroup in csrc/cloud.hip: the cases below are sized from it


def restore(pred, ymap, xmap):
    """pred [N,ph,pw] float32 -> [N,H,W] float32 through the maps."""
    inside = (ymap >= 0)[:, None] & (xmap >= 0)[None, :]
    full = pred[:, np.maximum(ymap, 0)][:, :, np.maximum(xmap, 0)]
    return np.where(inside[None], full, np.float32(0)).astype(np.float32)


def cloud(pred, ymap, xmap, K, min_depth, max_depth, step=1, frame=None):
    """-> per frame a dict: u, v (the kept pixels in raster order), xyz float64 [count,3], z float32 [count], rgba uint8 [count,4],
    bound float64 [count,2] (on |x|, |y| errors)."""
    full = restore(pred, ymap, xmap)
    N, H, W = full.shape
    lo, hi = np.float32(min_depth), np.float32(max_depth)
    out = []
    for n in range(N):
        sub = full[n, ::step, ::step]
        with np.errstate(invalid="ignore"):
            keep = np.isfinite(sub) & (lo < sub) & (sub <= hi)
        vc, uc = np.nonzero(keep)                                  # row-major: raster order
        u, v = uc * step, vc * step
        z = sub[vc, uc]
        d = z.astype(np.float64)
        fx, cx, fy, cy = (float(K[n, 0, 0]), float(K[n, 0, 2]), float(K[n, 1, 1]), float(K[n, 1, 2]))
        xyz = np.stack([d * (u - cx) / fx, d * (v - cy) / fy, d], 1)
        bound = 2.0 ** -24 * K_BOUND * np.abs(d)[:, None] * np.stack([np.abs(u / fx) + abs(cx / fx), np.abs(v / fy) + abs(cy / fy)], 1)
        rgba = np.full((z.size, 4), 255, np.uint8)
        if frame is not None:
            rgba[:, :3] = frame[n, v, u]
        out.append(dict(u=u, v=v, xyz=xyz, z=z, rgba=rgba, bound=bound))
    return out


def capacity(H, W, step):
    return -(-H // step) * -(-W // step)


def img_to_points(depth, R, t):
    """depth [B,1,H,W], R [B,3,3], t [B,3,1] or [B,3,H*W] torch tensors of one dtype -> [B,3,H,W]."""
    B, _, H, W = depth.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=depth.dtype), torch.arange(W, dtype=depth.dtype), indexing="ij")
    grid = torch.stack([xs, ys, torch.ones_like(xs)], 0)[None] * depth                        # [B,3,H,W]
    return (R.bmm(grid.reshape(B, 3, -1)) + t).reshape(B, 3, H, W)


def img_to_points_grads(depth, R, t, cot, dtype):
    """Forward and the gradients of sum(points * cot) in `dtype`: (points, ddepth, dR, dt), detached."""
    d, r, tt = (x.detach().clone().to(dtype).requires_grad_(True) for x in (depth, R, t))
    p = img_to_points(d, r, tt)
    (p * cot.to(dtype)).sum().backward()
    return p.detach(), d.grad, r.grad, tt.grad


def dense_inputs(H, W, per_pixel, seed):
    g = torch.Generator().manual_seed(seed)
    B = 2
    depth = torch.rand(B, 1, H, W, generator=g) * 60 + 1
    R = torch.randn(B, 3, 3, generator=g)
    t = torch.randn(B, 3, H * W if per_pixel else 1, generator=g)
    cot = torch.randn(B, 3, H, W, generator=g)
    return depth, R, t, cot


# ---- the inputs of the compacted-cloud cases ---------------------------------------------------------------------------------------------------
MIN_D, MAX_D = 1.0, 80.0
CASES = ("one_partial_block", "all_kept", "none_kept", "several_blocks_ragged", "scan_wider_than_one_wave", "scan_more_than_one_chunk",
         "two_frames_different_counts", "maps_with_outside", "step_3_odd_sizes", "nan_inf_and_bounds", "no_frame")


def _K(N, H, W):
    K = np.zeros((N, 3, 3), np.float32)
    for n in range(N):
        K[n] = [[721.5 - 200 * n, 0, W / 2 + 0.37 + n], [0, 715.25 - 190 * n, H / 2 - 0.21 - n], [0, 0, 1]]
    return K


def case_inputs(name):
    """-> dict(pred [N,ph,pw] float32, ymap [H], xmap [W] int32, frame [N,H,W,3] uint8 or None, K [N,3,3] float32, min_depth, max_depth, step)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    N, step, with_frame = 1, 1, True
    H, W = {"one_partial_block": (3, 5), "all_kept": (16, 20), "none_kept": (16, 20), "several_blocks_ragged": (37, 61),          # 2257 = 8 tiles + 209
            "scan_wider_than_one_wave": (131, 127),       # 16637 candidates = 65 workgroups: their counts span two waves of the scan
            "scan_more_than_one_chunk": (260, 257),       # 66820 candidates = 262 workgroups: the scan's second chunk of TILE counts, with a carry
            "two_frames_different_counts": (37, 61), "maps_with_outside": (27, 48), "step_3_odd_sizes": (37, 61), "nan_inf_and_bounds": (3, 5),
            "no_frame": (9, 31)}[name]
    ymap, xmap = np.arange(H, dtype=np.int32), np.arange(W, dtype=np.int32)
    ph, pw = H, W

    def depths(n, share_kept):
        d = rng.uniform(MIN_D + 0.5, MAX_D - 0.5, (n, ph, pw)).astype(np.float32)
        drop = rng.random((n, ph, pw)) >= share_kept
        return np.where(drop, np.where(rng.random((n, ph, pw)) < 0.5, np.float32(0.25), np.float32(95.0)), d).astype(np.float32)

    if name == "all_kept":
        pred = depths(1, 1.1)
    elif name == "none_kept":
        pred = depths(1, -1.0)
    elif name == "two_frames_different_counts":
        N = 2
        pred = np.concatenate([depths(1, 0.8), depths(1, 0.3)], 0)
    elif name == "maps_with_outside":                     # a prediction of half the size pasted into a larger frame: borders of -1 on three sides
        ph, pw = 10, 20
        ymap = np.concatenate([np.full(7, -1), np.arange(20) // 2]).astype(np.int32)
        xmap = np.concatenate([np.full(4, -1), np.arange(40) // 2, np.full(4, -1)]).astype(np.int32)
        pred = depths(1, 0.9)
    elif name == "nan_inf_and_bounds":
        lo, hi = np.float32(MIN_D), np.float32(MAX_D)
        pred = np.array([np.nan, np.inf, -np.inf, lo, hi, np.nextafter(lo, np.float32(0)), np.nextafter(lo, np.float32(2)), np.nextafter(hi, np.float32(0)),
                         np.nextafter(hi, np.float32(100)), 0.0, -0.0, -5.0, 40.0, 1e-38, 3e38], np.float32).reshape(1, 3, 5)
    else:
        if name == "step_3_odd_sizes":
            step = 3
        if name == "no_frame":
            with_frame = False
        pred = depths(1, 0.6)
    frame = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8) if with_frame else None
    return dict(pred=pred, ymap=ymap, xmap=xmap, frame=frame, K=_K(N, H, W), min_depth=MIN_D, max_depth=MAX_D, step=step)

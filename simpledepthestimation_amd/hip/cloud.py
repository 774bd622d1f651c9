"""ctypes binding of the point-cloud kernels (include/sde_hip.h, csrc/cloud.hip): sde_depth_cloud -- network outputs -> compacted, coloured
16-byte point records per frame, three launches, no host synchronisation -- and the dense, differentiable img_to_points."""
import numpy as np
import torch

from . import args as A
from . import lib as L
from . import present as HP

RECORD = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])
assert RECORD.itemsize == 16


def capacity(H, W, step=1):
    """Records a frame of H x W can yield at this step: ceil(H / step) * ceil(W / step)."""
    if int(step) < 1 or H <= 0 or W <= 0:
        raise ValueError(f"depth_cloud: H, W must be positive and step at least 1 (H={H}, W={W}, step={step})")
    return -(-int(H) // int(step)) * -(-int(W) // int(step))


def check_range(min_depth, max_depth, step):
    """The argument errors sde_depth_cloud refuses, raised as ValueError before anything touches the device."""
    if int(step) != step or int(step) < 1:
        raise ValueError(f"depth_cloud: step must be an integer >= 1, got {step!r}")
    if not float(min_depth) < float(max_depth):
        raise ValueError(f"depth_cloud: min_depth must lie below max_depth, got ({min_depth}, {max_depth})")
    return float(min_depth), float(max_depth), int(step)


def depth_cloud(pred, ymap, xmap, K, min_depth, max_depth, step=1, frame=None, out=None, workspace=None):
    """pred [N,ph,pw] (or [N,1,ph,pw] / [ph,pw]) fp32, ymap [H] / xmap [W] int32 (hip.present's maps: device tensors, or host arrays that are
    validated and uploaded), K [N,3,3] or [3,3] fp32 at the restored size, frame [N,H,W,3] uint8 or None (white points): CUDA tensors.
    Returns (points [N,cap,16] uint8, count [N] int32) on the device: frame n's records are points[n, :count[n]] in raster order (as_records
    gives the structured view); what lies behind them is whatever the buffer held.  out: optional (points, count) destinations; workspace:
    optional int32 tensor of at least workspace_numel(N, H, W, step) elements.  No host synchronisation (device maps: see depth_present)."""
    min_depth, max_depth, step = check_range(min_depth, max_depth, step)
    pred = A.as_pred("depth_cloud", pred)
    N, ph, pw = pred.shape
    dev = pred.device
    ymap, xmap = HP.ensure_checked(ymap, xmap, ph, pw, dev)
    H, W = ymap.numel(), xmap.numel()
    K = A.as_K("depth_cloud", K, N, dev)
    frame = A.as_frame("depth_cloud", frame, N, H, W, dev)
    cap = capacity(H, W, step)
    points, count = out if out is not None else (None, None)
    points = A.dst("depth_cloud", points, (N, cap, 16), torch.uint8, True, dev)
    count = A.dst("depth_cloud", count, (N,), torch.int32, True, dev)
    need = workspace_numel(N, H, W, step)
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.int32, device=dev)
    if workspace.dtype != torch.int32 or workspace.device != dev:
        raise L.SdeHipError(f"depth_cloud: workspace must be an int32 tensor on {dev}, got {workspace.dtype} on {workspace.device}")
    L.check(L.lib().sde_depth_cloud(L.ptr(pred), N, ph, pw, L.ptr(ymap), L.ptr(xmap), H, W, L.ptr(frame), L.ptr(K), min_depth, max_depth, step,
                                    L.ptr(workspace), workspace.numel() * 4, L.ptr(points), L.ptr(count), L.stream()), "sde_depth_cloud")
    return points, count


def workspace_numel(N, H, W, step=1):
    """int32 elements of workspace sde_depth_cloud asks for."""
    n = int(L.lib().sde_depth_cloud_ws_bytes(int(N), int(H), int(W), int(step)))
    if n == 0:
        raise L.SdeHipError(f"depth_cloud: unsupported size (N={N}, {H}x{W}, step {step})")
    return n // 4


def as_records(points, count):
    """points [N,cap,16] uint8 and count [N] (tensors or arrays; device tensors are copied to the host, which synchronises) -> a list of N numpy
    structured arrays with the fields x, y, z (float32), red, green, blue, alpha (uint8), cut at count[n]; views of host memory where the input
    was host memory.  points [cap,16] with a scalar count gives the one array."""
    p = points.cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    c = np.atleast_1d(count.cpu().numpy() if torch.is_tensor(count) else np.asarray(count))
    if p.dtype != np.uint8 or p.shape[-1] != 16 or p.ndim not in (2, 3):
        raise ValueError(f"as_records: points must be uint8 [N,cap,16] or [cap,16], got {p.dtype} {p.shape}")
    single = p.ndim == 2
    if single:
        p = p[None]
    if c.shape != (p.shape[0],) or int(c.min()) < 0 or int(c.max()) > p.shape[1]:
        raise ValueError(f"as_records: count {c.tolist()} does not fit points {p.shape}")
    p = np.ascontiguousarray(p)
    recs = [p[n].view(RECORD).reshape(-1)[:int(c[n])] for n in range(p.shape[0])]
    return recs[0] if single else recs


class _ImgToPoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, R, t):
        B, _, H, W = depth.shape
        d, r, tt = depth.contiguous(), R.contiguous(), t.contiguous()
        out = torch.empty((B, 3, H, W), dtype=torch.float32, device=depth.device)
        L.check(L.lib().sde_img_to_points_fwd(L.ptr(d), L.ptr(r), L.ptr(tt), int(t.shape[2] != 1), B, H, W, L.ptr(out), L.stream()), "sde_img_to_points_fwd")
        ctx.save_for_backward(d, r)
        ctx.t_shape = tuple(t.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        d, r = ctx.saved_tensors
        B, _, H, W = d.shape
        g = g.contiguous()
        need_d, need_R, need_t = ctx.needs_input_grad
        per_pixel = ctx.t_shape[2] != 1
        dd = dR = dt = None
        want_dt = need_t and not per_pixel
        if need_d or need_R or want_dt:          # a per-pixel t alone needs no launch; depth alone skips the sums and their finishing launch
            sums = need_R or want_dt
            part = torch.empty((B, L.lib().sde_img_to_points_num_blocks(H, W), 12), dtype=torch.float32, device=d.device) if sums else None
            dd = torch.empty_like(d)
            dR = torch.empty_like(r) if need_R else None
            dt = torch.empty((B, 3, 1), dtype=torch.float32, device=d.device) if want_dt else None
            L.check(L.lib().sde_img_to_points_bwd(L.ptr(g), L.ptr(d), L.ptr(r), B, H, W, L.ptr(part), L.ptr(dd), L.ptr(dR), L.ptr(dt), L.stream()),
                    "sde_img_to_points_bwd")
        if per_pixel and need_t:
            dt = g.reshape(B, 3, H * W)
        return (dd if need_d else None), (dR if need_R else None), dt


def img_to_points(depth, R, t):
    """depth [B,1,H,W], R [B,3,3], t [B,3,1] or [B,3,H*W], float32 device tensors -> points [B,3,H,W] = R (d [u,v,1]) + t; differentiable in all three."""
    if depth.dim() != 4 or depth.shape[1] != 1 or R.dim() != 3 or t.dim() != 3:
        raise L.SdeHipError(f"img_to_points: depth [B,1,H,W], R [B,3,3], t [B,3,1 or H*W] expected, got {tuple(depth.shape)}, {tuple(R.shape)}, {tuple(t.shape)}")
    B, _, H, W = depth.shape
    if tuple(R.shape) != (B, 3, 3) or tuple(t.shape[:2]) != (B, 3) or t.shape[2] not in (1, H * W):
        raise L.SdeHipError(f"img_to_points: R [{B},3,3] and t [{B},3,1] or [{B},3,{H * W}] expected, got {tuple(R.shape)} and {tuple(t.shape)}")
    if any(x.dtype != torch.float32 or not x.is_cuda for x in (depth, R, t)):
        raise L.SdeHipError("img_to_points: float32 device tensors expected; there is no CPU fallback")
    return _ImgToPoints.apply(depth, R, t)

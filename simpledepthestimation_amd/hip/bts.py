"""Autograd wrappers of the BTS decoder's operators (csrc/bts.hip, include/sde_hip.h "BTS decoder operators").

Activations are NHWC in the compute dtype with channels padded to the 16-byte group; the per-pixel depth maps the decoder returns (LPG
outputs, reduc1x1, the final depth) are planar [B,1,H,W] fp32, as in the reference.
"""
import ctypes
from ctypes import Structure, c_int32, c_void_p

import torch

from . import lib as L
from . import nn as HN

CAT_MAX = 6          # SDE_CAT_MAX
STATS_ROWS = 256     # SDE_STATS_ROWS


class CatPiece(Structure):
    _fields_ = [("p", c_void_p), ("C", c_int32), ("ld", c_int32), ("f32map", c_int32), ("reserved", c_int32)]


# prototypes: hip/lib.py (_PROTOS, "BTS decoder operators")


def _dt(t):
    return HN.dtype_code(t.dtype)


# ---------------------------------------------------------------------------------------------------------------
# dilated 3x3 convolution = split -> 3x3 pad-1 convolution (conv engine) -> merge
# ---------------------------------------------------------------------------------------------------------------
def _split(x, d):
    B, H, W, C = x.shape
    Hs, Ws = -(-H // d), -(-W // d)
    out = torch.empty(B * d * d, Hs, Ws, C, device=x.device, dtype=x.dtype)
    L.check(L.lib().sde_dilate_split(L.ptr(x), B, H, W, C, d, _dt(x), L.ptr(out), L.stream()), "sde_dilate_split")
    return out


def _merge(sub, B, H, W, d):
    C = sub.shape[3]
    out = torch.empty(B, H, W, C, device=sub.device, dtype=sub.dtype)
    L.check(L.lib().sde_dilate_merge(L.ptr(sub), B, H, W, C, d, _dt(sub), L.ptr(out), L.stream()), "sde_dilate_merge")
    return out


class _DilateSplit(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, d):
        ctx.cfg = (x.shape[0], x.shape[1], x.shape[2], d)
        return _split(x, d)

    @staticmethod
    def backward(ctx, dsub):
        B, H, W, d = ctx.cfg
        return _merge(dsub.contiguous(), B, H, W, d), None


class _DilateMerge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sub, B, H, W, d):
        ctx.d = d
        return _merge(sub, B, H, W, d)

    @staticmethod
    def backward(ctx, dy):
        return _split(dy.contiguous(), ctx.d), None, None, None, None


def dilated_conv3x3(conv, x, d):
    """nn.Conv2d(k=3, stride=1, padding=d, dilation=d, bias=False) of atrous_conv (BTSNet.py:L57-62) on NHWC x; conv: a HipConv2d (k=3, pad=1)."""
    if d == 1:
        return conv(x)
    B, H, W, _ = x.shape
    return _DilateMerge.apply(conv(_DilateSplit.apply(x, int(d))), B, H, W, int(d))


# ---------------------------------------------------------------------------------------------------------------
# nearest x2 up-sampling
# ---------------------------------------------------------------------------------------------------------------
class _Upsample2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        B, H, W, C = x.shape
        out = torch.empty(B, 2 * H, 2 * W, C, device=x.device, dtype=x.dtype)
        L.check(L.lib().sde_upsample2_fwd(L.ptr(x), B, H, W, C, _dt(x), L.ptr(out), L.stream()), "sde_upsample2_fwd")
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = dout.contiguous()
        B, H2, W2, C = dout.shape
        dx = torch.empty(B, H2 // 2, W2 // 2, C, device=dout.device, dtype=dout.dtype)
        L.check(L.lib().sde_upsample2_bwd(L.ptr(dout), B, H2 // 2, W2 // 2, C, _dt(dout), L.ptr(dx), L.stream()), "sde_upsample2_bwd")
        return dx


def upsample2(x):
    return _Upsample2.apply(x)


# ---------------------------------------------------------------------------------------------------------------
# multi-piece concatenation
# ---------------------------------------------------------------------------------------------------------------
class _Cat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, reals, maps, *tensors):
        x0 = tensors[0]
        B, H, W = x0.shape[:3]
        dt = x0.dtype
        V = HN.vec_of(dt)
        Ct = HN.pad_to(sum(reals), V)
        out = torch.empty(B, H, W, Ct, device=x0.device, dtype=dt)
        arr = (CatPiece * CAT_MAX)()
        for k, (t, c, m) in enumerate(zip(tensors, reals, maps)):
            arr[k].p, arr[k].C, arr[k].ld, arr[k].f32map = t.data_ptr(), int(c), (1 if m else int(t.shape[3])), int(m)
        L.check(L.lib().sde_cat_fwd(ctypes.cast(arr, c_void_p), len(tensors), B * H * W, Ct, HN.dtype_code(dt), L.ptr(out), L.stream()), "sde_cat_fwd")
        ctx.meta = (reals, maps, [t.shape for t in tensors], [t.dtype for t in tensors])
        return out

    @staticmethod
    def backward(ctx, dout):
        reals, maps, shapes, dtypes = ctx.meta
        dout = dout.contiguous()
        B, H, W, Ct = dout.shape
        grads = [torch.empty(s, device=dout.device, dtype=d) for s, d in zip(shapes, dtypes)]
        arr = (CatPiece * CAT_MAX)()
        for k, (g, c, m) in enumerate(zip(grads, reals, maps)):
            arr[k].p, arr[k].C, arr[k].ld, arr[k].f32map = g.data_ptr(), int(c), (1 if m else int(g.shape[3])), int(m)
        L.check(L.lib().sde_cat_bwd(L.ptr(dout), B * H * W, Ct, HN.dtype_code(dout.dtype), ctypes.cast(arr, c_void_p), len(grads), L.stream()), "sde_cat_bwd")
        return (None, None) + tuple(grads)


def cat(pieces):
    """torch.cat(dim=1) of the decoder: pieces = [(tensor, real_channels)]; an NHWC activation [B,H,W,ld] or a planar fp32 map [B,1,H,W] (real = 1)."""
    if not 1 <= len(pieces) <= CAT_MAX:
        raise L.SdeHipError(f"cat: 1..{CAT_MAX} pieces, got {len(pieces)}")
    tensors = [t.contiguous() for t, _ in pieces]
    reals = tuple(int(c) for _, c in pieces)
    H, W = tensors[0].shape[1:3]            # the first piece is an activation
    maps = tuple(bool(c == 1 and t.dim() == 4 and t.shape[1] == 1 and tuple(t.shape[2:]) == (H, W) and t.dtype == torch.float32)
                 for t, c in zip(tensors, reals))
    return _Cat.apply(reals, maps, *tensors)


# ---------------------------------------------------------------------------------------------------------------
# BatchNorm statistics of a stored tensor, ReLU
# ---------------------------------------------------------------------------------------------------------------
def channel_stats(x):
    """[tiles + REDUCE_ROWS][C][2] partial slab of (sum, sum^2) per channel -- what hip.nn.batch_norm_act reads as `stats`."""
    C = x.shape[-1]
    M = x.numel() // C
    lib = L.lib()
    tiles = lib.sde_channel_stats_tiles(M)
    part = torch.empty(tiles + HN.REDUCE_ROWS, C, 2, device=x.device, dtype=torch.float32)
    L.check(lib.sde_channel_stats(L.ptr(x), M, C, _dt(x), L.ptr(part), L.stream()), "sde_channel_stats")
    return part


class _ReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = torch.empty_like(x)
        L.check(L.lib().sde_relu_fwd(L.ptr(x), x.numel(), _dt(x), L.ptr(y), L.stream()), "sde_relu_fwd")
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = dy.contiguous()
        C = y.shape[-1]
        dz = torch.empty_like(y)
        L.check(L.lib().sde_act_bwd_bias(L.ptr(dy), L.ptr(y), HN.ACT_RELU, y.numel() // C, C, _dt(y), L.ptr(dz), None, None, 0, 0, L.stream()),
                "sde_act_bwd_bias")
        return dz


def relu(x):
    return _ReLU.apply(x.contiguous())


# ---------------------------------------------------------------------------------------------------------------
# plane head + local planar guidance; sigmoid heads
# ---------------------------------------------------------------------------------------------------------------
class _LPG(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, r, max_depth, ds):
        B, h, w, ld = y.shape
        H, W = h * r, w * r
        full = torch.empty(B, 1, H, W, device=y.device, dtype=torch.float32)
        down = torch.empty(B, 1, H // ds, W // ds, device=y.device, dtype=torch.float32) if ds else None
        L.check(L.lib().sde_lpg_fwd(L.ptr(y), B, h, w, ld, r, max_depth, ds, _dt(y), L.ptr(full), L.ptr(down), L.stream()), "sde_lpg_fwd")
        ctx.save_for_backward(y)
        ctx.cfg = (r, max_depth, ds)
        ctx.set_materialize_grads(False)
        return (full, down) if ds else full

    @staticmethod
    def backward(ctx, dfull, ddown=None):
        (y,) = ctx.saved_tensors
        r, max_depth, ds = ctx.cfg
        B, h, w, ld = y.shape
        if dfull is None and ddown is None:
            return None, None, None, None
        dy = torch.empty_like(y)
        dfull = dfull.contiguous() if dfull is not None else None
        ddown = ddown.contiguous() if ddown is not None else None
        L.check(L.lib().sde_lpg_bwd(L.ptr(y), L.ptr(dfull), L.ptr(ddown), B, h, w, ld, r, max_depth, ds, _dt(y), L.ptr(dy), L.stream()), "sde_lpg_bwd")
        return dy, None, None, None


def lpg(y, r, max_depth, ds=0):
    """Plane logits y [B,h,w,ld] -> depth / max_depth [B,1,h*r,w*r] fp32 (and the nearest 1/ds copy when ds > 0)."""
    return _LPG.apply(y.contiguous(), int(r), float(max_depth), int(ds))


class _SigmoidHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, scale, focal, focal_div, flip):
        B, H, W, ld = y.shape
        out = torch.empty(B, 1, H, W, device=y.device, dtype=torch.float32)
        L.check(L.lib().sde_sigmoid_head_fwd(L.ptr(y), B, H, W, ld, scale, L.ptr(focal), focal_div, int(flip), _dt(y), L.ptr(out), L.stream()),
                "sde_sigmoid_head_fwd")
        ctx.save_for_backward(y, focal)
        ctx.cfg = (scale, focal_div, flip)
        return out

    @staticmethod
    def backward(ctx, dout):
        y, focal = ctx.saved_tensors
        scale, focal_div, flip = ctx.cfg
        B, H, W, ld = y.shape
        dy = torch.empty_like(y)
        L.check(L.lib().sde_sigmoid_head_bwd(L.ptr(y), L.ptr(dout.contiguous()), B, H, W, ld, scale, L.ptr(focal), focal_div, int(flip), _dt(y), L.ptr(dy),
                                             L.stream()), "sde_sigmoid_head_bwd")
        return dy, None, None, None, None


def sigmoid_head(y, scale=1.0, focal=None, focal_div=1.0, flip=False):
    """Channel 0 of y [B,H,W,ld] -> sigmoid * scale [* focal[b] / focal_div] as [B,1,H,W] fp32 (mirrored along x when flip)."""
    if focal is not None:
        focal = focal.detach().float().contiguous()
    return _SigmoidHead.apply(y.contiguous(), float(scale), focal, float(focal_div), bool(flip))

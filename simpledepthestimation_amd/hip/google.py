"""Autograd wrappers of GoogleResNet's operators (csrc/google.hip, include/sde_hip.h "GoogleResNet operators").

Activations are NHWC in fp32 or bf16 with channels padded to the 16-byte group; the depth map is planar [B,1,H,W] fp32, as in the reference.
"""
import torch

from . import lib as L
from . import nn as HN

RLN_CHUNKS = 32      # SDE_RLN_CHUNKS
# prototypes: hip/lib.py (_PROTOS, "GoogleResNet operators")


def _dt(t):
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise L.SdeHipError(f"GoogleResNet operators run in fp32 or bf16, not {t.dtype}")
    return HN.dtype_code(t.dtype)


# ---------------------------------------------------------------------------------------------------------------
# RandLayerNorm (+ residual, + ReLU)
# ---------------------------------------------------------------------------------------------------------------
class _RandLayerNorm(torch.autograd.Function):
    """n_out > 1 returns that many aliases of the output, one per consumer; backward sums up to three of their gradients in the kernel
    (as hip.nn._BatchNormAct does)."""

    @staticmethod
    def forward(ctx, y, gamma, beta, z, stddev, residual, eps, train, relu, n_out):
        ctx.set_materialize_grads(False)
        B, H, W, C = y.shape
        Cr = gamma.numel()
        dev = y.device
        part = torch.empty(B, RLN_CHUNKS, C, 2, device=dev)
        rlnp = torch.empty(B, C, 2, device=dev)
        out = torch.empty_like(y)
        if residual is not None and (residual.shape != y.shape or residual.dtype != y.dtype):
            raise L.SdeHipError("rand_layer_norm: the residual must have the input's shape and dtype")
        L.check(L.lib().sde_randln_fwd(L.ptr(y), L.ptr(residual), L.ptr(HN._f32(gamma)), L.ptr(HN._f32(beta)), L.ptr(z), L.ptr(stddev), int(train), B, H * W,
                                       C, Cr, eps, int(relu), _dt(y), L.ptr(part), L.ptr(rlnp), L.ptr(out), L.stream()), "sde_randln_fwd")
        ctx.save_for_backward(y, out if relu else None, rlnp, gamma)
        ctx.params = (gamma, beta)
        ctx.cfg = (relu, residual is not None)
        return HN.aliases(out, n_out)

    @staticmethod
    def backward(ctx, *douts):
        y, out, rlnp, gamma = ctx.saved_tensors
        relu, has_res = ctx.cfg
        grads = [d for d in HN.fan_in(douts, 3) if d is not None]
        if not grads:
            return (None,) * 10
        B, H, W, C = y.shape
        Cr = gamma.numel()
        dev = y.device
        part = torch.empty(B, RLN_CHUNKS, C, 2, device=dev)
        gs, bs = HN._grad_slot(ctx.params[0]), HN._grad_slot(ctx.params[1])
        direct = gs is not None and bs is not None
        dgamma = gs if direct else torch.empty(Cr, device=dev)
        dbeta = bs if direct else torch.empty(Cr, device=dev)
        dx = torch.empty_like(y)
        # the masked sum of the incoming gradients is the residual's gradient: stored only when the residual needs it and it differs from d0
        gm = torch.empty_like(y) if (has_res and (relu or len(grads) > 1)) else None
        d0, d1, d2 = (grads + [None, None])[:3]
        L.check(L.lib().sde_randln_bwd(L.ptr(d0), L.ptr(d1), L.ptr(d2), L.ptr(out), L.ptr(y), L.ptr(rlnp), L.ptr(HN._f32(gamma)), int(relu), B, H * W, C, Cr,
                                       _dt(y), L.ptr(part), L.ptr(dgamma), L.ptr(dbeta), int(direct), L.ptr(gm), L.ptr(dx), L.stream()), "sde_randln_bwd")
        dres = (gm if gm is not None else d0) if has_res else None
        if direct:
            dgamma = dbeta = None
        return dx, dgamma, dbeta, None, None, dres, None, None, None, None


def rand_layer_norm(y, gamma, beta, z, stddev, eps=1e-3, train=True, residual=None, relu=False, n_out=1):
    """RandLayerNorm of NHWC y (gamma.numel() real channels) [+ residual] [-> ReLU].  z: [2,B,Cr] fp32 device draws (mean, variance), read in
    training only; stddev: a one-element fp32 device tensor (read by the kernel, so captured graphs follow later changes)."""
    if train:
        B, Cr = y.shape[0], gamma.numel()
        if z is None or tuple(z.shape) != (2, B, Cr) or z.dtype != torch.float32:
            raise L.SdeHipError(f"rand_layer_norm: z must be fp32 [2, {B}, {Cr}]")
        if stddev is None or stddev.numel() != 1 or stddev.dtype != torch.float32:
            raise L.SdeHipError("rand_layer_norm: stddev must be a one-element fp32 device tensor")
    if y.shape[1] * y.shape[2] < 2:
        raise L.SdeHipError("rand_layer_norm: the unbiased variance needs H x W >= 2 pixels")
    return _RandLayerNorm.apply(y.contiguous(), gamma, beta, z.contiguous() if (train and z is not None) else None, stddev if train else None,
                                residual.contiguous() if residual is not None else None, float(eps), bool(train), bool(relu), int(n_out))


# ---------------------------------------------------------------------------------------------------------------
# bilinear x2 (align_corners=True)
# ---------------------------------------------------------------------------------------------------------------
class _Bilinear2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        B, H, W, C = x.shape
        out = torch.empty(B, 2 * H, 2 * W, C, device=x.device, dtype=x.dtype)
        L.check(L.lib().sde_bilinear2_fwd(L.ptr(x), B, H, W, C, _dt(x), L.ptr(out), L.stream()), "sde_bilinear2_fwd")
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = dout.contiguous()
        B, H2, W2, C = dout.shape
        dx = torch.empty(B, H2 // 2, W2 // 2, C, device=dout.device, dtype=dout.dtype)
        L.check(L.lib().sde_bilinear2_bwd(L.ptr(dout), B, H2 // 2, W2 // 2, C, _dt(dout), L.ptr(dx), L.stream()), "sde_bilinear2_bwd")
        return dx


def bilinear2(x):
    """F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=True) on NHWC x."""
    return _Bilinear2.apply(x.contiguous())


# ---------------------------------------------------------------------------------------------------------------
# softplus depth head
# ---------------------------------------------------------------------------------------------------------------
class _SoftplusHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, flip):
        B, H, W, ld = y.shape
        out = torch.empty(B, 1, H, W, device=y.device, dtype=torch.float32)
        L.check(L.lib().sde_softplus_head_fwd(L.ptr(y), B, H, W, ld, int(flip), _dt(y), L.ptr(out), L.stream()), "sde_softplus_head_fwd")
        ctx.save_for_backward(y)
        ctx.flip = flip
        return out

    @staticmethod
    def backward(ctx, dout):
        (y,) = ctx.saved_tensors
        B, H, W, ld = y.shape
        dy = torch.empty_like(y)
        L.check(L.lib().sde_softplus_head_bwd(L.ptr(y), L.ptr(dout.contiguous().float()), B, H, W, ld, int(ctx.flip), _dt(y), L.ptr(dy), L.stream()),
                "sde_softplus_head_bwd")
        return dy, None


def softplus_head(y, flip=False):
    """Channel 0 of y [B,H,W,ld] -> F.softplus as [B,1,H,W] fp32 (mirrored along x when flip)."""
    return _SoftplusHead.apply(y.contiguous(), bool(flip))

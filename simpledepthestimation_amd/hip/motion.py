"""Autograd wrappers of the GoogleMotionNet / GooglePoseNet operators (csrc/motion.hip, include/sde_hip.h "GoogleMotionNet / GooglePoseNet operators").

Activations are NHWC in fp32 or bf16 with channels padded to the 16-byte group.  The 3-channel motion field is fp32 [B,h,w,4] (channel 3 zero)
in both modes: it is summed over eight refiners and costs 3 channels.  motion_pred is planar [B,3,H,W] fp32, as in the reference.
"""
import torch

from . import lib as L
from . import nn as HN

# prototypes: hip/lib.py (_PROTOS, "GoogleMotionNet / GooglePoseNet operators")


def _dt(t):
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise L.SdeHipError(f"motion operators run in fp32 or bf16, not {t.dtype}")
    return HN.dtype_code(t.dtype)


def _field_ok(f, name):
    if f.dtype != torch.float32 or f.dim() != 4 or f.shape[3] != 4:
        raise L.SdeHipError(f"{name}: the motion field must be fp32 [B,h,w,4]")


# ---------------------------------------------------------------------------------------------------------------
# differentiable input preparation
# ---------------------------------------------------------------------------------------------------------------
class _PrepInput(torch.autograd.Function):
    """Two aliases of the prepared tensor (the first convolution and refiner0's skip); backward sums their gradients in the kernel."""

    @staticmethod
    def forward(ctx, img, dtype):
        ctx.set_materialize_grads(False)
        x = HN.prep_input(img, None, None, dtype)
        ctx.shape = tuple(img.shape)
        return HN.aliases(x, 2)

    @staticmethod
    def backward(ctx, *douts):
        grads = HN.fan_in(douts, 2)
        if not grads:
            return None, None
        B, C, H, W = ctx.shape
        d0, d1 = grads
        dimg = torch.empty(ctx.shape, device=d0.device, dtype=torch.float32)
        L.check(L.lib().sde_prep_input_bwd(L.ptr(d0), L.ptr(d1), B, C, H, W, d0.shape[3], _dt(d0), L.ptr(dimg), L.stream()), "sde_prep_input_bwd")
        return dimg, None


def prep_input_grad(img, dtype):
    """hip.nn.prep_input(img, None, None, dtype) with a gradient for img (pose_net_input's depth channels come from the depth net).  Returns two
    aliases of the NHWC tensor, one per consumer.  An image that does not require grad takes the plain path: nothing downstream then computes a
    data gradient for it."""
    if not (img.requires_grad and torch.is_grad_enabled()):
        x = HN.prep_input(img, None, None, dtype)
        return x, x
    if img.dtype != torch.float32:
        raise L.SdeHipError("prep_input_grad expects a float32 NCHW image")
    return _PrepInput.apply(img.contiguous(), dtype)


# ---------------------------------------------------------------------------------------------------------------
# bilinear resize (align_corners=True, any ratio) + cat
# ---------------------------------------------------------------------------------------------------------------
class _ResizeCat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, field, skip, Cr):
        ctx.set_materialize_grads(False)
        B, h, w, _ = field.shape
        _, H, W, Cs = skip.shape
        V = HN.vec_of(skip.dtype)
        Cx = HN.pad_to(3 + Cr, V)
        X = torch.empty(B, H, W, Cx, device=skip.device, dtype=skip.dtype)
        up = torch.empty(B, H, W, 4, device=skip.device, dtype=torch.float32)
        L.check(L.lib().sde_motion_resize_cat_fwd(L.ptr(field), h, w, L.ptr(skip), B, H, W, Cs, Cr, Cx, _dt(skip), L.ptr(X), L.ptr(up), L.stream()),
                "sde_motion_resize_cat_fwd")
        ctx.meta = (B, h, w, H, W, Cs, Cr, Cx, skip.dtype)
        return HN.aliases(X, 2) + (up,)

    @staticmethod
    def backward(ctx, dXa, dXb, dup):
        B, h, w, H, W, Cs, Cr, Cx, dt = ctx.meta
        d0, d1 = HN.fan_in((dXa, dXb), 2) or (None, None)
        if d0 is None and dup is None:
            return None, None, None
        dev = (d0 if d0 is not None else dup).device
        dup = dup.contiguous() if dup is not None else None
        dfield = torch.empty(B, h, w, 4, device=dev, dtype=torch.float32)
        dskip = torch.empty(B, H, W, Cs, device=dev, dtype=dt) if ctx.needs_input_grad[1] else None
        L.check(L.lib().sde_motion_resize_cat_bwd(L.ptr(d0), L.ptr(d1), L.ptr(dup), B, H, W, Cx, Cr, Cs, h, w, HN.dtype_code(dt), L.ptr(dfield), L.ptr(dskip),
                                                  L.stream()), "sde_motion_resize_cat_bwd")
        return dfield, dskip, None


def resize_cat(field, skip, skip_channels):
    """MotionRefiner's input: cat([F.interpolate(field, skip's size, 'bilinear', align_corners=True), skip], 1).
    field: fp32 [B,h,w,4]; skip: NHWC [B,H,W,Cs] whose first `skip_channels` are real.  Returns (X, X', up): X [B,H,W,pad(3 + skip_channels)] in
    the skip's dtype, channels [field, skip, zeros], X' an alias for a second consumer, and up = the resized field as fp32 [B,H,W,4]."""
    _field_ok(field, "resize_cat")
    if skip.dim() != 4 or skip.shape[0] != field.shape[0] or not 0 < skip_channels <= skip.shape[3]:
        raise L.SdeHipError("resize_cat: skip must be NHWC with the field's batch size and at least skip_channels channels")
    return _ResizeCat.apply(field.contiguous(), skip.contiguous(), int(skip_channels))


# ---------------------------------------------------------------------------------------------------------------
# refiner tail
# ---------------------------------------------------------------------------------------------------------------
class _Tail(torch.autograd.Function):
    @staticmethod
    def forward(ctx, o1, o2, w3, up):
        B, H, W, ld = o1.shape
        mid = w3.shape[1] // 2
        out = torch.empty_like(up)
        L.check(L.lib().sde_motion_tail_fwd(L.ptr(o1), L.ptr(o2), L.ptr(w3), L.ptr(up), B * H * W, ld, mid, _dt(o1), L.ptr(out), L.stream()), "sde_motion_tail_fwd")
        ctx.save_for_backward(o1, o2, w3)
        return out

    @staticmethod
    def backward(ctx, dout):
        o1, o2, w3 = ctx.saved_tensors
        dout = dout.contiguous()
        B, H, W, ld = o1.shape
        P, mid = B * H * W, w3.shape[1] // 2
        lib = L.lib()
        nblk = lib.sde_motion_tail_blocks(P, ld, _dt(o1))
        part = torch.empty(nblk, 3, 2 * mid, device=o1.device, dtype=torch.float32)
        do1, do2 = torch.empty_like(o1), torch.empty_like(o2)
        dw3 = torch.empty_like(w3)
        L.check(lib.sde_motion_tail_bwd(L.ptr(dout), L.ptr(o1), L.ptr(o2), L.ptr(w3), P, ld, mid, _dt(o1), L.ptr(do1), L.ptr(do2), L.ptr(part), L.ptr(dw3),
                                        L.stream()), "sde_motion_tail_bwd")
        return do1, do2, dw3, dout


def refiner_tail(o1, o2, w3, up):
    """up + conv3(cat([o1, o2], 1)) for the bias-free 1x1 conv3 (weight [3, 2*mid, 1, 1]); o1, o2: NHWC with mid real channels; up and the result
    are fp32 [B,H,W,4]."""
    _field_ok(up, "refiner_tail")
    if o1.shape != o2.shape or o1.dtype != o2.dtype or o1.shape[:3] != up.shape[:3]:
        raise L.SdeHipError("refiner_tail: o1 and o2 must have one shape and dtype, and the field's B, H, W")
    if w3.dim() != 4 or w3.shape[0] != 3 or w3.shape[2:] != (1, 1) or w3.shape[1] % 2 or w3.shape[1] // 2 > o1.shape[3]:
        raise L.SdeHipError("refiner_tail: conv3's weight must be [3, 2*mid, 1, 1] with mid <= the channel stride of o1")
    return _Tail.apply(o1.contiguous(), o2.contiguous(), HN._f32(w3), up.contiguous())


# ---------------------------------------------------------------------------------------------------------------
# scale + mask + weight head
# ---------------------------------------------------------------------------------------------------------------
class _Head(torch.autograd.Function):
    @staticmethod
    def forward(ctx, field, scale, weight, mask):
        B, H, W, _ = field.shape
        lib = L.lib()
        dev = field.device
        part = keep = None
        if mask:
            part = torch.empty(lib.sde_motion_head_blocks(B * H * W), device=dev, dtype=torch.float32)
            keep = torch.empty(B * H * W, device=dev, dtype=torch.uint8)
        out = torch.empty(B, 3, H, W, device=dev, dtype=torch.float32)
        L.check(lib.sde_motion_head_fwd(L.ptr(field), L.ptr(scale), L.ptr(weight), int(mask), B, H, W, L.ptr(part), L.ptr(keep), L.ptr(out), L.stream()),
                "sde_motion_head_fwd")
        ctx.save_for_backward(field, scale, weight, keep)
        return out

    @staticmethod
    def backward(ctx, dout):
        field, scale, weight, keep = ctx.saved_tensors
        B, H, W, _ = field.shape
        lib = L.lib()
        part = torch.empty(lib.sde_motion_head_blocks(B * H * W), device=field.device, dtype=torch.float32)
        dfield = torch.empty_like(field)
        L.check(lib.sde_motion_head_bwd(L.ptr(dout.contiguous().float()), L.ptr(field), L.ptr(scale), L.ptr(weight), L.ptr(keep), B, H, W, L.ptr(dfield),
                                        L.ptr(part), L.stream()), "sde_motion_head_bwd")
        # the kernel leaves one partial per workgroup (<= 1024): their sum is the scale's gradient, no pass over the full tensor
        dscale = part.sum(dtype=torch.float64).to(torch.float32).reshape(scale.shape) if ctx.needs_input_grad[1] else None
        return dfield, dscale, None, None


def motion_head(field, scale, weight, mask):
    """motion_pred [B,3,H,W] fp32 = field * scale [* (|field * scale|_2 > its mean over the whole batch)] * weight.
    scale, weight: one-element fp32 device tensors read by the kernels (scale may require grad; the mask carries no gradient)."""
    _field_ok(field, "motion_head")
    for t, name in ((scale, "scale"), (weight, "weight")):
        if t.numel() != 1 or t.dtype != torch.float32:
            raise L.SdeHipError(f"motion_head: {name} must be a one-element fp32 device tensor")
    return _Head.apply(field.contiguous(), scale, weight, bool(mask))

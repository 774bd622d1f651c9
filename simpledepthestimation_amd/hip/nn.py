"""Autograd wrappers over the convolution engine and its surrounding layers (include/sde_hip.h).

Tensor convention: activations are NHWC torch tensors [B, H, W, C] (float32, bfloat16 or float16), C padded to 16 bytes;
parameters stay fp32 in the reference's layouts (conv weight OIHW) so state dicts are interchangeable.
"""
import contextlib
import ctypes
import functools
import os
import weakref
from collections import namedtuple
from ctypes import POINTER, Structure, c_float, c_int, c_int32, c_long, c_void_p

import torch

from . import lib as L

SRC_PLAIN, SRC_UPCAT, SRC_ZEROINS = 0, 1, 2
REDUCE_ROWS = 32   # SDE_REDUCE_ROWS: scratch rows every partial-sum slab carries behind its payload
ACT_NONE, ACT_ELU, ACT_RELU = 0, 1, 2


class ConvDesc(Structure):
    _fields_ = [("x0", c_void_p), ("x1", c_void_p), ("dtype", c_int32), ("C0", c_int32), ("C1", c_int32), ("H0", c_int32), ("W0", c_int32),
                ("IH", c_int32), ("IW", c_int32), ("src_mode", c_int32), ("KH", c_int32), ("KW", c_int32), ("stride", c_int32), ("pad", c_int32),
                ("reflect", c_int32), ("Bn", c_int32), ("OH", c_int32), ("OW", c_int32)]


_P, _I, _F, _LG = c_void_p, c_int, c_float, c_long
L.register_protos({
    "sde_pack_weight": ([_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P], c_int),
    "sde_pack_weights_batched": ([_P, _I, _LG, _I, _P], c_int),
    "sde_pack_item_blocks": ([_I, _I, _I, _I], c_int),
    "sde_conv_fwd": ([POINTER(ConvDesc), _P, _P, _I, _P, _I, _I, _P, _P], c_int),
    "sde_conv_fwd_tiles_m": ([POINTER(ConvDesc), _I], c_int),
    "sde_conv_fwd_ws_bytes": ([POINTER(ConvDesc), _I], ctypes.c_size_t),
    "sde_conv_fwd_ws": ([POINTER(ConvDesc), _P, _P, _I, _P, _I, _I, _P, _P, ctypes.c_size_t, _P], c_int),
    "sde_conv_fwd_variant": ([POINTER(ConvDesc), _I], c_int),
    "sde_conv_dgrad_bnbwd_rows": ([POINTER(ConvDesc), _I, _I], c_int),
    "sde_conv_dgrad_bnbwd": ([POINTER(ConvDesc), _P, _P, _I, _I, _P, _P, _P, _P], c_int),
    "sde_conv_dgrad_bnbwd_res_rows": ([POINTER(ConvDesc), _I, _I], c_int),
    "sde_conv_dgrad_bnbwd_res": ([POINTER(ConvDesc), _P, _P, _I, _I, _P, _P, _P, _P, _P, _P], c_int),
    "sde_bn_bwd_from_part": ([_P, _I, _P, _P, _P, _LG, _I, _I, _P, _P, _P, _I, _P, _P], c_int),
    "sde_conv_set_halo_min_blocks": ([_I], c_int),
    "sde_conv_set_option": ([_I, _I], c_int),
    "sde_kernel_lds_bytes": ([_I, _I], c_int),
    "sde_conv_wgrad_splits": ([POINTER(ConvDesc), _I], c_int),
    "sde_conv_wgrad_variant": ([POINTER(ConvDesc), _I, _I], c_int),
    "sde_conv_wgrad": ([POINTER(ConvDesc), _P, _I, _I, _I, _P, _I, _P, _I, _P], c_int),
    "sde_conv_wgrad_partial": ([POINTER(ConvDesc), _P, _I, _I, _P, _I, _P], c_int),
    "sde_wgrad_reduce_batched": ([_P, _I, _P], c_int),
    "sde_colsum_finalize_batched": ([_P, _I, _P], c_int),
    "sde_prep_input": ([_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P], c_int),
    "sde_bn_finalize": ([_P, _I, _I, _LG, _P, _P, _P, _P, _F, _F, _P, _P], c_int),
    "sde_bn_eval_params": ([_P, _P, _P, _P, _F, _I, _P, _P], c_int),
    "sde_bn_apply": ([_P, _P, _P, _I, _LG, _I, _I, _P, _P], c_int),
    "sde_bn_finalize_apply_ok": ([_I, _I, _I], c_int),
    "sde_bn_set_fuse": ([_I], c_int),
    "sde_bn_finalize_apply": ([_P, _I, _I, _LG, _P, _P, _P, _P, _F, _F, _P, _P, _P, _I, _I, _P, _P], c_int),
    "sde_reduce_num_blocks": ([_LG, _I], c_int),
    "sde_bn_bwd": ([_P, _P, _P, _P, _P, _P, _P, _I, _LG, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P], c_int),
    "sde_maxpool_fwd": ([_P, _I, _I, _I, _I, _I, _P, _P, _P], c_int),
    "sde_depth_head_bias_blocks": ([_I, _I, _I], c_int),
    "sde_depth_head_bwd_bias": ([_P, _P, _I, _I, _I, _I, _F, _F, _I, _I, _P, _P, _P, _I, _P], c_int),
    "sde_maxpool_bwd": ([_P, _P, _I, _I, _I, _I, _I, _P, _P], c_int),
    "sde_maxpool_bwd_sum": ([_P, _P, _P, _I, _I, _I, _I, _I, _P, _P], c_int),
    "sde_act_bwd_bias": ([_P, _P, _I, _LG, _I, _I, _P, _P, _P, _I, _I, _P], c_int),
    "sde_act_bwd_bias_sum": ([_P, _P, _P, _I, _LG, _I, _I, _P, _P, _P, _I, _I, _P], c_int),
    "sde_refl_fold": ([_P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P], c_int),
    "sde_depth_head_fwd": ([_P, _I, _I, _I, _I, _F, _F, _I, _I, _P, _P], c_int),
    "sde_depth_head_bwd": ([_P, _P, _I, _I, _I, _I, _F, _F, _I, _I, _P, _P], c_int),
    "sde_gn_relu_fwd": ([_P, _P, _P, _I, _I, _I, _I, _F, _I, _I, _P, _P, _P, _P], c_int),
    "sde_gn_relu_bwd": ([_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P], c_int),
    "sde_gn_relu_res_fwd": ([_P, _P, _P, _P, _I, _I, _I, _I, _F, _I, _I, _P, _P, _P, _P], c_int),
    "sde_gn_relu_res_bwd": ([_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P], c_int),
    "sde_space_to_depth": ([_P, _I, _I, _I, _I, _I, _P, _P], c_int),
    "sde_depth_to_space": ([_P, _I, _I, _I, _I, _I, _P, _P], c_int),
    "sde_concat_fwd": ([_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P], c_int),
    "sde_concat_bwd": ([_P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P], c_int),
    "sde_inv_depth_head_fwd": ([_P, _I, _I, _I, _I, _F, _F, _F, _I, _I, _P, _P, _P], c_int),
    "sde_inv_depth_head_bwd": ([_P, _P, _P, _I, _I, _I, _I, _F, _F, _F, _I, _I, _P, _P], c_int),
    "sde_conv3d_fwd": ([_P, _P, _P, _I, _I, _I, _I, _I, _P, _P], c_int),
    "sde_conv3d_dgrad": ([_P, _P, _I, _I, _I, _I, _I, _P, _P], c_int),
    "sde_conv3d_wgrad_num_blocks": ([_I, _I, _I, _I, _I], c_int),
    "sde_conv3d_wgrad": ([_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P], c_int),
    "sde_adam_step": ([_P, _P, _P, _P, _LG, _P, _P], c_int),
    "sde_adam_step_twin": ([_P, _P, _P, _P, _LG, _P, _P, _I, _P], c_int),
    "sde_grad_check": ([_P, _LG, _P, _P], c_int),
    "sde_grad_norm": ([_P, _LG, _P, _P, _F, _F, _P], c_int),
    "sde_loss_scale_update": ([_P, _F, _F, _I, _P], c_int),
})


OPT_PGEMM, OPT_PGEMM_DEPTH, OPT_PGEMM_3X3, OPT_PGEMM_TILE, OPT_SPLITK, OPT_WGRAD_BLOCKS, OPT_WGRAD_HALO, OPT_CONV_SMALL, OPT_WGRAD_DMA, OPT_BNBWD_FUSE, OPT_CU_RESERVE = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11      # SDE_OPT_* of include/sde_hip.h
OPT_WGRAD_DMA_RING, OPT_PGEMM_PER_CU = 12, 13
KERNEL_PGEMM, KERNEL_WGRAD_DMA, KERNEL_WGRAD_HALO, KERNEL_WGRAD_STAGED, KERNEL_WGRAD_SUM, KERNEL_WGRAD_REDUCE = 1, 2, 3, 4, 5, 6      # SDE_KERNEL_* (sde_kernel_lds_bytes)


def set_option(key, value):
    """sde_conv_set_option: returns the previous value."""
    old = L.lib().sde_conv_set_option(int(key), int(value))
    if old < 0:
        raise L.SdeHipError(f"sde_conv_set_option({key}, {value}) failed: {L.lib().sde_last_error().decode()}")
    return old


def kernel_lds_bytes(kind, variant=0):
    """sde_kernel_lds_bytes: dynamic LDS per workgroup of a kernel that shares compute units during backward (host-only query)."""
    n = L.lib().sde_kernel_lds_bytes(int(kind), int(variant))
    if n < 0:
        raise L.SdeHipError(f"sde_kernel_lds_bytes({kind}, {variant}): bad kind / variant")
    return n


WGRAD_HALO_KERNEL, WGRAD_DMA_KERNEL, WGRAD_STAGED_KERNEL = 1, 2, 3      # sde_conv_wgrad_variant


def dtype_code(dt):
    if dt == torch.float32:
        return L.F32
    if dt == torch.bfloat16:
        return L.BF16
    if dt == torch.float16:
        return L.F16
    raise L.SdeHipError(f"unsupported activation dtype {dt}")


def vec_of(dt):
    return 4 if dt == torch.float32 else 8


def pad_to(c, v):
    return (c + v - 1) // v * v


def is_ohwi(t):
    """A 4-D conv weight (or its gradient) stored channels-last: memory order [Cout][KH][KW][Cin] under the usual [Cout,Cin,KH,KW] shape -- the
    order of the packed operands and of the weight-gradient slabs (HipTrainer lays its flat buffers out this way)."""
    return t.dim() == 4 and not t.is_contiguous() and t.permute(0, 2, 3, 1).is_contiguous()


def _dense(t):
    return t.is_contiguous() or is_ohwi(t)


def _grad_slot(p):
    """A parameter's pre-allocated fp32 .grad (HipTrainer points it into the flat gradient buffer): kernels then accumulate
    straight into it and the Function returns None for that input, which skips autograd's per-parameter add kernel."""
    g = p.grad if (p is not None and p.is_leaf) else None
    if g is not None and g.dtype == torch.float32 and _dense(g) and g.shape == p.shape:
        return g
    return None


def _f32(t):
    if t.dtype != torch.float32:
        raise L.SdeHipError("parameters must be float32")
    return t.contiguous()


def aliases(out, n):
    """`out` itself for n == 1, else n aliases of it, one per consumer: backward then receives the consumers' gradients separately and the
    kernel sums them on the fly (see fan_in), instead of autograd launching an add kernel per extra consumer."""
    return out if n == 1 else (out,) + tuple(out.view(out.shape) for _ in range(n - 1))


def fan_in(douts, slots):
    """The gradients of aliases() for a backward kernel that sums `slots` of them: the None entries dropped, the others contiguous, any gradients
    beyond `slots` folded into the last slot by torch adds (left to right), None-padded to exactly `slots` entries.  () when no gradient arrived."""
    grads = [g.contiguous() for g in douts if g is not None]
    if not grads:
        return ()
    for g in grads[slots:]:
        grads[slots - 1] = grads[slots - 1] + g
    return tuple(grads[:slots]) + (None,) * (slots - len(grads))


# ---------------------------------------------------------------------------------------------------------------
# raw (non-autograd) helpers
# ---------------------------------------------------------------------------------------------------------------
def pack_weight(w, dtype, cin_pad, cout_pad, for_dgrad=False):
    w = _f32(w)
    Cout, Cin, KH, KW = w.shape
    shape = (cin_pad, KH, KW, cout_pad) if for_dgrad else (cout_pad, KH, KW, cin_pad)
    out = torch.empty(shape, device=w.device, dtype=dtype)
    L.check(L.lib().sde_pack_weight(L.ptr(w), L.ptr(out), dtype_code(dtype), Cout, Cin, KH, KW, cin_pad, cout_pad, int(for_dgrad), L.stream()),
            "sde_pack_weight")
    return out


def _desc(x0, x1, src_mode, KH, KW, stride, pad, reflect, IH, IW, OH, OW):
    d = ConvDesc()
    B, H0, W0, C0 = x0.shape
    d.x0 = x0.data_ptr(); d.x1 = x1.data_ptr() if x1 is not None else 0
    d.dtype = dtype_code(x0.dtype)
    d.C0, d.C1, d.H0, d.W0, d.IH, d.IW = C0, (x1.shape[3] if x1 is not None else 0), H0, W0, IH, IW
    d.src_mode, d.KH, d.KW, d.stride, d.pad, d.reflect = src_mode, KH, KW, stride, pad, int(reflect)
    d.Bn, d.OH, d.OW = B, OH, OW
    return d


_timed = L.timed


def conv_raw(d, x_dtype, w_packed, bias, act, Cout, ldy, want_stats, device, kind="igemm_fwd", flops=0.0):
    y = torch.empty(d.Bn, d.OH, d.OW, ldy, device=device, dtype=x_dtype)
    stats, tiles = None, 0
    lib = L.lib()
    if want_stats:
        tiles = lib.sde_conv_fwd_tiles_m(ctypes.byref(d), ldy)
        stats = torch.empty(tiles + REDUCE_ROWS, Cout, 2, device=device, dtype=torch.float32)
    variant = lib.sde_conv_fwd_variant(ctypes.byref(d), ldy) if L.PROFILE is not None else 0
    meta = None
    if L.PROFILE is not None:
        esz = 4 if x_dtype == torch.float32 else 2
        meta = dict(M=d.Bn * d.OH * d.OW, N=ldy, K=d.KH * d.KW * (d.C0 + d.C1), k=d.KH, s=d.stride, mode=d.src_mode,
                    bytes=esz * (d.Bn * d.H0 * d.W0 * d.C0 + d.Bn * d.IH * d.IW * d.C1 + d.Bn * d.OH * d.OW * ldy))
    ws_bytes = lib.sde_conv_fwd_ws_bytes(ctypes.byref(d), ldy)           # > 0: small-M, long-K layer that runs split-K
    ws = torch.empty(ws_bytes // 4, device=device, dtype=torch.float32) if ws_bytes else None
    _timed(kind, flops, variant, lambda: L.check(lib.sde_conv_fwd_ws(ctypes.byref(d), L.ptr(w_packed), L.ptr(bias), act, L.ptr(y), Cout, ldy, L.ptr(stats),
                                                                     L.ptr(ws), ws_bytes, L.stream()), "sde_conv_fwd_ws"), meta)
    return y, stats


class _Handovers:
    """What one autograd node leaves for a later one, keyed by the data_ptr of the tensor that links the two (size-capped: _put)."""

    def __init__(self):
        self.bn_out = {}        # residual-free BatchNorm+ReLU output -> (weakref, y, bnp): _BatchNormAct.forward -> the one _Conv2d.forward consuming it
        self.bn_out_res = {}    # the same of a residual BatchNorm+ReLU with two consumers; it stays until that BatchNorm's backward drops it
        self.bn_part = {}       # gradient a fused data-gradient GEMM returned -> (y.data_ptr(), partials, rows[, skip gradient's data_ptr]) for _BatchNormAct.backward
        self.res_grad = {}      # block input -> the gradient that arrived over the skip path: _BatchNormAct.backward -> the block's first _Conv2d.backward
        self.head_slot = {}     # one-channel bias convolution's output -> (weakref, its bias): _Conv2d.forward -> _DepthHead.forward
        self.head_done = {}     # logit gradient _DepthHead.backward returned -> id(the bias whose gradient it accumulated): -> _Conv2d.backward

    @staticmethod
    def _put(d, cap, t, ent):
        if len(d) > cap:
            d.clear()
        d[t.data_ptr()] = ent

    @staticmethod
    def _live(ent, t):
        # the weak reference pins the entry to THIS tensor object (Function.apply returns it as is): an address reused by another never matches
        return ent[1:] if (ent is not None and ent[0]() is t) else None

    def put_bn_out(self, out, y, bnp, res=False):
        (self.res_grad if res else self.bn_part).clear()      # (the backward side's entries live from one backward node to the next only)
        self._put(self.bn_out_res if res else self.bn_out, 64, out, (weakref.ref(out), y, bnp))

    def take_bn_out(self, x, res=False):
        return self._live(self.bn_out_res.get(x.data_ptr()) if res else self.bn_out.pop(x.data_ptr(), None), x)

    def drop_bn_out_res(self, ptr):
        self.bn_out_res.pop(ptr, None)

    def put_bn_part(self, g, ent):
        self._put(self.bn_part, 16, g, ent)

    def take_bn_part(self, g, res=False):
        """The partials left under gradient g; the residual form (four fields) is only taken when it is asked for."""
        ent = self.bn_part.get(g.data_ptr())
        return self.bn_part.pop(g.data_ptr()) if (ent is not None and (not res or len(ent) == 4)) else None

    def put_res_grad(self, ptr, g, if_expected=False):
        """if_expected: only while a residual BatchNorm+ReLU output is registered (some convolution may take the gradient)."""
        if self.bn_out_res or not if_expected:
            self.res_grad[ptr] = g

    def take_res_grad(self, x):
        return self.res_grad.pop(x.data_ptr(), None)

    def put_head_slot(self, y, bias):
        self.head_done.clear()                    # (entries live from a head's backward to its convolution's backward only)
        self._put(self.head_slot, 64, y, (weakref.ref(y), bias))

    def take_head_slot(self, y):
        return (self._live(self.head_slot.pop(y.data_ptr(), None), y) or (None,))[0]

    def put_head_done(self, dy, bias):
        self.head_done[dy.data_ptr()] = id(bias)

    def take_head_done(self, dy, bias):
        return self.head_done.pop(dy.data_ptr(), None) == id(bias)

    def drop_head_done(self, bias):
        """Drop every entry of this bias; True when there was one."""
        n = len(self.head_done)
        self.head_done = {k: v for k, v in self.head_done.items() if v != id(bias)}
        return len(self.head_done) < n

    def end_phase(self):
        self.res_grad.clear()
        self.bn_part.clear()


_HANDOVER = _Handovers()


def _dgrad_bnbwd(dd, wd, dz, x0, Cv, bn, flops, res):
    """Data gradient of a stride-1 convolution of x0 = relu(BatchNorm(y_bn)) (+ identity: `res`, adding the skip path's gradient) that masks it with
    relu'(x0) and leaves BatchNorm's partials under its address: _BatchNormAct.backward then skips its reduce pass.  None: no fused form here."""
    lib = L.lib()
    g_other = _HANDOVER.take_res_grad(x0) if res else None
    if res and (g_other is None or not (g_other.shape == x0.shape and g_other.dtype == x0.dtype and g_other.is_contiguous())):
        return None
    name = "sde_conv_dgrad_bnbwd_res" if res else "sde_conv_dgrad_bnbwd"
    rows = getattr(lib, name + "_rows")(ctypes.byref(dd), Cv, Cv)
    if rows <= 0:
        if res:
            _HANDOVER.put_res_grad(x0.data_ptr(), g_other)            # (no fused form for this layer after all: nothing consumed)
        return None
    y_bn, bnp = bn
    part = torch.empty(rows + REDUCE_ROWS, Cv, 2, device=x0.device, dtype=torch.float32)
    dx0 = torch.empty(x0.shape[:3] + (Cv,), device=x0.device, dtype=x0.dtype)
    variant = lib.sde_conv_fwd_variant(ctypes.byref(dd), Cv) if L.PROFILE is not None else 0
    meta = dict(M=dx0.numel() // Cv, N=Cv, K=dd.KH * dd.KW * dd.C0, k=dd.KH, s=1, mode=0,
                bytes=2 * (dz.numel() + (4 if res else 2) * dx0.numel())) if L.PROFILE is not None else None
    extra = (L.ptr(g_other), L.ptr(x0)) if res else ()
    _timed("igemm_dgrad", flops, variant, lambda: L.check(getattr(lib, name)(ctypes.byref(dd), L.ptr(wd), L.ptr(dx0), Cv, Cv, L.ptr(y_bn), L.ptr(bnp),
                                                                             L.ptr(part), *extra, L.stream()), name), meta)
    _HANDOVER.put_bn_part(dx0, (y_bn.data_ptr(), part, rows) + ((g_other.data_ptr(),) if res else ()))
    return dx0


# ---------------------------------------------------------------------------------------------------------------
# Convolution (+bias, +ELU, optional BatchNorm statistics) with every input mode of the path
# ---------------------------------------------------------------------------------------------------------------
class _Conv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, x1, weight, bias, stride, pad, reflect, act, upcat, want_stats, owner=None, n_out=1):
        ctx.set_materialize_grads(False)      # the statistics output never carries a gradient: do not launch zero fills for it
        if n_out > 1 and want_stats:
            raise L.SdeHipError("conv2d: output aliases (n_out) belong to the BatchNorm that follows when statistics are requested")
        if not x0.is_contiguous() or (x1 is not None and not x1.is_contiguous()):
            raise L.SdeHipError("conv2d: NHWC inputs must be contiguous")
        dt = x0.dtype
        V = vec_of(dt)
        B, H0, W0, C0 = x0.shape
        Cout, Cin, KH, KW = weight.shape
        C1 = x1.shape[3] if x1 is not None else 0
        if C0 % V or C1 % V:
            raise L.SdeHipError(f"conv2d: channel counts ({C0},{C1}) must be multiples of {V}")
        if Cin > C0 + C1 or (upcat and Cin != C0 + C1):
            raise L.SdeHipError(f"conv2d: weight expects {Cin} input channels, tensors carry {C0}+{C1}")
        IH, IW = (2 * H0, 2 * W0) if upcat else (H0, W0)
        OH = (IH + 2 * pad - KH) // stride + 1
        OW = (IW + 2 * pad - KW) // stride + 1
        ldy = pad_to(Cout, V)
        d = _desc(x0, x1, SRC_UPCAT if upcat else SRC_PLAIN, KH, KW, stride, pad, reflect, IH, IW, OH, OW)
        pre = getattr(owner, "_packed", None) if owner is not None else None
        if pre is not None and pre[0].dtype == dt and pre[0].shape == (ldy, KH, KW, C0 + C1):
            wp, ctx.wd_pre = pre                                   # operands packed once per step by WeightPacker
        else:
            wp, ctx.wd_pre = pack_weight(weight, dt, C0 + C1, ldy), None
            if owner is not None:
                owner._pack_shapes = (dt, C0 + C1, ldy)            # lets WeightPacker build its job table after a first step
        b32 = _f32(bias) if bias is not None else None
        flops = 2.0 * B * OH * OW * Cout * KH * KW * Cin          # algorithmic (real channels)
        plain = x1 is None and not upcat and not reflect and stride == 1
        # x0 = relu(BatchNorm(y_bn)) with this convolution as its only consumer: the data gradient below can carry BatchNorm's backward reduction
        ent = _HANDOVER.take_bn_out(x0)
        ctx.bn_in = ent if plain else None
        # x0 = relu(BatchNorm(y_bn) + identity) with this convolution and the next block's skip path as its two consumers: the data gradient below can take over
        # that BatchNorm's whole backward reduce pass, once the skip path's gradient has arrived
        ent = _HANDOVER.take_bn_out(x0, res=True) if RESBN_FUSED else None
        ctx.bn_in_res = ent if (plain and ctx.bn_in is None) else None
        y, stats = conv_raw(d, dt, wp, b32, act, Cout, ldy, want_stats, x0.device, "igemm_fwd", flops)
        ctx.save_for_backward(x0, x1, weight, y if act != ACT_NONE else None)
        ctx.params = (weight, bias)
        ctx.cfg = (stride, pad, reflect, act, upcat, bias is not None, IH, IW, OH, OW)
        ctx.want_stats = want_stats
        if HEAD_BIAS_FUSED and bias is not None and act == ACT_NONE and Cout == 1 and not want_stats and n_out == 1:
            _HANDOVER.put_head_slot(y, bias)          # a disparity head: depth_head's backward can produce this layer's bias gradient on its way
        if want_stats:
            ctx.mark_non_differentiable(stats)
            return y, stats
        return aliases(y, n_out)        # sde_act_bwd_bias_sum adds two of their gradients on the fly

    @staticmethod
    def backward(ctx, *douts):
        x0, x1, weight, y = ctx.saved_tensors
        dy, dy1 = fan_in(douts[:1] if ctx.want_stats else douts, 2) or (None, None)
        stride, pad, reflect, act, upcat, has_bias, IH, IW, OH, OW = ctx.cfg
        dt = x0.dtype
        V = vec_of(dt)
        lib = L.lib()
        dev = x0.device
        B, H0, W0, C0 = x0.shape
        C1 = x1.shape[3] if x1 is not None else 0
        Cout, Cin, KH, KW = weight.shape
        ldy = pad_to(Cout, V)
        if dy is None:
            return (None,) * 12
        off_main = MAIN_STREAM is not None and torch.cuda.current_stream() != MAIN_STREAM
        if off_main and not L.is_aux_stream(torch.cuda.current_stream()):
            # e.g. part of the forward pass ran under torch.cuda.stream(helper): autograd then replays this node's backward on that stream,
            # underneath fork / join events recorded against the trainer's stream (operands could be recycled while a GEMM still reads them)
            raise L.SdeHipError("conv2d backward is running on a different stream than the one the backward phase started on; the "
                                "weight-gradient side-stream bookkeeping supports one main stream (plus the registered auxiliary stream) only")
        # off_main: a layer of the network that runs on the auxiliary stream (PoseNet): both of its GEMMs stay on that stream, in order -- no fork,
        # no group queue; its slabs still join the phase's batched reduction, which the trainer launches after joining the auxiliary stream
        dy = dy.contiguous()
        M = B * OH * OW
        flops = 2.0 * M * Cout * KH * KW * Cin                    # algorithmic FLOPs of each of dgrad / wgrad
        # 1. activation backward + bias gradient
        dbias = None
        dz = dy
        # (the depth head's backward already summed this one-channel layer's bias gradient into its slot: nothing left to do in this step)
        head_did_bias = has_bias and act == ACT_NONE and dy1 is None and _HANDOVER.take_head_done(dy, ctx.params[1])
        if has_bias and not head_did_bias and _HANDOVER.drop_head_done(ctx.params[1]):
            # depth_head's backward already accumulated its share of this bias gradient, but the gradient arriving here is not the tensor it
            # returned: the logit has a second consumer and autograd summed the two -- adding the full column sum on top would count the
            # head's share twice (the slot call accumulates)
            raise L.SdeHipError("conv2d backward: the one-channel output feeding depth_head has a second consumer; the fused disparity-head bias "
                                "gradient supports exactly one (set hip.nn.HEAD_BIAS_FUSED = False for such a graph)")
        if (act != ACT_NONE or has_bias or dy1 is not None) and not head_did_bias:
            nblk = lib.sde_reduce_num_blocks(M, ldy)
            part = torch.empty(nblk + REDUCE_ROWS, ldy, device=dev) if has_bias else None
            bslot = _grad_slot(ctx.params[1]) if has_bias else None
            dbias = (bslot if bslot is not None else torch.empty(Cout, device=dev)) if has_bias else None
            dz = torch.empty_like(dy) if (act != ACT_NONE or dy1 is not None) else None
            # the column partials' final sum is nothing the chain waits for: into a gradient slot it rides in the phase's ONE batched finalize (flush)
            later = bslot is not None and WGRAD_DEFER.add_bias(part, nblk, ldy, Cout, bslot)
            L.check(lib.sde_act_bwd_bias_sum(L.ptr(dy), L.ptr(dy1), L.ptr(y), act, M, ldy, dtype_code(dt), L.ptr(dz), L.ptr(part), None if later else L.ptr(dbias), Cout,
                                             int(bslot is not None), L.stream()), "sde_act_bwd_bias_sum")
            if bslot is not None:
                dbias = None
            if dz is None:
                dz = dy
        need_dx = ctx.needs_input_grad[0] or (x1 is not None and ctx.needs_input_grad[1])
        # 2. weight gradient -- the phase's reducer places it (side stream when a data gradient follows, so the two independent GEMMs overlap).
        # It goes first: launching the data-gradient GEMM ahead of the fork measured 10 % slower end to end
        dw = side = None
        if ctx.needs_input_grad[2]:
            d = _desc(x0, x1, SRC_UPCAT if upcat else SRC_PLAIN, KH, KW, stride, pad, reflect, IH, IW, OH, OW)
            splits = lib.sde_conv_wgrad_splits(ctypes.byref(d), Cout)
            wslot = _grad_slot(ctx.params[0])
            esz = 4 if dt == torch.float32 else 2
            meta = dict(M=M, N=Cout, K=KH * KW * (C0 + C1), k=KH, s=stride, mode=int(upcat), splits=splits,
                        bytes=esz * (B * H0 * W0 * C0 + B * IH * IW * C1 + M * ldy) + 8 * splits * Cout * KH * KW * (C0 + C1)) if L.PROFILE is not None else None
            dw = wslot if wslot is not None else torch.empty(weight.shape, device=dev)      # a fresh gradient tensor is plain OIHW
            wflags = (1 if wslot is not None else 0) | (2 if is_ohwi(dw) else 0)                # SDE_WREDUCE_ACCUMULATE | SDE_WREDUCE_OHWI
            op_bytes = (dz.numel() + x0.numel() + (x1.numel() if x1 is not None else 0)) * dz.element_size()
            dw, side = WGRAD_DEFER.weight_grad(WGradJob(d, dz, x0, x1, Cout, ldy, Cin, C0 + C1, KH * KW, splits, wslot, dw, wflags,
                                                        4 * splits * Cout * KH * KW * (C0 + C1), op_bytes, need_dx, off_main, flops, meta))
        # 3. data gradient
        dx0 = dx1 = None
        if need_dx:
            Cv = C0 + C1
            wd = ctx.wd_pre if ctx.wd_pre is not None else pack_weight(weight, dt, Cv, ldy, for_dgrad=True)   # [Cv][KH][KW][ldy], taps flipped
            if reflect:
                dd = _desc(dz, None, SRC_PLAIN, KH, KW, 1, KH - 1, False, OH, OW, IH + 2, IW + 2)
                dxp, _ = conv_raw(dd, dt, wd, None, ACT_NONE, Cv, Cv, False, dev, "igemm_dgrad", flops)
                dx0 = torch.empty_like(x0)
                dx1 = torch.empty_like(x1) if x1 is not None else None
                L.check(lib.sde_refl_fold(L.ptr(dxp), B, IH, IW, Cv, C0, int(upcat), dtype_code(dt), L.ptr(dx0), L.ptr(dx1), L.stream()), "sde_refl_fold")
            else:
                if upcat:
                    raise L.SdeHipError("upsample+concat source is only supported with reflection padding (decoder)")
                if stride == 1:
                    dd = _desc(dz, None, SRC_PLAIN, KH, KW, 1, KH - 1 - pad, False, OH, OW, IH, IW)
                    if ctx.bn_in_res is not None:
                        dx0 = _dgrad_bnbwd(dd, wd, dz, x0, Cv, ctx.bn_in_res, flops, res=True)
                    elif ctx.bn_in is not None and BNBWD_FUSED:
                        dx0 = _dgrad_bnbwd(dd, wd, dz, x0, Cv, ctx.bn_in, flops, res=False)
                elif stride == 2:
                    # virtual zero-inserted gradient image: Z[2i, 2j] = dz[i, j]
                    dd = _desc(dz, None, SRC_ZEROINS, KH, KW, 1, KH - 1 - pad, False, 2 * OH - 1, 2 * OW - 1, IH, IW)
                else:
                    raise L.SdeHipError(f"stride {stride} not supported")
                if dx0 is None:
                    dx0, _ = conv_raw(dd, dt, wd, None, ACT_NONE, Cv, Cv, False, dev, "igemm_dgrad", flops)
        # 4. join a weight-gradient GEMM that forked alone (now or SDE_JOIN_LAG layers later); dz / x0 / x1 stay alive until then
        WGRAD_DEFER.join(side, (dz, x0, x1))
        return dx0, dx1, dw, dbias, None, None, None, None, None, None, None, None


def _wptr(t):
    """Device pointer of a dense conv-weight-shaped tensor in either memory order (L.ptr insists on torch-contiguous tensors)."""
    if not (t.is_cuda and _dense(t)):
        raise L.SdeHipError("weight gradient buffer must be a dense CUDA tensor (OIHW or channels-last)")
    return c_void_p(t.data_ptr())


EARLY_TAIL = True       # the last queued weight-gradient group is forked when the chain reaches a layer without a data gradient (A/B: False = at the flush)
BIAS_DEFER = True       # bias-gradient column sums of a backward phase in one launch at its end (False: one finalize launch per layer, on the chain)


class ColsumItem(Structure):
    _fields_ = [("part", c_void_p), ("out", c_void_p), ("rows", c_int32), ("ld", c_int32), ("C", c_int32), ("accumulate", c_int32)]


class WReduceItem(Structure):
    _fields_ = [("slab", c_void_p), ("dw", c_void_p), ("rows", c_int32), ("Cout", c_int32), ("KHW", c_int32), ("Cin_pad", c_int32),
                ("Cin_real", c_int32), ("accumulate", c_int32)]


# One convolution's weight-gradient GEMM as _Conv2d.backward hands it to the phase's reducer (dw: the gradient slot wslot, or a fresh OIHW tensor)
WGradJob = namedtuple("WGradJob", "d dz x0 x1 Cout ldy Cin Cin_pad KHW splits wslot dw flags slab_bytes op_bytes need_dx off_main flops meta")


def wgrad_group_rule(queued, queued_bytes, groups_done, op_bytes, need_dx, fork, first_group, group, max_bytes, budget_bytes, early_tail):
    """Side-stream group boundaries for one layer of a backward phase on the main stream, from plain numbers (the open group, the layer, the
    schedule knobs).  Returns (fork the open group first, "group" / "alone" (a fork of its own) / "inline", fork the group once this layer is queued)."""
    if not fork:
        # a layer without a data gradient (the stem) ends the chain: its GEMM runs on the main stream, so the open group goes to the side stream
        # NOW, underneath it, instead of after it at the phase's flush
        return queued > 0 and not need_dx and early_tail, "inline", False
    if group <= 1 or op_bytes > max_bytes:
        # layers with very large operands (PackNet's full-resolution 64-channel maps: 190 MB each) fork on their own, after the open group (layer
        # order): holding three of them alive for a group pushes the working set out of the Infinity Cache (PackNet-1A: 60.2 vs 58.4 ms/step)
        return queued > 0, "alone", False
    digits = str(first_group) if first_group else ""      # decimal digits = sizes of the first groups of the phase (33: 3 then 3)
    limit = int(digits[groups_done]) if groups_done < len(digits) else group
    # a group closes after `limit` layers or once its operands (kept alive until the group's GEMMs ran) reach the byte budget
    return False, "group", queued + 1 >= limit or queued_bytes + op_bytes >= budget_bytes


class WGradReducer:
    """Owns where each convolution's weight gradient of a backward phase runs (weight_grad, join) and its reduction: ONE batched launch at the end of
    the phase (phase, flush).  Nothing persists across steps: slabs come from the caching allocator (the graph pool under capture) and are released
    at flush.  defer=False, immediate mode (substitute optimizers, a backward outside any phase): every weight gradient is reduced and joined at once."""

    def __init__(self, defer=True):
        self.defer = defer
        self._drop()

    def _drop(self):
        self.first_group = None    # this phase's first-group digits when they differ from hip.lib.FIRST_GROUP (second phase of a two-phase backward)
        self.jobs, self._seen = [], set()                # (slab, gradient slot, WReduceItem fields) of the deferred slab reductions
        self.bias_jobs, self._seen_bias = [], set()      # (partial slab, rows, ld, C, gradient slot) of convolutions whose bias-gradient finalize is deferred
        self.pending = []          # (event behind side-stream work, its operands) whose join is lagging (SDE_JOIN_LAG)
        self.queue = []            # (launch, operands) of layers whose weight-gradient GEMM waits for its group's fork
        self.queue_bytes = 0       # operand bytes held by the queued layers
        self.groups_done = 0       # groups forked so far in this backward phase

    @contextlib.contextmanager
    def phase(self, device, phase_b=False):
        """One backward phase on ONE main stream: flushes on normal exit; after an exception it still joins the side stream and drops the rest."""
        global WGRAD_DEFER, MAIN_STREAM
        WGRAD_DEFER, MAIN_STREAM = self, (torch.cuda.current_stream() if device.type == "cuda" else None)
        self.first_group = L.FIRST_GROUP_B if phase_b else None
        try:
            yield
            self.flush()
        finally:
            WGRAD_DEFER, MAIN_STREAM = _NO_PHASE, None
            _HANDOVER.end_phase()           # no hand-over between backward nodes outlives the phase
            self.join_pending()
            self._drop()

    def weight_grad(self, j):
        """Launch or queue the GEMM of one WGradJob: straight into the gradient slot, slabs for the phase's batched reduction, or GEMM + reduction
        at once; queued into a group, forked alone or inline.  Returns (the weight gradient for autograd, the side stream to join() or None)."""
        fork = j.need_dx and L.SIDE_STREAM and L.PROFILE is None and not j.off_main
        if fork and L.FORK_MIN_BYTES:      # (A/B aid, default 0: every layer forks)
            fork = j.op_bytes >= L.FORK_MIN_BYTES
        run_first, place, close = False, ("alone" if fork else "inline"), False
        if self.defer and not j.off_main:
            run_first, place, close = wgrad_group_rule(len(self.queue), self.queue_bytes, self.groups_done, j.op_bytes, j.need_dx, fork,
                                                       L.FIRST_GROUP if self.first_group is None else self.first_group,
                                                       L.WGRAD_GROUP, L.GROUP_MAX_BYTES, L.GROUP_BUDGET_BYTES, EARLY_TAIL)
        if run_first:
            self.run_queue()
        side = L.side_stream() if place != "inline" else None
        if place == "alone":
            self.join_pending(keep=L.JOIN_LAG - 1)      # lagging joins of earlier layers
            side.wait_stream(torch.cuda.current_stream())
        # (a weight used twice in one phase reduces at once: two blocks of one batched launch must not accumulate into the same slot)
        ok = self.defer and j.wslot is not None and j.wslot.data_ptr() not in self._seen
        # one pixel range and a channels-last slot without channel padding: the GEMM's only "slab" IS the gradient row block -- it writes
        # straight into the (zeroed) flat gradient, nothing to reduce
        direct = (ok and j.splits == 1 and j.Cin_pad == j.Cin and (j.KHW == 1 or is_ohwi(j.wslot)) and j.wslot.data_ptr() % 16 == 0
                  and L.PROFILE is None)
        # small slab stacks wait for the phase's one batched reduction; big ones (ResNet-50's 20-40 MB stacks add up to ~1 GB per step)
        # are summed at once while they are still in the Infinity Cache and their block can be recycled
        deferred = ok and not direct and j.slab_bytes <= L.DEFER_MAX_BYTES
        slab = j.wslot if direct else torch.empty(j.splits, j.Cout, j.KHW * j.Cin_pad, device=j.x0.device)
        if direct or deferred:
            self._seen.add(j.wslot.data_ptr())
        if deferred:
            self.jobs.append((slab, j.wslot, (slab.data_ptr(), j.wslot.data_ptr(), j.splits, j.Cout, j.KHW, j.Cin_pad, j.Cin, j.flags)))
        launch = functools.partial(self._launch, j, slab, "direct" if direct else "deferred" if deferred else "reduce", side)
        if place == "group":      # launched by run_queue, in the group's side-stream context
            self.queue.append((launch, (j.dz, j.x0, j.x1, slab, j.dw)))
            self.queue_bytes += j.op_bytes
            if close:
                self.run_queue()
        else:
            with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
                launch()
        return (None if j.wslot is not None else j.dw), (side if place == "alone" else None)

    @staticmethod
    def _launch(j, slab, target, side):
        # a GEMM forked beside the data-gradient chain takes the family's slim LDS ring (two persistent-GEMM workgroups stay resident on its compute
        # unit); an inline one (the stem, layers without a data gradient) has nothing beside it and keeps whatever SDE_OPT_WGRAD_DMA_RING says
        ring = L.wgrad_dma_ring() if side is not None else 0
        if ring:
            old = set_option(OPT_WGRAD_DMA_RING, ring)
            try:
                return WGradReducer._launch_ring(j, slab, target, side)
            finally:
                set_option(OPT_WGRAD_DMA_RING, old)
        return WGradReducer._launch_ring(j, slab, target, side)

    @staticmethod
    def _launch_ring(j, slab, target, side):
        lib = L.lib()
        if target == "reduce" and L.PROFILE is None:
            L.check(lib.sde_conv_wgrad(ctypes.byref(j.d), L.ptr(j.dz), j.Cout, j.ldy, j.Cin, L.ptr(slab), j.splits, _wptr(j.dw), j.flags, L.stream()),
                    "sde_conv_wgrad")
        else:
            rows = 1 if target == "direct" else j.splits
            _timed("wgrad", j.flops, 0, lambda: L.check(lib.sde_conv_wgrad_partial(ctypes.byref(j.d), L.ptr(j.dz), j.Cout, j.ldy, _wptr(slab), rows,
                                                                                   L.stream()), "sde_conv_wgrad_partial"), j.meta)
            if target == "reduce":      # the same two launches, timed separately (bench.py's roofline pass: GEMM FLOPs against GEMM time)
                one = (WReduceItem * 1)(WReduceItem(slab.data_ptr(), j.dw.data_ptr(), j.splits, j.Cout, j.KHW, j.Cin_pad, j.Cin, j.flags))
                _timed("wgrad_reduce", 0.0, 0, lambda: L.check(lib.sde_wgrad_reduce_batched(one, 1, L.stream()), "sde_wgrad_reduce_batched"),
                       dict(jobs=1))
        if side is not None and target != "direct":
            slab.record_stream(side)

    def join(self, side, operands):
        """After the layer's data gradient: wait for a GEMM that forked alone onto `side`, SDE_JOIN_LAG layers later (lagging join: the main
        stream goes on with the next layers' backward; the operands stay alive until then) or at once."""
        if side is not None and L.JOIN_LAG > 0 and self.defer:
            self.pending.append((side.record_event(), operands))
        elif side is not None:
            torch.cuda.current_stream().wait_stream(side)

    def run_queue(self):
        """Launch the queued weight-gradient GEMMs of the last few layers behind ONE fork of the side stream (one cross-stream edge per group in
        the captured graph instead of one per layer) and leave one lagging join for the whole group."""
        if not self.queue:
            return
        side = L.side_stream()
        self.join_pending(keep=L.JOIN_LAG - 1)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for launch, _ in self.queue:
                launch()
        self.pending.append((side.record_event(), [operands for _, operands in self.queue]))
        self.queue, self.queue_bytes = [], 0
        self.groups_done += 1

    def join_pending(self, keep=0):
        """Make the current stream wait for all but the newest `keep` lagging weight-gradient GEMMs and release their operands."""
        while len(self.pending) > max(0, keep):
            torch.cuda.current_stream().wait_event(self.pending.pop(0)[0])

    def add_bias(self, part, rows, ld, C, bslot):
        """Leave a bias gradient's column partials to the phase's batched finalize (True), unless that is off or the bias was seen in this phase
        (two blocks of one launch must not accumulate into the same slot)."""
        if not (self.defer and BIAS_DEFER and L.PROFILE is None and bslot.data_ptr() not in self._seen_bias):
            return False
        self._seen_bias.add(bslot.data_ptr())
        self.bias_jobs.append((part, rows, ld, C, bslot))
        return True

    def flush(self):
        """End of a phase: the last group, every join, and the deferred bias and slab sums in one launch each."""
        self.run_queue()
        self.groups_done = 0
        self.join_pending()
        if self.bias_jobs:
            arr = (ColsumItem * len(self.bias_jobs))(*[ColsumItem(p.data_ptr(), b.data_ptr(), r, ld, C, 1) for p, r, ld, C, b in self.bias_jobs])
            L.check(L.lib().sde_colsum_finalize_batched(arr, len(self.bias_jobs), L.stream()), "sde_colsum_finalize_batched")
        self.bias_jobs, self._seen_bias = [], set()
        if not self.jobs:
            return
        items = []
        for slab, wslot, it in self.jobs:
            src, dwp, rows, Cout, KHW, Cin_pad, Cin_real, _ = it
            # host-side operand check: the rows to sum must lie inside the slab tensor, the gradient slot must have the OIHW size
            lo, hi = slab.data_ptr(), slab.data_ptr() + slab.numel() * 4
            if not (src is not None and lo <= src and src + rows * Cout * KHW * Cin_pad * 4 <= hi and wslot.numel() == Cout * Cin_real * KHW
                    and dwp == wslot.data_ptr() and Cin_real <= Cin_pad and rows >= 1):
                raise L.SdeHipError(f"WGradReducer: inconsistent job (slab {tuple(slab.shape)}, src offset {None if src is None else src - lo}, "
                                    f"rows {rows}, Cout {Cout}, KHW {KHW}, Cin_pad {Cin_pad}, Cin_real {Cin_real}, slot {tuple(wslot.shape)})")
            items.append(WReduceItem(*it))
        arr = (WReduceItem * len(items))(*items)
        _timed("wgrad_reduce", 0.0, 0, lambda: L.check(L.lib().sde_wgrad_reduce_batched(arr, len(items), L.stream()), "sde_wgrad_reduce_batched"),
               dict(jobs=len(items)))
        self.jobs, self._seen = [], set()


FUSE_BN_FINALIZE = True  # BatchNorm finalize + apply in one launch where the partial slab is short (A/B: set False)
BNBWD_FUSED = True      # BatchNorm's backward reduce pass in the epilogue of the data-gradient GEMM that produces its incoming gradient (A/B, tests: False)
BNBWD_HITS = 0          # times the fused path ran (tests)
RESBN_FUSED = os.environ.get("SDE_RESBN", "1") != "0"      # ... and the whole reduce pass of a residual BatchNorm in the data gradient of the next block's first convolution (A/B, tests: False)
RESBN_HITS = 0
_NO_PHASE = WGradReducer(defer=False)
WGRAD_DEFER = _NO_PHASE  # the reducer of the running backward phase (WGradReducer.phase)
MAIN_STREAM = None      # ... and the stream it runs on (None: no phase)
FOLD_ROWS = 16          # SDE_WGRAD_FOLD_ROWS


class PackItem(Structure):
    _fields_ = [("src", c_void_p), ("dst_fwd", c_void_p), ("dst_dgrad", c_void_p), ("Cout", c_int32), ("Cin", c_int32), ("KH", c_int32), ("KW", c_int32),
                ("Cin_pad", c_int32), ("Cout_pad", c_int32), ("src_layout", c_int32), ("reserved", c_int32), ("end", ctypes.c_int64)]


W_OIHW, W_OHWI, W_TWIN16 = 0, 1, 2      # SDE_W_*: sde_pack_item.src_layout
TWIN_ALIGN = 16                          # bytes: every GEMM loader fetches a packed operand in 16-byte pieces (uint4 loads, LDS-DMA dwordx4), see DESIGN.md 5.2


def twin_eligible(Cout, Cin, cin_pad, ldy, ohwi, slot_offset, esize=2, base_align=0):
    """True when a convolution's forward operand [ldy][KH][KW][cin_pad] is exactly the cast of its master slot, so that the slot of the 16-bit twin
    (sde_adam_step_twin) can BE the operand: channels-last master, no channel padding on either side, whole 16-byte pieces along both channel axes
    (the data-gradient pack moves 8 elements at a time), and the slot's twin address on the loaders' 16-byte boundary.
    slot_offset: elements from the start of the flat buffer; base_align: the twin allocation's address modulo TWIN_ALIGN (torch allocations: 0).
    Slots are multiples of 4 elements only, so a slot behind a one-element bias sits at 8 bytes modulo 16 and stays on the per-step pack."""
    per = TWIN_ALIGN // esize
    return bool(ohwi and esize == 2 and ldy == Cout and cin_pad == Cin and Cout % per == 0 and Cin % per == 0
                and (base_align + slot_offset * esize) % TWIN_ALIGN == 0)


class WeightPacker:
    """Packs the forward and data-gradient operands of every convolution of a model in ONE kernel launch per step.

    Build it after one forward pass (each HipConv2d then knows the padded shapes its operands need); call run() whenever the master
    weights changed (HipTrainer does, at the start of every step, inside the captured graph).

    With `twin` (HipTrainer(twin_operands=True): the 16-bit image of the flat parameter buffer that the Adam kernel keeps, `offset_of(weight)` = the
    weight's slot offset in it) every layer that twin_eligible() accepts gets its slot of the twin as forward operand and leaves the fp32 table:
    run() packs the rest (stem, one-channel heads, misaligned slots) from fp32 as before -- everything the forward pass reads, so also, from the twin, the
    "data-gradient" operand of a shared transposed convolution, which is that layer's forward operand; run_dgrad() builds the other shared layers'
    data-gradient operands from the twin and is safe to run beside the forward pass; refresh() re-derives everything, twin slots included, from the fp32 masters (eager; whenever someone other than the Adam
    kernel wrote parameters)."""

    def __init__(self, model, twin=None, offset_of=None):
        import numpy as np
        convs = [m for m in model.modules() if getattr(m, "_pack_shapes", None) is not None]
        if not convs:
            raise L.SdeHipError("WeightPacker: run one forward pass first")
        self.dtype = convs[0]._pack_shapes[0]
        if twin is not None and not (twin.dtype == self.dtype and twin.element_size() == 2 and twin.is_contiguous()):
            raise L.SdeHipError(f"WeightPacker: the twin is {twin.dtype}, the operands {self.dtype}")
        rest, dgrad, full = [], [], []        # per-step table of the head of the step, per-step twin table, refresh table; `end` is each table's own prefix sum
        n_shared = 0
        self._keep = []
        for m in convs:
            dt, cin_pad, ldy = m._pack_shapes
            if dt != self.dtype:
                raise L.SdeHipError("WeightPacker: mixed compute dtypes")
            w = m.weight
            Cout, Cin, KH, KW = w.shape
            nb = L.lib().sde_pack_item_blocks(ldy, cin_pad, KH, KW)
            if nb <= 0:
                raise L.SdeHipError(f"WeightPacker: unsupported kernel size {KH}x{KW}")
            if not _dense(w):
                raise L.SdeHipError("WeightPacker: conv weights must be dense (OIHW or channels-last)")
            off = offset_of(w) if twin is not None else None
            ohwi = is_ohwi(w) or (KH * KW == 1 and w.is_contiguous())        # (a 1x1 weight is the same memory either way)
            shared = off is not None and twin_eligible(Cout, Cin, cin_pad, ldy, ohwi, off, twin.element_size(), twin.data_ptr() % TWIN_ALIGN)
            wp = twin[off:off + w.numel()].view(ldy, KH, KW, cin_pad) if shared else torch.empty(ldy, KH, KW, cin_pad, device=w.device, dtype=dt)
            wd = torch.empty(cin_pad, KH, KW, ldy, device=w.device, dtype=dt)
            m._packed = (wp, wd)
            shape = (Cout, Cin, KH, KW, cin_pad, ldy)
            item = (w.data_ptr(), wp.data_ptr(), wd.data_ptr()) + shape + (W_OHWI if is_ohwi(w) else W_OIHW, 0)
            full.append(item + (nb,))
            if shared:
                # a layer whose forward pass reads the "data-gradient" operand (a transposed convolution IS the data gradient of its adjoint) needs it at the
                # head of the step like any forward operand: its twin item rides in run()'s table, not in the one that may run beside the forward pass
                early = bool(getattr(m, "FORWARD_READS_DGRAD_OPERAND", False))
                (rest if early else dgrad).append((wp.data_ptr(), None, wd.data_ptr()) + shape + (W_TWIN16, 0, nb))
                n_shared += 1
            else:
                rest.append(item + (nb,))
            self._keep.append((w, wp, wd))
        dev = convs[0].weight.device

        def table(rows):
            if not rows:
                return None, 0, 0
            end, out = 0, []
            for it in rows:
                end += it[-1]
                out.append(PackItem(*it[:-1], end))
            arr = (PackItem * len(out))(*out)
            return torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).to(dev), len(out), end
        self.items, self.n, self.total = table(rest)
        self.items_dgrad, self.n_dgrad, self.total_dgrad = table(dgrad)
        self.items_full, self.n_full, self.total_full = table(full) if n_shared else (self.items, self.n, self.total)
        self.n_shared = n_shared
        self._ptrs = [w.data_ptr() for w, _, _ in self._keep]

    def _launch(self, items, n, total):
        if any(w.data_ptr() != p for (w, _, _), p in zip(self._keep, self._ptrs)):
            raise L.SdeHipError("WeightPacker: a weight tensor moved (e.g. flattened after the packer was built); rebuild the packer")
        if n:
            L.check(L.lib().sde_pack_weights_batched(L.ptr(items), n, total, dtype_code(self.dtype), L.stream()), "sde_pack_weights_batched")

    def run(self):
        """Both operands of every layer that does not share the twin, from the fp32 masters (all layers when there is no twin), and the operands that a
        shared layer's FORWARD pass reads besides its slot of the twin (transposed convolutions)."""
        self._launch(self.items, self.n, self.total)

    def run_dgrad(self):
        """The data-gradient operands of the layers whose forward operand is a slot of the twin, transposed from that slot: read by backward only."""
        self._launch(self.items_dgrad, self.n_dgrad, self.total_dgrad)

    def refresh(self):
        """Every operand of every layer from the fp32 masters, the shared slots of the twin included."""
        self._launch(self.items_full, self.n_full, self.total_full)


def conv2d(x, weight, bias=None, stride=1, pad=0, reflect=False, act=ACT_NONE, skip=None, upsample=False, bn_stats=False, owner=None, n_out=1):
    """y = act(conv(x) + bias) on NHWC tensors.

    upsample=True: the input is cat(nearest_x2(x), skip) (skip may be None) -- depth_decoder.py:L102-105 -- gathered on the fly.
    bn_stats=True additionally returns the per-tile (sum, sum^2) slab BatchNorm needs.
    n_out > 1 returns that many aliases of the output, one per consumer: their gradients are summed by the activation-backward kernel instead
    of by an autograd add kernel per extra consumer.
    """
    return _Conv2d.apply(x, skip, weight, bias, int(stride), int(pad), bool(reflect), int(act), bool(upsample), bool(bn_stats), owner, int(n_out))


# ---------------------------------------------------------------------------------------------------------------
# Transposed convolution 3x3 / stride 2 / padding 1 / output_padding 1 (+bias, +ReLU): GoogleResNetv2's up-sampling layer
# ---------------------------------------------------------------------------------------------------------------
DECONV_DIRECT = True    # forward on the parity-split kernel (sde_deconv3x3s2_fwd); False: the zero-insertion route through the convolution engine + its
                        # ReLU pass (A/B baseline, and a second implementation to test against)
DECONV_RULE = True      # ... except the layers deconv_direct() sends back to that route; False: every layer takes the kernel (tests, A/B)


def deconv_direct(B, H, W, C, ldy, esize):
    """Whether the forward of a layer takes the parity-split kernel.  Its workgroup (an 8 x 16 pixel tile x 32 output channels) walks the input channels
    in serial 64-byte steps; a layer with 16 or more steps whose grid has fewer workgroups than the device has compute units (256) leaves that walk
    exposed, and the engine's split-K GEMM over the zero-inserted image was measured faster there: GoogleResNetv2's 512 -> 256 layer at 16 x 6 x 10,
    19.6 against 18.5 us (profiles/google_v2_bench.txt).  Every other layer of that network takes the kernel (1.12 - 5.0 x faster)."""
    if not DECONV_DIRECT:
        return False
    if not DECONV_RULE:
        return True
    workgroups = B * ((H + 7) // 8) * ((W + 15) // 16) * ((ldy + 31) // 32 if ldy > 16 else 1)
    return not (C * esize >= 16 * 64 and workgroups < 256)


class _ConvTranspose2d(torch.autograd.Function):
    """y = act(ConvTranspose2d(x) + bias).  The weight [Cin,Cout,3,3], read as OIHW, is the weight of the adjoint Conv2d(Cout -> Cin, 3, stride 2,
    padding 1): the forward is that convolution's data gradient (operand: its for_dgrad pack), the data gradient its forward, the weight gradient its
    weight gradient with x in the role of the output gradient -- every backward GEMM is the engine's, in the phase's weight-gradient schedule."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, owner=None):
        if not x.is_contiguous():
            raise L.SdeHipError("conv_transpose2d: the NHWC input must be contiguous")
        if act not in (ACT_NONE, ACT_RELU):
            raise L.SdeHipError(f"conv_transpose2d: activation {act} is not supported (ACT_NONE, ACT_RELU)")
        dt = x.dtype
        if dt not in (torch.float32, torch.bfloat16):
            raise L.SdeHipError(f"conv_transpose2d runs in fp32 or bf16, not {dt}")
        V = vec_of(dt)
        B, H, W, C = x.shape
        Cin, Cout, KH, KW = weight.shape
        if (KH, KW) != (3, 3):
            raise L.SdeHipError("conv_transpose2d: 3x3 kernels only")
        if C % V or Cin > C:
            raise L.SdeHipError(f"conv_transpose2d: weight expects {Cin} input channels, the tensor carries {C} (multiples of {V})")
        ldy = pad_to(Cout, V)
        pre = getattr(owner, "_packed", None) if owner is not None else None
        if pre is not None and pre[0].dtype == dt and pre[0].shape == (C, 3, 3, ldy):
            ctx.wb_pre, wf = pre                                   # (adjoint forward operand, its flipped data-gradient operand), packed once per step
        else:
            wf, ctx.wb_pre = pack_weight(weight, dt, ldy, C, for_dgrad=True), None     # [ldy][3][3][C], taps flipped
            if owner is not None:
                owner._pack_shapes = (dt, ldy, C)                  # WeightPacker's (dtype, Cin_pad, Cout_pad) of the ADJOINT convolution
        b32 = _f32(bias) if bias is not None else None
        flops = 2.0 * B * H * W * 9 * Cin * Cout                   # algorithmic: nine tap products per input pixel
        lib = L.lib()
        if deconv_direct(B, H, W, C, ldy, x.element_size()):
            y = torch.empty(B, 2 * H, 2 * W, ldy, device=x.device, dtype=dt)
            meta = dict(M=4 * B * H * W, N=ldy, K=9 * C // 4, k=3, s=2, mode=3, bytes=x.element_size() * (x.numel() + y.numel())) if L.PROFILE is not None else None
            _timed("igemm_fwd", flops, 0, lambda: L.check(lib.sde_deconv3x3s2_fwd(L.ptr(x), L.ptr(wf), L.ptr(b32), act, B, H, W, C, Cout, ldy, dtype_code(dt),
                                                                                   L.ptr(y), L.stream()), "sde_deconv3x3s2_fwd"), meta)
        else:
            # the layer as the data gradient of its adjoint: nine taps per output pixel over the virtual zero-inserted image Z[2i, 2j] = x[i, j]
            d = _desc(x, None, SRC_ZEROINS, 3, 3, 1, 1, False, 2 * H - 1, 2 * W - 1, 2 * H, 2 * W)
            y, _ = conv_raw(d, dt, wf, b32, ACT_NONE, Cout, ldy, False, x.device, "igemm_fwd", flops)
            if act == ACT_RELU:
                z, y = y, torch.empty_like(y)
                L.check(lib.sde_relu_fwd(L.ptr(z), z.numel(), dtype_code(dt), L.ptr(y), L.stream()), "sde_relu_fwd")
        ctx.save_for_backward(x, weight, y if act != ACT_NONE else None)
        ctx.params = (weight, bias)
        ctx.act = act
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        act, has_bias = ctx.act, ctx.params[1] is not None
        dt = x.dtype
        V = vec_of(dt)
        lib = L.lib()
        dev = x.device
        B, H, W, C = x.shape
        Cin, Cout = weight.shape[:2]
        ldy = pad_to(Cout, V)
        off_main = MAIN_STREAM is not None and torch.cuda.current_stream() != MAIN_STREAM
        if off_main and not L.is_aux_stream(torch.cuda.current_stream()):
            raise L.SdeHipError("conv_transpose2d backward is running on a different stream than the one the backward phase started on")
        dy = dy.contiguous()
        M = B * 4 * H * W
        flops = 2.0 * B * H * W * 9 * Cin * Cout
        # 1. activation backward + bias gradient (as _Conv2d.backward: the column partials' final sum rides in the phase's batched finalize)
        dbias, dz = None, dy
        if act != ACT_NONE or has_bias:
            nblk = lib.sde_reduce_num_blocks(M, ldy)
            part = torch.empty(nblk + REDUCE_ROWS, ldy, device=dev) if has_bias else None
            bslot = _grad_slot(ctx.params[1]) if has_bias else None
            dbias = (bslot if bslot is not None else torch.empty(Cout, device=dev)) if has_bias else None
            dz = torch.empty_like(dy) if act != ACT_NONE else None
            later = bslot is not None and WGRAD_DEFER.add_bias(part, nblk, ldy, Cout, bslot)
            L.check(lib.sde_act_bwd_bias_sum(L.ptr(dy), None, L.ptr(y), act, M, ldy, dtype_code(dt), L.ptr(dz), L.ptr(part), None if later else L.ptr(dbias), Cout,
                                             int(bslot is not None), L.stream()), "sde_act_bwd_bias_sum")
            if bslot is not None:
                dbias = None
            if dz is None:
                dz = dy
        need_dx = ctx.needs_input_grad[0]
        # the adjoint convolution: dz [B,2H,2W,ldy] -> [B,H,W,C], 3x3, stride 2, padding 1
        d = _desc(dz, None, SRC_PLAIN, 3, 3, 2, 1, False, 2 * H, 2 * W, H, W)
        # 2. weight gradient = the adjoint's, with x in the role of its output gradient: it lands in [Cin,Cout,3,3], the weight's own order
        dw = side = None
        if ctx.needs_input_grad[1]:
            splits = lib.sde_conv_wgrad_splits(ctypes.byref(d), Cin)
            wslot = _grad_slot(ctx.params[0])
            esz = 4 if dt == torch.float32 else 2
            meta = dict(M=B * H * W, N=Cin, K=9 * ldy, k=3, s=2, mode=0, splits=splits,
                        bytes=esz * (dz.numel() + x.numel()) + 8 * splits * Cin * 9 * ldy) if L.PROFILE is not None else None
            dw = wslot if wslot is not None else torch.empty(weight.shape, device=dev)
            wflags = (1 if wslot is not None else 0) | (2 if is_ohwi(dw) else 0)
            op_bytes = (dz.numel() + x.numel()) * dz.element_size()
            dw, side = WGRAD_DEFER.weight_grad(WGradJob(d, x, dz, None, Cin, C, Cout, ldy, 9, splits, wslot, dw, wflags, 4 * splits * Cin * 9 * ldy, op_bytes,
                                                        need_dx, off_main, flops, meta))
        # 3. data gradient = the adjoint's forward (a plain stride-2 convolution of dz: no zero insertion)
        dx = None
        if need_dx:
            wb = ctx.wb_pre if ctx.wb_pre is not None else pack_weight(weight, dt, ldy, C)       # [C][3][3][ldy]
            dx, _ = conv_raw(d, dt, wb, None, ACT_NONE, Cin, C, False, dev, "igemm_dgrad", flops)
        WGRAD_DEFER.join(side, (dz, x))
        return dx, dw, dbias, None, None


def conv_transpose2d(x, weight, bias=None, act=ACT_NONE, owner=None):
    """y = act(F.conv_transpose2d(x, weight, bias, stride=2, padding=1, output_padding=1)) on NHWC tensors: x [B,H,W,C] -> [B,2H,2W,pad(Cout)];
    weight [Cin,Cout,3,3] (torch's ConvTranspose2d layout), act ACT_NONE or ACT_RELU."""
    return _ConvTranspose2d.apply(x, weight, bias, int(act), owner)


# ---------------------------------------------------------------------------------------------------------------
# Grouped 3x3 convolution (padding 1, stride 1 or 2, no bias): the 3x3 of a ResNeXt bottleneck
# ---------------------------------------------------------------------------------------------------------------
GCONV_DIRECT = True     # the grouped kernels (csrc/gconv.hip); False: a dense block-diagonal weight through conv2d, 32 x the useful FLOPs at 32 groups
                        # (A/B baseline, and a second implementation to test against)
GCONV_CG = (4, 8, 16, 32, 64)       # supported channels per group


def _gconv_check(x, weight, groups, stride):
    if x.dim() != 4 or weight.dim() != 4:
        raise L.SdeHipError("grouped_conv3x3: x is NHWC [B,H,W,C], weight [C, C/groups, 3, 3]")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise L.SdeHipError(f"grouped_conv3x3 runs in fp32 or bf16, not {x.dtype}")
    C, Cg, KH, KW = weight.shape
    if (KH, KW) != (3, 3):
        raise L.SdeHipError(f"grouped_conv3x3: 3x3 kernels only, got {KH}x{KW}")
    if stride not in (1, 2):
        raise L.SdeHipError(f"grouped_conv3x3: stride 1 or 2 only, got {stride}")
    if groups <= 0 or C != Cg * groups or x.shape[3] != C:
        raise L.SdeHipError(f"grouped_conv3x3: channel mismatch: the weight {tuple(weight.shape)} with {groups} groups maps {Cg * groups} -> {C} channels, "
                            f"the tensor carries {x.shape[3]} (input and output channels must be equal)")
    if Cg not in GCONV_CG or C % 16:
        raise L.SdeHipError(f"grouped_conv3x3: {Cg} channels per group of {C} are not supported: channels per group in {GCONV_CG}, channels a multiple of 16")
    if weight.dtype != torch.float32 or not _dense(weight):
        raise L.SdeHipError("grouped_conv3x3: the weight must be a dense float32 tensor (OIHW or channels-last)")
    if not x.is_contiguous():
        raise L.SdeHipError("grouped_conv3x3: the NHWC input must be contiguous")


class _GroupedConv3x3(torch.autograd.Function):
    """y = conv2d(x, weight, padding=1, stride, groups).  The kernels read the fp32 master weight in either memory order: nothing is packed.  Backward runs
    the data gradient and then the weight gradient on the current stream: the layer joins neither WGradReducer's groups nor its side stream."""

    @staticmethod
    def forward(ctx, x, weight, groups, stride, want_stats, n_out):
        ctx.set_materialize_grads(False)
        if n_out > 1 and want_stats:
            raise L.SdeHipError("grouped_conv3x3: output aliases (n_out) belong to the BatchNorm that follows when statistics are requested")
        # x may be a BatchNorm + ReLU output registered for a fused backward reduction: this layer's data gradient does not carry one, and the entry must not linger
        _HANDOVER.take_bn_out(x)
        B, H, W, C = x.shape
        Cg = C // groups
        OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
        lib, code = L.lib(), dtype_code(x.dtype)
        y = torch.empty(B, OH, OW, C, device=x.device, dtype=x.dtype)
        stats = None
        if want_stats:
            rows = lib.sde_gconv3x3_stats_rows(B, H, W, C, groups, stride, code)
            if rows <= 0:
                raise L.SdeHipError(f"sde_gconv3x3_stats_rows failed: {lib.sde_last_error().decode()}")
            stats = torch.empty(rows + REDUCE_ROWS, C, 2, device=x.device, dtype=torch.float32)
        flops = 2.0 * B * OH * OW * C * 9 * Cg                     # algorithmic
        meta = dict(M=B * OH * OW, N=C, K=9 * Cg, k=3, s=stride, mode=4, bytes=x.element_size() * (x.numel() + y.numel())) if L.PROFILE is not None else None
        _timed("igemm_fwd", flops, 0, lambda: L.check(lib.sde_gconv3x3_fwd(L.ptr(x), _wptr(weight), int(is_ohwi(weight)), B, H, W, C, groups, stride, code, L.ptr(y),
                                                                           L.ptr(stats), L.stream()), "sde_gconv3x3_fwd"), meta)
        ctx.save_for_backward(x, weight)
        ctx.param = weight
        ctx.cfg = (groups, stride, want_stats)
        if want_stats:
            ctx.mark_non_differentiable(stats)
            return y, stats
        return aliases(y, n_out)

    @staticmethod
    def backward(ctx, *douts):
        x, weight = ctx.saved_tensors
        groups, stride, want_stats = ctx.cfg
        grads = fan_in(douts[:1] if want_stats else douts, 1)
        if not grads:
            return (None,) * 6
        dz = grads[0]
        B, H, W, C = x.shape
        Cg = C // groups
        M = B * dz.shape[1] * dz.shape[2]
        lib, code = L.lib(), dtype_code(x.dtype)
        flops = 2.0 * M * C * 9 * Cg
        esz = x.element_size()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            meta = dict(M=B * H * W, N=C, K=9 * Cg, k=3, s=stride, mode=4, bytes=esz * (dz.numel() + dx.numel())) if L.PROFILE is not None else None
            _timed("igemm_dgrad", flops, 0, lambda: L.check(lib.sde_gconv3x3_dgrad(L.ptr(dz), _wptr(weight), int(is_ohwi(weight)), B, H, W, C, groups, stride, code,
                                                                                   L.ptr(dx), L.stream()), "sde_gconv3x3_dgrad"), meta)
        if ctx.needs_input_grad[1]:
            wslot = _grad_slot(ctx.param)
            dw = wslot if wslot is not None else torch.empty(weight.shape, device=x.device)      # a fresh gradient tensor is plain OIHW
            wflags = (1 if wslot is not None else 0) | (2 if is_ohwi(dw) else 0)                   # SDE_WREDUCE_ACCUMULATE | SDE_WREDUCE_OHWI
            ws_bytes = lib.sde_gconv3x3_wgrad_ws_bytes(B, H, W, C, groups, stride, code)
            ws = torch.empty(ws_bytes // 4, device=x.device, dtype=torch.float32)
            meta = dict(M=M, N=C, K=9 * Cg, k=3, s=stride, mode=4, bytes=esz * (dz.numel() + x.numel()) + 2 * ws_bytes) if L.PROFILE is not None else None
            def call():
                L.check(lib.sde_gconv3x3_wgrad(L.ptr(x), L.ptr(dz), B, H, W, C, groups, stride, code, L.ptr(ws), ws_bytes, _wptr(dw), wflags, L.stream()), "sde_gconv3x3_wgrad")
            # (the profiler repeats a timed launch PROFILE_REPEAT times back to back: only the overwriting form is idempotent)
            if wslot is None or L.PROFILE_REPEAT == 1:
                _timed("wgrad", flops, 0, call, meta)
            else:
                call()
            if wslot is not None:
                dw = None
        return dx, dw, None, None, None, None


def _gconv_dense_weight(weight, groups):
    """The dense [C,C,3,3] weight with the groups' blocks on its diagonal and zeros elsewhere; autograd gathers the blocks back."""
    C, Cg = weight.shape[:2]
    co = torch.arange(C, device=weight.device)
    ci = (co // Cg * Cg)[:, None] + torch.arange(Cg, device=weight.device)[None, :]
    return torch.zeros(C, C, 3, 3, device=weight.device, dtype=weight.dtype).index_put((co[:, None], ci), weight)


def grouped_conv3x3(x, weight, groups, stride=1, bn_stats=False, n_out=1):
    """y = F.conv2d(x, weight, None, stride, 1, groups=groups) on NHWC tensors, input and output channels equal: weight [C, C/groups, 3, 3] (torch's).
    Supported: fp32 / bf16, 3x3, stride 1 or 2, C % 16 == 0, C / groups in GCONV_CG.  bn_stats / n_out as conv2d's."""
    groups, stride = int(groups), int(stride)
    _gconv_check(x, weight, groups, stride)
    if GCONV_DIRECT:
        return _GroupedConv3x3.apply(x, weight, groups, stride, bool(bn_stats), int(n_out))
    return conv2d(x, _gconv_dense_weight(weight, groups), None, stride, 1, bn_stats=bn_stats, n_out=n_out)


# ---------------------------------------------------------------------------------------------------------------
# BatchNorm (+ReLU, +residual)
# ---------------------------------------------------------------------------------------------------------------
class _BatchNormAct(torch.autograd.Function):
    """BatchNorm (+residual, +ReLU).  n_out > 1 returns that many aliases of the output, one per consumer (next block's first convolution, its
    residual / down-sampling path, a decoder skip): backward then receives the consumers' gradients separately and the kernels sum them on the
    fly, instead of autograd launching an add kernel per extra consumer (23 per step on ResNet-50, 1.5 GB of traffic)."""

    @staticmethod
    def forward(ctx, y, stats, gamma, beta, running_mean, running_var, residual, relu, momentum, eps, training, n_out):
        ctx.set_materialize_grads(False)
        dt = y.dtype
        C = y.shape[-1]
        M = y.numel() // C
        lib = L.lib()
        dev = y.device
        bnp = torch.empty(4, C, device=dev)
        out = torch.empty_like(y)
        tiles = stats.shape[0] - REDUCE_ROWS if training else 0
        if training and FUSE_BN_FINALIZE and lib.sde_bn_finalize_apply_ok(tiles, C, dtype_code(dt)):
            # short partial slabs (one row per persistent workgroup of the producing GEMM): finalize + apply in one launch
            L.check(lib.sde_bn_finalize_apply(L.ptr(stats), tiles, C, M, L.ptr(_f32(gamma)), L.ptr(_f32(beta)), L.ptr(running_mean), L.ptr(running_var),
                                              momentum, eps, L.ptr(bnp), L.ptr(y), L.ptr(residual), int(relu), dtype_code(dt), L.ptr(out), L.stream()),
                    "sde_bn_finalize_apply")
        else:
            if training:
                L.check(lib.sde_bn_finalize(L.ptr(stats), tiles, C, M, L.ptr(_f32(gamma)), L.ptr(_f32(beta)), L.ptr(running_mean), L.ptr(running_var),
                                            momentum, eps, L.ptr(bnp), L.stream()), "sde_bn_finalize")
            else:
                L.check(lib.sde_bn_eval_params(L.ptr(_f32(gamma)), L.ptr(_f32(beta)), L.ptr(running_mean), L.ptr(running_var), eps, C, L.ptr(bnp), L.stream()),
                        "sde_bn_eval_params")
            L.check(lib.sde_bn_apply(L.ptr(y), L.ptr(bnp), L.ptr(residual), int(relu), M, C, dtype_code(dt), L.ptr(out), L.stream()), "sde_bn_apply")
        # backward needs the ReLU mask: with a residual it comes from the saved output; without one sde_bn_bwd re-derives it from y and the
        # BatchNorm parameters (out = NULL), so that tensor is neither kept for backward nor read by it
        ctx.save_for_backward(y, out if (relu and residual is not None) else None, bnp, gamma)
        ctx.params = (gamma, beta)
        ctx.cfg = (relu, residual is not None, training)
        if training and relu and residual is None and n_out == 1 and dt != torch.float32 and C % 64 == 0 and ctx.needs_input_grad[0] and BNBWD_FUSED:
            # candidates for the fused backward reduction: the convolution that consumes `out` (and nothing else does: n_out == 1) picks this up
            _HANDOVER.put_bn_out(out, y, bnp)
        ctx.res_ptr = residual.data_ptr() if residual is not None else None
        if training and relu and residual is not None and n_out == 2 and dt != torch.float32 and C % 64 == 0 and ctx.needs_input_grad[0] and BNBWD_FUSED and RESBN_FUSED:
            # residual BatchNorm + ReLU with two consumers (torchvision's blocks: the next block's first convolution and its skip path): that convolution's
            # data gradient can carry this BatchNorm's backward reduce pass (residual form), see _Conv2d.backward
            _HANDOVER.put_bn_out(out, y, bnp, res=True)
            ctx.res_tag = out.data_ptr()              # (this BatchNorm's backward drops the entry: the consuming convolution took its references in forward)
        return aliases(out, n_out)

    @staticmethod
    def backward(ctx, *douts):
        y, out, bnp, gamma = ctx.saved_tensors
        relu, has_res, training = ctx.cfg
        if getattr(ctx, "res_tag", None) is not None:
            _HANDOVER.drop_bn_out_res(ctx.res_tag)
        if not training:
            raise L.SdeHipError("BatchNorm backward in eval mode is not on the path")
        grads = [d for d in fan_in(douts, 3) if d is not None]
        if not grads:
            return (None,) * 12
        dt = y.dtype
        C = y.shape[-1]
        M = y.numel() // C
        lib = L.lib()
        dev = y.device
        coef = torch.empty(2, C, device=dev)
        gs, bs = _grad_slot(ctx.params[0]), _grad_slot(ctx.params[1])
        direct = gs is not None and bs is not None
        dgamma = gs if direct else torch.empty(C, device=dev)
        dbeta = bs if direct else torch.empty(C, device=dev)
        dy = torch.empty_like(y)
        # the data-gradient GEMM that produced this gradient already masked and reduced it (sde_conv_dgrad_bnbwd; residual form: the next block's first
        # convolution formed gm = (its data gradient + the skip gradient) * relu'(out) and reduced it): finalize + apply only
        ent = _HANDOVER.take_bn_part(grads[0], res=has_res) if (relu and len(grads) == 1 + has_res) else None
        fits = ent is not None and ent[0] == y.data_ptr() and grads[0].shape == y.shape and grads[0].dtype == dt
        if has_res and ent is not None and not (fits and ent[3] == grads[1].data_ptr()):
            raise L.SdeHipError("BatchNorm backward: a data gradient that already contains the skip path's gradient arrived at a BatchNorm it was not "
                                "formed for (hip.nn.RESBN_FUSED = False selects the separate reduce pass)")
        if fits:
            global BNBWD_HITS, RESBN_HITS
            RESBN_HITS += has_res
            BNBWD_HITS += not has_res
            gm = grads[0]
            L.check(lib.sde_bn_bwd_from_part(L.ptr(ent[1]), ent[2], L.ptr(gm), L.ptr(y), L.ptr(bnp), M, C, dtype_code(dt), L.ptr(coef), L.ptr(dgamma),
                                             L.ptr(dbeta), int(direct), L.ptr(dy), L.stream()), "sde_bn_bwd_from_part")
            if has_res and ctx.res_ptr is not None:
                _HANDOVER.put_res_grad(ctx.res_ptr, gm)
            if direct:
                dgamma = dbeta = None
            return dy, None, dgamma, dbeta, None, None, (gm if has_res else None), None, None, None, None, None
        part = torch.empty(lib.sde_reduce_num_blocks(M, C) + REDUCE_ROWS, C, 2, device=dev)
        # gm = relu'(out) * (sum of the incoming gradients): needed when there is anything to mask or to sum; it is also the residual's gradient
        gm = torch.empty_like(y) if (relu or len(grads) > 1) else None
        d0, d1, d2 = (grads + [None, None])[:3]
        L.check(lib.sde_bn_bwd(L.ptr(d0), L.ptr(d1), L.ptr(d2), L.ptr(out), L.ptr(y), L.ptr(bnp), L.ptr(gamma), int(relu), M, C, dtype_code(dt), L.ptr(part),
                               L.ptr(coef), L.ptr(dgamma), L.ptr(dbeta), int(direct), L.ptr(gm), L.ptr(dy), L.stream()), "sde_bn_bwd")
        dres = (gm if gm is not None else d0) if has_res else None
        if dres is not None and ctx.res_ptr is not None and RESBN_FUSED:
            _HANDOVER.put_res_grad(ctx.res_ptr, dres, if_expected=True)         # the skip path's gradient, for the data gradient of the convolution that shares the block input (residual form)
        if direct:
            dgamma = dbeta = None
        return dy, None, dgamma, dbeta, None, None, dres, None, None, None, None, None


def batch_norm_act(y, stats, gamma, beta, running_mean, running_var, residual=None, relu=True, momentum=0.1, eps=1e-5, training=True, n_out=1):
    return _BatchNormAct.apply(y, stats, gamma, beta, running_mean, running_var, residual, bool(relu), float(momentum), float(eps), bool(training), int(n_out))


# ---------------------------------------------------------------------------------------------------------------
# MaxPool 3x3 / 2
# ---------------------------------------------------------------------------------------------------------------
class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, n_out=1):
        ctx.set_materialize_grads(False)
        B, H, W, C = x.shape
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        out = torch.empty(B, OH, OW, C, device=x.device, dtype=x.dtype)
        idx = torch.empty(B, OH, OW, C, device=x.device, dtype=torch.uint8)
        L.check(L.lib().sde_maxpool_fwd(L.ptr(x.contiguous()), B, H, W, C, dtype_code(x.dtype), L.ptr(out), L.ptr(idx), L.stream()), "sde_maxpool_fwd")
        ctx.save_for_backward(idx)
        ctx.shape = (B, H, W, C)
        return aliases(out, n_out)

    @staticmethod
    def backward(ctx, *douts):
        (idx,) = ctx.saved_tensors
        B, H, W, C = ctx.shape
        grads = fan_in(douts, 2)
        if not grads:
            return None, None
        d0, d1 = grads
        dx = torch.empty(B, H, W, C, device=d0.device, dtype=d0.dtype)
        L.check(L.lib().sde_maxpool_bwd_sum(L.ptr(d0), L.ptr(d1), L.ptr(idx), B, H, W, C, dtype_code(d0.dtype), L.ptr(dx), L.stream()), "sde_maxpool_bwd_sum")
        return dx, None


def max_pool_3x3_s2(x, n_out=1):
    """n_out > 1: that many aliases of the pooled tensor (layer1's first block reads it twice); backward sums their gradients in the kernel."""
    return _MaxPool.apply(x, int(n_out))


# ---------------------------------------------------------------------------------------------------------------
# Input preparation and the depth head tail
# ---------------------------------------------------------------------------------------------------------------
def prep_input(img, mean, std, dtype, flip=False):
    """NCHW fp32 image -> (img - mean)/std as NHWC `dtype` with channels padded to 16 bytes (no autograd: images carry no grad)."""
    if img.dtype != torch.float32:
        raise L.SdeHipError("prep_input expects a float32 NCHW image")
    img = img.contiguous()
    B, C, H, W = img.shape
    Cp = pad_to(C, vec_of(dtype))
    out = torch.empty(B, H, W, Cp, device=img.device, dtype=dtype)
    m = _f32(mean.reshape(-1)) if mean is not None else None
    s = _f32(std.reshape(-1)) if std is not None else None
    L.check(L.lib().sde_prep_input(L.ptr(img), L.ptr(m), L.ptr(s), B, C, H, W, Cp, int(bool(flip)), dtype_code(dtype), L.ptr(out), L.stream()), "sde_prep_input")
    return out


HEAD_BIAS_HITS = 0       # times the fused path below ran (tests)
HEAD_BIAS_FUSED = True   # the bias gradient of a one-channel convolution feeding depth_head comes out of depth_head's backward (False: separate pass; tests)


class _DepthHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, min_depth, max_depth, flip):
        ctx.bias_param = _HANDOVER.take_head_slot(y)
        B, H, W, ld = y.shape
        depth = torch.empty(B, 1, H, W, device=y.device, dtype=torch.float32)
        L.check(L.lib().sde_depth_head_fwd(L.ptr(y.contiguous()), B, H, W, ld, min_depth, max_depth, int(flip), dtype_code(y.dtype), L.ptr(depth), L.stream()),
                "sde_depth_head_fwd")
        ctx.save_for_backward(y)
        ctx.cfg = (min_depth, max_depth, flip)
        return depth

    @staticmethod
    def backward(ctx, ddepth):
        (y,) = ctx.saved_tensors
        min_depth, max_depth, flip = ctx.cfg
        B, H, W, ld = y.shape
        dy = torch.empty_like(y)
        lib = L.lib()
        bslot = _grad_slot(ctx.bias_param) if ctx.bias_param is not None else None
        if bslot is not None and bslot.numel() == 1:
            # the convolution in front has ONE output channel: its bias gradient is the sum of the logit gradients this kernel writes -- summed here,
            # into the flat gradient, instead of by a separate pass over the (8-channel padded) gradient tensor in the convolution's backward
            part = torch.empty(lib.sde_depth_head_bias_blocks(B, H, W), device=y.device)
            L.check(lib.sde_depth_head_bwd_bias(L.ptr(y), L.ptr(ddepth.contiguous().float()), B, H, W, ld, min_depth, max_depth, int(flip), dtype_code(y.dtype),
                                                L.ptr(dy), L.ptr(part), L.ptr(bslot), 1, L.stream()), "sde_depth_head_bwd_bias")
            global HEAD_BIAS_HITS
            HEAD_BIAS_HITS += 1
            _HANDOVER.put_head_done(dy, ctx.bias_param)
        else:
            L.check(lib.sde_depth_head_bwd(L.ptr(y), L.ptr(ddepth.contiguous().float()), B, H, W, ld, min_depth, max_depth, int(flip), dtype_code(y.dtype),
                                           L.ptr(dy), L.stream()), "sde_depth_head_bwd")
        return dy, None, None, None


def depth_head(y, min_depth, max_depth, flip=False):
    """softplus + disp_to_depth(...)[1] (+ flip) on channel 0 of y -> [B,1,H,W] fp32 depth."""
    return _DepthHead.apply(y, float(min_depth), float(max_depth), bool(flip))


# ---------------------------------------------------------------------------------------------------------------
# GroupNorm + ReLU
# ---------------------------------------------------------------------------------------------------------------
class _GroupNormReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, relu, res=None):
        B, H, W, C = x.shape
        dev = x.device
        part = torch.empty(B, GN_CHUNKS, C, 2, device=dev)
        gnp = torch.empty(B, groups, 2, device=dev)
        out = torch.empty_like(x)
        x = x.contiguous()
        if res is not None:
            if res.shape != x.shape or res.dtype != x.dtype:
                raise L.SdeHipError("group_norm_relu: the residual must have the input's shape and dtype")
            res = res.contiguous()
        L.check(L.lib().sde_gn_relu_res_fwd(L.ptr(x), L.ptr(res), L.ptr(_f32(gamma)), L.ptr(_f32(beta)), B, H * W, C, groups, eps, int(relu), dtype_code(x.dtype),
                                            L.ptr(part), L.ptr(gnp), L.ptr(out), L.stream()), "sde_gn_relu_res_fwd")
        ctx.save_for_backward(x, out, gnp, gamma, res)
        ctx.params = (gamma, beta)
        ctx.cfg = (groups, relu)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, out, gnp, gamma, res = ctx.saved_tensors
        groups, relu = ctx.cfg
        B, H, W, C = x.shape
        dev = x.device
        part = torch.empty(B, GN_CHUNKS, C, 2, device=dev)
        coef = torch.empty(B, groups, 2, device=dev)
        gs, bs = _grad_slot(ctx.params[0]), _grad_slot(ctx.params[1])
        direct = gs is not None and bs is not None
        dgamma = gs if direct else torch.empty(C, device=dev)
        dbeta = bs if direct else torch.empty(C, device=dev)
        dx = torch.empty_like(x)
        L.check(L.lib().sde_gn_relu_res_bwd(L.ptr(dout.contiguous()), L.ptr(out), L.ptr(x), L.ptr(res), L.ptr(gnp), L.ptr(_f32(gamma)), B, H * W, C, groups, int(relu),
                                            dtype_code(x.dtype), L.ptr(part), L.ptr(coef), L.ptr(dgamma), L.ptr(dbeta), int(direct), L.ptr(dx), L.stream()),
                "sde_gn_relu_res_bwd")
        if direct:
            dgamma = dbeta = None
        # the normalised tensor is x + res: both receive the same gradient (one tensor, no copy)
        return dx, dgamma, dbeta, None, None, None, (dx if res is not None else None)


GN_CHUNKS = 64          # SDE_GN_CHUNKS
GN_ACT = {False: 0, True: 1, "none": 0, "relu": 1, "elu": 2}


def group_norm_relu(x, gamma, beta, groups=16, eps=1e-5, relu=True, residual=None):
    """GroupNorm + activation; relu: True / "relu" (PoseNet.py:L13-20), "elu" (layers01.py:L33-40), False / "none".
    residual: the normalised tensor is x + residual (layers01.py:L74-76), summed inside the kernels."""
    if x.shape[-1] != gamma.numel():
        raise L.SdeHipError("group_norm_relu: channel padding is not supported (PoseNet / PackNet channels are multiples of 16)")
    return _GroupNormReLU.apply(x, gamma, beta, int(groups), float(eps), GN_ACT[relu], residual)


# ---------------------------------------------------------------------------------------------------------------
# PackNet01's data movement (csrc/packnet.hip): space-to-depth / depth-to-space, channel concatenation, the inverse-depth head
# ---------------------------------------------------------------------------------------------------------------
def _s2d(x, inverse):
    x = x.contiguous()
    B, H, W, C = x.shape
    if inverse:
        y = torch.empty(B, 2 * H, 2 * W, C // 4, device=x.device, dtype=x.dtype)
        L.check(L.lib().sde_depth_to_space(L.ptr(x), B, H, W, C, dtype_code(x.dtype), L.ptr(y), L.stream()), "sde_depth_to_space")
    else:
        y = torch.empty(B, H // 2, W // 2, 4 * C, device=x.device, dtype=x.dtype)
        L.check(L.lib().sde_space_to_depth(L.ptr(x), B, H, W, C, dtype_code(x.dtype), L.ptr(y), L.stream()), "sde_space_to_depth")
    return y


class _SpaceToDepth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, inverse):
        ctx.inverse = inverse
        return _s2d(x, inverse)

    @staticmethod
    def backward(ctx, dy):
        return _s2d(dy, not ctx.inverse), None


def space_to_depth(x):
    """layers01.py:L138-160 `packing` (r = 2) on NHWC: out[b,y,x,c*4+dy*2+dx] = in[b,2y+dy,2x+dx,c]."""
    return _SpaceToDepth.apply(x, False)


def depth_to_space(x):
    """nn.PixelShuffle(2) on NHWC: out[b,2y+dy,2x+dx,c] = in[b,y,x,c*4+dy*2+dx]."""
    return _SpaceToDepth.apply(x, True)


class _Concat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p0, p1, inv, add):
        p0 = p0.contiguous()
        B, H, W, C0 = p0.shape
        V = vec_of(p0.dtype)
        C1 = p1.shape[3] if p1 is not None else 0
        if p1 is not None:
            p1 = p1.contiguous()
            if p1.dtype != p0.dtype or p1.shape[:3] != p0.shape[:3]:
                raise L.SdeHipError("concat: sources differ in dtype or spatial size")
        if inv is not None:
            inv = inv.contiguous()
            if inv.dtype != torch.float32 or tuple(inv.shape) != (B, H // 2, W // 2):
                raise L.SdeHipError(f"concat: the inverse-depth map must be fp32 [B, H/2, W/2], got {tuple(inv.shape)} {inv.dtype}")
        Ct = pad_to(C0 + (0 if add else C1) + (1 if inv is not None else 0), V)
        out = torch.empty(B, H, W, Ct, device=p0.device, dtype=p0.dtype)
        L.check(L.lib().sde_concat_fwd(L.ptr(p0), L.ptr(p1), L.ptr(inv), int(add), B, H, W, C0, C1, Ct, dtype_code(p0.dtype), L.ptr(out), L.stream()), "sde_concat_fwd")
        ctx.cfg = (B, H, W, C0, C1, Ct, add, inv is not None, p1 is not None)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, H, W, C0, C1, Ct, add, has_inv, has_p1 = ctx.cfg
        dout = dout.contiguous()
        d0 = torch.empty(B, H, W, C0, device=dout.device, dtype=dout.dtype)
        d1 = torch.empty(B, H, W, C1, device=dout.device, dtype=dout.dtype) if (has_p1 and not add) else None
        dinv = torch.empty(B, H // 2, W // 2, device=dout.device, dtype=torch.float32) if (has_inv and ctx.needs_input_grad[2]) else None
        L.check(L.lib().sde_concat_bwd(L.ptr(dout), int(add), B, H, W, C0, C1, Ct, dtype_code(dout.dtype), L.ptr(d0), L.ptr(d1), L.ptr(dinv), L.stream()), "sde_concat_bwd")
        return d0, (d0 if (add and has_p1) else d1), dinv, None


def concat(p0, p1=None, inv_depth=None, add=False):
    """cat([p0, p1(, nearest_x2(inv_depth))], channel) -- or [p0 + p1(, ...)] with add=True -- zero-filled to the 16-byte group, in one pass
    (PackNet01.py:L150-199).  inv_depth: fp32 [B, H/2, W/2]."""
    return _Concat.apply(p0, p1, inv_depth, bool(add))


class _InvDepthHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, min_depth_head, min_depth, max_depth, flip):
        y = y.contiguous()
        B, H, W, ld = y.shape
        inv = torch.empty(B, H, W, device=y.device, dtype=torch.float32)
        depth = torch.empty(B, 1, H, W, device=y.device, dtype=torch.float32)
        L.check(L.lib().sde_inv_depth_head_fwd(L.ptr(y), B, H, W, ld, min_depth_head, min_depth, max_depth, int(flip), dtype_code(y.dtype), L.ptr(inv), L.ptr(depth),
                                               L.stream()), "sde_inv_depth_head_fwd")
        ctx.save_for_backward(y)
        ctx.cfg = (min_depth_head, min_depth, max_depth, flip)
        ctx.set_materialize_grads(False)
        return inv, depth

    @staticmethod
    def backward(ctx, d_inv, d_depth):
        (y,) = ctx.saved_tensors
        if d_inv is None and d_depth is None:
            return None, None, None, None, None
        mdh, mn, mx, flip = ctx.cfg
        B, H, W, ld = y.shape
        dy = torch.empty_like(y)
        di = d_inv.contiguous().float() if d_inv is not None else None
        dd = d_depth.contiguous().float() if d_depth is not None else None
        L.check(L.lib().sde_inv_depth_head_bwd(L.ptr(y), L.ptr(di), L.ptr(dd), B, H, W, ld, mdh, mn, mx, int(flip), dtype_code(y.dtype), L.ptr(dy), L.stream()),
                "sde_inv_depth_head_bwd")
        return dy, None, None, None, None


def inv_depth_head(y, min_depth_head, min_depth, max_depth, flip=False):
    """(sigmoid(y[...,0]) / min_depth_head  [B,H,W] fp32,  disp_to_depth(.)[1] [B,1,H,W] fp32, mirrored along x when flip) -- layers01.py:L105-133 and
    PackNet01.py:L120-123,L199."""
    return _InvDepthHead.apply(y, float(min_depth_head), float(min_depth), float(max_depth), bool(flip))


# ---------------------------------------------------------------------------------------------------------------
# PackNet's Conv3d(1, 8, 3, padding=1) over the (channel, y, x) volume (layers01.py:L223-298)
# ---------------------------------------------------------------------------------------------------------------
class _Conv3dPack(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        B, H, W, D = x.shape
        lib = L.lib()
        x = x.contiguous()
        y = torch.empty(B, H, W, 8 * D, device=x.device, dtype=x.dtype)
        L.check(lib.sde_conv3d_fwd(L.ptr(x), L.ptr(_f32(weight)), L.ptr(_f32(bias)), B, H, W, D, dtype_code(x.dtype), L.ptr(y), L.stream()), "sde_conv3d_fwd")
        ctx.save_for_backward(x, weight)
        ctx.params = (weight, bias)
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return None, None, None
        x, weight = ctx.saved_tensors
        B, H, W, D = x.shape
        lib = L.lib()
        dy = dy.contiguous()
        dc = dtype_code(x.dtype)
        ws, bs = _grad_slot(ctx.params[0]), _grad_slot(ctx.params[1])
        direct = ws is not None and bs is not None
        dw = ws if direct else torch.empty_like(weight)
        db = bs if direct else torch.empty(8, device=x.device)
        part = torch.empty(lib.sde_conv3d_wgrad_num_blocks(B, H, W, D, dc), 224, device=x.device)
        L.check(lib.sde_conv3d_wgrad(L.ptr(x), L.ptr(dy), B, H, W, D, dc, L.ptr(part), L.ptr(dw), L.ptr(db), int(direct), L.stream()), "sde_conv3d_wgrad")
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            L.check(lib.sde_conv3d_dgrad(L.ptr(dy), L.ptr(_f32(weight)), B, H, W, D, dc, L.ptr(dx), L.stream()), "sde_conv3d_dgrad")
        return dx, (None if direct else dw), (None if direct else db)


def conv3d_pack(x, weight, bias):
    """x: NHWC [B,H,W,D]; weight [8,1,3,3,3] fp32; bias [8] -> [B,H,W,8*D] (channel = feature*D + ch, as view(b, c*d, h, w))."""
    if tuple(weight.shape) != (8, 1, 3, 3, 3):
        raise L.SdeHipError(f"conv3d_pack: weight shape {tuple(weight.shape)} (expected [8,1,3,3,3])")
    return _Conv3dPack.apply(x, weight, bias)


# ---------------------------------------------------------------------------------------------------------------
# Fused Adam / AdamW over a flat buffer
# ---------------------------------------------------------------------------------------------------------------
ADAM_MAX_SEG = 8       # SDE_ADAM_MAX_SEG
GRAD_NORM_WORK = 1024  # SDE_GRAD_NORM_WORK: floats of sde_grad_norm's workspace


class AdamDesc(Structure):
    _fields_ = [("seg_end", c_long * ADAM_MAX_SEG), ("seg_lr", c_float * ADAM_MAX_SEG), ("seg_wd", c_float * ADAM_MAX_SEG), ("nseg", c_int32),
                ("decoupled_wd", c_int32), ("beta1", c_float), ("beta2", c_float), ("eps", c_float), ("bias_corr1", c_float), ("bias_corr2", c_float),
                ("grad_scale", c_float), ("scale_state", c_void_p), ("beta1_d", ctypes.c_double), ("beta2_d", ctypes.c_double), ("clip_state", c_void_p)]


def adam_step(p, g, m, v, seg_end, seg_lr, seg_wd, bias_corr, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, decoupled_wd=False, scale_state=None,
              clip_state=None, twin=None):
    """seg_end / seg_lr / seg_wd: HOST sequences (one entry per segment); everything travels by value in the kernel arguments.
    scale_state: optional device float[4] {loss_scale, found_inf, growth_tracker, applied_steps} (fp16 dynamic loss scaling); with it the
    kernel forms the bias corrections itself from the device-side count of APPLIED steps and `bias_corr` is ignored.
    clip_state: optional device float[2] {total_norm, clip_coef} that grad_norm() filled: the gradient enters the update times clip_coef.
    twin: optional bf16 / fp16 device tensor of p.numel() elements: the kernel also leaves twin[i] = cast(p[i]) (sde_adam_step_twin; same p, m, v)."""
    nseg = len(seg_end)
    if not (0 < nseg <= ADAM_MAX_SEG and len(seg_lr) == nseg and len(seg_wd) == nseg):
        raise L.SdeHipError(f"adam_step: {nseg} segments (at most {ADAM_MAX_SEG})")
    d = AdamDesc()
    for i in range(nseg):
        d.seg_end[i], d.seg_lr[i], d.seg_wd[i] = int(seg_end[i]), float(seg_lr[i]), float(seg_wd[i])
    d.nseg, d.decoupled_wd = nseg, int(bool(decoupled_wd))
    d.beta1, d.beta2, d.eps, d.bias_corr1, d.bias_corr2, d.grad_scale = beta1, beta2, eps, float(bias_corr[0]), float(bias_corr[1]), grad_scale
    d.scale_state = scale_state.data_ptr() if scale_state is not None else None
    d.beta1_d, d.beta2_d = float(beta1), float(beta2)
    if clip_state is not None and not (clip_state.is_cuda and clip_state.dtype == torch.float32 and clip_state.is_contiguous() and clip_state.numel() >= 2):
        raise L.SdeHipError("adam_step: clip_state must be a device float32 tensor of 2 elements {total_norm, clip_coef}")
    d.clip_state = clip_state.data_ptr() if clip_state is not None else None
    if scale_state is not None and scale_state.numel() < 4:
        raise L.SdeHipError("adam_step: scale_state must hold 4 floats {loss_scale, found_inf, growth_tracker, applied_steps}")
    if twin is not None:
        if not (twin.is_cuda and twin.dtype in (torch.bfloat16, torch.float16) and twin.is_contiguous() and twin.numel() == p.numel()):
            raise L.SdeHipError("adam_step: twin must be a contiguous bf16 / fp16 device tensor with as many elements as p")
        L.check(L.lib().sde_adam_step_twin(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), ctypes.byref(d), L.ptr(twin), dtype_code(twin.dtype), L.stream()),
                "sde_adam_step_twin")
        return
    L.check(L.lib().sde_adam_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), ctypes.byref(d), L.stream()), "sde_adam_step")


def grad_check(g, scale_state):
    """scale_state[1] = 1 when any element of the flat fp32 gradient is inf / nan (device side, no host sync)."""
    L.check(L.lib().sde_grad_check(L.ptr(g), g.numel(), L.ptr(scale_state), L.stream()), "sde_grad_check")


def grad_norm(g, clip_state, max_norm, grad_scale=1.0, work=None):
    """clip_state[0] = grad_scale * ||g||_2 over the flat fp32 gradient, clip_state[1] = min(1, max_norm / (clip_state[0] + 1e-6)): torch's
    clip_grad_norm_ coefficient, left on the device for adam_step(clip_state=...) (no host sync, no atomics; g is read once and not changed).
    work: device float32[GRAD_NORM_WORK] scratch (allocated when None)."""
    if work is None:
        work = torch.empty(GRAD_NORM_WORK, device=g.device, dtype=torch.float32)
    if g.dtype != torch.float32 or clip_state.dtype != torch.float32 or work.dtype != torch.float32 or clip_state.numel() < 2 or work.numel() < GRAD_NORM_WORK:
        raise L.SdeHipError(f"grad_norm: float32 tensors, clip_state of 2 and work of {GRAD_NORM_WORK} elements")
    L.check(L.lib().sde_grad_norm(L.ptr(g), g.numel(), L.ptr(work), L.ptr(clip_state), float(grad_scale), float(max_norm), L.stream()), "sde_grad_norm")
    return clip_state


def loss_scale_update(scale_state, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
    """torch.cuda.amp.GradScaler.update() on the device scalar triple."""
    L.check(L.lib().sde_loss_scale_update(L.ptr(scale_state), growth_factor, backoff_factor, int(growth_interval), L.stream()), "sde_loss_scale_update")

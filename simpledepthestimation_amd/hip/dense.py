"""Autograd wrappers of the concat-free dense-block operators (csrc/dense.hip, include/sde_hip.h "DenseNet dense blocks").

A dense block is a ``DenseBlock``: the block input plus one tensor per layer (the pieces, NHWC in the compute dtype) and the block's
statistics table.  ``dense_bn_relu`` is torchvision's ``relu(norm1(torch.cat(features, 1)))`` of a layer (or of the transition / norm5 behind
the block); ``dense_piece`` is an identity behind each 3x3 convolution that files its output as the next piece.

Backward: ``dense_bn_relu`` keeps the pieces as autograd inputs, so the engine runs a piece's producer after all of its consumers, but it
returns no gradient for them: it leaves its ``dx`` [M,Cin] in the block's hand-over.  ``dense_piece``'s backward then sums the column slices
of those tensors (plus whatever arrived from outside the block) in one launch.

DENSE_DIRECT = False selects the composed route through the existing operators (hip.bts.cat + hip.bts.channel_stats + HipBatchNorm2d): the
A/B baseline, and a second implementation to test against.
"""
import ctypes
from ctypes import Structure, c_int32, c_void_p

import torch

from . import bts as HB
from . import lib as L
from . import nn as HN

DENSE_DIRECT = True
DENSE_MAX = 40       # SDE_DENSE_MAX


class DenseDesc(Structure):
    _fields_ = [("p", c_void_p * DENSE_MAX), ("C", c_int32 * DENSE_MAX), ("n", c_int32), ("reserved", c_int32)]


# prototypes: hip/lib.py (_PROTOS, "DenseNet dense blocks")


def _desc(tensors):
    if not 1 <= len(tensors) <= DENSE_MAX:
        raise L.SdeHipError(f"dense block: 1..{DENSE_MAX} pieces per launch, got {len(tensors)}")
    d = DenseDesc()
    for k, t in enumerate(tensors):
        d.p[k], d.C[k] = t.data_ptr(), int(t.shape[-1])
    d.n = len(tensors)
    return d


def bwd_rows(M, Cin, dtype):
    """Partial rows of sde_dense_bn_relu_bwd's workspace (shape-only; raises for an unsupported dtype or width)."""
    r = L.lib().sde_dense_bwd_rows(int(M), int(Cin), HN.dtype_code(dtype))
    if r < 0:
        raise L.SdeHipError(f"sde_dense_bwd_rows failed ({r}): {L.lib().sde_last_error().decode()}")
    return r


class DenseBlock:
    """One dense block during one forward pass.  channels: the block's final width (the statistics table's rows); track: batch statistics are
    wanted (some norm of the block is in training mode)."""

    def __init__(self, channels, track=True):
        self.channels, self.track = int(channels), bool(track)
        self.pieces, self.off = [], [0]
        self.table = None        # [channels][2] fp32 (mean, biased variance), filled piece by piece
        self.consumers = []      # number of pieces each dense_bn_relu of this block read, in forward order
        self.dx = {}             # hand-over: consumer index -> its dx [B,H,W,Cin]
        self._cat = None         # composed route: the running concatenation

    @property
    def width(self):
        return self.off[-1]

    def close(self):
        """The forward pass is through with the block: drop the piece list (the pieces' autograd nodes refer to the block, so keeping them here
        would leave the activations to the cycle collector).  Backward needs the offsets, the reader counts and the hand-over only."""
        self.pieces, self.table, self._cat = None, None, None

    def cat(self):
        """The composed route's torch.cat(features, 1): one more copy of the whole map per new piece."""
        if self._cat is None or self._cat[1] < len(self.pieces):
            x, n = self._cat if self._cat is not None else (self.pieces[0], 1)
            for k in range(n, len(self.pieces)):
                x = HB.cat([(x, self.off[k]), (self.pieces[k], self.off[k + 1] - self.off[k])])
            self._cat = (x, len(self.pieces))
        return self._cat[0]


class _DensePiece(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, stats, blk):
        ctx.set_materialize_grads(False)
        C = y.shape[-1]
        M = y.numel() // C
        j = len(blk.pieces)
        if blk.width + C > blk.channels:
            raise L.SdeHipError(f"dense block: piece {j} ({C} channels) exceeds the block's {blk.channels} channels")
        if stats is not None and DENSE_DIRECT:
            if blk.table is None:
                blk.table = torch.empty(blk.channels, 2, device=y.device, dtype=torch.float32)
            L.check(L.lib().sde_dense_stats(L.ptr(stats), stats.shape[0] - HN.REDUCE_ROWS, C, M, L.ptr(blk.table), blk.width, L.stream()), "sde_dense_stats")
        out = y.view(y.shape)
        ctx.blk, ctx.j, ctx.off = blk, j, blk.width
        blk.pieces.append(out)
        blk.off.append(blk.width + C)
        return out

    @staticmethod
    def backward(ctx, gout):
        blk, j, off = ctx.blk, ctx.j, ctx.off
        srcs = [blk.dx[k] for k, n in enumerate(blk.consumers) if n > j and k in blk.dx]
        if j == 0:
            blk.dx = {}              # every other piece has been served: the producers of later pieces run before the block input's
        if not srcs:
            return gout, None, None
        ref = srcs[0]
        g = blk.off[j + 1] - off
        B, H, W = ref.shape[:3]
        out = torch.empty(B, H, W, g, device=ref.device, dtype=ref.dtype)
        gout = gout.contiguous() if gout is not None else None
        L.check(L.lib().sde_dense_grad_gather(ctypes.byref(_desc(srcs)), B * H * W, off, g, HN.dtype_code(ref.dtype), L.ptr(gout), L.ptr(out), L.stream()),
                "sde_dense_grad_gather")
        return out, None, None


def dense_piece(y, blk, stats=None):
    """File y [B,H,W,g] as the block's next piece (its first call files the block input).  stats: the (sum, sum^2) slab of y from the producing
    convolution's epilogue or hip.bts.channel_stats (training).  Returns the piece: an alias of y whose backward gathers the gradients of all
    of its later readers inside the block, plus the gradient of whoever else reads the returned tensor."""
    if not y.is_contiguous():
        raise L.SdeHipError("dense_piece: pieces must be contiguous NHWC tensors")
    if blk.track and stats is None and DENSE_DIRECT:
        raise L.SdeHipError("dense_piece: a block that tracks batch statistics needs the statistics slab of every piece")
    if blk.pieces and (y.shape[:3] != blk.pieces[0].shape[:3] or y.dtype != blk.pieces[0].dtype):
        raise L.SdeHipError("dense_piece: pieces of one block share the batch, the spatial size and the dtype")
    return _DensePiece.apply(y, stats if blk.track else None, blk)


class _DenseBnRelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, blk, gamma, beta, running_mean, running_var, momentum, eps, training, *pieces):
        ctx.set_materialize_grads(False)
        x0 = pieces[0]
        B, H, W = x0.shape[:3]
        Cin = sum(p.shape[-1] for p in pieces)
        out = torch.empty(B, H, W, Cin, device=x0.device, dtype=x0.dtype)
        bnp = torch.empty(4, Cin, device=x0.device, dtype=torch.float32)
        table = blk.table if training else None
        if training and table is None:
            raise L.SdeHipError("dense_bn_relu: training-mode BatchNorm in a block that does not track batch statistics")
        L.check(L.lib().sde_dense_bn_relu_fwd(ctypes.byref(_desc(pieces)), B * H * W, HN.dtype_code(x0.dtype), L.ptr(table), L.ptr(HN._f32(gamma)), L.ptr(HN._f32(beta)),
                                              L.ptr(running_mean), L.ptr(running_var), momentum, eps, L.ptr(bnp), L.ptr(out), L.stream()), "sde_dense_bn_relu_fwd")
        ctx.save_for_backward(bnp, *pieces)
        ctx.params = (gamma, beta)
        ctx.blk, ctx.key, ctx.training = blk, len(blk.consumers), training
        blk.consumers.append(len(pieces))
        return out

    @staticmethod
    def backward(ctx, g):
        n_in = 8 + len(ctx.saved_tensors) - 1
        if g is None:
            return (None,) * n_in
        if not ctx.training:
            raise L.SdeHipError("BatchNorm backward in eval mode is not on the path")
        bnp, pieces = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        g = g.contiguous()
        B, H, W, Cin = g.shape
        M = B * H * W
        dev = g.device
        gamma, beta = ctx.params
        want = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        gs, bs = HN._grad_slot(gamma), HN._grad_slot(beta)
        direct = want and gs is not None and bs is not None
        dgamma = (gs if direct else torch.empty(Cin, device=dev)) if want else None
        dbeta = (bs if direct else torch.empty(Cin, device=dev)) if want else None
        part = torch.empty(bwd_rows(M, Cin, g.dtype), Cin, 2, device=dev, dtype=torch.float32)
        dx = torch.empty_like(g)
        L.check(L.lib().sde_dense_bn_relu_bwd(ctypes.byref(_desc(pieces)), M, HN.dtype_code(g.dtype), L.ptr(g), L.ptr(bnp), L.ptr(part), L.ptr(dgamma), L.ptr(dbeta),
                                              int(direct), L.ptr(dx), L.stream()), "sde_dense_bn_relu_bwd")
        ctx.blk.dx[ctx.key] = dx           # for the gathers of the pieces' own backward nodes (which the engine runs after this one)
        if direct or not want:
            dgamma = dbeta = None
        return (None, dgamma, dbeta) + (None,) * (n_in - 3)


def dense_bn_relu(blk, norm):
    """relu(norm(torch.cat(pieces, 1))) over the block's pieces so far -> [B,H,W,Cin]; norm: a HipBatchNorm2d holder of Cin features."""
    if not blk.pieces:
        raise L.SdeHipError("dense_bn_relu: the block has no pieces yet")
    if norm.num_features != blk.width:
        raise L.SdeHipError(f"dense_bn_relu: norm of {norm.num_features} features over {blk.width} channels")
    if not DENSE_DIRECT:
        x = blk.cat()
        return norm(x, HB.channel_stats(x) if norm.training else None, relu=True)
    if norm.training:
        norm._pending_batches += 1
    return _DenseBnRelu.apply(blk, norm.weight, norm.bias, norm.running_mean, norm.running_var, float(norm.momentum), float(norm.eps), bool(norm.training),
                              *blk.pieces)


class _AvgPool2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        B, H, W, C = x.shape
        out = torch.empty(B, H // 2, W // 2, C, device=x.device, dtype=x.dtype)
        L.check(L.lib().sde_avgpool2x2_fwd(L.ptr(x), B, H, W, C, HN.dtype_code(x.dtype), L.ptr(out), L.stream()), "sde_avgpool2x2_fwd")
        ctx.shape = (B, H, W, C)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, H, W, C = ctx.shape
        dout = dout.contiguous()
        dx = torch.empty(B, H, W, C, device=dout.device, dtype=dout.dtype)
        L.check(L.lib().sde_avgpool2x2_bwd(L.ptr(dout), B, H, W, C, HN.dtype_code(dout.dtype), L.ptr(dx), L.stream()), "sde_avgpool2x2_bwd")
        return dx


def avg_pool_2x2(x):
    """nn.AvgPool2d(kernel_size=2, stride=2) on NHWC x (odd sizes floor)."""
    return _AvgPool2.apply(x.contiguous())

"""Autograd wrappers over the MotionLearning loss entry points of libsde_hip.so (include/sde_hip.h, csrc/motion_loss.hip).

Like hip/photometric.py: each Function owns the tensors its backward needs, kernels never allocate, everything is enqueued on torch's current
stream and nothing synchronises or sizes an allocation by a device value (hipGraph-capture safe).
"""
import ctypes

import torch

from . import lib as L


def _f32c(t):
    if t.dtype != torch.float32:
        raise L.SdeHipError(f"expected float32 tensor, got {t.dtype}")
    if not t.is_cuda:
        raise L.SdeHipError("simpledepthestimation_amd ops need CUDA (HIP) tensors; there is no CPU fallback")
    return t.contiguous()


def _shape(t, shape, name):
    if tuple(t.shape) != tuple(shape):
        raise L.SdeHipError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")


def view_synthesis_pp(image_B, depth_A, K, R, t):
    """camera.py:L166-202 with t [B,3,H,W], forward only (the parity surface): dict(sampled, Z, grid, valid)."""
    image_B, depth_A, K, R, t = _f32c(image_B), _f32c(depth_A), _f32c(K), _f32c(R), _f32c(t)
    B, C, H, W = image_B.shape
    _shape(depth_A, (B, 1, H, W), "depth_A"); _shape(K, (B, 3, 3), "intrinsics"); _shape(R, (B, 3, 3), "R"); _shape(t, (B, 3, H, W), "t")
    dev = image_B.device
    out = {"sampled": torch.empty(B, C, H, W, device=dev), "Z": torch.empty(B, 1, H, W, device=dev),
           "grid": torch.empty(B, H, W, 2, device=dev), "valid": torch.empty(B, 1, H, W, device=dev, dtype=torch.uint8)}
    L.check(L.lib().sde_view_synthesis_pp(L.ptr(image_B), L.ptr(depth_A), L.ptr(K), L.ptr(R), L.ptr(t), B, C, H, W, L.ptr(out["sampled"]), L.ptr(out["Z"]),
                                          L.ptr(out["grid"]), L.ptr(out["valid"]), L.stream()), "sde_view_synthesis_pp")
    return out


def _rgbd_desc(fA, fB, dA, dB, K, R, t, ssim, C1, C2):
    d = L.RgbdDesc()
    d.frame_A, d.frame_B, d.depth_A, d.depth_B = fA.data_ptr(), fB.data_ptr(), dA.data_ptr(), dB.data_ptr()
    d.K, d.R, d.t = K.data_ptr(), R.data_ptr(), t.data_ptr()
    d.N, _, d.H, d.W = fA.shape
    d.ssim, d.C1, d.C2 = int(ssim), C1, C2
    return d


class _Rgbd(torch.autograd.Function):
    """MotionLearning.py:L248-291 up to the per-sample sums: (rgb_l1 [N], ssim [N], depth_l1 [N], grid, occlusion mask, depth proximity weight)."""

    @staticmethod
    def forward(ctx, depth_A, R, t, frame_A, frame_B, depth_B, K, ssim, C1, C2):
        fA, fB, dA, dB, K, R, t = (_f32c(v) for v in (frame_A, frame_B, depth_A, depth_B, K, R, t))
        N, _, H, W = fA.shape
        _shape(fA, (N, 3, H, W), "frame_A"); _shape(fB, (N, 3, H, W), "frame_B"); _shape(dA, (N, 1, H, W), "depth_A"); _shape(dB, (N, 1, H, W), "depth_B")
        _shape(K, (N, 3, 3), "intrinsics"); _shape(R, (N, 3, 3), "R_A2B"); _shape(t, (N, 3, H, W), "t_A2B")
        dev = fA.device
        lib = L.lib()
        nb = lib.sde_rgbd_num_blocks(N, H, W)
        e = lambda *s, **k: torch.empty(*s, device=dev, **k)
        sampled, grid, occ, err, valid = e(N, 3, H, W), e(N, H, W, 2), e(N, 1, H, W), e(N, 1, H, W), e(N, 1, H, W, dtype=torch.uint8)
        dpw = e(N, 1, H, W) if ssim else None
        part1, part2, stats = e(nb, 4), (e(nb) if ssim else None), e(4, N)
        d = _rgbd_desc(fA, fB, dA, dB, K, R, t, ssim, C1, C2)
        L.check(lib.sde_rgbd_fwd(ctypes.byref(d), L.ptr(sampled), L.ptr(grid), L.ptr(occ), L.ptr(err), L.ptr(valid), L.ptr(dpw), L.ptr(part1), L.ptr(part2),
                                 L.ptr(stats), L.stream()), "sde_rgbd_fwd")
        ctx.save_for_backward(fA, fB, dA, dB, K, R, t, sampled, occ, err, dpw, stats)
        ctx.cfg = (ssim, C1, C2)
        outs = (stats[0], stats[1], stats[2], grid, occ, dpw if ssim else e(0))
        ctx.mark_non_differentiable(*outs[3:])
        return outs

    @staticmethod
    def backward(ctx, g_l1, g_ssim, g_dl1, *_):
        fA, fB, dA, dB, K, R, t, sampled, occ, err, dpw, stats = ctx.saved_tensors
        ssim, C1, C2 = ctx.cfg
        N, _, H, W = fA.shape
        dev = fA.device
        lib = L.lib()
        nb = lib.sde_rgbd_num_blocks(N, H, W)
        use_ssim = bool(ssim) and g_ssim is not None
        coef = torch.empty(N, 3, H, W, 4, device=dev) if use_ssim else None
        d_depth, d_t, dR = torch.empty_like(dA), torch.empty_like(t), torch.empty(N, 3, 3, device=dev)
        pp = torch.empty(nb, 9, device=dev)
        g = [None if v is None else _f32c(v) for v in (g_l1, g_ssim if use_ssim else None, g_dl1)]
        d = _rgbd_desc(fA, fB, dA, dB, K, R, t, ssim, C1, C2)
        L.check(lib.sde_rgbd_bwd(ctypes.byref(d), L.ptr(sampled), L.ptr(occ), L.ptr(err), L.ptr(dpw), L.ptr(stats), L.ptr(g[0]), L.ptr(g[1]), L.ptr(g[2]), 1.0,
                                 L.ptr(coef), L.ptr(d_depth), L.ptr(d_t), L.ptr(pp), L.ptr(dR), L.stream()), "sde_rgbd_bwd")
        return d_depth, dR, d_t, None, None, None, None, None, None, None


def rgbd_consistency(frame_A, frame_B, depth_A, depth_B, K, R, t, ssim=True, C1=float("inf"), C2=9e-6):
    """Per-sample sums of the RGB-D consistency loss: dict(rgb_l1 [N], ssim [N], depth_l1 [N] (already divided by the normalizer), coords_A_in_B,
    occlusion_mask, depth_proximity_weight (None without the SSIM term)).  Gradients reach depth_A, R and t only."""
    o = _Rgbd.apply(depth_A, R, t, frame_A, frame_B, depth_B, K, bool(ssim), float(C1), float(C2))
    return {"rgb_l1": o[0], "ssim": o[1], "depth_l1": o[2], "coords_A_in_B": o[3], "occlusion_mask": o[4], "depth_proximity_weight": o[5] if ssim else None}


class _WeightedSSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, w, C1, C2):
        x, y, w = _f32c(x), _f32c(y), _f32c(w)
        if x.shape != y.shape or x.dim() != 4:
            raise L.SdeHipError(f"WeightedSSIM: x and y must be [B,C,H,W] of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
        N, C, H, W = x.shape
        _shape(w, (N, 1, H, W), "w")
        out, avg_w = torch.empty_like(x), torch.empty_like(w)
        L.check(L.lib().sde_wssim_fwd(L.ptr(x), L.ptr(y), L.ptr(w), N, C, H, W, C1, C2, L.ptr(out), L.ptr(avg_w), L.stream()), "sde_wssim_fwd")
        ctx.save_for_backward(x, y, w)
        ctx.cfg = (C1, C2)
        ctx.mark_non_differentiable(avg_w)
        return out, avg_w

    @staticmethod
    def backward(ctx, gout, _gavg):
        x, y, w = ctx.saved_tensors
        C1, C2 = ctx.cfg
        N, C, H, W = x.shape
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dy = torch.empty_like(y) if ctx.needs_input_grad[1] else None
        if dx is None and dy is None:
            return None, None, None, None, None
        coef = torch.empty(N, C, H, W, 4, device=x.device)
        L.check(L.lib().sde_wssim_bwd(L.ptr(x), L.ptr(y), L.ptr(w), L.ptr(_f32c(gout)), N, C, H, W, C1, C2, L.ptr(coef), L.ptr(dx), L.ptr(dy), L.stream()),
                "sde_wssim_bwd")
        return dx, dy, None, None, None


def weighted_ssim(x, y, w, C1=1e-4, C2=9e-4):
    """ssim_loss.py:L56-111: (clamp((1 - SSIM_w(x, y)) / 2, 0, 1) [B,C,H,W], avg_w [B,1,H,W]).  w is a constant (the model detaches it)."""
    if w.requires_grad:
        raise L.SdeHipError("WeightedSSIM: the weight is a constant on this path (detach it)")
    return _WeightedSSIM.apply(x, y, w, float(C1), float(C2))


class _MotionConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, R1, R2, tA, tB, grid, mask):
        R1, R2, tA, tB, grid, mask = (_f32c(v) for v in (R1, R2, tA, tB, grid, mask))
        N, _, H, W = tA.shape
        _shape(tA, (N, 3, H, W), "t_A2B"); _shape(tB, (N, 3, H, W), "t_B2A"); _shape(grid, (N, H, W, 2), "coords_A_in_B"); _shape(mask, (N, 1, H, W), "mask")
        _shape(R1, (N, 3, 3), "R_A2B"); _shape(R2, (N, 3, 3), "R_B2A")
        lib = L.lib()
        part = torch.empty(lib.sde_rgbd_num_blocks(N, H, W), device=tA.device)
        out = torch.empty(2, device=tA.device)
        L.check(lib.sde_motion_consistency_fwd(L.ptr(grid), L.ptr(mask), L.ptr(R1), L.ptr(R2), L.ptr(tA), L.ptr(tB), N, H, W, L.ptr(part), L.ptr(out), L.stream()),
                "sde_motion_consistency_fwd")
        ctx.save_for_backward(R1, R2, tA, tB, grid, mask)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_rot, g_trans):
        R1, R2, tA, tB, grid, mask = ctx.saved_tensors
        N, _, H, W = tA.shape
        dev = tA.device
        lib = L.lib()
        d_tA, d_tB = torch.empty_like(tA), torch.zeros_like(tB)
        dR1, dR2 = torch.empty_like(R1), torch.empty_like(R2)
        pp = torch.empty(lib.sde_rgbd_num_blocks(N, H, W), 9, device=dev)
        g_rot = None if g_rot is None else _f32c(g_rot)
        g_trans = None if g_trans is None else _f32c(g_trans)
        L.check(lib.sde_motion_consistency_bwd(L.ptr(grid), L.ptr(mask), L.ptr(R1), L.ptr(R2), L.ptr(tA), L.ptr(tB), L.ptr(g_rot), L.ptr(g_trans), N, H, W,
                                               L.ptr(d_tA), L.ptr(d_tB), L.ptr(pp), L.ptr(dR1), L.ptr(dR2), L.stream()), "sde_motion_consistency_bwd")
        return dR1, dR2, d_tA, d_tB, None, None


def motion_consistency(coords_A_in_B, mask, R_A2B, R_B2A, t_A2B, t_B2A):
    """motion_loss.py:L7-48 -> (rot_error, trans_error); the grid and the mask are constants."""
    return _MotionConsistency.apply(R_A2B, R_B2A, t_A2B, t_B2A, coords_A_in_B.detach(), mask.detach())


class _MotionSmooth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f):
        f = _f32c(f)
        B, C, H, W = f.shape
        lib = L.lib()
        part = torch.empty(lib.sde_motion_smooth_num_blocks(B * C, H, W), device=f.device)
        out = torch.empty((), device=f.device)
        L.check(lib.sde_motion_smooth_fwd(L.ptr(f), B * C, H, W, L.ptr(part), L.ptr(out), L.ptr(L.ticket(f.device)), L.stream()), "sde_motion_smooth_fwd")
        ctx.save_for_backward(f)
        return out

    @staticmethod
    def backward(ctx, gout):
        (f,) = ctx.saved_tensors
        B, C, H, W = f.shape
        df = torch.empty_like(f)
        L.check(L.lib().sde_motion_smooth_bwd(L.ptr(f), L.ptr(_f32c(gout)), B * C, H, W, L.ptr(df), L.stream()), "sde_motion_smooth_bwd")
        return df


def motion_smoothness(motion_field):
    """motion_loss.py:L51-55."""
    return _MotionSmooth.apply(motion_field)


class _MotionSparsity(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f):
        f = _f32c(f)
        B, C, H, W = f.shape
        mean, part = torch.empty(B * C, device=f.device), torch.empty(B * C, device=f.device)
        out = torch.empty((), device=f.device)
        L.check(L.lib().sde_motion_sparsity_fwd(L.ptr(f), B * C, H * W, L.ptr(mean), L.ptr(part), L.ptr(out), L.ptr(L.ticket(f.device)), L.stream()),
                "sde_motion_sparsity_fwd")
        ctx.save_for_backward(f, mean)
        return out

    @staticmethod
    def backward(ctx, gout):
        f, mean = ctx.saved_tensors
        B, C, H, W = f.shape
        df = torch.empty_like(f)
        L.check(L.lib().sde_motion_sparsity_bwd(L.ptr(f), L.ptr(mean), L.ptr(_f32c(gout)), B * C, H * W, L.ptr(df), L.stream()), "sde_motion_sparsity_bwd")
        return df


def motion_sparsity(motion_map):
    """motion_loss.py:L58-64 (the per-plane mean is a constant, as in the reference)."""
    return _MotionSparsity.apply(motion_map)


class _AvgPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, h, w):
        image = _f32c(image)
        B, C, H, W = image.shape
        out = torch.empty(B, C, h, w, device=image.device)
        L.check(L.lib().sde_avgpool_fwd(L.ptr(image), L.ptr(out), B * C, H, W, h, w, L.stream()), "sde_avgpool_fwd")
        ctx.shape = (B, C, H, W)
        return out

    @staticmethod
    def backward(ctx, gout):
        B, C, H, W = ctx.shape
        h, w = gout.shape[-2:]
        din = torch.empty(B, C, H, W, device=gout.device)
        L.check(L.lib().sde_avgpool_bwd(L.ptr(_f32c(gout)), L.ptr(din), B * C, H, W, h, w, L.stream()), "sde_avgpool_bwd")
        return din, None, None


def avgpool(image, size):
    """camera.py:L49-54 resize_img_avgpool = F.adaptive_avg_pool2d; the image itself when the sizes match."""
    h, w = int(size[-2]), int(size[-1])
    if image.shape[-2] == h and image.shape[-1] == w:
        _f32c(image)
        return image
    return _AvgPool.apply(image, h, w)


class _PairPrep(torch.autograd.Function):
    """sde_motion_prep_fwd / _bwd: (depth_r, depth_n or empty, t, m_norm or empty, t_sw, depth_n_sw, overall)."""

    @staticmethod
    def forward(ctx, depth, motion, t_pose, mask01, h, w, normalize):
        depth, t_pose = _f32c(depth), _f32c(t_pose)
        N, _, H0, W0 = depth.shape
        _shape(depth, (N, 1, H0, W0), "depth"); _shape(t_pose, (N, 3), "t_pose")
        if motion is not None:
            motion = _f32c(motion)
            _shape(motion, (N, 3, H0, W0), "motion")
        if mask01 is not None:
            if motion is None:
                raise L.SdeHipError("pair_prep: a mask without a motion field")
            mask01 = _f32c(mask01)
            _shape(mask01, (N, 1, H0, W0), "mask01")
        if N % 2 or not (0 < h <= H0 and 0 < w <= W0):
            raise L.SdeHipError(f"pair_prep: N must be even (both directions stacked) and the target no larger than the input, got N={N} {H0}x{W0} -> {h}x{w}")
        dev = depth.device
        lib = L.lib()
        e = lambda *s: torch.empty(*s, device=dev)
        depth_r, t, t_sw, dn_sw = e(N, 1, h, w), e(N, 3, h, w), e(N, 3, h, w), e(N, 1, h, w)
        depth_n, overall = (e(N, 1, h, w), e(N, 3, h, w)) if normalize else (None, None)
        m_norm = e(N, 3, h, w) if motion is not None else None
        partial, stats = e(lib.sde_rgbd_num_blocks(N, h, w), 2), e(2 + 4 * N)
        L.check(lib.sde_motion_prep_fwd(L.ptr(depth), L.ptr(motion), L.ptr(t_pose), L.ptr(mask01), N, H0, W0, h, w, int(normalize), L.ptr(depth_r), L.ptr(depth_n),
                                        L.ptr(t), L.ptr(overall), L.ptr(m_norm), L.ptr(dn_sw), L.ptr(t_sw), L.ptr(partial), L.ptr(stats), L.ptr(L.ticket(dev)),
                                        L.stream()), "sde_motion_prep_fwd")
        ctx.save_for_backward(mask01, depth_n, t, m_norm, stats)
        ctx.cfg = (N, H0, W0, h, w, bool(normalize))
        ctx.set_materialize_grads(False)          # an output no loss term reads sends None, not a zero map
        outs = (depth_r, depth_n if normalize else e(0), t, m_norm if m_norm is not None else e(0), t_sw, dn_sw, overall if normalize else e(0))
        ctx.mark_non_differentiable(dn_sw, outs[6], *([] if normalize else [outs[1]]), *([] if m_norm is not None else [outs[3]]))
        return outs

    @staticmethod
    def backward(ctx, g_dr, g_dn, g_t, g_mn, g_tsw, *_):
        mask01, depth_n, t, m_norm, stats = ctx.saved_tensors
        N, H0, W0, h, w, normalize = ctx.cfg
        dev = t.device
        lib = L.lib()
        if not normalize:
            g_dn = None
        if m_norm is None:
            g_mn = None
        g = [None if v is None else _f32c(v) for v in (g_dr, g_dn, g_t, g_tsw, g_mn)]
        e = lambda *s: torch.empty(*s, device=dev)
        d_depth, d_tpose = e(N, 1, H0, W0), e(N, 3)
        d_motion = e(N, 3, H0, W0) if m_norm is not None else None
        partial, bstats = e(lib.sde_rgbd_num_blocks(N, h, w), 9), e(1 + 10 * N)
        L.check(lib.sde_motion_prep_bwd(L.ptr(mask01), L.ptr(depth_n), L.ptr(t), L.ptr(m_norm), L.ptr(stats), L.ptr(g[0]), L.ptr(g[1]), L.ptr(g[2]), L.ptr(g[3]),
                                        L.ptr(g[4]), N, H0, W0, h, w, int(normalize), L.ptr(partial), L.ptr(bstats), L.ptr(L.ticket(dev)), L.ptr(d_depth),
                                        L.ptr(d_motion), L.ptr(d_tpose), L.stream()), "sde_motion_prep_bwd")
        return d_depth, d_motion, d_tpose, None, None, None, None


def pair_prep(depth, motion, t_pose, mask01, size, scale_normalize=False):
    """The per-scale glue of MotionLearningModel (MotionLearning.py:L126-166, L205-208) for both directions stacked along the batch (N = 2B: first half
    frame 1 -> 2, second half 2 -> 1): dict(depth_r, depth_n (depth_r itself when not normalising), t, m_norm (None without motion), overall_motion (t before
    the division by the depth mean, no gradient), and t_sw / depth_n_sw: t and depth_n with the halves of the batch exchanged, i.e. t_B2A of motion
    consistency (its gradient flows back into t) and depth_B of the stacked RGB-D call (no gradient, as depth_B has none)).
    Gradients reach depth, motion (times the mask) and t_pose; mask01 is a constant 0/1 map, already dilated."""
    if mask01 is not None and mask01.requires_grad:
        raise L.SdeHipError("pair_prep: the mask is a constant")
    o = _PairPrep.apply(depth, motion, t_pose, mask01, int(size[-2]), int(size[-1]), bool(scale_normalize))
    return {"depth_r": o[0], "depth_n": o[1] if scale_normalize else o[0], "t": o[2], "m_norm": o[3] if motion is not None else None, "t_sw": o[4],
            "depth_n_sw": o[5], "overall_motion": o[6] if scale_normalize else o[2].detach()}


def dilate_mask(mask, d):
    """F.max_pool2d((mask > 0).float(), 2d + 1, stride=1, padding=d) of a [N,1,H,W] map as a 0/1 float map (MotionLearning.py:L109-114); no gradient.
    d = 0 is the threshold alone."""
    d = int(d)
    if d <= 0:
        return (mask > 0).float()
    mask = _f32c(mask.detach().float())
    N, C, H, W = mask.shape
    tmp, out = torch.empty_like(mask), torch.empty_like(mask)
    L.check(L.lib().sde_mask_dilate(L.ptr(mask), L.ptr(tmp), L.ptr(out), N * C, H, W, d, L.stream()), "sde_mask_dilate")
    return out

"""Autograd wrappers over the photometric-path entry points of libsde_hip.so (include/sde_hip.h).

Each Function owns the tensors its backward needs; kernels never allocate.  Everything is enqueued on
torch's current stream and never synchronises (hipGraph-capture safe).
"""
import ctypes

import torch

from . import lib as L


def _f32c(t):
    if t.dtype != torch.float32:
        raise L.SdeHipError(f"expected float32 tensor, got {t.dtype}")
    return t.contiguous()


def resize(image, size, mode="bilinear"):
    """camera.py:L40-46 resize_img (no autograd: only images / ground truth are resized on this path)."""
    image = _f32c(image)
    B, C, H, W = image.shape
    h, w = int(size[0]), int(size[1])
    if (H, W) == (h, w):
        return image
    out = torch.empty(B, C, h, w, device=image.device, dtype=torch.float32)
    L.check(L.lib().sde_resize(L.ptr(image), L.ptr(out), B * C, H, W, h, w, 0 if mode == "bilinear" else 1, L.stream()), "sde_resize")
    return out


def view_synthesis_raw(image_B, depth_A, K, pose, sx=1.0, sy=1.0, want_indices=True):
    """camera.py:L166-202 forward only.  Returns dict(sampled, Z, grid, valid, fx, fy)."""
    image_B, depth_A, K, pose = _f32c(image_B), _f32c(depth_A), _f32c(K), _f32c(pose)
    B, C, H, W = image_B.shape
    dev = image_B.device
    out = {"sampled": torch.empty(B, C, H, W, device=dev), "Z": torch.empty(B, 1, H, W, device=dev),
           "grid": torch.empty(B, H, W, 2, device=dev), "valid": torch.empty(B, 1, H, W, device=dev, dtype=torch.uint8)}
    if want_indices:
        out["fx"] = torch.empty(B, H, W, device=dev, dtype=torch.int32)
        out["fy"] = torch.empty(B, H, W, device=dev, dtype=torch.int32)
    L.check(L.lib().sde_view_synthesis(L.ptr(image_B), L.ptr(depth_A), L.ptr(K), L.ptr(pose), sx, sy, B, C, H, W, L.ptr(out["sampled"]),
                                       L.ptr(out["Z"]), L.ptr(out["grid"]), L.ptr(out["valid"]), L.ptr(out.get("fx")), L.ptr(out.get("fy")),
                                       L.stream()), "sde_view_synthesis")
    return out


class _PoseVec2Mat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vec):
        vec = _f32c(vec)
        n = vec.shape[0]
        mat = torch.empty(n, 4, 4, device=vec.device)
        L.check(L.lib().sde_pose_vec2mat(L.ptr(vec), L.ptr(mat), n, L.stream()), "sde_pose_vec2mat")
        ctx.save_for_backward(vec)
        return mat

    @staticmethod
    def backward(ctx, dmat):
        (vec,) = ctx.saved_tensors
        dvec = torch.empty_like(vec)
        L.check(L.lib().sde_pose_vec2mat_bwd(L.ptr(vec), L.ptr(_f32c(dmat)), L.ptr(dvec), vec.shape[0], L.stream()), "sde_pose_vec2mat_bwd")
        return dvec


def pose_vec2mat(vec):
    """pose_utils.py:L130-137."""
    return _PoseVec2Mat.apply(vec)


def _desc(d, A, ctxs, poses, depth, K, sx, sy, ssim_w, C1, C2, automask, reduce_mean, clip_thr=None):
    d.clip_thr = clip_thr.data_ptr() if clip_thr is not None else 0
    B, _, h, w = depth.shape
    d.A = A.data_ptr(); d.depth = depth.data_ptr(); d.K = K.data_ptr()
    for j, (c, p) in enumerate(zip(ctxs, poses)):
        d.ctx[j] = c.data_ptr(); d.pose[j] = p.data_ptr()
    d.B, d.h, d.w, d.nctx = B, h, w, len(ctxs)
    d.automask, d.reduce_mean = int(bool(automask)), int(bool(reduce_mean))
    d.sx, d.sy, d.ssim_w, d.C1, d.C2 = sx, sy, ssim_w, C1, C2


PH_MAX_SCALES = 4     # PH_MAX_SCALES of csrc/photometric.hip


class _PackedScales:
    """n scales of the photometric term marshalled for the sde_photo_* / sde_mono_loss_* entries: the PhotoDesc array and the per-scale pointer arrays
    (sampled [n][MAX_CTX], sel [n], ...); the single-scale entries take the same arrays with n = 1.  Forward (saved is None) allocates what backward
    re-reads (sampled, sels) and the partial slabs; backward is given saved = (sampled, sels) and allocates d_depths, the pose partials and d_pose.
    depths / As: per scale, ctxs: scale-major, scales[s] = (sx, sy), cfg = (ssim_w, C1, C2, automask, reduce_mean)."""

    def __init__(self, K, depths, As, ctxs, poses, scales, cfg, clip_thr=None, saved=None):
        n, nctx = len(depths), len(poses)
        B, dev, lib = depths[0].shape[0], K.device, L.lib()
        arr = lambda: (ctypes.c_void_p * n)()
        forward = saved is None
        self.n = n
        self.descs = (L.PhotoDesc * n)()
        self.samp_arr, self.sel_arr = (ctypes.c_void_p * (n * L.MAX_CTX))(), arr()
        if forward:
            self.sampled, self.sels, self.partials, self.part_arr = [], [], [], arr()
        else:
            self.sampled, self.sels = saved
            self.d_depths, self.pps, self.dd_arr, self.pp_arr = [], [], arr(), arr()
        pixels = 0
        for s in range(n):
            _, _, h, w = depths[s].shape
            _desc(self.descs[s], As[s], ctxs[s * nctx:(s + 1) * nctx], poses, depths[s], K, *scales[s], *cfg, clip_thr)
            if forward:
                self.sampled += [torch.empty(B, 3, h, w, device=dev) for _ in range(nctx)]
                self.sels.append(torch.empty(B, h, w, device=dev, dtype=torch.uint8))
                self.partials.append(torch.empty(lib.sde_photo_num_blocks(B, h, w, 0), device=dev)); self.part_arr[s] = self.partials[-1].data_ptr()
            else:
                self.d_depths.append(torch.empty_like(depths[s])); self.dd_arr[s] = self.d_depths[-1].data_ptr()
                self.pps.append(torch.empty(lib.sde_photo_num_blocks(B, h, w, 1) * nctx * 12, device=dev)); self.pp_arr[s] = self.pps[-1].data_ptr()
            for j in range(nctx):
                self.samp_arr[s * L.MAX_CTX + j] = self.sampled[s * nctx + j].data_ptr()
            self.sel_arr[s] = self.sels[s].data_ptr()
            pixels += B * h * w
        if not forward:
            self.d_pose = [torch.empty(B, 4, 4, device=dev) for _ in range(nctx)]
        # algorithmic bytes per pixel, fp32.  Forward: target 12 + contexts 12 each + depth 4; backward: target 12 + (context 12 +
        # saved warped frame 12) per context + depth 4 + arg-min 1 + d_depth 4
        self.nbytes = pixels * ((16 + 12 * nctx) if forward else (21 + 24 * nctx))
        self.meta = dict(B=B, h=depths[0].shape[-2], w=depths[0].shape[-1])

    @staticmethod
    def unpack(t, n, nctx):
        """(K, depths, As, ctxs, poses, sampled, sels, rest) of tensors saved as (K, *depths, *As, *ctxs, *poses, *sampled, *sels, *rest)."""
        out, o = [t[0]], 1
        for k in (n, n, n * nctx, nctx, n * nctx, n):
            out.append(t[o:o + k]); o += k
        return (*out, t[o:])

    def backward_with_pose_handover(self, pose_stream, launch):
        """launch(d_pose) enqueues the backward kernel on the current stream; d_pose is None when the pose partials are summed on pose_stream instead."""
        # PoseNet on the auxiliary stream (MonoDepth2Model.forward): the pose side of this backward -- summing the partials -- goes there as well, and is
        # enqueued BEFORE the main stream's next kernel.  Besides taking a launch off the main chain this shapes the captured graph: the HIP runtime gives
        # a node's first captured dependant the node's own queue and the later ones the next queues round robin, and with the pose chain as the SECOND
        # dependant it landed on the queue of the depth network's data-gradient chain and ran after it (in-graph markers, profiles/README.md round 3)
        # (pose_stream is the caller's statement that every consumer of the pose gradients runs on that stream)
        aux = pose_stream if L.PROFILE is None else None
        L.timed("photo_bwd", self.nbytes, len(self.d_pose), lambda: launch(None if aux is not None else L.ptr_array(self.d_pose)), dict(self.meta, scales=self.n))
        if aux is not None:
            aux.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(aux):
                L.check(L.lib().sde_photo_multi_pose_finalize(self.descs, self.n, self.pp_arr, L.ptr_array(self.d_pose), L.stream()), "sde_photo_multi_pose_finalize")
            for t_ in self.pps + self.d_pose:
                t_.record_stream(aux)


class _PhotoScale(torch.autograd.Function):
    """One scale of MonoDepth2's photometric loss (MonoDepth2.py:L78-101,L116-124): returns mean(reduced map)."""

    @staticmethod
    def forward(ctx, depth, K, A, sx, sy, ssim_w, C1, C2, automask, reduce_mean, clip, nctx, *rest):
        ctxs, poses = rest[:nctx], rest[nctx:]
        depth, K, A = _f32c(depth), _f32c(K), _f32c(A)
        ctxs = [_f32c(c) for c in ctxs]
        poses = [_f32c(p) for p in poses]
        thr = None
        if clip > 0.0:
            # LOSS.CLIP (MonoDepth2.py:L147-149): every map is clamped at mean + clip * std of ITSELF; one extra forward yields the unclipped
            # maps, the per-map statistics stay on the device (the reference converts them to a python float: same fp32 value, no gradient)
            maps = photometric_maps(depth, K, A, ctxs, poses, sx, sy, ssim_w, C1, C2, automask, "mean" if reduce_mean else "min")["maps"]
            thr = (maps.mean((0, 2, 3)) + clip * maps.std((0, 2, 3))).contiguous()
        cfg = (ssim_w, C1, C2, automask, reduce_mean)
        p = _PackedScales(K, [depth], [A], ctxs, poses, [(sx, sy)], cfg, thr)
        loss = torch.empty((), device=depth.device)
        L.timed("photo_fwd", p.nbytes, nctx,
                lambda: L.check(L.lib().sde_photo_fwd(p.descs, p.samp_arr, L.ptr(p.sels[0]), None, L.ptr(p.partials[0]), L.ptr(loss), 1.0, 0, L.stream()),
                                "sde_photo_fwd"), dict(p.meta, moved=depth.numel() * (16 + 24 * nctx + 1)))
        ctx.save_for_backward(K, depth, A, *ctxs, *poses, *p.sampled, *p.sels)
        ctx.cfg = (cfg, (sx, sy), nctx)
        ctx.thr = thr
        return loss

    @staticmethod
    def backward(ctx, gout):
        cfg, scale, nctx = ctx.cfg
        K, depths, As, ctxs, poses, sampled, sels, _ = _PackedScales.unpack(ctx.saved_tensors, 1, nctx)
        p = _PackedScales(K, depths, As, ctxs, poses, [scale], cfg, ctx.thr, saved=(sampled, sels))
        gout = _f32c(gout)
        L.timed("photo_bwd", p.nbytes, nctx,
                lambda: L.check(L.lib().sde_photo_bwd(p.descs, p.samp_arr, L.ptr(sels[0]), L.ptr(gout), 1.0, L.ptr(p.d_depths[0]), 0, L.ptr(p.pps[0]),
                                                      L.ptr_array(p.d_pose), 0, L.stream()), "sde_photo_bwd"), p.meta)
        return (p.d_depths[0], None, None, None, None, None, None, None, None, None, None, None) + (None,) * nctx + tuple(p.d_pose)


def photometric_scale_loss(depth, K, A, ctxs, poses, sx, sy, ssim_w=0.85, C1=1e-4, C2=9e-4, automask=True, reduce="min", clip=0.0):
    if reduce not in ("min", "mean"):
        raise NotImplementedError(reduce)           # MonoDepth2.py:L121-122
    return _PhotoScale.apply(depth, K, A, float(sx), float(sy), float(ssim_w), float(C1), float(C2), bool(automask), reduce == "mean",
                             float(clip), len(ctxs), *ctxs, *poses)


def _split_scales(rest, n, nctx):
    """(depths, As, ctxs scale-major, poses) of an autograd argument tail, as contiguous fp32 tensors."""
    rest = [_f32c(t) for t in rest]
    return rest[:n], rest[n:2 * n], rest[2 * n:2 * n + n * nctx], rest[2 * n + n * nctx:]


class _PhotoMulti(torch.autograd.Function):
    """Every scale of MonoDepth2's photometric loss (MonoDepth2.py:L78-112) in one launch per phase: returns the [n] per-scale means."""

    @staticmethod
    def forward(ctx, K, ssim_w, C1, C2, automask, reduce_mean, n, nctx, scales, pose_stream, *rest):
        K = _f32c(K)
        depths, As, ctxs, poses = _split_scales(rest, n, nctx)
        cfg = (ssim_w, C1, C2, automask, reduce_mean)
        p = _PackedScales(K, depths, As, ctxs, poses, scales, cfg)
        loss = torch.empty(n, device=K.device)
        L.timed("photo_fwd", p.nbytes, nctx, lambda: L.check(L.lib().sde_photo_multi_fwd(p.descs, n, p.samp_arr, p.sel_arr, p.part_arr, L.ptr(loss), L.stream()),
                                                             "sde_photo_multi_fwd"), dict(p.meta, scales=n))
        ctx.save_for_backward(K, *depths, *As, *ctxs, *poses, *p.sampled, *p.sels)
        ctx.cfg = (cfg, n, nctx, scales)
        ctx.pose_stream = pose_stream
        return loss

    @staticmethod
    def backward(ctx, gout):
        cfg, n, nctx, scales = ctx.cfg
        K, depths, As, ctxs, poses, sampled, sels, _ = _PackedScales.unpack(ctx.saved_tensors, n, nctx)
        p = _PackedScales(K, depths, As, ctxs, poses, scales, cfg, saved=(sampled, sels))
        gout = _f32c(gout)
        p.backward_with_pose_handover(ctx.pose_stream, lambda d_pose: L.check(
            L.lib().sde_photo_multi_bwd(p.descs, n, p.samp_arr, p.sel_arr, L.ptr(gout), p.dd_arr, p.pp_arr, d_pose, L.stream()), "sde_photo_multi_bwd"))
        return (None,) * 10 + tuple(p.d_depths) + (None,) * n + (None,) * (n * nctx) + tuple(p.d_pose)


def photometric_multi_loss(depths, K, As, ctxs_per_scale, poses, scales, ssim_w=0.85, C1=1e-4, C2=9e-4, automask=True, reduce="min", pose_stream=None):
    """All scales in one launch per phase.  depths / As: per scale; ctxs_per_scale[s]: the context frames at scale s; scales[s] = (w_s / W, h_s / H).
    Returns a [n] tensor: photometric_scale_loss of every scale (no LOSS.CLIP: that option keeps the per-scale path).
    pose_stream: the stream the network that produced `poses` ran on when that is not the current one (its backward runs there): the pose gradients
    are then summed on that stream."""
    if reduce not in ("min", "mean"):
        raise NotImplementedError(reduce)
    n, nctx = len(depths), len(poses)
    if not (1 <= n <= PH_MAX_SCALES and len(As) == n and len(ctxs_per_scale) == n and all(len(c) == nctx for c in ctxs_per_scale)):
        raise L.SdeHipError("photometric_multi_loss: 1-4 scales, one target and nctx context frames per scale")
    flat_ctx = [c for cs in ctxs_per_scale for c in cs]
    return _PhotoMulti.apply(K, float(ssim_w), float(C1), float(C2), bool(automask), reduce == "mean", n, nctx, tuple((float(a), float(b)) for a, b in scales),
                             pose_stream, *depths, *As, *flat_ctx, *poses)


_ticket = L.ticket      # the finalize kernel's arrival counter (the name the tests read it by)


class _MonoLoss(torch.autograd.Function):
    """Photometric + smoothness terms of every scale (MonoDepth2.py:L78-126): (rec_loss, smooth_loss, per-scale values [2n]) in four launches forward and
    two backward; the depth gradient of a scale is written once (photometric) and accumulated once (smoothness) instead of being summed by autograd."""

    @staticmethod
    def forward(ctx, K, ssim_w, C1, C2, automask, reduce_mean, n, nctx, scales, photo_w, smooth_w, pose_stream, *rest):
        K = _f32c(K)
        depths, As, ctxs, poses = _split_scales(rest, n, nctx)
        dev = K.device
        lib = L.lib()
        cfg = (ssim_w, C1, C2, automask, reduce_mean)
        p = _PackedScales(K, depths, As, ctxs, poses, scales, cfg)
        sm, loss_parts = [], []        # loss_parts: workspaces the launch below writes; they must stay allocated until it is enqueued
        arr = lambda: (ctypes.c_void_p * n)()
        mean_arr, dn_arr, lp_arr, sp_arr = arr(), arr(), arr(), arr()
        if smooth_w is not None:
            for s, d in enumerate(depths):
                B, _, h, w = d.shape
                nb = lib.sde_smooth_num_blocks(B, h, w)
                mean_part, dn, loss_part, s_part = torch.empty(B * 32, device=dev), torch.empty(B, h, w, device=dev), torch.empty(nb, device=dev), torch.empty(nb, device=dev)
                sm += [mean_part, dn, s_part]; loss_parts.append(loss_part)
                mean_arr[s], dn_arr[s], lp_arr[s], sp_arr[s] = mean_part.data_ptr(), dn.data_ptr(), loss_part.data_ptr(), s_part.data_ptr()
        per_scale = torch.empty(2 * n, device=dev)
        totals = torch.empty(2, device=dev)
        pw = (ctypes.c_float * n)(*photo_w)
        sw = (ctypes.c_float * n)(*smooth_w) if smooth_w is not None else None
        L.timed("photo_fwd", p.nbytes, nctx, lambda: L.check(lib.sde_mono_loss_fwd(p.descs, n, pw, sw, p.samp_arr, p.sel_arr, p.part_arr, mean_arr, dn_arr, lp_arr, sp_arr,
                                                                                   L.ptr(per_scale), L.ptr(totals), L.ptr(L.ticket(dev)), L.stream()), "sde_mono_loss_fwd"),
                dict(p.meta, scales=n))
        ctx.save_for_backward(K, *depths, *As, *ctxs, *poses, *p.sampled, *p.sels, *sm)
        ctx.cfg = (cfg, n, nctx, scales, photo_w, smooth_w)
        ctx.pose_stream = pose_stream
        ctx.mark_non_differentiable(per_scale)
        return totals[0], totals[1], per_scale

    @staticmethod
    def backward(ctx, g_rec, g_smooth, _g_per_scale):
        cfg, n, nctx, scales, photo_w, smooth_w = ctx.cfg
        K, depths, As, ctxs, poses, sampled, sels, sm = _PackedScales.unpack(ctx.saved_tensors, n, nctx)
        dev = K.device
        lib = L.lib()
        p = _PackedScales(K, depths, As, ctxs, poses, scales, cfg, saved=(sampled, sels))
        if g_rec is None:                       # rec_loss not part of the objective: its gradient is zero
            g_rec = torch.zeros((), device=dev)
        g_rec = _f32c(g_rec)
        g_smooth = _f32c(g_smooth) if (g_smooth is not None and smooth_w is not None) else None
        pw = (ctypes.c_float * n)(*photo_w)
        p.backward_with_pose_handover(ctx.pose_stream, lambda d_pose: L.check(
            lib.sde_mono_loss_bwd(p.descs, n, pw, None, p.samp_arr, p.sel_arr, L.ptr(g_rec), None, None, None, None, p.dd_arr, p.pp_arr, d_pose, L.stream()),
            "sde_mono_loss_bwd"))
        if g_smooth is not None:
            sw = (ctypes.c_float * n)(*smooth_w)
            mean_arr, dn_arr, sp_arr = ((ctypes.c_void_p * n)(*[sm[3 * s + k].data_ptr() for s in range(n)]) for k in range(3))
            L.check(lib.sde_smooth_multi_bwd(p.descs, n, sw, L.ptr(g_smooth), mean_arr, dn_arr, sp_arr, p.dd_arr, 1, L.stream()), "sde_smooth_multi_bwd")
        return (None,) * 12 + tuple(p.d_depths) + (None,) * n + (None,) * (n * nctx) + tuple(p.d_pose)


def mono_loss(depths, K, As, ctxs_per_scale, poses, scales, photo_w, smooth_w=None, ssim_w=0.85, C1=1e-4, C2=9e-4, automask=True, reduce="min", pose_stream=None):
    """MonoDepth2's loss loop over the scales (MonoDepth2.py:L78-126), photometric and smoothness terms: returns (rec_loss, smooth_loss, per_scale) with
    rec_loss = sum_s photo_w[s] * photometric_scale_loss(scale s), smooth_loss = sum_s smooth_w[s] * smoothness_loss(scale s) (zero without smooth_w) and
    per_scale [2n] the unweighted terms (no gradient).  Arguments as for photometric_multi_loss."""
    if reduce not in ("min", "mean"):
        raise NotImplementedError(reduce)
    n, nctx = len(depths), len(poses)
    if not (1 <= n <= PH_MAX_SCALES and len(As) == n and len(ctxs_per_scale) == n and all(len(c) == nctx for c in ctxs_per_scale) and len(photo_w) == n
            and (smooth_w is None or len(smooth_w) == n)):
        raise L.SdeHipError("mono_loss: 1-4 scales, one target, nctx context frames and one weight per scale")
    flat_ctx = [c for cs in ctxs_per_scale for c in cs]
    return _MonoLoss.apply(K, float(ssim_w), float(C1), float(C2), bool(automask), reduce == "mean", n, nctx, tuple((float(a), float(b)) for a, b in scales),
                           tuple(float(v) for v in photo_w), None if smooth_w is None else tuple(float(v) for v in smooth_w), pose_stream,
                           *depths, *As, *flat_ctx, *poses)


def photometric_maps(depth, K, A, ctxs, poses, sx, sy, ssim_w=0.85, C1=1e-4, C2=9e-4, automask=True, reduce="min"):
    """Forward only, exposing the individual maps / sampled frames / arg-min (tests, debugging)."""
    depth, K, A = _f32c(depth), _f32c(K), _f32c(A)
    ctxs = [_f32c(c) for c in ctxs]; poses = [_f32c(p) for p in poses]
    B, _, h, w = depth.shape
    p = _PackedScales(K, [depth], [A], ctxs, poses, [(sx, sy)], (ssim_w, C1, C2, automask, reduce == "mean"))
    maps = torch.empty(B, 2 * len(ctxs) if automask else len(ctxs), h, w, device=depth.device)
    loss = torch.empty((), device=depth.device)
    L.check(L.lib().sde_photo_fwd(p.descs, p.samp_arr, L.ptr(p.sels[0]), L.ptr(maps), L.ptr(p.partials[0]), L.ptr(loss), 1.0, 0, L.stream()), "sde_photo_fwd")
    return {"loss": loss, "maps": maps, "sampled": p.sampled, "sel": p.sels[0]}


class _Smooth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, image):
        depth, image = _f32c(depth), _f32c(image)
        B, _, h, w = depth.shape
        dev = depth.device
        lib = L.lib()
        nb = lib.sde_smooth_num_blocks(B, h, w)
        mean_part = torch.empty(B * 32, device=dev)
        dn = torch.empty(B, h, w, device=dev)
        loss_part = torch.empty(nb, device=dev)
        s_part = torch.empty(nb, device=dev)
        loss = torch.empty((), device=dev)
        L.check(lib.sde_smooth_fwd(L.ptr(depth), L.ptr(image), B, h, w, L.ptr(mean_part), L.ptr(dn), L.ptr(loss_part), L.ptr(s_part), L.ptr(loss),
                                   1.0, 0, L.stream()), "sde_smooth_fwd")
        ctx.save_for_backward(depth, dn, mean_part, s_part)
        return loss

    @staticmethod
    def backward(ctx, gout):
        depth, dn, mean_part, s_part = ctx.saved_tensors
        B, _, h, w = depth.shape
        d_depth = torch.empty_like(depth)
        L.check(L.lib().sde_smooth_bwd(L.ptr(depth), L.ptr(dn), L.ptr(mean_part), L.ptr(s_part), L.ptr(_f32c(gout)), 1.0, B, h, w, L.ptr(d_depth),
                                       0, L.stream()), "sde_smooth_bwd")
        return d_depth, None


def smoothness_loss(depth, image):
    """smoothness_loss.py:L42-80."""
    return _Smooth.apply(depth, image)


class _SSIMMap(torch.autograd.Function):
    """The stand-alone SSIM distance map (ssim_loss.py:L34-53) with gradients to both images."""

    @staticmethod
    def forward(ctx, x, y, C1, C2):
        x, y = _f32c(x), _f32c(y)
        if x.shape != y.shape or x.dim() != 4:
            raise L.SdeHipError(f"SSIM: x and y must be [B,C,H,W] of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
        B, C, H, W = x.shape
        out = torch.empty_like(x)
        L.check(L.lib().sde_ssim_fwd(L.ptr(x), L.ptr(y), B, C, H, W, C1, C2, L.ptr(out), L.stream()), "sde_ssim_fwd")
        ctx.save_for_backward(x, y)
        ctx.cfg = (C1, C2)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, y = ctx.saved_tensors
        B, C, H, W = x.shape
        C1, C2 = ctx.cfg
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dy = torch.empty_like(y) if ctx.needs_input_grad[1] else None
        if dx is None and dy is None:
            return None, None, None, None
        ws = torch.empty(B * C * H * W, 4, device=x.device)
        L.check(L.lib().sde_ssim_bwd(L.ptr(x), L.ptr(y), L.ptr(_f32c(gout)), B, C, H, W, C1, C2, L.ptr(ws), L.ptr(dx), L.ptr(dy), L.stream()), "sde_ssim_bwd")
        return dx, dy, None, None


def ssim_map(x, y, C1=1e-4, C2=9e-4):
    """clamp((1 - SSIM(x, y)) / 2, 0, 1) per pixel and channel, [B,C,H,W] fp32 (ssim_loss.py:L34-53)."""
    return _SSIMMap.apply(x, y, float(C1), float(C2))


class _Silog(torch.autograd.Function):
    @staticmethod
    def forward(ctx, est, gt, vf):
        est, gt = _f32c(est), _f32c(gt)
        B, _, h, w = est.shape
        H, W = gt.shape[-2:]
        dev = est.device
        lib = L.lib()
        part = torch.empty(lib.sde_silog_num_blocks(B, h, w) * 3, device=dev)
        stats = torch.empty(4, device=dev)
        L.check(lib.sde_silog_fwd(L.ptr(est), L.ptr(gt), B, h, w, H, W, vf, L.ptr(part), L.ptr(stats), L.stream()), "sde_silog_fwd")
        ctx.save_for_backward(est, gt, stats)
        ctx.vf = vf
        return stats[3].clone()

    @staticmethod
    def backward(ctx, gout):
        est, gt, stats = ctx.saved_tensors
        B, _, h, w = est.shape
        H, W = gt.shape[-2:]
        d_est = torch.empty_like(est)
        L.check(L.lib().sde_silog_bwd(L.ptr(est), L.ptr(gt), L.ptr(stats), L.ptr(_f32c(gout)), 1.0, ctx.vf, B, h, w, H, W, L.ptr(d_est), 0,
                                      L.stream()), "sde_silog_bwd")
        return d_est, None, None


class _SilogMulti(torch.autograd.Function):
    """sum_k weights[k] * SILog(ests[k], nearest(gt)) over the prediction scales: one forward launch + one finalize, one backward launch."""

    @staticmethod
    def forward(ctx, gt, vf, weights, *ests):
        ests = [_f32c(e) for e in ests]
        gt = _f32c(gt)
        n, B = len(ests), ests[0].shape[0]
        H, W = gt.shape[-2:]
        dev = gt.device
        lib = L.lib()
        hs = (ctypes.c_int * n)(*[e.shape[-2] for e in ests])
        ws = (ctypes.c_int * n)(*[e.shape[-1] for e in ests])
        wt = (ctypes.c_float * n)(*[float(x) for x in weights])
        ep = (ctypes.c_void_p * n)(*[e.data_ptr() for e in ests])
        part = torch.empty(lib.sde_silog_multi_num_blocks(B, hs, ws, n) * 3, device=dev)
        stats = torch.empty(n, 4, device=dev)
        total = torch.empty((), device=dev)
        L.check(lib.sde_silog_multi_fwd(ep, L.ptr(gt), B, hs, ws, wt, n, H, W, vf, L.ptr(part), L.ptr(stats), L.ptr(total), L.stream()), "sde_silog_multi_fwd")
        ctx.save_for_backward(gt, stats, *ests)
        ctx.cfg = (vf, tuple(float(x) for x in weights))
        return total

    @staticmethod
    def backward(ctx, gout):
        gt, stats, *ests = ctx.saved_tensors
        vf, weights = ctx.cfg
        n, B = len(ests), ests[0].shape[0]
        H, W = gt.shape[-2:]
        d = [torch.empty_like(e) for e in ests]
        hs = (ctypes.c_int * n)(*[e.shape[-2] for e in ests])
        ws = (ctypes.c_int * n)(*[e.shape[-1] for e in ests])
        wt = (ctypes.c_float * n)(*weights)
        ep = (ctypes.c_void_p * n)(*[e.data_ptr() for e in ests])
        dp = (ctypes.c_void_p * n)(*[x.data_ptr() for x in d])
        L.check(L.lib().sde_silog_multi_bwd(ep, L.ptr(gt), L.ptr(stats), L.ptr(_f32c(gout)), 1.0, vf, B, hs, ws, wt, n, H, W, dp, L.stream()), "sde_silog_multi_bwd")
        return (None, None, None) + tuple(d)


MAX_SILOG_SCALES = 4


def silog_loss_multi(depth_ests, depth_gt_full, variance_focus, weights):
    """sum_k weights[k] * silog_loss(depth_ests[k], depth_gt_full) (Supervised.py:L42-47) in one launch per phase."""
    if not 1 <= len(depth_ests) <= MAX_SILOG_SCALES or len(weights) != len(depth_ests):
        raise L.SdeHipError(f"silog_loss_multi: 1..{MAX_SILOG_SCALES} scales with one weight each, got {len(depth_ests)} / {len(weights)}")
    return _SilogMulti.apply(depth_gt_full, float(variance_focus), tuple(weights), *depth_ests)


def silog_loss(depth_est, depth_gt_full, variance_focus=0.85):
    """losses.py:L10-13 applied to (pred, resize_img(gt, pred.shape, 'nearest')) -- Supervised.py:L44-45 -- in one kernel."""
    return _Silog.apply(depth_est, depth_gt_full, float(variance_focus))

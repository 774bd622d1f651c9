"""Loader for the C-ABI library declared in include/sde_hip.h.

The product path has NO fallback: if libsde_hip.so is missing or a call fails, this raises.
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_int32, c_size_t, c_void_p

import torch

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("SDE_HIP_LIB", os.path.join(_HERE, "libsde_hip.so"))   # override: A/B builds of the same ABI
MAX_CTX = 4
F32, BF16, F16 = 0, 1, 2


class SdeHipError(RuntimeError):
    pass


class PhotoDesc(Structure):
    _fields_ = [("A", c_void_p), ("ctx", c_void_p * MAX_CTX), ("pose", c_void_p * MAX_CTX), ("depth", c_void_p), ("K", c_void_p),
                ("B", c_int32), ("h", c_int32), ("w", c_int32), ("nctx", c_int32), ("automask", c_int32), ("reduce_mean", c_int32),
                ("sx", c_float), ("sy", c_float), ("ssim_w", c_float), ("C1", c_float), ("C2", c_float), ("clip_thr", c_void_p)]


class RgbdDesc(Structure):
    _fields_ = [("frame_A", c_void_p), ("frame_B", c_void_p), ("depth_A", c_void_p), ("depth_B", c_void_p), ("K", c_void_p), ("R", c_void_p), ("t", c_void_p),
                ("N", c_int32), ("H", c_int32), ("W", c_int32), ("ssim", c_int32), ("C1", c_float), ("C2", c_float)]


_P, _I, _F = c_void_p, c_int, c_float
_PROTOS = {
    "sde_version": ([], c_int),
    "sde_mark_time": ([_P, _P], c_int),
    "sde_wall_clock_khz": ([], c_int),
    "sde_store_u64": ([_P, ctypes.c_uint64, _P], c_int),
    "sde_resize": ([_P, _P, _I, _I, _I, _I, _I, _I, _P], c_int),
    "sde_pose_vec2mat": ([_P, _P, _I, _P], c_int),
    "sde_pose_vec2mat_bwd": ([_P, _P, _P, _I, _P], c_int),
    "sde_view_synthesis": ([_P, _P, _P, _P, _F, _F, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P], c_int),
    "sde_photo_num_blocks": ([_I, _I, _I, _I], c_int),
    "sde_photo_fwd": ([POINTER(PhotoDesc), POINTER(c_void_p), _P, _P, _P, _P, _F, _I, _P], c_int),
    "sde_photo_bwd": ([POINTER(PhotoDesc), POINTER(c_void_p), _P, _P, _F, _P, _I, _P, POINTER(c_void_p), _I, _P], c_int),
    "sde_photo_multi_fwd": ([_P, _I, _P, _P, _P, _P, _P], c_int),
    "sde_photo_multi_bwd": ([_P, _I, _P, _P, _P, _P, _P, _P, _P], c_int),
    "sde_photo_multi_pose_finalize": ([_P, _I, _P, _P, _P], c_int),
    "sde_mono_loss_fwd": ([_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P], c_int),
    "sde_mono_loss_bwd": ([_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P], c_int),
    "sde_smooth_multi_bwd": ([_P, _I, _P, _P, _P, _P, _P, _P, _I, _P], c_int),
    "sde_ssim_fwd": ([_P, _P, _I, _I, _I, _I, _F, _F, _P, _P], c_int),
    "sde_ssim_bwd": ([_P, _P, _P, _I, _I, _I, _I, _F, _F, _P, _P, _P, _P], c_int),
    "sde_smooth_num_blocks": ([_I, _I, _I], c_int),
    "sde_smooth_fwd": ([_P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _F, _I, _P], c_int),
    "sde_smooth_bwd": ([_P, _P, _P, _P, _P, _F, _I, _I, _I, _P, _I, _P], c_int),
    "sde_silog_num_blocks": ([_I, _I, _I], c_int),
    "sde_silog_fwd": ([_P, _P, _I, _I, _I, _I, _I, _F, _P, _P, _P], c_int),
    "sde_silog_bwd": ([_P, _P, _P, _P, _F, _F, _I, _I, _I, _I, _I, _P, _I, _P], c_int),
    "sde_silog_multi_num_blocks": ([_I, _P, _P, _I], c_int),
    "sde_silog_multi_fwd": ([_P, _P, _I, _P, _P, _P, _I, _I, _I, _F, _P, _P, _P, _P], c_int),
    "sde_silog_multi_bwd": ([_P, _P, _P, _P, _F, _F, _I, _P, _P, _P, _I, _I, _I, _P, _P], c_int),
    # BTS decoder operators (csrc/bts.hip; autograd wrappers in hip/bts.py)
    "sde_dilate_split": ([_P, _I, _I, _I, _I, _I, _I, _P, _P], c_int),
    "sde_dilate_merge": ([_P, _I, _I, _I, _I, _I, _I, _P, _P], c_int),
    "sde_upsample2_fwd": ([_P, _I, _I, _I, _I, _I, _P, _P], c_int),
    "sde_upsample2_bwd": ([_P, _I, _I, _I, _I, _I, _P, _P], c_int),
    "sde_cat_fwd": ([_P, _I, ctypes.c_long, _I, _I, _P, _P], c_int),
    "sde_cat_bwd": ([_P, ctypes.c_long, _I, _I, _P, _I, _P], c_int),
    "sde_channel_stats_tiles": ([ctypes.c_long], c_int),
    "sde_channel_stats": ([_P, ctypes.c_long, _I, _I, _P, _P], c_int),
    "sde_relu_fwd": ([_P, ctypes.c_long, _I, _P, _P], c_int),
    "sde_lpg_fwd": ([_P, _I, _I, _I, _I, _I, _F, _I, _I, _P, _P, _P], c_int),
    "sde_lpg_bwd": ([_P, _P, _P, _I, _I, _I, _I, _I, _F, _I, _I, _P, _P], c_int),
    "sde_sigmoid_head_fwd": ([_P, _I, _I, _I, _I, _F, _P, _F, _I, _I, _P, _P], c_int),
    "sde_sigmoid_head_bwd": ([_P, _P, _I, _I, _I, _I, _F, _P, _F, _I, _I, _P, _P], c_int),
    # GoogleResNet operators (csrc/google.hip; autograd wrappers in hip/google.py)
    "sde_randln_chunks": ([_I], c_int),
    "sde_randln_fwd": ([_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _I, _I, _P, _P, _P, _P], c_int),
    "sde_randln_bwd": ([_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P, _P], c_int),
    "sde_bilinear2_fwd": ([_P, _I, _I, _I, _I, _I, _P, _P], c_int),
    "sde_bilinear2_bwd": ([_P, _I, _I, _I, _I, _I, _P, _P], c_int),
    "sde_softplus_head_fwd": ([_P, _I, _I, _I, _I, _I, _I, _P, _P], c_int),
    "sde_softplus_head_bwd": ([_P, _P, _I, _I, _I, _I, _I, _I, _P, _P], c_int),
    # GoogleResNetv2's transposed convolution (csrc/deconv.hip; autograd wrapper in hip/nn.py)
    "sde_deconv3x3s2_fwd": ([_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P], c_int),
    # grouped 3x3 convolution of the ResNeXt bottleneck (csrc/gconv.hip; autograd wrapper in hip/nn.py)
    "sde_gconv3x3_stats_rows": ([_I, _I, _I, _I, _I, _I, _I], c_int),
    "sde_gconv3x3_fwd": ([_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P], c_int),
    "sde_gconv3x3_dgrad": ([_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P], c_int),
    "sde_gconv3x3_wgrad_ws_bytes": ([_I, _I, _I, _I, _I, _I, _I], c_size_t),
    "sde_gconv3x3_wgrad": ([_P, _P, _I, _I, _I, _I, _I, _I, _I, _P, c_size_t, _P, _I, _P], c_int),
    # DenseNet dense blocks without the concatenation (csrc/dense.hip; autograd wrappers in hip/dense.py)
    "sde_dense_stats": ([_P, _I, _I, ctypes.c_long, _P, _I, _P], c_int),
    "sde_dense_bwd_rows": ([ctypes.c_long, _I, _I], c_int),
    "sde_dense_bn_relu_fwd": ([_P, ctypes.c_long, _I, _P, _P, _P, _P, _P, _F, _F, _P, _P, _P], c_int),
    "sde_dense_bn_relu_bwd": ([_P, ctypes.c_long, _I, _P, _P, _P, _P, _P, _I, _P, _P], c_int),
    "sde_dense_grad_gather": ([_P, ctypes.c_long, _I, _I, _I, _P, _P, _P], c_int),
    "sde_avgpool2x2_fwd": ([_P, _I, _I, _I, _I, _I, _P, _P], c_int),
    "sde_avgpool2x2_bwd": ([_P, _I, _I, _I, _I, _I, _P, _P], c_int),
    # GoogleMotionNet / GooglePoseNet operators (csrc/motion.hip; autograd wrappers in hip/motion.py)
    "sde_motion_resize_cat_fwd": ([_P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P], c_int),
    "sde_motion_resize_cat_bwd": ([_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P], c_int),
    "sde_motion_tail_fwd": ([_P, _P, _P, _P, ctypes.c_long, _I, _I, _I, _P, _P], c_int),
    "sde_motion_tail_blocks": ([ctypes.c_long, _I, _I], c_int),
    "sde_motion_tail_bwd": ([_P, _P, _P, _P, ctypes.c_long, _I, _I, _I, _P, _P, _P, _P, _P], c_int),
    "sde_motion_head_blocks": ([ctypes.c_long], c_int),
    "sde_motion_head_fwd": ([_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P], c_int),
    "sde_motion_head_bwd": ([_P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P], c_int),
    "sde_prep_input_bwd": ([_P, _P, _I, _I, _I, _I, _I, _I, _P, _P], c_int),
    # MotionLearning loss stack (csrc/motion_loss.hip; autograd wrappers in hip/motion_loss.py)
    "sde_view_synthesis_pp": ([_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P], c_int),
    "sde_rgbd_num_blocks": ([_I, _I, _I], c_int),
    "sde_rgbd_fwd": ([POINTER(RgbdDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P], c_int),
    "sde_rgbd_bwd": ([POINTER(RgbdDesc), _P, _P, _P, _P, _P, _P, _P, _P, _F, _P, _P, _P, _P, _P, _P], c_int),
    "sde_wssim_fwd": ([_P, _P, _P, _I, _I, _I, _I, _F, _F, _P, _P, _P], c_int),
    "sde_wssim_bwd": ([_P, _P, _P, _P, _I, _I, _I, _I, _F, _F, _P, _P, _P, _P], c_int),
    "sde_motion_consistency_fwd": ([_P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P], c_int),
    "sde_motion_consistency_bwd": ([_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P], c_int),
    "sde_motion_smooth_num_blocks": ([_I, _I, _I], c_int),
    "sde_motion_smooth_fwd": ([_P, _I, _I, _I, _P, _P, _P, _P], c_int),
    "sde_motion_smooth_bwd": ([_P, _P, _I, _I, _I, _P, _P], c_int),
    "sde_motion_sparsity_fwd": ([_P, _I, ctypes.c_long, _P, _P, _P, _P, _P], c_int),
    "sde_motion_sparsity_bwd": ([_P, _P, _P, _I, ctypes.c_long, _P, _P], c_int),
    "sde_avgpool_fwd": ([_P, _P, _I, _I, _I, _I, _I, _P], c_int),
    "sde_avgpool_bwd": ([_P, _P, _I, _I, _I, _I, _I, _P], c_int),
    "sde_motion_prep_fwd": ([_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P], c_int),
    "sde_motion_prep_bwd": ([_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P], c_int),
    "sde_mask_dilate": ([_P, _P, _P, _I, _I, _I, _I, _P], c_int),
    # point clouds (csrc/cloud.hip; binding and autograd wrapper in hip/cloud.py)
    "sde_depth_cloud_capacity": ([_I, _I, _I], ctypes.c_long),
    "sde_depth_cloud_ws_bytes": ([_I, _I, _I, _I], c_size_t),
    "sde_depth_cloud": ([_P, _I, _I, _I, _P, _P, _I, _I, _P, _P, _F, _F, _I, _P, c_size_t, _P, _P, _P], c_int),
    "sde_img_to_points_num_blocks": ([_I, _I], c_int),
    "sde_img_to_points_fwd": ([_P, _P, _P, _I, _I, _I, _I, _P, _P], c_int),
    "sde_img_to_points_bwd": ([_P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P], c_int),
    # raw LiDAR scans -> sparse depth maps (csrc/lidar.hip; binding and host twin in hip/lidar.py)
    "sde_lidar_depth": ([_P, _I, _I, _P, _I, _P, _P, _I, _I, _I, _F, _P, _P], c_int),
    # optical flow from depth and relative pose (csrc/flow.hip; binding in hip/flow.py)
    "sde_pair_flow": ([_P, _I, _I, _I, _P, _P, _I, _I, _P, _P, _P, _P, _I, _F, _P, _P, _P, _P, _P], c_int),
    # temporally fused depth: forward warp, z-buffer, blend (csrc/temporal.hip; binding and host twin in hip/temporal.py)
    "sde_depth_warp_fuse": ([_P, _P, _P, _P, _P, _I, _I, _I, _F, _F, _P, _P, _P, _P, _P], c_int),
    # a sequence's depth fused into one TSDF volume (csrc/volume.hip; binding and host twins in hip/volume.py); origin is a host float[3]
    "sde_pose_compose": ([_P, _P, _P], c_int),
    "sde_tsdf_integrate": ([_P, _I, _I, _P, _P, _I, _I, _P, _P, _P, POINTER(c_float), _F, _F, _F, _F, _F, _P, _P, _P, _I, _I, _I, _P], c_int),
    "sde_tsdf_points_ws_bytes": ([_I, _I, _I], c_size_t),
    "sde_tsdf_points": ([_P, _P, _P, _I, _I, _I, POINTER(c_float), _F, _F, _P, c_size_t, _P, ctypes.c_long, _P, _P], c_int),
    "sde_tsdf_mesh_ws_bytes": ([_I, _I, _I], c_size_t),
    "sde_tsdf_mesh": ([_P, _P, _P, _I, _I, _I, POINTER(c_float), _F, _F, _P, c_size_t, _P, ctypes.c_long, _P, ctypes.c_long, _P, _P], c_int),
    "sde_tsdf_render": ([_P, _P, _P, _I, _I, _I, POINTER(c_float), _F, _F, _P, _P, _I, _I, _F, _F, _I, _P, _P, _P, _P], c_int),
    # frame-to-model alignment against the rendered volume (csrc/align.hip; binding and host twins in hip/align.py)
    "sde_frame_align_ws_bytes": ([_I, _I], c_size_t),
    "sde_frame_align_reset": ([_P, _P], c_int),
    "sde_frame_align": ([_P, _I, _I, _P, _P, _I, _I, _P, _P, _P, _F, _F, _F, _F, _I, _F, _I, _P, _P, c_size_t, _P], c_int),
}

_lib = None
PROFILE = None   # bench.py sets this to a list to collect (kind, flops, variant, start_event, end_event, meta, repeat) per GEMM launch
PROFILE_REPEAT = 1


def timed(kind, work, variant, call, meta=None):
    """Run `call` bracketed by events on the current stream when PROFILE is a list (bench.py's roofline pass).
    `work` = the launch's algorithmic FLOPs (GEMM kinds) or bytes (photo_* kinds)."""
    if PROFILE is None:
        return call()
    # An event pair around ONE launch also times the launch path itself (8-12 us on this stack: the per-kernel durations of a rocprofv3 trace of
    # the same step were that much shorter), so the idempotent GEMM launches are issued PROFILE_REPEAT times back to back between the two events
    # and the record carries the count: duration = elapsed / repeat (what remains on top of rocprofv3's figure is one kernel boundary, ~1.5 us).
    rep = PROFILE_REPEAT if (kind.startswith("igemm") or kind == "wgrad") else 1
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(rep):
        r = call()
    e1.record()
    PROFILE.append((kind, float(work), variant, e0, e1, meta, rep))
    return r


def register_protos(protos):
    """Other binding modules (conv, norm, ...) add their prototypes here before first use."""
    _PROTOS.update(protos)
    if _lib is not None:
        _bind(_lib, protos)


def _bind(L, protos):
    for name, (args, res) in protos.items():
        fn = getattr(L, name)   # AttributeError => the .so does not export what the header declares: fail loudly
        fn.argtypes = args
        fn.restype = res


def available():
    return os.path.exists(LIB_PATH)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SdeHipError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(make -C simpledepthestimation_amd/csrc). There is no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH)
        L.sde_last_error.restype = c_char_p
        _bind(L, _PROTOS)
        _lib = L
    return _lib


def check(rc, name):
    if rc != 0:
        raise SdeHipError(f"{name} failed ({rc}): {lib().sde_last_error().decode()}")


def ptr(t):
    """Device pointer of a contiguous CUDA tensor (None -> NULL)."""
    if t is None:
        return c_void_p(0)
    if not t.is_cuda:
        raise SdeHipError("simpledepthestimation_amd ops need CUDA (HIP) tensors; there is no CPU fallback")
    if not t.is_contiguous():
        raise SdeHipError("non-contiguous tensor passed to a HIP op")
    return c_void_p(t.data_ptr())


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


_TICKET = {}


def ticket(dev):
    """Arrival counter of the loss kernels whose last workgroup finishes the reduction (csrc/reduce.h: sde_arrive_last): one int per device, zero between
    launches (the last arriver resets it).  Every launch that is given it counts on this same int, so such launches must be ordered on ONE stream: two
    of them that overlap on different streams would see each other's arrivals.  The current users: the mono loss' finalize, motion smoothness and
    sparsity, and pair_prep's two finalize kernels."""
    if dev not in _TICKET:
        _TICKET[dev] = torch.zeros(1, dtype=torch.int32, device=dev)
    return _TICKET[dev]


_side = {}
# Weight-gradient GEMMs run on ONE side stream, forked in groups and joined late (hip/nn.py: WGradReducer, wgrad_group_rule).  The values below
# were each decided by an A/B run inside one gpurun call in round 1 (DESIGN.md 6.1 keeps the measurements); the environment switches that
# selected the losing variants (late join per phase, several side streams, packing on the side stream) were removed with those variants.
SIDE_STREAM = True      # hip.lib.SIDE_STREAM = False (bench.py --no-side-stream): single-stream backward (profiling, debugging)
JOIN_LAG = 1            # the main stream joins all but the newest JOIN_LAG - 1 groups before it forks the next one
WGRAD_GROUP = 6         # weight-gradient GEMMs of that many consecutive layers behind one fork
# The two constants are set per network family when a HipTrainer is built (apply_schedule), from A/B runs inside one gpurun call each:
#   round 1 (register-staged weight gradients): lag 0 / 1 / 2 / 3 -> 9.54 / 9.20 / 9.01 / 9.10, group 1 / 2 / 3 / 4 -> 9.22 / 8.85 / 8.84 / 8.91 ms/step;
#   round 2 (LDS-DMA / halo weight gradients, faster slab sums: the side queue got a third shorter), Supervised-R50: (lag, group) = (2, 3) 7.21,
#   (1, 3) 7.09, (1, 4) 7.10, (1, 5) 7.06, (1, 6) 6.98-7.00, (1, 7) 7.10, (1, 8) 7.00, (1, 10) 7.07, (0, 6) 6.98, (0, 8) 7.00, (2, 8) 7.13;
#   MonoDepth2-R18 5.48 -> 5.33, R50 8.98 -> 8.74 with (1, 6); PackNet-1A the other way: (2, 3) 53.8, (1, 3) 55.9, (1, 6) 56.0 ms/step.
#   FIRST_GROUP (layers in the first group of a phase; until it closes nothing runs next to the chain; it also shifts every later group boundary):
#   bottleneck ResNets 0 (= 6) 6.77 against 6.89-6.94 ms/step for 1 / 2 / 3 / 4 / 5 / 7 / 8 / 9 (Supervised-R50), MonoDepth2-R50 8.06 vs 8.09 at 3;
#   basic-block ResNets 3: Supervised-R18 3.50 -> 3.42, MonoDepth2-R18 4.69 -> 4.60 (2: 4.62, 4: 4.74, 5: 4.66).
SCHEDULES = {"resnet": (1, 6, 0), "resnet_basic": (1, 6, 3), "packnet": (2, 3, 0)}
# ... and the workgroup target of the weight-gradient GEMMs' pixel splits (SDE_OPT_WGRAD_BLOCKS).  Round 3, one call: ResNet-50 256 / 384 / 512 / 768 -> 6.37 / 6.45 /
# 6.50 / 6.64 ms/step; PackNet-1A (weight gradients over 1.47 M pixels with 64 ... 512 channels) 256 / 512 / 768 / 1024 / 1536 / 2048 / 4096 -> 50.7-51.4 / 48.8 /
# 48.4 / 47.9-48.0 / 48.1 / 48.6 / 50.5 (profiles/r03ah_packnet_sweep.txt)
WGRAD_BLOCKS = {"resnet": 256, "resnet_basic": 256, "packnet": 1024}
WGRAD_BLOCKS_LOCKED = False      # bench.py --opt 6=... pins the value for an A/B run
# LDS ring of the LDS-DMA weight-gradient launches that are forked beside the data-gradient chain (SDE_OPT_WGRAD_DMA_RING: 0 = 64 pixels x 3 stages, 72 KB;
# 1 = 32 x 4, 48 KB; 2 = 32 x 3, 36 KB), per schedule family: beside a 72 KB workgroup ONE workgroup of the persistent GEMM fits on a compute unit, beside a
# slim one two.  Same results bit for bit.  profiles/corun_lds_ab.txt, alternating runs in one call: ResNet-50 supervised 6.39 -> 6.30 (ring 1), 6.35 (ring 2),
# MonoDepth2-R50 7.24 -> 7.11 / 7.12 ms/step; PackNet (1024 weight-gradient workgroups per launch) keeps the wide ring (profiles/README.md item 46).
WGRAD_DMA_RINGS = {"resnet": 1, "resnet_basic": 0, "packnet": 0}
WGRAD_DMA_RING = -1              # >= 0 (bench.py --const WGRAD_DMA_RING=...): pins the ring for an A/B run; -1: the family's
_FAMILY = None                   # the family of the last HipTrainer built (apply_schedule); None: no trainer, ring 0
SCHEDULE_LOCKED = False  # bench.py --const JOIN_LAG=... / WGRAD_GROUP=... pins the values for an A/B run


def wgrad_dma_ring():
    """The ring for a weight-gradient GEMM that is forked beside a data gradient (hip/nn.py: WGradReducer._launch)."""
    return WGRAD_DMA_RING if WGRAD_DMA_RING >= 0 else WGRAD_DMA_RINGS.get(_FAMILY, 0)


def apply_schedule(family):
    global JOIN_LAG, WGRAD_GROUP, FIRST_GROUP, _FAMILY
    _FAMILY = family
    if not SCHEDULE_LOCKED:
        JOIN_LAG, WGRAD_GROUP, FIRST_GROUP = SCHEDULES[family]
FIRST_GROUP_B = None            # first-group digits of the SECOND phase of a two-phase (data-parallel) backward; None = FIRST_GROUP.  The group boundaries decide
                                # how much weight-gradient work is left behind the phase's last data-gradient layer (its exposed tail)
FIRST_GROUP = 0                 # sizes of the first groups of a backward phase as decimal digits (3: the first group has 3 layers; 33: the first two), 0: none;
                                # set per network family (SCHEDULES)
GROUP_MAX_BYTES = 128 << 20     # layers with more operand bytes fork alone (PackNet's 190 MB maps: 57.7 vs 60.2 ms/step)
GROUP_BUDGET_BYTES = 384 << 20  # ... and a group also closes once its layers' operands add up to this much
DEFER_MAX_BYTES = 2 << 20       # slab stacks up to this size join the phase's batched reduction; bigger ones are summed at once, cache-resident
FORK_MIN_BYTES = 0              # layers with fewer operand bytes keep their weight-gradient GEMM on the main stream (0: every layer forks; measured
                                # 10 / 25 / 50 / 100 MB -> 7.52 / 7.93 / 8.77 / 7.78 ms/step against 7.26-7.28 at 0: bench.py --const FORK_MIN_BYTES=...)


# HipTrainer's 16-bit twin of the flat parameter buffer (engine/trainer.py; profiles/twin_operands_ab.txt keeps the A/B runs):
TWIN_OPERANDS = 1       # 0: per-step full weight pack from fp32 + sde_adam_step, the route before the twin (bench.py --const TWIN_OPERANDS=0)
TWIN_PACK_FORK = 1      # 1: the twin's data-gradient transposes on the side stream under the forward pass, joined before backward; 0: head of the step.
                        # Supervised-R50, four alternating runs each: full pack 6.264, twin at the head 6.244, forked 6.215 ms/step (parent spread 0.013)


def side_stream():
    """Per-device helper stream: weight-gradient GEMMs run there concurrently with the data-gradient GEMM of the same layers (fork / join with
    stream / event waits, so they are captured into the step's hipGraph as a parallel branch)."""
    d = torch.cuda.current_device()
    if d not in _side:
        _side[d] = torch.cuda.Stream(device=d)
    return _side[d]


_aux = {}
# MonoDepth2: PoseNet (seven small layers, every kernel of it launch-bound at batch 12) runs on an auxiliary stream underneath the depth network's forward
# pass, and -- autograd replays a node's backward on the stream its forward ran on -- its backward underneath the depth network's backward.  HipTrainer
# switches this on for single-process training (the two-phase backward of the data-parallel path keeps one stream).
POSE_STREAM = False
AUX_USED = False        # set by the forward pass that forked the auxiliary stream; the trainer joins it after backward


def aux_stream():
    d = torch.cuda.current_device()
    if d not in _aux:
        _aux[d] = torch.cuda.Stream(device=d)
    return _aux[d]


def is_aux_stream(st):
    return any(st == a for a in _aux.values())


def join_aux():
    """Make the current stream wait for the auxiliary stream's work of this step (no-op when nothing was forked)."""
    global AUX_USED
    if AUX_USED:
        torch.cuda.current_stream().wait_stream(aux_stream())
        AUX_USED = False


# Timeline markers (bench.py --marks): mark(name) enqueues one sde_mark_time launch on the current stream; under graph capture it becomes a node of the
# step's graph, so every replay refreshes the slot.  MARKS is None unless a diagnostic run switched them on: mark() is then a no-op.
MARKS = None


def marks_enable(device):
    global MARKS
    MARKS = {"names": [], "slots": torch.zeros(128, dtype=torch.int64, device=device)}


def mark(name):
    if MARKS is None:
        return
    if name not in MARKS["names"]:
        MARKS["names"].append(name)
    i = MARKS["names"].index(name)
    check(lib().sde_mark_time(c_void_p(MARKS["slots"].data_ptr() + 8 * i), stream()), "sde_mark_time")


def marks_read(origin=None):
    """{name: microseconds since the `origin` marker (default: the earliest one)} of the last step's markers (synchronises)."""
    if MARKS is None:
        return {}
    torch.cuda.synchronize()
    khz = lib().sde_wall_clock_khz()
    t = MARKS["slots"][:len(MARKS["names"])].tolist()
    t0 = t[MARKS["names"].index(origin)] if origin in MARKS["names"] else min(t)
    return {n: (v - t0) * 1e3 / khz for n, v in zip(MARKS["names"], t)}


def ptr_array(tensors):
    arr = (c_void_p * MAX_CTX)()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr() if t is not None else 0
    return arr

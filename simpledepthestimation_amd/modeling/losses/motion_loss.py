"""The MotionLearning loss terms with the reference's names (detectron2/modeling/losses/motion_loss.py and the rgbd_consistency_loss method of
detectron2/modeling/meta_arch/MotionLearning.py:L248-291), computed by libsde_hip.so (csrc/motion_loss.hip)."""
from ...hip import motion_loss as HM


def motion_consistency_loss(coords_A_in_B, mask, R_A2B, R_B2A, t_A2B, t_B2A):
    """motion_loss.py:L7-48 -> (rot_error, trans_error).  Gradients reach the two rotations and the two translation fields; the one into t_B2A is a
    scatter through the bilinear taps (fp32 atomic adds: not bit-reproducible, like grid_sample's own backward)."""
    return HM.motion_consistency(coords_A_in_B, mask, R_A2B, R_B2A, t_A2B, t_B2A)


def motion_smoothness_loss_fn(motion_field, warp_around=False):
    """motion_loss.py:L51-55 (``warp_around`` is unused there as well)."""
    return HM.motion_smoothness(motion_field)


def motion_sparsity_loss_fn(motion_map):
    """motion_loss.py:L58-64."""
    return HM.motion_sparsity(motion_map)


def rgbd_consistency_loss(frame_A, frame_B, depth_A, depth_B, intrinsics, R_A2B, t_A2B, *, depth_l1_w, ssim_w, C1, C2):
    """MotionLearning.py:L248-291 as a free function: dict(coords_A_in_B, occlusion_mask, rgb_l1_loss, [depth_l1_loss], [ssim_loss,
    depth_proximity_weight]).  Samples are independent up to the final means, so both directions of a pair may be stacked along the batch.
    Gradients reach depth_A, R_A2B and t_A2B; frame_*, intrinsics and depth_B get none (sampled depth_B only enters through a comparison and
    detached terms)."""
    o = HM.rgbd_consistency(frame_A, frame_B, depth_A, depth_B, intrinsics, R_A2B, t_A2B, ssim=ssim_w > 0.0, C1=C1, C2=C2)
    N, _, H, W = frame_A.shape
    out = {"coords_A_in_B": o["coords_A_in_B"], "occlusion_mask": o["occlusion_mask"]}
    if depth_l1_w > 0:
        out["depth_l1_loss"] = o["depth_l1"].mean() * depth_l1_w
    out["rgb_l1_loss"] = o["rgb_l1"].sum() / (N * 3 * H * W)
    if ssim_w > 0.0:
        out["depth_proximity_weight"] = o["depth_proximity_weight"]
        out["ssim_loss"] = o["ssim"].sum() / (N * 3 * H * W) * ssim_w * 0.5
    return out

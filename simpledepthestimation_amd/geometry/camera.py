"""Camera geometry entry points with the reference's names (detectron2/geometry/camera.py), computed by libsde_hip.so."""
import torch

from ..hip import motion_loss as HM
from ..hip import photometric as HP


def scale_intrinsics(K, x_scale, y_scale):
    """camera.py:L14-22 (in place, like the reference).  The fused loss kernels take the scale factors instead."""
    K[..., 0, 0] *= x_scale
    K[..., 1, 1] *= y_scale
    K[..., 0, 2] *= x_scale
    K[..., 1, 2] *= y_scale
    return K


def resize_img(image, dst_size, mode="bilinear"):
    """camera.py:L40-46."""
    return HP.resize(image, dst_size, mode)


def resize_img_avgpool(image, dst_size):
    """camera.py:L49-54 (F.adaptive_avg_pool2d; the image itself when the sizes match)."""
    return HM.avgpool(image, dst_size)


def view_synthesis(image_B, depth_A, intrinsics, R_A_to_B, t_A_to_B):
    """camera.py:L166-202 -> (sampled_B, depth_in_B, grid, valid_mask).  t [B,3] or [B,3,1,1]: one translation per sample (sde_view_synthesis);
    t [B,3,H,W]: one per pixel (sde_view_synthesis_pp, the same projection with K @ t formed per pixel)."""
    B = image_B.shape[0]
    if t_A_to_B.dim() == 4 and t_A_to_B.shape[-2] * t_A_to_B.shape[-1] > 1:
        o = HM.view_synthesis_pp(image_B, depth_A, intrinsics, R_A_to_B, t_A_to_B)
        return o["sampled"], o["Z"], o["grid"], o["valid"].bool()
    t = t_A_to_B.reshape(B, 3)
    pose = torch.zeros(B, 4, 4, device=image_B.device, dtype=torch.float32)
    pose[:, :3, :3] = R_A_to_B
    pose[:, :3, 3] = t
    pose[:, 3, 3] = 1.0
    o = HP.view_synthesis_raw(image_B, depth_A, intrinsics, pose, 1.0, 1.0, want_indices=False)
    return o["sampled"], o["Z"], o["grid"], o["valid"].bool()

"""Camera geometry entry points with the reference's names (detectron2/geometry/camera.py), computed by libsde_hip.so."""
from functools import lru_cache

import numpy as np
import torch

from ..hip import cloud as HC
from ..hip import motion_loss as HM
from ..hip import photometric as HP


def scale_intrinsics(K, x_scale, y_scale):
    """camera.py:L14-22 (in place, like the reference).  The fused loss kernels take the scale factors instead."""
    K[..., 0, 0] *= x_scale
    K[..., 1, 1] *= y_scale
    K[..., 0, 2] *= x_scale
    K[..., 1, 2] *= y_scale
    return K


def inv_intrinsics(K):
    """K [B,3,3] -> the inverse of a pinhole matrix as a new tensor: 1/fx, 1/fy on the diagonal, (-1*cx)/fx, (-1*cy)/fy in the last column (that
    operation order: sde_depth_cloud and the recorded fixture share it).  Every other entry -- skew, last row -- is carried over unchanged."""
    assert K.dim() == 3, f"inv_intrinsics: K must be [B,3,3], got {tuple(K.shape)}"
    focal = K.diagonal(dim1=1, dim2=2)[:, :2]              # [B,2]: fx, fy
    centre = K[:, :2, 2]                                    # [B,2]: cx, cy
    out = K.clone()
    out.diagonal(dim1=1, dim2=2)[:, :2] = 1.0 / focal
    out[:, :2, 2] = (-1.0 * centre) / focal
    return out


@lru_cache(maxsize=None)
def _axes(H, W, dtype, device, normalized):
    """The column and row coordinates of an H x W image as 1-D tensors: 0 .. W-1 / 0 .. H-1, or both spread over [-1, 1]."""
    if normalized:
        return tuple(torch.linspace(-1.0, 1.0, n, dtype=dtype, device=device) for n in (W, H))
    return tuple(torch.arange(n, device=device).to(dtype) for n in (W, H))


def meshgrid(B, H, W, dtype, device, normalized=False):
    """-> (xs, ys), each [B,H,W] of `dtype` on `device`: every pixel's column and row coordinate (in [-1, 1] when normalized).  Plain torch; the
    tensors are the caller's own."""
    cols, rows = _axes(H, W, dtype, device, bool(normalized))
    return cols.view(1, 1, W).expand(B, H, W).contiguous(), rows.view(1, H, 1).expand(B, H, W).contiguous()


def image_grid(B, H, W, dtype, device, normalized=False):
    """-> grid [B,3,H,W]: channel 0 the column coordinate, channel 1 the row coordinate, channel 2 ones (homogeneous pixel coordinates)."""
    cols, rows = _axes(H, W, dtype, device, bool(normalized))
    grid = torch.ones((B, 3, H, W), dtype=dtype, device=device)
    grid[:, 0] = cols.view(1, 1, W)
    grid[:, 1] = rows.view(1, H, 1)
    return grid


def img_to_points(depth, R, t):
    """camera.py:L125-138: depth [B,1,H,W], R [B,3,3], t [B,3,1] or [B,3,H*W] -> points [B,3,H,W] = R (depth * image_grid) + t, one launch
    (sde_img_to_points_fwd), differentiable in depth, R and t.  The compacted, coloured cloud of a prediction is hip.cloud.depth_cloud."""
    return HC.img_to_points(depth, R, t)


def points_to_img(points, R, t):
    """camera.py:L141-163: points [B,3,H,W], R [B,3,3], t [B,3,1] or [B,3,H*W] -> (coords [B,H,W,2] = (X, Y) of R points + t divided by its
    depth + 1e-6, Z [B,H,W,1] = that depth clamped to >= 1e-5, valid [B,H,W,1] bool = X, Y finite, 0 <= X < W - 1, 0 <= Y < H - 1 and depth > 0).
    With R = K R_AB and t = K t_AB the coordinates are pixels of frame B.  Torch operators on any device and dtype, differentiable; the fused
    training path is view_synthesis, the fused inference path (depth and pose -> flow, validity, colours) is hip.flow.pair_flow."""
    if points.dim() != 4 or points.shape[1] != 3 or R.dim() != 3 or t.dim() != 3:
        raise ValueError(f"points_to_img: points [B,3,H,W], R [B,3,3], t [B,3,1 or H*W] expected, got {tuple(points.shape)}, {tuple(R.shape)}, {tuple(t.shape)}")
    B, _, H, W = points.shape
    proj = R.bmm(points.reshape(B, 3, -1)) + t
    depth = proj[:, 2]
    X = proj[:, 0] / (depth + 1e-6)
    Y = proj[:, 1] / (depth + 1e-6)
    valid = X.isfinite() & (X >= 0) & (X < W - 1) & Y.isfinite() & (Y >= 0) & (Y < H - 1) & (depth > 0)
    return torch.stack([X, Y], -1).view(B, H, W, 2), depth.clamp(min=1e-5).view(B, H, W, 1), valid.view(B, H, W, 1)


def velo_to_image(cam_calib, velo_calib, cam):
    """The scanner-to-image matrix of a KITTI raw date -> [3,4] float32: P_rect_0c @ R_rect_00 @ Tr_velo_to_cam, the `P_velo2im` of the published
    generate_depth_map.  cam_calib / velo_calib: the parsed calib_cam_to_cam.txt / calib_velo_to_cam.txt ({key: array}); cam: 'image_02', '02' or 2.
    The product is formed in float64 from the parsed values and rounded once.  The matrix is what hip.lidar.lidar_depth takes as `proj`."""
    c = str(cam)[-1]
    R = np.eye(4, dtype=np.float64)
    R[:3, :3] = np.asarray(cam_calib["R_rect_00"], dtype=np.float64).reshape(3, 3)
    T = np.eye(4, dtype=np.float64)
    T[:3, :3] = np.asarray(velo_calib["R"], dtype=np.float64).reshape(3, 3)
    T[:3, 3] = np.asarray(velo_calib["T"], dtype=np.float64).reshape(3)
    P = np.asarray(cam_calib[f"P_rect_0{c}"], dtype=np.float64).reshape(3, 4)
    return (P @ R @ T).astype(np.float32)


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

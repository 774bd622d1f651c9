"""Plain-torch restatement of the MotionLearning loss stack (view synthesis with a per-pixel translation, WeightedSSIM, the RGB-D consistency loss,
motion consistency / smoothness / sparsity, adaptive average pool), written from the formulas for tests and the benchmark's torch baseline.
Works in whatever dtype / device its inputs have (tests: float64 on the CPU; scripts/bench_motion_loss.py: float32 on the GPU)."""
import torch
import torch.nn.functional as F


def view_synthesis(image_B, depth_A, K, R, t):
    """t: [B,3,1,1] or [B,3,H,W] -> (sampled, depth_in_B [B,1,H,W], grid [B,H,W,2], valid [B,1,H,W] bool)."""
    B, _, H, W = depth_A.shape
    dt, dev = depth_A.dtype, depth_A.device
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt, device=dev), torch.arange(W, dtype=dt, device=dev), indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)], 0)[None] * depth_A                     # [B,3,H,W]
    Kinv = K.clone()
    Kinv[:, 0, 0] = 1.0 / K[:, 0, 0]; Kinv[:, 1, 1] = 1.0 / K[:, 1, 1]
    Kinv[:, 0, 2] = -K[:, 0, 2] / K[:, 0, 0]; Kinv[:, 1, 2] = -K[:, 1, 2] / K[:, 1, 1]
    pts = Kinv.bmm(pix.reshape(B, 3, -1))
    q = K.bmm(R).bmm(pts) + K.bmm(t.expand(B, 3, H, W).reshape(B, 3, -1))
    X, Y, Z = q[:, 0] / (q[:, 2] + 1e-6), q[:, 1] / (q[:, 2] + 1e-6), q[:, 2]
    valid = X.isfinite() & (X >= 0) & (X < W - 1) & Y.isfinite() & (Y >= 0) & (Y < H - 1) & (Z > 0)
    Z = Z.clamp(min=1e-5)
    Xs = 2 * X.nan_to_num().clamp(0, W - 1) / (W - 1) - 1.0
    Ys = 2 * Y.nan_to_num().clamp(0, H - 1) / (H - 1) - 1.0
    grid = torch.stack([Xs, Ys], -1).view(B, H, W, 2)
    sampled = F.grid_sample(image_B, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    return sampled, Z.view(B, 1, H, W), grid, valid.view(B, 1, H, W)


def weighted_ssim(x, y, w, C1, C2):
    pool = lambda v: F.avg_pool2d(F.pad(v, (1, 1, 1, 1), mode="reflect"), 3, 1)
    avg_w = F.avg_pool2d(w, 3, 1, 1)
    wp = w + 1e-2
    inv = 1.0 / (avg_w + 1e-2)
    wavg = lambda v: pool(v * wp) * inv
    mu_x, mu_y = wavg(x), wavg(y)
    sx, sy, sxy = wavg(x * x) - mu_x * mu_x, wavg(y * y) - mu_y * mu_y, wavg(x * y) - mu_x * mu_y
    if C1 == float("inf"):
        n, d = 2 * sxy + C2, sx + sy + C2
    elif C2 == float("inf"):
        n, d = 2 * mu_x * mu_y + C1, mu_x * mu_x + mu_y * mu_y + C1
    else:
        n, d = (2 * sxy + C2) * (2 * mu_x * mu_y + C1), (sx + sy + C2) * (mu_x * mu_x + mu_y * mu_y + C1)
    return torch.clamp((1.0 - n / d) / 2.0, 0.0, 1.0), avg_w


def rgbd_consistency_loss(frame_A, frame_B, depth_A, depth_B, K, R, t, depth_l1_w, ssim_w, C1, C2):
    out = {}
    sampled, Z, grid, valid = view_synthesis(torch.cat([frame_B, depth_B], 1), depth_A, K, R, t)
    sF, sD = sampled[:, :3], sampled[:, 3:]
    occ = (Z < sD).to(Z.dtype) * valid.to(Z.dtype)
    out["coords_A_in_B"], out["occlusion_mask"] = grid, occ
    nrm = occ.sum([1, 2, 3]) + 1
    if depth_l1_w > 0:
        out["depth_l1_loss"] = (((sD.detach() - Z).abs() * occ).sum([1, 2, 3]) / nrm).mean() * depth_l1_w
    out["rgb_l1_loss"] = ((sF - frame_A).abs() * occ).mean()
    if ssim_w > 0.0:
        err = (Z - sD) ** 2
        m2 = ((err * occ).sum([1, 2, 3]) / nrm + 1e-4).view(-1, 1, 1, 1)
        dpw = ((m2 / (err + m2)) * valid.to(Z.dtype)).detach()
        smap, avg_w = weighted_ssim(sF, frame_A, dpw, C1, C2)
        out["depth_proximity_weight"] = dpw
        out["ssim_loss"] = (smap * avg_w).mean() * ssim_w * 0.5
    return out


def motion_consistency_loss(coords, mask, R_A2B, R_B2A, t_A2B, t_B2A):
    B, _, H, W = t_A2B.shape
    s = F.grid_sample(t_B2A, coords.detach(), mode="bilinear", padding_mode="zeros", align_corners=True)
    eye = torch.eye(3, dtype=t_A2B.dtype, device=t_A2B.device)[None]
    e = torch.einsum("bij,bjhw->bihw", R_A2B, s) + t_A2B
    msq = lambda m: (m ** 2).mean(dim=[1, 2])
    rot = (msq(R_A2B @ R_B2A - eye) / (msq(R_A2B - eye) + msq(R_B2A - eye) + 1e-24)).mean()
    te = (e ** 2).sum(1) / ((t_A2B ** 2).sum(1) + (s ** 2).sum(1) + 1e-24)
    return rot, (mask[:, 0] * te).mean()


def motion_smoothness_loss_fn(f):
    gx = (f[:, :, :, 1:] - f[:, :, :, :-1])[:, :, 1:, :]
    gy = (f[:, :, 1:, :] - f[:, :, :-1, :])[:, :, :, 1:]
    return torch.sqrt(1e-24 + gx ** 2 + gy ** 2).mean()


def motion_sparsity_loss_fn(f):
    a = f.abs()
    m = a.mean([2, 3], keepdim=True).detach()
    return (2 * m * torch.sqrt(a / (m + 1e-24) + 1)).mean()


def resize_img_avgpool(image, size):
    if tuple(image.shape[-2:]) == tuple(size):
        return image
    return F.adaptive_avg_pool2d(image, size)

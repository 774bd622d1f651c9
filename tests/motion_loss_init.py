"""Deterministic inputs of the MotionLearning loss tests (tests/golden/motion_loss.npz is the reference's run on exactly these).

The recipe keeps the reference away from its decision boundaries (occlusion comparison, projection mask, bilinear cell edges): smooth frames, a depth
ramp of 8-42 m decreasing down the image, KITTI-like intrinsics, rotations below 0.01 rad, and a translation of about (0.05, -0.02, 0.6) plus a
Gaussian-blob motion field."""
import math

import torch

SIZES = {"small": (2, 32, 104), "full": (2, 128, 416)}
SSIM_CONSTS = [(float("inf"), 9e-6), (1e-4, float("inf"))]       # (C1, C2): the project's Base.yaml setting, and the other special branch
DEPTH_L1_WS = [0.0, 1.0]
SSIM_W = 3.0
# (size, C1, C2, depth_l1_w)
CASES = [(s, c1, c2, w) for s in ("small", "full") for (c1, c2) in SSIM_CONSTS for w in DEPTH_L1_WS]


def first_case(size):
    """Index of the first case of a size: the one whose golden entry carries the arrays that the settings do not change (coords, weight, g_t21)."""
    return next(i for i, c in enumerate(CASES) if c[0] == size)


FULL_ROWS = [0, 1, 37, 64, 126, 127]      # rows of the gradient maps kept for the 128 x 416 cases


def euler(a):
    """[N,3] angles (x, y, z) -> [N,3,3] = Rz Ry Rx."""
    cx, cy, cz, sx, sy, sz = a[:, 0].cos(), a[:, 1].cos(), a[:, 2].cos(), a[:, 0].sin(), a[:, 1].sin(), a[:, 2].sin()
    o, z = torch.ones_like(cx), torch.zeros_like(cx)
    Rx = torch.stack([o, z, z, z, cx, -sx, z, sx, cx], 1).view(-1, 3, 3)
    Ry = torch.stack([cy, z, sy, z, o, z, -sy, z, cy], 1).view(-1, 3, 3)
    Rz = torch.stack([cz, -sz, z, sz, cz, z, z, z, o], 1).view(-1, 3, 3)
    return Rz @ Ry @ Rx


def frames(g, N, H, W, phase):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32) / H, torch.arange(W, dtype=torch.float32) / W, indexing="ij")
    out = []
    for n in range(N):
        ch = [0.5 + 0.2 * torch.sin(2 * math.pi * ((1.5 + c) * xs + 0.3 * n + phase)) + 0.2 * torch.cos(2 * math.pi * ((1.0 + 0.5 * c) * ys + 0.7 * xs + phase))
              for c in range(3)]
        out.append(torch.stack(ch))
    return (torch.stack(out) + 0.05 * torch.rand(N, 3, H, W, generator=g)).clamp(0, 1)


def depth(g, N, H, W, phase):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32) / (H - 1), torch.arange(W, dtype=torch.float32) / W, indexing="ij")
    d = 42.0 - 34.0 * ys + 4.0 * torch.sin(2 * math.pi * (1.3 * xs + phase)) * (1 - ys)
    return (d[None, None].repeat(N, 1, 1, 1) + 0.2 * torch.randn(N, 1, H, W, generator=g)).clamp_min(1.0)


def intrinsics(N, H, W):
    K = torch.zeros(N, 3, 3)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 0.58 * W, 1.92 * H, 0.5 * W, 0.5 * H, 1.0
    return K


def motion_field(g, N, H, W, sign):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32) / H, torch.arange(W, dtype=torch.float32) / W, indexing="ij")
    base = sign * torch.tensor([0.05, -0.02, 0.6]).view(1, 3, 1, 1)
    t = base.repeat(N, 1, H, W)
    for n in range(N):
        cx, cy = 0.3 + 0.4 * torch.rand((), generator=g), 0.4 + 0.3 * torch.rand((), generator=g)
        blob = torch.exp(-(((xs - cx) / 0.12) ** 2 + ((ys - cy) / 0.2) ** 2))
        amp = 0.4 * (2 * torch.rand(3, generator=g) - 1)
        t[n] += amp.view(3, 1, 1) * blob
    return t + 0.01 * torch.randn(N, 3, H, W, generator=g)


def inputs(N, H, W, seed=0):
    """dict of float32 CPU tensors: frame1/2, depth1/2, K, R12/R21, t12/t21."""
    g = torch.Generator().manual_seed(1000 + seed)
    ang = 0.01 * (2 * torch.rand(N, 3, generator=g) - 1)
    return {"frame1": frames(g, N, H, W, 0.0), "frame2": frames(g, N, H, W, 0.013), "depth1": depth(g, N, H, W, 0.0), "depth2": depth(g, N, H, W, 0.02),
            "K": intrinsics(N, H, W), "R12": euler(ang), "R21": euler(-ang + 0.001 * (2 * torch.rand(N, 3, generator=g) - 1)),
            "t12": motion_field(g, N, H, W, 1.0), "t21": motion_field(g, N, H, W, -1.0)}


# ---------------------------------------------------------------------------------------------------------------------------------------
# running a case and comparing it with the golden file (shared by the CPU and the GPU test)
# ---------------------------------------------------------------------------------------------------------------------------------------
LOSSES = ("rgb_l1_loss", "ssim_loss", "depth_l1_loss", "rot_error", "trans_error")
GRADS = ("depth", "t12", "t21", "R12", "R21")
OUT_TOL, GRAD_TOL, D_FACTOR, MAX_OFF = 1e-4, 3e-3, 8.0, 1e-3


def run_stack(rgbd, mcl, inp, C1, C2, dl1_w, dtype, device):
    """frame 1 -> 2 RGB-D consistency + motion consistency on its coords / mask, objective = sum of the losses; rgbd(fA, fB, dA, dB, K, R, t, dl1_w, ssim_w, C1, C2)
    and mcl(coords, mask, R12, R21, t12, t21) are the implementation under test."""
    v = {k: x.detach().clone().to(device=device, dtype=dtype) for k, x in inp.items()}
    for k in ("depth1", "t12", "t21", "R12", "R21"):
        v[k].requires_grad_(True)
    o = dict(rgbd(v["frame1"], v["frame2"], v["depth1"], v["depth2"], v["K"], v["R12"], v["t12"], dl1_w, SSIM_W, C1, C2))
    o["rot_error"], o["trans_error"] = mcl(o["coords_A_in_B"], o["occlusion_mask"], v["R12"], v["R21"], v["t12"], v["t21"])
    sum(o[k] for k in LOSSES if k in o).backward()
    res = {k: o[k].detach() for k in LOSSES if k in o}
    res.update(coords=o["coords_A_in_B"].detach(), occ=o["occlusion_mask"].detach(), dpw=o["depth_proximity_weight"].detach())
    res.update({"g_" + k: v[n].grad for k, n in zip(GRADS, ("depth1", "t12", "t21", "R12", "R21"))})
    return res


def compare_with_golden(res, gold, ci, out_tol, grad_tol, exact):
    """Failures (strings) of a run_stack result against case ci of the golden file.  Bounds: max(out_tol or grad_tol, D_FACTOR * d) with d the reference's
    own fp32-vs-fp64 difference.  exact: every mask pixel and gradient element must agree; otherwise up to MAX_OFF of the mask pixels may differ and up
    to MAX_OFF of a gradient map's elements may be off by more than the bound (the norm of every gradient must be within it all the same)."""
    import numpy as np
    size = CASES[ci][0]
    N, H, W = SIZES[size]
    p, ps = f"case{ci}_", f"case{first_case(size)}_"
    rows = (lambda t, dim: t) if size == "small" else (lambda t, dim: t.index_select(dim, torch.tensor(FULL_ROWS)))
    dbl = lambda t: t.detach().double().cpu()
    bad = []

    def check(name, got, bound):
        print(f"  case {ci} {name}: {got:.3e} (bound {bound:.3e})")
        if not got <= bound:
            bad.append(f"{name}: {got:.3e} > {bound:.3e}")

    for k in LOSSES:
        if p + k in gold.files:
            ref = float(gold[p + k])
            check(k, abs(float(res[k]) - ref) / abs(ref), max(out_tol, D_FACTOR * float(gold[p + "d_" + k])))
    occ = torch.from_numpy(np.unpackbits(gold[ps + "occ"])[:N * H * W].reshape(N, 1, H, W).astype(np.float64))
    check("occlusion_mask flips", float((dbl(res["occ"]) != occ).double().mean()), 0.0 if exact else MAX_OFF)
    for k, dim in (("coords", 1), ("dpw", 2)):
        ref = torch.from_numpy(gold[ps + k]).double()
        check(k, float((rows(dbl(res[k]), dim) - ref).abs().max() / ref.abs().max()), max(out_tol, D_FACTOR * float(gold[p + "d_" + k])))
    for k in GRADS:
        g = dbl(res["g_" + k])
        tol = max(grad_tol, D_FACTOR * float(gold[p + "d_g_" + k]))
        ref = torch.from_numpy(gold[(ps if k == "t21" else p) + "g_" + k]).double()
        diff = ((rows(g, 2) if g.dim() == 4 else g) - ref).abs() / ref.abs().max()
        if exact or g.dim() != 4:
            check("g_" + k, float(diff.max()), tol)
        else:
            check("g_" + k + " elements off", float((diff > tol).double().mean()), MAX_OFF)
        ref_n = float(gold[p + "gn_" + k])
        check("|g_" + k + "|", abs(float(g.norm()) - ref_n) / ref_n, max(grad_tol, D_FACTOR * float(gold[p + "d_gn_" + k])))
    return bad

"""Bit-for-bit record of the loss kernels' reductions: every output and gradient of the loss operators, hashed, against tests/golden/loss_bits.json.

The JSON is written by scripts/record_loss_bits.py from this module's case table with a library of the same ABI (SDE_HIP_LIB); a refactor of the
reduce passes must reproduce it unchanged.  One SHA-256 per tensor, over the fp32 bytes of t + 0.0 (the sign of a zero is canonical).

Shapes: the smallest at which each reduce helper can go wrong, not the workload's.  The 64 x 4 pixel kernels have ceil(W / 64) * ceil(H / 4) workgroups per
sample: 10 x 70 -> 6 (ragged tiles both ways, fewer partials than lanes), 36 x 520 -> 81 (the 64-lane walks take a second, ragged trip), 348 x 130 -> 261 (so
do the 256-thread walks).  N = 2 throughout: the halves are swapped.  Every case runs twice in one process and must hash alike: the arrival ticket is
left at zero.  Inputs come from seeded CPU generators; upstream gradients are random, so that no sum is identically zero.
The one sum without a fixed order -- motion consistency's d t_B2A, an atomic scatter -- is left out.
"""
import hashlib
import json
import os

import pytest
import torch

import motion_loss_init as MI

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_bits.json")
SHAPES = [(10, 70), (36, 520), (348, 130)]
PHOTO_BASE = (128, 416)      # 4 scales down to 16 x 52: 165 backward workgroups per sample at the largest scale, 4 at the smallest (checked below)


def sha(t):
    return hashlib.sha256((t.detach().float().cpu() + 0.0).contiguous().numpy().tobytes()).hexdigest()


def _gen(*key):
    return torch.Generator().manual_seed(int(hashlib.sha256(repr(key).encode()).hexdigest()[:8], 16))


def _leaf(t):
    return t.clone().to(DEV).requires_grad_(True)


def _objective(g, outs):
    """sum_k <out_k, random cotangent_k>: a non-zero random upstream gradient for every output."""
    return sum((o * torch.randn(o.shape, generator=g).to(DEV)).sum() for o in outs)


# ---- MotionLearning losses --------------------------------------------------------------------------------------------------------------------
def _rgbd(H, W, ssim):
    from simpledepthestimation_amd.hip import motion_loss as HM
    v = MI.inputs(2, H, W, seed=H)
    d, R, t = _leaf(v["depth1"]), _leaf(v["R12"]), _leaf(v["t12"])
    o = HM.rgbd_consistency(v["frame1"].to(DEV), v["frame2"].to(DEV), d, v["depth2"].to(DEV), v["K"].to(DEV), R, t, ssim=ssim)
    keys = ["rgb_l1", "depth_l1"] + (["ssim"] if ssim else [])
    _objective(_gen("rgbd", H, W, ssim), [o[k] for k in keys]).backward()
    res = {k: o[k] for k in keys + ["coords_A_in_B", "occlusion_mask"]}
    if ssim:
        res["depth_proximity_weight"] = o["depth_proximity_weight"]
    res.update(g_depth=d.grad, g_R=R.grad, g_t=t.grad)
    return res


def _wssim(H, W):
    from simpledepthestimation_amd.hip import motion_loss as HM
    v = MI.inputs(2, H, W, seed=H + 1)
    g = _gen("wssim", H, W)
    x, y, w = _leaf(v["frame1"]), _leaf(v["frame2"]), torch.rand(2, 1, H, W, generator=g).to(DEV)
    out, avg_w = HM.weighted_ssim(x, y, w)
    _objective(g, [out]).backward()
    return dict(out=out, avg_w=avg_w, g_x=x.grad, g_y=y.grad)


def _motion_consistency(H, W):
    from simpledepthestimation_amd.hip import motion_loss as HM
    v = MI.inputs(2, H, W, seed=H + 2)
    with torch.no_grad():
        o = HM.rgbd_consistency(*(v[k].to(DEV) for k in ("frame1", "frame2", "depth1", "depth2", "K", "R12", "t12")), ssim=False)
    R1, R2, tA, tB = (_leaf(v[k]) for k in ("R12", "R21", "t12", "t21"))
    rot, trans = HM.motion_consistency(o["coords_A_in_B"], o["occlusion_mask"], R1, R2, tA, tB)
    _objective(_gen("mc", H, W), [rot, trans]).backward()
    return dict(rot=rot, trans=trans, g_R1=R1.grad, g_R2=R2.grad, g_tA=tA.grad)


def _field_loss(H, W, which):
    from simpledepthestimation_amd.hip import motion_loss as HM
    f = _leaf(MI.inputs(2, H, W, seed=H + 3)["t12"])
    loss = getattr(HM, which)(f)
    _objective(_gen(which, H, W), [loss]).backward()
    return dict(loss=loss, g_field=f.grad)


def _pair_prep(H, W, normalize):
    """Pooled to H x W (the size that sets the workgroup count) from a slightly larger, not commensurate input."""
    from simpledepthestimation_amd.hip import motion_loss as HM
    H0, W0 = H + 3, W + 5
    v = MI.inputs(2, H0, W0, seed=H + 4)
    g = _gen("prep", H, W, normalize)
    depth, motion, tpose = _leaf(v["depth1"]), _leaf(v["t12"]), _leaf(torch.randn(2, 3, generator=g))
    mask = (torch.rand(2, 1, H0, W0, generator=g) > 0.3).float().to(DEV)
    o = HM.pair_prep(depth, motion, tpose, mask, (H, W), scale_normalize=normalize)
    diff = ["depth_r", "t", "m_norm", "t_sw"] + (["depth_n"] if normalize else [])
    _objective(g, [o[k] for k in diff]).backward()
    res = {k: o[k] for k in diff + ["depth_n_sw", "overall_motion"]}
    res.update(g_depth=depth.grad, g_motion=motion.grad, g_tpose=tpose.grad)
    return res


# ---- photometric, smoothness, mono loss -------------------------------------------------------------------------------------------------------
def _photo_inputs(B, n, nctx):
    from oracle import geometry as G
    from oracle.gen_golden import kitti_K, smooth_images
    from simpledepthestimation_amd.hip import lib as L
    H, W = PHOTO_BASE
    g = _gen("photo", B, n, nctx)
    nb = [L.lib().sde_photo_num_blocks(1, H >> i, W >> i, 1) for i in range(n)]
    assert nb[0] > 64 and (n == 1 or nb[-1] < 64), nb      # the pose finalize walks the largest slab in several trips and the smallest in one ragged one
    Ds, As, Cs, scales = [], [], [], []
    for i in range(n):
        h, w = H >> i, W >> i
        A, C0, C1 = smooth_images(g, B, h, w)
        D = torch.rand(B, 1, h, w, generator=g) * 30 + 2
        Ds.append(_leaf(torch.nn.functional.avg_pool2d(torch.nn.functional.pad(D, (2, 2, 2, 2), mode="replicate"), 5, 1)))
        As.append(A.to(DEV)); Cs.append([c.to(DEV) for c in (C0, C1)[:nctx]]); scales.append((w / W, h / H))
    vec = torch.tensor([[0.05, -0.01, 0.3, 0.002, -0.004, 0.001], [-0.03, 0.02, -0.25, -0.001, 0.003, 0.002]])[:B]
    poses = [_leaf(G.pose_vec2mat(s * vec)) for s in (1.0, -1.0)[:nctx]]
    return g, Ds, kitti_K(B, H, W).to(DEV), As, Cs, poses, scales


def _photo_multi(B, n, nctx):
    from simpledepthestimation_amd.hip import photometric as P
    g, Ds, K, As, Cs, poses, scales = _photo_inputs(B, n, nctx)
    losses = P.photometric_multi_loss(Ds, K, As, Cs, poses, scales)
    _objective(g, [losses]).backward()
    res = dict(losses=losses)
    res.update({f"g_depth{i}": d.grad for i, d in enumerate(Ds)})
    res.update({f"g_pose{j}": p.grad for j, p in enumerate(poses)})
    return res


def _mono(B, n, nctx):
    from simpledepthestimation_amd.hip import photometric as P
    g, Ds, K, As, Cs, poses, scales = _photo_inputs(B, n, nctx)
    pw = [float(x) for x in torch.rand(n, generator=g) + 0.5]
    sw = [float(x) for x in torch.rand(n, generator=g) * 1e-2 + 1e-3]
    rec, smooth, per_scale = P.mono_loss(Ds, K, As, Cs, poses, scales, pw, sw)
    _objective(g, [rec, smooth]).backward()
    res = dict(rec=rec, smooth=smooth, per_scale=per_scale)
    res.update({f"g_depth{i}": d.grad for i, d in enumerate(Ds)})
    res.update({f"g_pose{j}": p.grad for j, p in enumerate(poses)})
    return res


def _silog():
    """Four scales against one 64 x 208 ground truth, B = 2: 26, 7 and 2 blocks, and the 8 x 26 scale owns a single one."""
    from simpledepthestimation_amd.hip import lib as L, photometric as P
    g = _gen("silog")
    B, H, W = 2, 64, 208
    assert L.lib().sde_silog_num_blocks(B, H >> 3, W >> 3) == 1
    gt = torch.rand(B, 1, H, W, generator=g) * 80
    gt[torch.rand(B, 1, H, W, generator=g) < 0.3] = 0.0          # no measurement
    ests = [_leaf(torch.rand(B, 1, H >> i, W >> i, generator=g) * 60 + 1.5) for i in range(4)]
    loss = P.silog_loss_multi(ests, gt.to(DEV), 0.85, [1.0, 0.7, 0.5, 0.3])
    _objective(g, [loss]).backward()
    res = dict(loss=loss)
    res.update({f"g_est{i}": e.grad for i, e in enumerate(ests)})
    return res


def _img_to_points(H, W):
    from simpledepthestimation_amd.hip.cloud import img_to_points
    g = _gen("i2p", H, W)
    d, R, t = _leaf(torch.rand(2, 1, H, W, generator=g) * 30 + 1), _leaf(MI.inputs(2, 8, 8, seed=H + 5)["R12"]), _leaf(torch.randn(2, 3, 1, generator=g))
    p = img_to_points(d, R, t)
    _objective(g, [p]).backward()
    return dict(points=p, g_depth=d.grad, g_R=R.grad, g_t=t.grad)


def _cases():
    c = {}
    for H, W in SHAPES:
        s = f"{H}x{W}"
        c[f"rgbd_ssim_{s}"] = lambda H=H, W=W: _rgbd(H, W, True)
        c[f"rgbd_{s}"] = lambda H=H, W=W: _rgbd(H, W, False)
        c[f"wssim_{s}"] = lambda H=H, W=W: _wssim(H, W)
        c[f"motion_consistency_{s}"] = lambda H=H, W=W: _motion_consistency(H, W)
        c[f"motion_smoothness_{s}"] = lambda H=H, W=W: _field_loss(H, W, "motion_smoothness")
        c[f"motion_sparsity_{s}"] = lambda H=H, W=W: _field_loss(H, W, "motion_sparsity")      # hw = 700 < 1024; 18720 and 45240: no multiples of 1024
        c[f"pair_prep_{s}"] = lambda H=H, W=W: _pair_prep(H, W, False)
        c[f"pair_prep_normalize_{s}"] = lambda H=H, W=W: _pair_prep(H, W, True)
        c[f"img_to_points_{s}"] = lambda H=H, W=W: _img_to_points(H, W)
    for B, n, nctx in [(2, 4, 2), (1, 1, 1)]:
        c[f"photo_multi_B{B}_n{n}_ctx{nctx}"] = lambda a=(B, n, nctx): _photo_multi(*a)
        c[f"mono_loss_B{B}_n{n}_ctx{nctx}"] = lambda a=(B, n, nctx): _mono(*a)
    c["silog_multi"] = _silog
    return c


CASES = _cases()


def run_case(name):
    """{output name: sha256} of one case."""
    out = {k: sha(v) for k, v in CASES[name]().items()}
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_table_and_record_agree(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_loss_bits(golden, name):
    first, second = run_case(name), run_case(name)
    assert first == second, sorted(k for k in first if first[k] != second[k])                 # the ticket is back at zero, nothing depends on the run
    assert first == golden[name], sorted(k for k in first if first[k] != golden[name].get(k))

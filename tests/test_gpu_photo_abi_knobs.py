"""The scaling and accumulation parameters of the single-scale loss entries of libsde_hip.so, called through ctypes.

`loss_scale`, `gscale` and the `accumulate*` flags of sde_photo_fwd/_bwd, sde_smooth_fwd/_bwd and sde_silog_bwd are part of the C ABI
(include/sde_hip.h); the autograd wrappers only ever pass the neutral values (1, 1, 0).  Reference of every case: the same entry called with the
neutral values.  Accumulating adds one fp32 value to another and a power-of-two gscale scales every product exactly, so those cases are compared
with torch.equal; loss_scale = 2.5 is applied to the mean before the sum is rounded, hence rtol 1e-6 there.

Shapes: B = 2, two contexts, 37 x 75 (a multiple of neither the forward nor the backward tile, several workgroups per sample, B > 1 so that the
sample index of a workgroup matters); SILog 12 x 20 estimates against 24 x 40 ground truth.
"""
import ctypes

import pytest
import torch

from oracle import geometry as G
from oracle.gen_golden import kitti_K, smooth_images

pytestmark = pytest.mark.gpu
dev = "cuda"
B, H, W, NCTX = 2, 37, 75, 2


@pytest.fixture(scope="module")
def L():
    from simpledepthestimation_amd.hip import lib
    lib.lib()
    return lib


def _dev_scalar(v):
    return torch.tensor(v, device=dev)


@pytest.fixture(scope="module")
def photo(L):
    """Inputs, descriptor and the neutral forward / backward results of one photometric scale."""
    g = torch.Generator().manual_seed(5)
    A, C0, C1 = smooth_images(g, B, H, W)
    D = torch.rand(B, 1, H, W, generator=g) * 30 + 2
    D = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(D, (2, 2, 2, 2), mode="replicate"), 5, 1)
    vec = torch.tensor([[0.05, -0.01, 0.3, 0.002, -0.004, 0.001], [-0.03, 0.02, -0.25, -0.001, 0.003, 0.002]])
    t = dict(A=A, ctx=[C0, C1], depth=D, K=kitti_K(B, H, W), pose=[G.pose_vec2mat(vec), G.pose_vec2mat(-vec)])
    t = {k: [x.to(dev).contiguous() for x in v] if isinstance(v, list) else v.to(dev).contiguous() for k, v in t.items()}
    d = L.PhotoDesc()
    d.A, d.depth, d.K = t["A"].data_ptr(), t["depth"].data_ptr(), t["K"].data_ptr()
    for j in range(NCTX):
        d.ctx[j], d.pose[j] = t["ctx"][j].data_ptr(), t["pose"][j].data_ptr()
    d.B, d.h, d.w, d.nctx, d.automask, d.reduce_mean = B, H, W, NCTX, 1, 0
    d.sx, d.sy, d.ssim_w, d.C1, d.C2 = 1.0, 1.0, 0.85, 1e-4, 9e-4
    d.clip_thr = 0
    lib = L.lib()
    c = dict(t=t, d=d, sampled=[torch.empty(B, 3, H, W, device=dev) for _ in range(NCTX)], sel=torch.empty(B, H, W, device=dev, dtype=torch.uint8),
             partial=torch.empty(lib.sde_photo_num_blocks(B, H, W, 0), device=dev),
             pose_partial=torch.empty(lib.sde_photo_num_blocks(B, H, W, 1) * NCTX * 12, device=dev), gout=_dev_scalar(0.7))
    c["loss"] = _photo_fwd(L, c, torch.full((), float("nan"), device=dev), 1.0, 0)
    c["d_depth"], c["d_pose"] = _photo_bwd(L, c, torch.full((B, 1, H, W), float("nan"), device=dev),
                                           [torch.full((B, 4, 4), float("nan"), device=dev) for _ in range(NCTX)], 1.0, 0, 0)
    torch.cuda.synchronize()
    assert torch.isfinite(c["loss"]) and c["loss"] > 0 and torch.isfinite(c["d_depth"]).all() and c["d_depth"].abs().sum() > 0
    assert all(torch.isfinite(p).all() and p.abs().sum() > 0 and (p[:, 3] == 0).all() for p in c["d_pose"])
    return c


def _photo_fwd(L, c, loss_out, loss_scale, accumulate):
    L.check(L.lib().sde_photo_fwd(ctypes.byref(c["d"]), L.ptr_array(c["sampled"]), L.ptr(c["sel"]), None, L.ptr(c["partial"]), L.ptr(loss_out),
                                  loss_scale, accumulate, L.stream()), "sde_photo_fwd")
    return loss_out


def _photo_bwd(L, c, d_depth, d_pose, gscale, acc_depth, acc_pose):
    L.check(L.lib().sde_photo_bwd(ctypes.byref(c["d"]), L.ptr_array(c["sampled"]), L.ptr(c["sel"]), L.ptr(c["gout"]), gscale, L.ptr(d_depth), acc_depth,
                                  L.ptr(c["pose_partial"]), L.ptr_array(d_pose), acc_pose, L.stream()), "sde_photo_bwd")
    return d_depth, d_pose


def test_photo_fwd_loss_scale_and_accumulate(L, photo):
    pre = 0.75
    out = _photo_fwd(L, photo, _dev_scalar(pre), 1.0, 1)
    assert torch.equal(out, _dev_scalar(pre) + photo["loss"])
    out = _photo_fwd(L, photo, _dev_scalar(pre), 2.5, 1)
    torch.testing.assert_close(out, _dev_scalar(pre) + 2.5 * photo["loss"], rtol=1e-6, atol=0)
    out = _photo_fwd(L, photo, torch.full((), float("nan"), device=dev), 2.5, 0)
    torch.testing.assert_close(out, 2.5 * photo["loss"], rtol=1e-6, atol=0)


def test_photo_bwd_accumulate_and_gscale(L, photo):
    g = torch.Generator().manual_seed(6)
    pre_d = torch.randn(B, 1, H, W, generator=g).to(dev)
    pre_p = [torch.randn(B, 4, 4, generator=g).to(dev) for _ in range(NCTX)]
    dd, dp = _photo_bwd(L, photo, pre_d.clone(), [p.clone() for p in pre_p], 1.0, 1, 1)
    assert torch.equal(dd, pre_d + photo["d_depth"])
    for a, p, ref in zip(dp, pre_p, photo["d_pose"]):
        assert torch.equal(a, p + ref)
    # one flag at a time: the other output is written, not accumulated
    dd, dp = _photo_bwd(L, photo, pre_d.clone(), [p.clone() for p in pre_p], 1.0, 1, 0)
    assert torch.equal(dd, pre_d + photo["d_depth"]) and all(torch.equal(a, ref) for a, ref in zip(dp, photo["d_pose"]))
    dd, dp = _photo_bwd(L, photo, pre_d.clone(), [p.clone() for p in pre_p], 1.0, 0, 1)
    assert torch.equal(dd, photo["d_depth"]) and all(torch.equal(a, p + ref) for a, p, ref in zip(dp, pre_p, photo["d_pose"]))
    dd, dp = _photo_bwd(L, photo, torch.empty_like(pre_d), [torch.empty_like(p) for p in pre_p], 2.0, 0, 0)
    assert torch.equal(dd, 2.0 * photo["d_depth"])
    for a, ref in zip(dp, photo["d_pose"]):
        assert torch.equal(a, 2.0 * ref)


@pytest.fixture(scope="module")
def smooth(L):
    g = torch.Generator().manual_seed(7)
    img = smooth_images(g, B, H, W, 1)[0].to(dev).contiguous()
    depth = (torch.rand(B, 1, H, W, generator=g) * 40 + 0.5).to(dev)
    nb = L.lib().sde_smooth_num_blocks(B, H, W)
    c = dict(img=img, depth=depth, mean_part=torch.empty(B * 32, device=dev), dn=torch.empty(B, H, W, device=dev), loss_part=torch.empty(nb, device=dev),
             s_part=torch.empty(nb, device=dev), gout=_dev_scalar(0.7))
    c["loss"] = _smooth_fwd(L, c, torch.full((), float("nan"), device=dev), 1.0, 0)
    c["d_depth"] = _smooth_bwd(L, c, torch.full((B, 1, H, W), float("nan"), device=dev), 1.0, 0)
    torch.cuda.synchronize()
    assert torch.isfinite(c["loss"]) and c["loss"] > 0 and torch.isfinite(c["d_depth"]).all() and c["d_depth"].abs().sum() > 0
    return c


def _smooth_fwd(L, c, loss_out, loss_scale, accumulate):
    L.check(L.lib().sde_smooth_fwd(L.ptr(c["depth"]), L.ptr(c["img"]), B, H, W, L.ptr(c["mean_part"]), L.ptr(c["dn"]), L.ptr(c["loss_part"]), L.ptr(c["s_part"]),
                                   L.ptr(loss_out), loss_scale, accumulate, L.stream()), "sde_smooth_fwd")
    return loss_out


def _smooth_bwd(L, c, d_depth, gscale, accumulate):
    L.check(L.lib().sde_smooth_bwd(L.ptr(c["depth"]), L.ptr(c["dn"]), L.ptr(c["mean_part"]), L.ptr(c["s_part"]), L.ptr(c["gout"]), gscale, B, H, W,
                                   L.ptr(d_depth), accumulate, L.stream()), "sde_smooth_bwd")
    return d_depth


def test_smooth_fwd_loss_scale_and_accumulate(L, smooth):
    pre = 0.75
    out = _smooth_fwd(L, smooth, _dev_scalar(pre), 1.0, 1)
    assert torch.equal(out, _dev_scalar(pre) + smooth["loss"])
    out = _smooth_fwd(L, smooth, _dev_scalar(pre), 2.5, 1)
    torch.testing.assert_close(out, _dev_scalar(pre) + 2.5 * smooth["loss"], rtol=1e-6, atol=0)
    out = _smooth_fwd(L, smooth, torch.full((), float("nan"), device=dev), 2.5, 0)
    torch.testing.assert_close(out, 2.5 * smooth["loss"], rtol=1e-6, atol=0)


def test_smooth_bwd_accumulate_and_gscale(L, smooth):
    pre = torch.randn(B, 1, H, W, generator=torch.Generator().manual_seed(8)).to(dev)
    assert torch.equal(_smooth_bwd(L, smooth, pre.clone(), 1.0, 1), pre + smooth["d_depth"])
    assert torch.equal(_smooth_bwd(L, smooth, torch.empty_like(pre), 2.0, 0), 2.0 * smooth["d_depth"])
    assert torch.equal(_smooth_bwd(L, smooth, pre.clone(), 2.0, 1), pre + 2.0 * smooth["d_depth"])


def test_silog_bwd_accumulate_and_gscale(L):
    h, w, Hg, Wg, vf = 12, 20, 24, 40, 0.85
    g = torch.Generator().manual_seed(9)
    est = (torch.rand(B, 1, h, w, generator=g) * 60 + 0.3).to(dev)
    gt = torch.where(torch.rand(B, 1, Hg, Wg, generator=g) < 0.5, torch.rand(B, 1, Hg, Wg, generator=g) * 79 + 1, torch.zeros(1)).to(dev)
    lib = L.lib()
    part = torch.empty(lib.sde_silog_num_blocks(B, h, w) * 3, device=dev)
    stats = torch.full((4,), float("nan"), device=dev)
    L.check(lib.sde_silog_fwd(L.ptr(est), L.ptr(gt), B, h, w, Hg, Wg, vf, L.ptr(part), L.ptr(stats), L.stream()), "sde_silog_fwd")
    gout = _dev_scalar(0.7)

    def bwd(d_est, gscale, accumulate):
        L.check(lib.sde_silog_bwd(L.ptr(est), L.ptr(gt), L.ptr(stats), L.ptr(gout), gscale, vf, B, h, w, Hg, Wg, L.ptr(d_est), accumulate, L.stream()), "sde_silog_bwd")
        return d_est

    ref = bwd(torch.full((B, 1, h, w), float("nan"), device=dev), 1.0, 0)
    assert torch.isfinite(stats).all() and stats[0] > 0 and stats[3] > 0 and torch.isfinite(ref).all() and ref.abs().sum() > 0
    pre = torch.randn(B, 1, h, w, generator=g).to(dev)
    assert torch.equal(bwd(pre.clone(), 1.0, 1), pre + ref)
    assert torch.equal(bwd(torch.empty_like(pre), 2.0, 0), 2.0 * ref)
    assert torch.equal(bwd(pre.clone(), 2.0, 1), pre + 2.0 * ref)

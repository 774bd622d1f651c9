"""Plain-torch restatement of MotionLearningModel's training forward (reference: detectron2/modeling/meta_arch/MotionLearning.py:L78-241), written from the
formulas with the functions of tests/motion_loss_ref.py, one call per direction as the reference is written.  Works in whatever dtype / device its inputs
have.  Also here, shared by scripts/gen_golden_motion_model.py and the CPU / GPU tests: the stub networks whose predictions are parameters, the cases of
tests/golden/motion_model.npz, and the comparison with that file."""
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import motion_loss_init as MI
import motion_loss_ref as R

# ---------------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
BASE = dict(num_scales=1, depth_l1_loss_w=0.0, ssim_loss_w=3.0, C1=float("inf"), C2=9e-6, clip_loss=0.0, smooth_loss_w=1e-3, sup_loss_w=0.0,
            variance_focus=0.85, var_loss_w=0.0, motion_smooth_loss_w=1.0, motion_sparsity_loss_w=0.2, rot_cycle_loss_w=1e-3, trans_cycle_loss_w=5e-2,
            scale_normalize=False, pose_use_depth=True, with_mask=False, mask_dilation=8, return_loss=False)     # projects/MotionLearning/configs/Base.yaml


def silog(est, gt, variance_focus):
    m = gt > 1.0
    d = torch.log(est[m]) - torch.log(gt[m])
    return torch.sqrt((d ** 2).mean() - variance_focus * (d.mean() ** 2)) * 10.0


def variance_loss(depth):
    return 1 / ((depth / depth.mean() - 1.0) ** 2).mean()


def smoothness_loss(depth, image):
    inv = 1.0 / depth.clamp(min=1e-6)
    inv = inv / inv.mean(2, True).mean(3, True).clamp(min=1e-6)
    gx = lambda v: v[:, :, :, :-1] - v[:, :, :, 1:]
    gy = lambda v: v[:, :, :-1, :] - v[:, :, 1:, :]
    wx = torch.exp(-gx(image).abs().mean(1, keepdim=True))
    wy = torch.exp(-gy(image).abs().mean(1, keepdim=True))
    return (gx(inv) * wx).abs().mean() + (gy(inv) * wy).abs().mean()


def forward(s, batch, depth_net, pose_net, record=None):
    """s: namespace of the settings (the model's attribute names); record: a list that receives the occlusion masks, [2B,1,h,w] per scale (1 -> 2 | 2 -> 1),
    coarsest scale first.  Returns the batch with the loss entries, depth_proximity_weight and overall_motion."""
    frame1, frame2 = batch["img"], batch["ctx_img"][0]
    batch["depth_net_input"] = torch.cat([(frame1 - s.pixel_mean) / s.pixel_std, (frame2 - s.pixel_mean) / s.pixel_std], 0)
    batch = depth_net(batch)
    depth1, depth2 = torch.chunk(batch["depth_pred"][0], 2, dim=0)
    in1, in2 = frame1, frame2
    if s.pose_use_depth:
        in1, in2 = torch.cat([in1, depth1], 1), torch.cat([in2, depth2], 1)
    batch["pose_net_input"] = torch.cat([torch.cat([in1, in2], 1), torch.cat([in2, in1], 1)], 0)
    batch = pose_net(batch)
    pose12, pose21 = torch.chunk(batch["pose_pred"], 2, dim=0)
    has_motion = "motion_pred" in batch
    if has_motion:
        m12, m21 = torch.chunk(batch["motion_pred"], 2, dim=0)
        if s.with_mask:
            k1, k2 = (batch["mask"] > 0).to(m12.dtype), (batch["ctx_mask"][0] > 0).to(m12.dtype)
            if s.mask_dilation > 0:
                k1, k2 = (F.max_pool2d(k, 2 * s.mask_dilation + 1, stride=1, padding=s.mask_dilation) for k in (k1, k2))
            m12, m21 = m12 * k1, m21 * k2
    batch["depth_proximity_weight"], batch["overall_motion"] = [], []
    losses = {}

    def add(name, value, weight=1.0):
        losses[name] = losses.get(name, 0) + value * weight

    H0, W0 = depth1.shape[-2:]
    R12, R21 = pose12[:, :3, :3], pose21[:, :3, :3]
    for i in reversed(range(s.num_scales)):
        sw = 1.0 / 2 ** i
        size = (int(H0 * sw), int(W0 * sw))
        f1, f2 = R.resize_img_avgpool(frame1, size), R.resize_img_avgpool(frame2, size)
        K = batch["intrinsics"].clone()
        K[:, :2] = K[:, :2] * sw
        d1, d2 = R.resize_img_avgpool(depth1, size), R.resize_img_avgpool(depth2, size)
        t12, t21 = pose12[:, :3, 3, None, None], pose21[:, :3, 3, None, None]
        if has_motion:
            r12, r21 = R.resize_img_avgpool(m12, size), R.resize_img_avgpool(m21, size)
            t12, t21 = t12 + r12, t21 + r21
        else:
            t12, t21 = t12.expand(-1, -1, *size), t21.expand(-1, -1, *size)
        batch["overall_motion"].append((t12, t21))
        if s.scale_normalize:
            mean = torch.mean(torch.cat([d1, d2], 0))
            n1, n2, t12, t21 = d1 / mean, d2 / mean, t12 / mean, t21 / mean
            if has_motion:
                r12, r21 = r12 / mean, r21 / mean
        else:
            n1, n2 = d1, d2
        o12 = R.rgbd_consistency_loss(f1, f2, n1, n2, K, R12, t12, s.depth_l1_loss_w, s.ssim_loss_w, s.C1, s.C2)
        o21 = R.rgbd_consistency_loss(f2, f1, n2, n1, K, R21, t21, s.depth_l1_loss_w, s.ssim_loss_w, s.C1, s.C2)
        for o in (o12, o21):
            for k, v in o.items():
                if "loss" in k:
                    add(k, v, sw)
        batch["depth_proximity_weight"].append((o12.get("depth_proximity_weight"), o21.get("depth_proximity_weight")))
        if record is not None:
            record.append(torch.cat([o12["occlusion_mask"], o21["occlusion_mask"]], 0).detach())
        if s.rot_cycle_loss_w > 0 or s.trans_cycle_loss_w > 0:
            for o, a in ((o12, (R12, R21, t12, t21)), (o21, (R21, R12, t21, t12))):
                rot, trans = R.motion_consistency_loss(o["coords_A_in_B"], o["occlusion_mask"], *a)
                add("rot_loss", rot, sw * s.rot_cycle_loss_w)
                add("trans_loss", trans, sw * s.trans_cycle_loss_w)
        if has_motion:
            for r, t in ((r12, t12), (r21, t21)):
                m = r / torch.sqrt(t.pow(2).mean([1, 2, 3], keepdim=True) * 3.0 + 1e-12)
                if s.motion_smooth_loss_w > 0.0:
                    add("motion_smooth_loss", R.motion_smoothness_loss_fn(m), sw * s.motion_smooth_loss_w)
                if s.motion_sparsity_loss_w > 0.0:
                    add("motion_sparsity_loss", R.motion_sparsity_loss_fn(m), sw * s.motion_sparsity_loss_w)
        if s.sup_loss_w > 0.0:
            for d, gt in ((d1, batch["depth"]), (d2, batch["ctx_depth"][0])):
                gt = gt if tuple(gt.shape[-2:]) == size else F.interpolate(gt, size=size, mode="nearest")
                add("sup_loss", silog(d, gt, s.variance_focus), sw * s.sup_loss_w)
        if s.smooth_loss_w > 0.0:
            add("smooth_loss", smoothness_loss(n1, f1), sw * s.smooth_loss_w)
            add("smooth_loss", smoothness_loss(n2, f2), sw * s.smooth_loss_w)
        if s.var_loss_w > 0.0:
            add("var_loss", variance_loss(d1), sw * s.var_loss_w)
            add("var_loss", variance_loss(d2), sw * s.var_loss_w)
    batch.update(losses)
    return batch


def pair_prep(depth, motion, t_pose, mask01, size, scale_normalize):
    """The restatement of hip.motion_loss.pair_prep alone (stacked, N = 2B): dict(depth_r, depth_n, t, m_norm, t_sw, depth_n_sw, overall_motion)."""
    N = depth.shape[0]
    sw = lambda v: torch.cat([v[N // 2:], v[:N // 2]], 0)
    d = R.resize_img_avgpool(depth, size)
    t = t_pose[:, :, None, None].expand(-1, -1, *size)
    r = None
    if motion is not None:
        r = R.resize_img_avgpool(motion * mask01 if mask01 is not None else motion, size)
        t = t + r
    overall, n = t.detach(), d
    if scale_normalize:
        mean = d.mean()
        n, t = d / mean, t / mean
        r = r / mean if r is not None else None
    m = None
    if r is not None:
        m = r / torch.sqrt(t.pow(2).mean([1, 2, 3], keepdim=True) * 3.0 + 1e-12)
    return {"depth_r": d, "depth_n": n, "t": t, "m_norm": m, "t_sw": sw(t), "depth_n_sw": sw(n).detach(), "overall_motion": overall}


# ---------------------------------------------------------------------------------------------------------------------------------------
# stub networks: the predictions are parameters
# ---------------------------------------------------------------------------------------------------------------------------------------
class StubDepthNet(nn.Module):
    dtype = torch.float32      # what MotionLearningModel asks its depth net for when it prepares the input

    def __init__(self, depth):
        super().__init__()
        self.depth = nn.Parameter(depth.clone())

    def forward(self, batch):
        batch["depth_pred"] = [self.depth]
        return batch


class StubPoseNet(nn.Module):
    """pose_pred from the parameters rot [2B,3,3] and trans [2B,3]; motion_pred = the parameter motion [2B,3,H,W] plus a small linear function of the depth
    channels of pose_net_input (so the gradient that USE_DEPTH sends into the depth net is part of the test).  motion = None: no motion_pred."""
    COEF = (2e-3, -1e-3, 5e-4)

    def __init__(self, rot, trans, motion):
        super().__init__()
        self.rot, self.trans = nn.Parameter(rot.clone()), nn.Parameter(trans.clone())
        self.motion = nn.Parameter(motion.clone()) if motion is not None else None

    def forward(self, batch):
        x = batch["pose_net_input"]
        N = self.rot.shape[0]
        pose = torch.zeros(N, 4, 4, dtype=self.rot.dtype, device=self.rot.device)
        pose[:, 3, 3] = 1.0
        pose = torch.cat([torch.cat([self.rot, self.trans[:, :, None]], 2), pose[:, 3:]], 1)
        batch["pose_pred"] = pose
        if self.motion is not None:
            field = self.motion
            if x.shape[1] == 8:
                coef = torch.tensor(self.COEF, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
                field = field + coef * (x[:, 3:4] - x[:, 7:8])
            batch["motion_pred"] = field
        return batch


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/golden/motion_model.npz (B = 2 each)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _rect_mask(H, W, rects):
    m = torch.zeros(2, 1, H, W)
    for n, y0, y1, x0, x1 in rects:
        m[n, 0, y0:y1, x0:x1] = 1.0
    return m


# seed: that of motion_loss_init.inputs.  Seed 1 is left out: it has a pixel at which the reference's own fp32 depth gradient is 6 % of the map's maximum
# away from its fp64 one, which breaks the generator's caps.
CASES = {
    "base": dict(size=(32, 104), seed=0, settings={}),
    "options": dict(size=(30, 70), seed=4, settings=dict(num_scales=3, scale_normalize=True, depth_l1_loss_w=1.0, var_loss_w=1e-4, sup_loss_w=0.1), sup=True),
    "mask8": dict(size=(32, 104), seed=2, settings=dict(with_mask=True, mask_dilation=8), mask=True),
    "mask2": dict(size=(32, 104), seed=5, settings=dict(with_mask=True, mask_dilation=2), mask=True),
    "nomotion": dict(size=(32, 104), seed=3, settings={}, motion=False),
}
B = 2
PARAMS = ("depth", "rot", "trans", "motion")
OUT_TOL, GRAD_TOL, D_FACTOR, MAX_OFF = MI.OUT_TOL, MI.GRAD_TOL, MI.D_FACTOR, MI.MAX_OFF


def settings(name):
    s = dict(BASE)
    s.update(CASES[name]["settings"])
    return s


def case_inputs(name):
    """(batch of float32 CPU tensors, dict of the stub networks' float32 parameters) from the recipe of tests/motion_loss_init.py."""
    c = CASES[name]
    H, W = c["size"]
    v = MI.inputs(B, H, W, seed=c["seed"])
    batch = {"img": v["frame1"], "ctx_img": [v["frame2"]], "intrinsics": v["K"]}
    g = torch.Generator().manual_seed(77)
    if c.get("sup"):        # sparse ground truth near the prediction: about a third of the pixels are 0 (<= 1: outside the SILog mask)
        for key, d in (("depth", v["depth1"]), ("ctx_depth", v["depth2"])):
            gt = d * (1.0 + 0.1 * torch.randn(d.shape, generator=g)) * (torch.rand(d.shape, generator=g) > 0.35)
            batch[key] = gt if key == "depth" else [gt]
    if c.get("mask"):       # a few rectangles that touch the border; values other than 1 where set: the model thresholds at > 0
        batch["mask"] = 3.0 * _rect_mask(H, W, [(0, 0, 9, 0, 20), (0, 20, 32, 60, 75), (1, 10, 18, 90, 104)])
        batch["ctx_mask"] = [_rect_mask(H, W, [(0, 25, 32, 0, 12), (1, 0, 6, 40, 70), (1, 14, 20, 50, 58)])]
    params = {"depth": torch.cat([v["depth1"], v["depth2"]], 0), "rot": torch.cat([v["R12"], v["R21"]], 0),
              "trans": torch.tensor([[0.05, -0.02, 0.6]] * B + [[-0.05, 0.02, -0.6]] * B)}
    if c.get("motion", True):
        base = torch.tensor([0.05, -0.02, 0.6]).view(1, 3, 1, 1)
        params["motion"] = torch.cat([v["t12"] - base, v["t21"] + base], 0)         # the blobs and the noise of the recipe, without its constant part
    return batch, params


def to(batch, dtype, device):
    f = lambda x: x.detach().clone().to(device=device, dtype=dtype)
    return {k: [f(x) for x in v] if isinstance(v, list) else f(v) for k, v in batch.items()}


def make_instance(cls, s, depth_net, pose_net, ssim, supervise_loss, dtype, device):
    """A model of class cls (the reference's, or this package's) without the registries: __new__ + nn.Module.__init__ + the attributes its forward reads."""
    m = cls.__new__(cls)
    nn.Module.__init__(m)
    m.depth_net, m.pose_net, m.ssim, m.supervise_loss = depth_net, pose_net, ssim, supervise_loss
    for k, v in s.items():
        if k not in ("C1", "C2", "variance_focus"):
            setattr(m, k, v)
    m.register_buffer("pixel_mean", torch.tensor([0.485, 0.456, 0.406], dtype=dtype, device=device).view(1, -1, 1, 1))
    m.register_buffer("pixel_std", torch.tensor([0.229, 0.224, 0.225], dtype=dtype, device=device).view(1, -1, 1, 1))
    return m.train()


def run_case(name, fn, dtype, device):
    """fn(batch, depth_net, pose_net, record) -> batch with the losses; the objective is the sum of all entries whose name contains 'loss'.
    Returns dict(losses, grads (per PARAMS), occ: [per-scale masks])."""
    batch, params = case_inputs(name)
    batch = to(batch, dtype, device)
    p = {k: v.to(device=device, dtype=dtype) for k, v in params.items()}
    depth_net, pose_net = StubDepthNet(p["depth"]), StubPoseNet(p["rot"], p["trans"], p.get("motion"))
    record = []
    out = fn(batch, depth_net, pose_net, record)
    losses = {k: v for k, v in out.items() if "loss" in k}
    sum(losses.values()).backward()
    grads = {"depth": depth_net.depth.grad, "rot": pose_net.rot.grad, "trans": pose_net.trans.grad}
    if pose_net.motion is not None:
        grads["motion"] = pose_net.motion.grad
    return {"losses": {k: v.detach() for k, v in losses.items()}, "grads": grads, "occ": record}


def restatement_fn(name, dtype, device):
    s = types.SimpleNamespace(**settings(name))
    s.pixel_mean = torch.tensor([0.485, 0.456, 0.406], dtype=dtype, device=device).view(1, -1, 1, 1)
    s.pixel_std = torch.tensor([0.229, 0.224, 0.225], dtype=dtype, device=device).view(1, -1, 1, 1)
    return lambda batch, dn, pn, record: forward(s, batch, dn, pn, record)


def compare_with_golden(res, gold, name, out_tol=OUT_TOL, grad_tol=GRAD_TOL):
    """Failures (strings) of a run_case result against case `name` of the golden file.  Bounds: max(out_tol or grad_tol, D_FACTOR x d), d = the reference's own
    fp32-vs-fp64 difference.  At most MAX_OFF of the occlusion pixels may differ and at most MAX_OFF of a gradient map's elements may be off by more than
    the bound; the norm of every gradient is held to the bound all the same."""
    p = name + "_"
    dbl = lambda t: t.detach().double().cpu()
    bad = []

    def check(what, got, bound):
        print(f"  {name} {what}: {got:.3e} (bound {bound:.3e})")
        if not got <= bound:
            bad.append(f"{name} {what}: {got:.3e} > {bound:.3e}")

    names = [str(k) for k in gold[p + "loss_names"]]
    if sorted(res["losses"]) != sorted(names):
        bad.append(f"{name}: loss entries {sorted(res['losses'])}, the reference has {sorted(names)}")
        return bad
    for k in names:
        ref = float(gold[p + k])
        check(k, abs(float(res["losses"][k]) - ref) / abs(ref), max(out_tol, D_FACTOR * float(gold[p + "d_" + k])))
    shapes = gold[p + "occ_shapes"]
    if len(res["occ"]) != len(shapes):
        bad.append(f"{name}: {len(res['occ'])} occlusion masks, the reference has {len(shapes)}")
        return bad
    for i, shape in enumerate(shapes):
        n = int(np.prod(shape))
        occ = torch.from_numpy(np.unpackbits(gold[p + f"occ{i}"])[:n].reshape(tuple(shape)).astype(np.float64))
        check(f"occlusion_mask[{i}] flips", float((dbl(res["occ"][i]) != occ).double().mean()), MAX_OFF)
    for k in PARAMS:
        if p + "g_" + k not in gold.files:
            if k in res["grads"]:
                bad.append(f"{name}: a gradient for {k} that the reference does not have")
            continue
        g, ref = dbl(res["grads"][k]), torch.from_numpy(gold[p + "g_" + k]).double()
        tol = max(grad_tol, D_FACTOR * float(gold[p + "d_g_" + k]))
        diff = (g - ref).abs() / ref.abs().max()
        if g.dim() == 4:
            check("g_" + k + " elements off", float((diff > tol).double().mean()), MAX_OFF)
        else:
            check("g_" + k, float(diff.max()), tol)
        ref_n = float(gold[p + "gn_" + k])
        check("|g_" + k + "|", abs(float(g.norm()) - ref_n) / ref_n, max(grad_tol, D_FACTOR * float(gold[p + "d_gn_" + k])))
    return bad

"""MotionLearningModel (reference: detectron2/modeling/meta_arch/MotionLearning.py:L28-291) on the HIP path.

Both directions of the frame pair (1 -> 2 and 2 -> 1) are stacked along the batch (N = 2B) from the depth network to the losses: the networks already run
that way in the reference, and here the per-scale glue and the loss operators do as well.  Per scale: one ``pair_prep`` (sde_motion_prep_fwd: pools,
t = t_pose + motion, depth-mean and motion-scale normalisation, the half-swapped operands), one stacked RGB-D consistency loss, one stacked motion
consistency loss, motion smoothness / sparsity, SILog, depth smoothness and the variance term.  A mean over the stacked batch is half the sum of the
reference's two per-direction means, so those terms carry a factor 2; SILog and the variance term are not linear in the batch and run once per half.

``FUSED_PREP = False`` selects the composed path: resize_img_avgpool plus torch glue, one call per direction, as the reference is written (the A/B and
parity baseline)."""
import torch
import torch.nn.functional as F

from ...geometry.camera import resize_img_avgpool
from ...hip import motion_loss as HM
from ...hip import nn as HN
from ...utils.memory import to_cuda
from ..losses.losses import silog_loss, variance_loss
from ..losses.motion_loss import motion_consistency_loss, motion_smoothness_loss_fn, motion_sparsity_loss_fn, rgbd_consistency_loss
from ..losses.smoothness_loss import smoothness_loss
from ..losses.ssim_loss import WeightedSSIM
from ..pose_net import build_pose_net
from .build import META_ARCH_REGISTRY
from .common import HipMetaArch

# One sde_motion_prep_fwd / _bwd per scale for both directions (hip.motion_loss.pair_prep) instead of the reference's chain of small operations per
# direction.  scripts/bench_motion_model.py measures both paths in one process (profiles/motion_model_bench.txt).
FUSED_PREP = True


@META_ARCH_REGISTRY.register()
class MotionLearningModel(HipMetaArch):
    def __init__(self, cfg):
        HipMetaArch.__init__(self, cfg)
        self.pose_net = build_pose_net(cfg)
        loss = cfg.LOSS
        self.num_scales = loss.NUM_SCALES
        self.depth_l1_loss_w = loss.DEPTH_L1_WEIGHT
        self.ssim_loss_w = loss.SSIM_WEIGHT
        self.ssim = WeightedSSIM(loss.C1, loss.C2)
        self.clip_loss = loss.CLIP
        self.smooth_loss_w = loss.SMOOTHNESS_WEIGHT
        self.sup_loss_w = loss.SUPERVISED_WEIGHT
        self.supervise_loss = silog_loss(loss.VARIANCE_FOCUS)
        self.var_loss_w = loss.VAR_LOSS_WEIGHT
        self.motion_smooth_loss_w = loss.MOTION_SMOOTHNESS_WEIGHT
        self.motion_sparsity_loss_w = loss.MOTION_SPARSITY_WEIGHT
        self.rot_cycle_loss_w = loss.ROT_CYCLE_WEIGHT
        self.trans_cycle_loss_w = loss.TRANS_CYCLE_WEIGHT
        self.scale_normalize = loss.SCALE_NORMALIZE
        self.pose_use_depth = cfg.MODEL.POSE_NET.USE_DEPTH
        self.with_mask = cfg.MODEL.get("WITH_MASK", False)
        self.mask_dilation = cfg.MODEL.get("MASK_DILATION", 8)
        self.return_loss = cfg.MODEL.get("RETURN_LOSS", False)

    def forward(self, batch):
        if not (self.training or self.return_loss):
            # the reference returns the whole batch with depth_pred as a list (MotionLearning.py:L243-246), which its evaluators can only use at batch
            # size 1; like the other two meta-architectures this one returns the full-resolution map
            batch = self.run_depth_net(batch)
            return {"depth_pred": batch["depth_pred"][0]}
        batch = to_cuda(batch, self.device)
        frame1, frame2 = batch["img"], batch["ctx_img"][0]
        B = frame1.shape[0]
        frames = torch.cat([frame1, frame2], 0)                                           # [2B,3,H,W]: frame A of the stacked directions
        frames_sw = torch.cat([frame2, frame1], 0)                                        # frame B
        batch["depth_net_input_nhwc"] = HN.prep_input(frames, self.pixel_mean, self.pixel_std, self.depth_net.dtype, False)   # L83-84
        batch = self.depth_net(batch)
        depth = batch["depth_pred"][0]                                                    # [2B,1,H,W]: depth1 | depth2
        if self.pose_use_depth:
            a = torch.cat([frames, depth], 1)                                             # the depth channels carry the gradient into the depth net
            batch["pose_net_input"] = torch.cat([a, torch.cat([a[B:], a[:B]], 0)], 1)     # L90-98: (1, 2) | (2, 1)
        else:
            batch["pose_net_input"] = torch.cat([frames, frames_sw], 1)
        batch = self.pose_net(batch)
        return self.losses_from_predictions(batch, frames, frames_sw, depth, batch["pose_pred"], batch.get("motion_pred"))

    def losses_from_predictions(self, batch, frames, frames_sw, depth, pose, motion):
        """MotionLearning.py:L102-241 from the stacked predictions: depth [2B,1,H,W], pose [2B,4,4], motion [2B,3,H,W] or None."""
        N = frames.shape[0]
        B = N // 2
        mask01 = None
        if motion is not None and self.with_mask:                                         # L108-116
            mask01 = HM.dilate_mask(torch.cat([batch["mask"], batch["ctx_mask"][0]], 0), self.mask_dilation)
        R = pose[:, :3, :3].contiguous()
        t_pose = pose[:, :3, 3].contiguous()
        K = batch["intrinsics"].float()
        K = torch.cat([K, K], 0)
        H0, W0 = depth.shape[-2:]
        cycle = self.rot_cycle_loss_w > 0 or self.trans_cycle_loss_w > 0
        R_sw = torch.cat([R[B:], R[:B]], 0) if cycle else None
        batch["depth_proximity_weight"], batch["overall_motion"] = [], []
        terms = {}                                                                        # loss name -> ([0-d tensors], [weights]), in the reference's order

        def add(name, value, weight):
            vals, ws = terms.setdefault(name, ([], []))
            vals.append(value); ws.append(weight)

        sizes = [(int(H0 * (1.0 / 2 ** i)), int(W0 * (1.0 / 2 ** i))) for i in range(self.num_scales)]
        # the frames' pyramid needs neither network: built once, for both operand orders
        pyramid = [(resize_img_avgpool(frames, s), resize_img_avgpool(frames_sw, s)) for s in sizes]
        for i in reversed(range(self.num_scales)):
            scale_w = 1.0 / 2 ** i
            h, w = sizes[i]
            fA, fB = pyramid[i]
            Ks = K.clone()
            Ks[:, :2] *= scale_w                                                          # scale_intrinsics(K, scale_w, scale_w): fx, fy, cx, cy
            if FUSED_PREP:
                p = HM.pair_prep(depth, motion, t_pose, mask01, (h, w), self.scale_normalize)
            else:
                p = self._composed_prep(depth, motion, t_pose, mask01, (h, w))
            depth_r, depth_n, t, m_norm = p["depth_r"], p["depth_n"], p["t"], p["m_norm"]
            batch["overall_motion"].append((p["overall_motion"][:B], p["overall_motion"][B:]))
            o = rgbd_consistency_loss(fA, fB, depth_n, p["depth_n_sw"], Ks, R, t, depth_l1_w=self.depth_l1_loss_w, ssim_w=self.ssim_loss_w,
                                      C1=self.ssim.C1, C2=self.ssim.C2)
            for k in ("depth_l1_loss", "rgb_l1_loss", "ssim_loss"):                       # merge_loss: the sum of the two directions = 2 x the stacked mean
                if k in o:
                    add(k, o[k], 2.0 * scale_w)
            dpw = o.get("depth_proximity_weight")
            batch["depth_proximity_weight"].append((dpw[:B], dpw[B:]) if dpw is not None else (None, None))
            if cycle:
                rot, trans = motion_consistency_loss(o["coords_A_in_B"], o["occlusion_mask"], R, R_sw, t, p["t_sw"])
                add("rot_loss", rot, 2.0 * scale_w * self.rot_cycle_loss_w)
                add("trans_loss", trans, 2.0 * scale_w * self.trans_cycle_loss_w)
            if motion is not None:
                if self.motion_smooth_loss_w > 0.0:
                    add("motion_smooth_loss", motion_smoothness_loss_fn(m_norm), 2.0 * scale_w * self.motion_smooth_loss_w)
                if self.motion_sparsity_loss_w > 0.0:
                    add("motion_sparsity_loss", motion_sparsity_loss_fn(m_norm), 2.0 * scale_w * self.motion_sparsity_loss_w)
            if self.sup_loss_w > 0.0:
                # SILog is not linear in the batch: one call per frame; the nearest resize of the ground truth happens inside the loss kernel
                add("sup_loss", self.supervise_loss(depth_r[:B], batch["depth"]), scale_w * self.sup_loss_w)
                add("sup_loss", self.supervise_loss(depth_r[B:], batch["ctx_depth"][0]), scale_w * self.sup_loss_w)
            if self.smooth_loss_w > 0.0:
                add("smooth_loss", smoothness_loss(depth_n, fA), 2.0 * scale_w * self.smooth_loss_w)
            if self.var_loss_w > 0.0:
                add("var_loss", variance_loss(depth_r[:B]), scale_w * self.var_loss_w)
                add("var_loss", variance_loss(depth_r[B:]), scale_w * self.var_loss_w)
        for name, (vals, ws) in terms.items():
            batch[name] = self._weighted_sum(vals, ws)
        return batch

    def _composed_prep(self, depth, motion, t_pose, mask01, size):
        """The same quantities as hip.motion_loss.pair_prep from the operators the package already had: resize_img_avgpool and torch glue, one call per
        direction (MotionLearning.py:L126-166, L205-208)."""
        B = depth.shape[0] // 2
        h, w = size
        halves = lambda v: (v[:B], v[B:])
        d1, d2 = (resize_img_avgpool(d, size) for d in halves(depth))
        ts = [tp[:, :, None, None] for tp in halves(t_pose)]
        ms = [None, None]
        if motion is not None:
            mm = motion * mask01 if mask01 is not None else motion
            ms = [resize_img_avgpool(m.contiguous(), size) for m in halves(mm)]
            ts = [tp + m for tp, m in zip(ts, ms)]
        else:
            ts = [tp.expand(-1, -1, h, w) for tp in ts]
        overall = torch.cat(ts, 0).detach()
        if self.scale_normalize:
            depth_mean = torch.mean(torch.cat([d1, d2], 0))
            n1, n2 = d1 / depth_mean, d2 / depth_mean
            ts = [tv / depth_mean for tv in ts]
            if motion is not None:
                ms = [m / depth_mean for m in ms]
        else:
            n1, n2 = d1, d2
        m_norm = None
        if motion is not None:
            m_norm = torch.cat([m / torch.sqrt(tv.pow(2).mean([1, 2, 3], keepdim=True) * 3.0 + 1e-12) for m, tv in zip(ms, ts)], 0)
        depth_r = torch.cat([d1, d2], 0)
        depth_n = torch.cat([n1, n2], 0) if self.scale_normalize else depth_r
        return {"depth_r": depth_r, "depth_n": depth_n, "t": torch.cat(ts, 0).contiguous(), "m_norm": m_norm, "t_sw": torch.cat(ts[::-1], 0).contiguous(),
                "depth_n_sw": torch.cat([n2, n1], 0).detach(), "overall_motion": overall}

"""DepthPredictor: a trained model on raw camera frames (what the reference's tools/demo.py:L42-104 does per frame), without host round trips.

The reference loads a frame, runs the CPU preprocess chain, the model, copies the prediction to the host, undoes the chain with numpy and renders
the picture with matplotlib.  Here the uint8 frame is uploaded from pinned memory and everything after that is device work on one stream:

    sde_image_prep_u8     the forward chain (KBCrop / CropTopTo / Resize + ToTensor) as two tap tables: a crop is an offset added to the taps,
                          an axis that is not resized gets identity taps (i, i, 2048, 0) -- the fixed-point rule then returns the source byte;
    model(batch)          eval mode, torch.no_grad();
    sde_depth_present     the backward chain as the two index maps of evaluation.depth_evaluation.backward_maps, the restored depth, the 16-bit
                          depth and the coloured, frame-stacked picture in one launch (hip/present.py);
    sde_depth_cloud       on request (cloud=dict(min_depth=, max_depth=, step=1)): the restored depth lifted through the source-size intrinsics
                          into a compacted list of coloured 16-byte points per frame, three launches behind the present kernel (hip/cloud.py).

The three stages are captured once per (source size, batch size) into a graph and replayed; `stream` adds a copy stream that uploads the next
frame and downloads the previous picture while the current frame is computed.

PairPredictor (below) runs a model that has a pose network on a window of frames: the same chain, plus the pose network and sde_pair_flow, the
relative camera poses and the dense optical flow they imply with the target's depth (hip/flow.py)."""
import numpy as np
import torch

from ..data.device_aug import DeviceImageAug
from ..data.preprocess.augmentation import _linear_coefs
from ..evaluation.depth_evaluation import backward_maps
from ..geometry.pose_utils import invert_pose_np
from ..hip import cloud as HC
from ..hip import flow as HF
from ..hip import present as HP
from ..hip import temporal as HT
from ..hip.align import AlignState, unpack_state

IMAGE_STEPS = ("KBCrop", "CropTopTo", "Resize")       # the steps with a backward(): DatasetEvaluator.preprocess_chain keeps the same three
KB_H, KB_W = 352, 1216


def _step_name(s):
    return s if isinstance(s, str) else (s["NAME"] if isinstance(s, dict) else s.NAME)


def chain_steps(cfg, chain=None):
    """[(name, step config)] of the predictor's chain.  chain: step names (the form of DatasetEvaluator.preprocess_chain) or step dicts; None: the
    image steps of cfg.DATASETS.TEST.PREPROCESS, ("KBCrop",) when it has none (demo.py:L43).  A name takes its sizes from the config's step."""
    configured = []
    if cfg is not None and "DATASETS" in cfg and "TEST" in cfg.DATASETS:
        configured = [dict(s) for s in cfg.DATASETS.TEST.get("PREPROCESS", [])]
    if chain is None:
        chain = [s for s in configured if _step_name(s) in IMAGE_STEPS] or ["KBCrop"]
    steps = []
    for s in chain:
        name = _step_name(s)
        if name not in IMAGE_STEPS:
            raise ValueError(f"DepthPredictor: chain step {name!r} is not one of {IMAGE_STEPS}")
        if isinstance(s, str):
            s = next((c for c in configured if c["NAME"] == name), {"NAME": name})
        steps.append((name, dict(s)))
    return steps


def _identity_taps(n):
    i = np.arange(n, dtype=np.int64)
    return np.stack([i, i, np.full(n, 2048, np.int64), np.zeros(n, np.int64)], 1)


def _resize_taps(src, dst):
    return _identity_taps(src) if src == dst else np.stack(_linear_coefs(src, dst), 1)


class SizePlan:
    """Everything the predictor derives from one source size: the tap tables of the forward chain (int32 [w][4] / [h][4], taps in source
    coordinates), the network input size, the metadata the chain's steps record, and how they move the intrinsics."""

    def __init__(self, steps, Hs, Ws):
        self.Hs, self.Ws, self.chain = int(Hs), int(Ws), tuple(n for n, _ in steps)
        self.meta, self.k_ops = {}, []
        h, w, oy, ox, ytab, xtab = self.Hs, self.Ws, 0, 0, None, None

        def crop(y0, nh, x0, nw):
            nonlocal h, w, oy, ox, ytab, xtab
            if y0 < 0 or x0 < 0 or y0 + nh > h or x0 + nw > w:
                raise ValueError(f"DepthPredictor: a {nh} x {nw} crop does not fit the {h} x {w} image ({self.Hs} x {self.Ws} frames, chain {self.chain})")
            if ytab is None:
                oy, ox = oy + y0, ox + x0                           # before the resize: an offset, folded into the taps below
            else:
                ytab, xtab = ytab[y0:y0 + nh], xtab[x0:x0 + nw]      # after it: the rows and columns of the tables
            h, w = nh, nw

        for name, cfg in steps:
            if name == "KBCrop":
                x0, y0 = int((w - KB_W) / 2), int(h - KB_H)
                self.meta.update(kb_y_start=y0, kb_x_start=x0, h_before_kb_crop=h, w_before_kb_crop=w)
                crop(y0, KB_H, x0, KB_W)
                self.k_ops.append(("shift", x0, y0))
            elif name == "CropTopTo":
                y0 = int(h - int(cfg["IMG_H"]))
                self.meta.update(crop_y_start=y0, h_before_crop=h, w_before_crop=w)
                crop(y0, h - y0, 0, w)
                self.k_ops.append(("shift", 0, y0))
            else:
                if ytab is not None:
                    raise ValueError("DepthPredictor: two Resize steps do not compose into one 2-tap table")
                th, tw = int(cfg["IMG_H"]), int(cfg["IMG_W"])
                self.meta.update(h_before_resize=h, w_before_resize=w)
                ytab, xtab = _resize_taps(h, th), _resize_taps(w, tw)
                ytab[:, :2] += oy
                xtab[:, :2] += ox
                self.k_ops.append(("scale", tw / w, th / h))
                h, w = th, tw
        if ytab is None:
            ytab, xtab = _identity_taps(h), _identity_taps(w)
            ytab[:, :2] += oy
            xtab[:, :2] += ox
        self.h, self.w = h, w
        self.ytab, self.xtab = np.ascontiguousarray(ytab, dtype=np.int32), np.ascontiguousarray(xtab, dtype=np.int32)
        self._maps = {}

    def maps(self, pred_hw):
        """(ymap [Hs], xmap [Ws]) int32 host arrays for a network output of size pred_hw: backward_maps of the recorded metadata."""
        pred_hw = (int(pred_hw[0]), int(pred_hw[1]))
        if pred_hw not in self._maps:
            rows, cols = backward_maps(pred_hw, self.meta, self.chain)
            if (rows.size, cols.size) != (self.Hs, self.Ws):
                raise ValueError(f"DepthPredictor: chain {self.chain} restores {rows.size} x {cols.size}, the frames are {self.Hs} x {self.Ws}")
            self._maps[pred_hw] = (np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(cols, dtype=np.int32))
        return self._maps[pred_hw]

    def intrinsics(self, K):
        """K [3,3] or [N,3,3] as the forward steps leave it (KBCrop / CropTopTo move the principal point, Resize scales), in K's own dtype."""
        K = np.array(K.cpu().numpy() if torch.is_tensor(K) else K, copy=True)
        if not np.issubdtype(K.dtype, np.floating):
            K = K.astype(np.float64)
        for op, a, b in self.k_ops:
            if op == "shift":
                K[..., 0, 2] -= a
                K[..., 1, 2] -= b
            else:
                K[..., 0, 0] *= a; K[..., 0, 2] *= a
                K[..., 1, 1] *= b; K[..., 1, 2] *= b
        return K


class _Slot:
    """One set of pinned and device buffers for N frames of one size, and the graph that runs on them."""

    def __init__(self, N, Hs, Ws, device):
        self.frames_pin = torch.empty((N, Hs, Ws, 3), dtype=torch.uint8).pin_memory()
        self.frames = torch.empty((N, Hs, Ws, 3), dtype=torch.uint8, device=device)
        self.K = None                # [N,3,3] float32 device tensor once intrinsics are used
        self.K_host = None
        self.K_src = None            # [N,3,3] float32 device tensor: the intrinsics as given (source size), for the point cloud
        self.K_src_host = None
        self.graphs = {}             # (present, frame_in_canvas, want_u16, has K) -> (graph, outputs)
        self.host = {}               # name -> pinned host tensor of the downloaded output
        self.uploaded = torch.cuda.Event()
        self.computed = torch.cuda.Event()
        self.downloaded = torch.cuda.Event()
        self.out = None


class _Predictor:
    """What DepthPredictor and PairPredictor share: the model, the chain's per-size tables, the slots of pinned and device buffers, eager run or
    graph capture and replay, and the two-slot pipeline behind `stream`."""
    NAME = "DepthPredictor"

    def __init__(self, cfg, model=None, chain=None, device="cuda", use_graph=None, vmax=None, gamma=0.8):
        self.cfg = cfg
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if model is None:
            from ..checkpoint.checkpoint import DetectionCheckpointer
            from ..modeling import build_model
            model = build_model(cfg)
            if cfg.MODEL.WEIGHTS:
                DetectionCheckpointer(model).load(cfg.MODEL.WEIGHTS)
        self.model = model.to(self.device).eval()
        self.steps = chain_steps(cfg, chain)
        self.vmax = float(cfg.MODEL.MAX_DEPTH if vmax is None else vmax)
        self.gamma = float(gamma)
        if not (self.vmax > 0 and self.gamma > 0):
            raise ValueError(f"{self.NAME}: vmax and gamma must be positive ({self.vmax}, {self.gamma})")
        self.use_graph = (self.device.type == "cuda") if use_graph is None else bool(use_graph)
        self._aug = DeviceImageAug(self.device)
        self._plans, self._dev_maps, self._params, self._slots = {}, {}, {}, {}
        self._copy_stream = None

    # ---- per-size tables ------------------------------------------------------------------------------------------------------------------
    def plan(self, Hs, Ws):
        key = (int(Hs), int(Ws))
        if key not in self._plans:
            self._plans[key] = SizePlan(self.steps, *key)
        return self._plans[key]

    def _maps_on_device(self, plan, pred_hw):
        key = (plan.Hs, plan.Ws, int(pred_hw[0]), int(pred_hw[1]))
        if key not in self._dev_maps:
            self._dev_maps[key] = HP.device_maps(*plan.maps(pred_hw), key[2], key[3], self.device)       # validated on the host, once
        return self._dev_maps[key]

    def _no_jitter(self, N):
        if N not in self._params:
            p = torch.tensor([1.0, 1.0, 1.0, 0.0, -1.0, -1.0, -1.0, -1.0], dtype=torch.float32).repeat(N, 1)
            self._params[N] = p.to(self.device)
        return self._params[N]

    def _slot(self, N, plan, i=0):
        key = (N, plan.Hs, plan.Ws, i)
        if key not in self._slots:
            if len(self._slots) >= 16:          # a handful of source sizes per dataset: anything more is a leak, start over
                torch.cuda.synchronize(self.device)
                self._slots.clear()
            self._slots[key] = _Slot(N, plan.Hs, plan.Ws, self.device)
        return self._slots[key]

    def _device_copy(self, slot, field, value, N):
        """The slot's device copy `field` ("K": the intrinsics at the network's size, plan.intrinsics applied by the caller; "K_src": as given, at
        the source size, for the point cloud and the flow) of the host intrinsics `value` ([3,3] or [N,3,3]), refreshed when they change;
        None without any."""
        if value is None:
            return None
        value = np.array(np.broadcast_to(np.asarray(value, dtype=np.float32), (N, 3, 3)))          # a copy: broadcast views are read-only
        if getattr(slot, field) is None:
            setattr(slot, field, torch.empty((N, 3, 3), dtype=torch.float32, device=self.device))
        if getattr(slot, field + "_host") is None or not np.array_equal(getattr(slot, field + "_host"), value):
            getattr(slot, field).copy_(torch.from_numpy(value))
            setattr(slot, field + "_host", value)
        return getattr(slot, field)

    @staticmethod
    def _host_K(name, intrinsics, N):
        """intrinsics [3,3] or [N,3,3] (array or tensor) -> a float32 [N,3,3] host copy; ValueError unless finite with non-zero focal lengths."""
        K = np.asarray(intrinsics.cpu().numpy() if torch.is_tensor(intrinsics) else intrinsics, dtype=np.float32)
        if K.shape not in ((3, 3), (N, 3, 3)) or not (np.all(np.isfinite(K)) and np.all(K[..., 0, 0] != 0) and np.all(K[..., 1, 1] != 0)):
            raise ValueError(f"{name}: intrinsics must be a finite [3,3] or [{N},3,3] matrix with non-zero focal lengths")
        return np.array(np.broadcast_to(K, (N, 3, 3)))

    def _replay(self, slot, key, chain, persistent=()):
        """chain() on the current stream: eager, or the slot's graph of that key (captured at first use, after one eager run).  persistent:
        tensors the chain updates in place from run to run; the eager run before the capture must not count as a step, so they are put back
        to what they held before it."""
        if not self.use_graph:
            return chain()
        if key not in slot.graphs:
            cur = torch.cuda.current_stream()
            saved = [t.clone() for t in persistent]
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):           # tables, caches and the allocator's blocks come into being here, outside the capture
                chain()
            cur.wait_stream(side)
            torch.cuda.synchronize(self.device)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                out = chain()
            for t, keep in zip(persistent, saved):
                t.copy_(keep)
            slot.graphs[key] = (graph, out)
        graph, out = slot.graphs[key]
        graph.replay()
        return out

    @staticmethod
    def _as_frames(frames):
        """One frame or N of one size -> (uint8 [N,H,W,3] tensor, host or device; whether a single frame came in)."""
        if isinstance(frames, (list, tuple)):
            frames = np.stack([f.cpu().numpy() if torch.is_tensor(f) else np.asarray(f) for f in frames], 0)
        t = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames))
        single = t.dim() == 3
        if single:
            t = t[None]
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3:
            raise ValueError(f"DepthPredictor: frames must be uint8 [H,W,3] or [N,H,W,3] RGB, got {t.dtype} {tuple(t.shape)}")
        return t.contiguous(), single

    def _upload(self, slot, t):
        """Frames t (uint8 [N,H,W,3], host or device) into the slot's device buffer, on the current stream."""
        if t.is_cuda:
            slot.frames.copy_(t)
        else:
            slot.uploaded.synchronize()              # the pinned buffer's previous upload has left it
            slot.frames_pin.copy_(t)
            slot.frames.copy_(slot.frames_pin, non_blocking=True)
            slot.uploaded.record()

    # ---- streaming ------------------------------------------------------------------------------------------------------------------------
    def _download(self, slot, names):
        """Enqueue, on the copy stream, the device -> pinned host copies of the slot's outputs once its compute has finished."""
        cs = self._copy_stream
        cs.wait_event(slot.computed)
        with torch.cuda.stream(cs):
            for k in names:
                v = slot.out[k]
                if v is None:
                    continue
                h = slot.host.get(k)
                if h is None or h.shape != v.shape or h.dtype != v.dtype:
                    h = slot.host[k] = torch.empty(v.shape, dtype=v.dtype).pin_memory()
                h.copy_(v, non_blocking=True)
            slot.downloaded.record(cs)

    def _pump(self, items, names, run, result):
        """The two-slot pipeline behind `stream`.  items: host uint8 tensors [N,H,W,3], one per result; run(slot, plan) enqueues the chain on the
        slot's buffers and returns its outputs; result(slot, names) turns the downloaded outputs into what is yielded.  While item i is computed
        on the current stream, the copy stream uploads item i+1 and downloads the outputs of item i-1; result i-1 is yielded once item i is
        enqueued.  An item of another size drains the slots and switches tables.  No threads."""
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=self.device)
        cs = self._copy_stream
        pending, size, i = None, None, 0
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream()
            for t in items:
                if size is not None and tuple(t.shape) != size and pending is not None:
                    self._download(pending, names)                      # another size: drain what is in flight, then switch tables
                    yield result(pending, names)
                    pending = None
                size = tuple(t.shape)
                plan = self.plan(size[1], size[2])
                slot = self._slot(size[0], plan, i % 2)
                i += 1
                # upload item i: its pinned buffer was last read by the upload of item i-2 and its device buffer by the compute of item i-2,
                # whose result has been yielded -- both are over
                slot.frames_pin.copy_(t)
                cs.wait_event(slot.computed)
                with torch.cuda.stream(cs):
                    slot.frames.copy_(slot.frames_pin, non_blocking=True)
                    slot.uploaded.record(cs)
                if pending is not None:
                    self._download(pending, names)                      # behind the upload on the copy stream, beside this item's compute
                cur.wait_event(slot.uploaded)
                cur.wait_event(slot.downloaded)                         # the slot's outputs of item i-2 have left the device
                slot.out = run(slot, plan)
                slot.computed.record(cur)
                if pending is not None:
                    yield result(pending, names)
                pending = slot
            if pending is not None:
                self._download(pending, names)
                yield result(pending, names)


class DepthPredictor(_Predictor):
    # ---- the device chain -----------------------------------------------------------------------------------------------------------------
    def _chain(self, plan, frames, K, present, frame_in_canvas, want_u16, cloud=None, K_src=None):
        """frames: uint8 [N,Hs,Ws,3] on the device, K: [N,3,3] float32 on the device or None; cloud: (min_depth, max_depth, step) or None, K_src: the
        source-size intrinsics the cloud uses.  Everything on the current stream, nothing synchronises once the tables of this size are on the
        device (the first call of a size puts them there)."""
        N = frames.shape[0]
        img, _ = self._aug.prep(frames, self._no_jitter(N), plan.h, plan.w, tabs=(plan.xtab, plan.ytab))
        batch = {"img": img}
        if K is not None:
            batch["intrinsics"] = K
        with torch.no_grad():
            pred = self.model(batch)["depth_pred"]
        pred = pred.detach().float()
        if pred.dim() == 4:
            pred = pred[:, 0]
        pred = pred.contiguous()
        out = {"depth_net": pred, "depth": None, "canvas": None, "depth_u16": None}
        if present:
            ymap, xmap = self._maps_on_device(plan, pred.shape[-2:])
            out["canvas"], out["depth"], out["depth_u16"] = HP.depth_present(pred, ymap, xmap, self.vmax, self.gamma, frame=frames if frame_in_canvas else None,
                                                                             want_depth=True, want_u16=want_u16)
        if cloud is not None:
            ymap, xmap = self._maps_on_device(plan, pred.shape[-2:])
            out["points"], out["count"] = HC.depth_cloud(pred, ymap, xmap, K_src, *cloud, frame=frames)
        return out

    @staticmethod
    def _cloud_args(cloud, intrinsics, N):
        """cloud=None -> (None, None); a dict -> ((min_depth, max_depth, step), the source-size K as a float32 [N,3,3] host array).  ValueError for
        a cloud without intrinsics, unknown keys, an empty depth range, step < 1 or a zero focal length; nothing here touches the device."""
        if cloud is None:
            return None, None
        if not isinstance(cloud, dict) or not {"min_depth", "max_depth"} <= set(cloud) <= {"min_depth", "max_depth", "step"}:
            raise ValueError(f"DepthPredictor: cloud must be None or dict(min_depth=..., max_depth=..., step=1), got {cloud!r}")
        args = HC.check_range(cloud["min_depth"], cloud["max_depth"], cloud.get("step", 1))
        if intrinsics is None:
            raise ValueError("DepthPredictor: cloud needs intrinsics (the source-size K [3,3] or [N,3,3] of the frames)")
        return args, _Predictor._host_K("DepthPredictor", intrinsics, N)

    def _run(self, slot, plan, K, flags, cloud=None, K_src=None):
        """The chain on the slot's buffers, on the current stream: eager, or the slot's graph (captured at first use, after one eager run)."""
        key = flags + (K is not None,) + ((cloud,) if cloud is not None else ())       # without a cloud: the key of before
        return self._replay(slot, key, lambda: self._chain(plan, slot.frames, K, *flags, cloud=cloud, K_src=K_src))

    def predict(self, frames, intrinsics=None, present=True, frame_in_canvas=True, want_u16=False, cloud=None):
        """frames: one uint8 [H,W,3] RGB array / tensor, or N of one size.  Returns a dict of device tensors: `depth` [N,H,W] (the prediction restored
        to the frame's size; None with present=False), `depth_net` [N,h,w] (the network output), `canvas` [N,2H or H,W,3] uint8, `depth_u16` with
        want_u16 (int16 tensor holding write_depth's uint16 bits).  A single frame keeps the leading 1.  cloud=dict(min_depth=, max_depth=, step=1)
        adds `points` [N,cap,16] uint8 and `count` [N] int32 (hip.cloud.depth_cloud of the restored depth, the frames' colours and `intrinsics` as
        given, which it then requires; hip.cloud.as_records reads them on the host).  No host synchronisation after the first call of a size."""
        t, _ = self._as_frames(frames)
        N, Hs, Ws, _ = t.shape
        cloud, K_cloud = self._cloud_args(cloud, intrinsics, N)
        plan = self.plan(Hs, Ws)
        slot = self._slot(N, plan)
        flags = (bool(present), bool(frame_in_canvas), bool(want_u16))
        with torch.cuda.device(self.device):
            self._upload(slot, t)
            K = self._device_copy(slot, "K", None if intrinsics is None else plan.intrinsics(intrinsics), N)
            out = self._run(slot, plan, K, flags, cloud, self._device_copy(slot, "K_src", K_cloud, N))
            # the slot's tensors are written again by the next call: hand out copies
            return {k: (v.clone() if v is not None else None) for k, v in out.items()}

    def _result(self, slot, names):
        slot.downloaded.synchronize()
        res = {k: (slot.host[k].numpy() if k in ("points", "count") else slot.host[k].numpy()[0]) for k in names if slot.out[k] is not None}
        if "depth_u16" in res:
            res["depth_u16"] = res["depth_u16"].view(np.uint16)
        return res

    def stream(self, frames_iter, intrinsics=None, present=True, frame_in_canvas=True, want_u16=False, cloud=None):
        """Generator over host frames (uint8 [H,W,3] RGB, one at a time): yields, in order, a dict of host arrays per frame -- `depth` [H,W] fp32,
        `canvas` [2H or H,W,3] uint8, `depth_u16` with want_u16; with present=False only `depth_net` [h,w].  The arrays are views of pinned buffers and stay valid until the next
        iteration.  Two slots of pinned and device buffers: while frame i is computed on the current stream, the copy stream uploads frame i+1 and
        downloads the outputs of frame i-1; result i-1 is yielded once frame i is enqueued.  A frame of another size drains the slots and switches
        tables.  No threads.  cloud (see predict) adds `points` [1,cap,16] uint8 and `count` [1] int32, the whole buffer downloaded like the other
        outputs: hip.cloud.as_records(res["points"], res["count"])[0] is the frame's cloud."""
        cloud, K_cloud = self._cloud_args(cloud, intrinsics, 1)
        flags = (bool(present), bool(frame_in_canvas), bool(want_u16))
        names = [k for k, on in (("depth", present), ("canvas", present), ("depth_u16", present and want_u16), ("depth_net", not present),
                                 ("points", cloud is not None), ("count", cloud is not None)) if on]

        def items():
            for frame in frames_iter:
                t, _ = self._as_frames(frame)
                if t.is_cuda or t.shape[0] != 1:
                    raise ValueError("DepthPredictor.stream takes one host frame [H,W,3] per item")
                yield t

        def run(slot, plan):
            K = self._device_copy(slot, "K", None if intrinsics is None else plan.intrinsics(intrinsics), 1)
            return self._run(slot, plan, K, flags, cloud, self._device_copy(slot, "K_src", K_cloud, 1))
        yield from self._pump(items(), names, run, self._result)


# ---- frame pairs: ego-motion and optical flow ------------------------------------------------------------------------------------------------
PAIR_ARCHS = ("MonoDepth2Model", "MotionLearningModel")
SINGLE_CONTEXT_NETS = ("GooglePoseNet", "GoogleMotionNet")


def window_offsets(cfg):
    """The frame offsets of the model's context frames relative to the target, in the order the dataset emits `ctx_img`: ascending from
    -BACKWARD_CONTEXT * STRIDE to +FORWARD_CONTEXT * STRIDE without 0 (DATASETS.TRAIN, data/datasets/kitti_v2.py).  Their number must be the
    pose network's: MODEL.POSE_NET.NUM_CONTEXTS for PoseNet, 1 for GooglePoseNet / GoogleMotionNet.  A config without the three keys gets the
    projects' layouts: (+1,) for one context, (-1, +1) for two.  ValueError for a meta-architecture without a pose network."""
    arch = cfg.MODEL.META_ARCHITECTURE
    if arch not in PAIR_ARCHS:
        raise ValueError(f"PairPredictor: {arch} has no pose network (pose_net); use DepthPredictor for depth alone")
    n = 1 if cfg.MODEL.POSE_NET.NAME in SINGLE_CONTEXT_NETS else int(cfg.MODEL.POSE_NET.NUM_CONTEXTS)
    train = cfg.DATASETS.TRAIN if "DATASETS" in cfg and "TRAIN" in cfg.DATASETS else {}
    back, fwd, stride = (int(train.get(k, 0)) for k in ("BACKWARD_CONTEXT", "FORWARD_CONTEXT", "STRIDE"))
    if back == 0 and fwd == 0:
        if n not in (1, 2):
            raise ValueError(f"PairPredictor: {n} context frames need DATASETS.TRAIN.BACKWARD_CONTEXT / FORWARD_CONTEXT / STRIDE")
        return (1,) if n == 1 else (-1, 1)
    if stride <= 0:
        raise ValueError("PairPredictor: DATASETS.TRAIN.STRIDE must be positive when BACKWARD_CONTEXT / FORWARD_CONTEXT ask for context frames")
    offsets = tuple(o for o in range(-back * stride, fwd * stride + 1, stride) if o != 0)
    if len(offsets) != n:
        raise ValueError(f"PairPredictor: the dataset emits {len(offsets)} context frames {offsets}, the pose network takes {n}")
    return offsets


def next_context(offsets):
    """Which context gives the pose target -> next frame: (index into the contexts, whether that pose has to be inverted).  The context at
    +STRIDE when there is one, else the one at -STRIDE inverted (STRIDE: the smallest distance among the offsets)."""
    stride = min(abs(o) for o in offsets)
    if stride in offsets:
        return offsets.index(stride), False
    return offsets.index(-stride), True


def temporal_context(offsets):
    """The context whose pose steps the temporal fusion from one frame to the next: next_context(offsets), which must lie one frame away."""
    j, inverted = next_context(offsets)
    if abs(offsets[j]) != 1:
        raise ValueError(f"PairPredictor: temporal fusion needs a context one frame away, the model's context offsets are {tuple(offsets)}")
    return j, inverted


def temporal_args(temporal):
    """temporal=None -> None; dict(alpha=0.5, tol=0.05) (either key may be left out) -> (alpha, tol) as the kernel receives them."""
    if temporal is None:
        return None
    if not isinstance(temporal, dict) or not set(temporal) <= {"alpha", "tol"}:
        raise ValueError(f"PairPredictor: temporal must be None or dict(alpha=0.5, tol=0.05), got {temporal!r}")
    return HT.check_params(temporal.get("alpha", 0.5), temporal.get("tol", 0.05))


class _TemporalState:
    """What the temporal fusion keeps on the device from one window to the next, for one network size: the fused depth of the last target, the
    pose (and motion field) that carries it into the next target, and the z-buffer.  The graphs of both slots read and write these tensors."""

    def __init__(self, h, w, with_motion, device):
        self.depth = torch.zeros((1, h, w), dtype=torch.float32, device=device)
        self.eye = torch.eye(4, dtype=torch.float32, device=device)[None].contiguous()
        self.T = self.eye.clone()
        self.motion = torch.zeros((1, 3, h, w), dtype=torch.float32, device=device) if with_motion else None
        self.zbuf = torch.empty((1, h, w), dtype=torch.int32, device=device)

    def tensors(self):
        return [t for t in (self.depth, self.T, self.motion) if t is not None]

    def reset(self):
        """An empty state, on the current stream: a depth of zeros scatters nothing, so the next window comes out as it was predicted."""
        self.depth.zero_()
        self.T.copy_(self.eye)
        if self.motion is not None:
            self.motion.zero_()


def volume_arg(volume, device=None):
    """volume=None -> None; else the hip.volume.TsdfVolume itself, which must live on the predictor's device."""
    if volume is None:
        return None
    from ..hip.volume import TsdfVolume
    if not isinstance(volume, TsdfVolume):
        raise ValueError(f"PairPredictor: volume must be None or a hip.volume.TsdfVolume, got {type(volume).__name__}")
    if device is not None and volume.device != device:
        raise ValueError(f"PairPredictor: the volume lives on {volume.device}, the predictor on {device}")
    return volume


def render_arg(render, volume):
    """render=None -> None; else dict(normals=True, picture=True, min_weight=1, near=None, far=None, step=None), the arguments of
    hip.volume.TsdfVolume.render, checked against the volume -> (normals, picture, min_weight, near, far, step): part of the replay key."""
    if render is None:
        return None
    if volume is None:
        raise ValueError("PairPredictor: render= shows the volume the sequence is fused into, it needs volume=TsdfVolume(...)")
    known = ("normals", "picture", "min_weight", "near", "far", "step")
    if not isinstance(render, dict) or set(render) - set(known):
        raise ValueError(f"PairPredictor: render must be None or a dict with keys from {known}, got {render!r}")
    from ..hip.volume import check_min_weight, check_render
    normals, picture = bool(render.get("normals", True)), bool(render.get("picture", True))
    if picture and not volume.colour:
        raise ValueError("PairPredictor: render=dict(picture=True) needs a volume with colour; pass picture=False")
    near, far, step = (float(np.float32(d if render.get(k) is None else render[k])) for k, d in (("near", volume.min_depth), ("far", volume.max_depth),
                                                                                                ("step", volume.voxel)))
    check_render((1, 1), near, far, step)                     # the sample count; the picture's size is checked when the first frame is seen
    return normals, picture, check_min_weight(render.get("min_weight", 1)), near, far, step


TRACK_KEYS = ("schedule", "scale", "dist_tol", "scale_tol", "min_count", "damping", "min_weight", "near", "far", "step")


def track_arg(track, volume):
    """track=None -> None; else dict(schedule=None, scale=True, dist_tol=, scale_tol=, min_count=, damping=, min_weight=1, near=, far=, step=), the
    arguments of hip.volume.TsdfVolume.track, checked against the volume -> (schedule, dist_tol, scale_tol, min_count, damping, min_weight, near,
    far, step): part of the replay key.  scale=False takes the SCALE bit out of every iteration of the schedule (the depth keeps its scale)."""
    if track is None:
        return None
    if volume is None:
        raise ValueError("PairPredictor: track= aligns every frame with the volume the sequence is fused into, it needs volume=TsdfVolume(...)")
    if not isinstance(track, dict) or set(track) - set(TRACK_KEYS):
        raise ValueError(f"PairPredictor: track must be None or a dict with keys from {TRACK_KEYS}, got {track!r}")
    from ..hip import align as AL
    from ..hip.volume import check_min_weight, check_render
    schedule = AL.DEFAULT_SCHEDULE if track.get("schedule") is None else tuple(track["schedule"])
    kw = {k: AL.DEFAULTS[k] if track.get(k) is None else track[k] for k in ("dist_tol", "scale_tol", "min_count", "damping")}
    checked = [AL.check_align(mode=m, min_depth=volume.min_depth, max_depth=volume.max_depth, **kw) for m in schedule]
    if not bool(track.get("scale", True)):
        checked = [c for c in checked if c[4] & AL.POSE]
        schedule = tuple(AL.POSE for _ in checked)
    else:
        schedule = tuple(c[4] for c in checked)
    if not schedule:
        raise ValueError(f"PairPredictor: track's schedule must name at least one iteration (with scale=False: one with the POSE bit), got {track.get('schedule')!r}")
    near, far, step = (float(np.float32(d if track.get(k) is None else track[k])) for k, d in (("near", volume.min_depth), ("far", volume.max_depth),
                                                                                              ("step", volume.voxel)))
    check_render((1, 1), near, far, step)
    dist_tol, scale_tol, min_count, damping = checked[0][:4]
    return schedule, dist_tol, scale_tol, min_count, damping, check_min_weight(track.get("min_weight", 1)), near, far, step


class _VolumeState:
    """What the volume fusion keeps on the device from one window to the next, beside the temporal state: C, the world-to-camera pose of the
    window's target (the first target of a sequence is the world), and T, the step previous target -> this one that C is advanced by before the
    window is integrated -- the form _TemporalState keeps its pose in, the identity until a window has run (`started`, for a model that only
    looks back and so brings the step into its own window along).  The graphs of both slots read and write these tensors.  `align` is the
    hip.align.AlignState of track=: scratch that every window resets, made when the first tracked window of the size runs."""

    def __init__(self, device):
        self.eye = torch.eye(4, dtype=torch.float32, device=device)
        self.C, self.T, self.inv = self.eye.clone(), self.eye.clone(), self.eye.clone()
        self.started = torch.zeros((1,), dtype=torch.bool, device=device)
        self.align = None

    def tensors(self):
        return [self.C, self.T, self.started]

    def reset(self):
        """The next window is the world, on the current stream.  The volume itself is the caller's and is left as it is."""
        self.C.copy_(self.eye)
        self.T.copy_(self.eye)
        self.started.zero_()


def as_window(frames, n):
    """A window of 1 + n frames (the target, then the contexts in `ctx_img` order; a list or one [1+n,H,W,3] array) -> uint8 [1+n,H,W,3] tensor."""
    if isinstance(frames, (list, tuple)):
        if len(frames) != 1 + n:
            raise ValueError(f"PairPredictor: a window holds the target and {n} context frame(s), got {len(frames)} frame(s)")
        shapes = {tuple(f.shape) for f in frames}
        if len(shapes) != 1:
            raise ValueError(f"PairPredictor: the frames of a window must have one size, got {sorted(shapes)}")
    t, _ = _Predictor._as_frames(frames)
    if t.shape[0] != 1 + n:
        raise ValueError(f"PairPredictor: a window holds the target and {n} context frame(s), got {t.shape[0]} frame(s)")
    return t


class PairPredictor(_Predictor):
    """A trained MonoDepth2 or MotionLearning model on a window of raw frames: depth of the target as DepthPredictor gives it, the relative
    camera pose target -> context of every context frame, and the dense optical flow those two imply.  Device work on one stream:

        sde_image_prep_u8     every frame of the window, one launch;
        depth net             on the target (MotionLearning with POSE_NET.USE_DEPTH: on target and context, whose depth the pose input carries);
        pose net              on the input the meta-architecture assembles in training: MonoDepth2 cat([img] + ctx_img, 1) of the prepared,
                              un-normalised frames; MotionLearning both directions stacked along the batch, of which target -> context is kept;
        sde_pair_flow         one launch over the n contexts: flow, validity and the wheel-coloured picture at the frame's size, from the network
                              output, the poses (and GoogleMotionNet's motion field unless rigid_only) and the source-size intrinsics;
        sde_depth_present     the target's restored depth and stacked picture.

    Captured once per (source size, flags) into a graph and replayed.  Poses and flow are up to the scale of the monocular depth.

    `stream(..., temporal=dict(alpha=0.5, tol=0.05))` makes the sequence's depth consistent over time (hip/temporal.py, sde_depth_warp_fuse): the
    fused depth of the previous target is forward-projected into the current camera with the pose the model estimated, and blended with the
    current prediction where the two agree.  With a context at +1 the pose (and, unless rigid_only, the motion field) of window k is kept on
    the device for the warp of window k + 1; a model that only looks back inverts the current window's pose to the context at -1 on the device
    and warps rigidly, because its motion field lies on the current frame's grid, not on the previous one's.  The pictures come from the fused
    map; the flow, the pose network and the depth network keep the raw prediction.  The intrinsics of the warp are the network-size ones, so
    the depth network's output must have the network's input size.

    `stream(..., volume=vol)` fuses the sequence into one TSDF volume (hip/volume.py): sde_pose_compose chains the world-to-camera pose from the
    model's step poses on the device and sde_tsdf_integrate averages every window's depth -- the one the pictures show -- into the caller's grid
    through it, inside the same graph.  With `render=dict(...)` as well, sde_tsdf_render then shows the volume from the window's own camera, and
    the record holds the model's depth, normal and colour for the frame.  With `track=dict(...)` the chained pose is corrected against the model
    before the window's depth goes in (hip/align.py: sde_frame_align, frame-to-model alignment of pose and depth scale)."""
    NAME = "PairPredictor"

    def __init__(self, cfg, model=None, chain=None, device="cuda", use_graph=None, vmax=None, gamma=0.8):
        self.offsets = window_offsets(cfg)                   # raises for a configuration without a pose network, before anything is built
        self.n = len(self.offsets)
        self.next_context = next_context(self.offsets)
        _Predictor.__init__(self, cfg, model=model, chain=chain, device=device, use_graph=use_graph, vmax=vmax, gamma=gamma)
        if not hasattr(self.model, "pose_net"):
            raise ValueError(f"PairPredictor: {type(self.model).__name__} has no pose_net; use DepthPredictor for depth alone")
        self.stacked = cfg.MODEL.POSE_NET.NAME in SINGLE_CONTEXT_NETS          # MotionLearning's both-directions input
        self.pose_use_depth = self.stacked and bool(cfg.MODEL.POSE_NET.USE_DEPTH)
        self._temporal = {}                                   # source size -> _TemporalState
        self._volume = {}                                     # source size -> _VolumeState

    def pose_input(self, img, depth_all=None):
        """The pose network's input from the prepared window img [1+n,3,h,w] (and, with USE_DEPTH, the depth [2,1,h,w] of target and context)."""
        if not self.stacked:
            return torch.cat([img[j:j + 1] for j in range(1 + self.n)], 1)                 # MonoDepth2.py: cat([img] + ctx_img, 1)
        a = torch.cat([img, depth_all], 1) if self.pose_use_depth else img                  # MotionLearning.py:L63-75: (1, 2) | (2, 1)
        return torch.cat([a, torch.cat([a[1:], a[:1]], 0)], 1)

    def _temporal_state(self, plan):
        key = (plan.Hs, plan.Ws)
        if key not in self._temporal:
            self._temporal[key] = _TemporalState(plan.h, plan.w, self.stacked, self.device)
        return self._temporal[key]

    def _volume_state(self, plan):
        key = (plan.Hs, plan.Ws)
        if key not in self._volume:
            self._volume[key] = _VolumeState(self.device)
        return self._volume[key]

    def _chain(self, plan, frames, K, K_src, present, rigid_only, max_flow, temporal=None, want_u16=False, cloud=None, volume=None, render=None, track=None):
        N = 1 + self.n
        img, _ = self._aug.prep(frames, self._no_jitter(N), plan.h, plan.w, tabs=(plan.xtab, plan.ytab))
        nd = 2 if self.pose_use_depth else 1                   # frames the depth net sees
        batch = {"img": img[:nd]}
        if K is not None:
            batch["intrinsics"] = K[:nd]
        with torch.no_grad():
            depth_all = self.model.run_depth_net(batch)["depth_pred"][0].detach().float()
            pb = self.model.pose_net({"pose_net_input": self.pose_input(img, depth_all if self.pose_use_depth else None)})
        pose = (pb["pose_pred"][:1] if self.stacked else torch.cat(list(pb["pose_pred"]), 0)).detach().float().contiguous()      # [n,4,4]
        motion = pb.get("motion_pred") if self.stacked else None
        if motion is not None:
            motion = motion[:1].detach().float().contiguous()
        pred = depth_all[:1, 0].contiguous()
        out = {"depth_net": pred, "depth": None, "canvas": None, "pose": pose, "motion": motion}
        ymap, xmap = self._maps_on_device(plan, pred.shape[-2:])
        shown = pred
        if temporal is not None:
            alpha, tol, st = temporal
            j, inverted = temporal_context(self.offsets)
            if tuple(pred.shape) != tuple(st.depth.shape):
                raise ValueError(f"PairPredictor: temporal fusion needs the depth at the network's size {tuple(st.depth.shape[1:])}, "
                                 f"the depth network gives {tuple(pred.shape[1:])}")
            if inverted:                                        # previous -> current = the inverse of this window's pose to the context at -1
                Rt, t = pose[j, :3, :3].t(), pose[j, :3, 3]       # [R^T | -R^T t], term by term: separate fp32 roundings, left to right
                st.T[0, :3, :3].copy_(Rt)
                st.T[0, :3, 3].copy_(-(Rt[:, 0] * t[0] + Rt[:, 1] * t[1] + Rt[:, 2] * t[2]))
            carried = not inverted and not rigid_only and motion is not None
            _, out["temporal_state"], _ = HT.warp_fuse(st.depth, pred, K[:1], st.T, motion=st.motion if carried else None, alpha=alpha, tol=tol,
                                                       out=st.depth, zbuf=st.zbuf)
            shown = st.depth.clone()                            # the state moves on with the next window, on the other slot: this slot's copy
            out["depth_net"], out["depth_net_raw"] = shown, pred
            if not inverted:                                    # this window's pose to the frame at +1 carries the fused map into the next window
                st.T.copy_(pose[j:j + 1])
                if carried:
                    st.motion.copy_(motion)
        if volume is not None:                                  # the depth the pictures show, through the pose chained on the device
            vol, vs = volume
            j, inverted = temporal_context(self.offsets)
            if inverted:                                        # previous -> current: this window's pose to the context at -1, inverted as above;
                Rt, t = pose[j, :3, :3].t(), pose[j, :3, 3]       # the first window of a sequence is the world and takes no step
                vs.inv[:3, :3].copy_(Rt)
                vs.inv[:3, 3].copy_(-(Rt[:, 0] * t[0] + Rt[:, 1] * t[1] + Rt[:, 2] * t[2]))
                vs.T.copy_(torch.where(vs.started, vs.inv, vs.eye))
            vol.compose(vs.T, vs.C)
            fused = shown
            if track is not None:                               # the predicted pose against the model: C <- D^-1 C, and the depth goes in times the scale
                schedule, dist_tol, scale_tol, min_count, damping, min_weight, near, far, step = track
                if vs.align is None or (vs.align.H, vs.align.W) != (plan.Hs, plan.Ws):
                    vs.align = AlignState((plan.Hs, plan.Ws), self.device)
                vol.track(shown, ymap, xmap, K_src[:1], vs.C, (plan.Hs, plan.Ws), schedule=schedule, dist_tol=dist_tol, scale_tol=scale_tol, min_count=min_count,
                          damping=damping, min_weight=min_weight, near=near, far=far, step=step, state=vs.align)
                vol.compose(vs.align.Dinv, vs.C)
                fused = shown * vs.align.scale                  # a device scalar: the first window's empty volume leaves D = I and scale = 1 by itself
                out["track_state"] = vs.align.state.clone()
            vol.integrate(fused, ymap, xmap, K_src[:1], vs.C, frame=frames[:1])
            out["world_to_camera"] = vs.C.clone()               # the state moves on with the next window, on the other slot: this slot's copy
            if render is not None:                              # the model as this camera sees it, this window's depth included
                normals, picture, min_weight, near, far, step = render
                out["model_depth"], out["model_normal"], out["model_picture"] = vol.render(
                    K_src[:1], vs.C, (plan.Hs, plan.Ws), near=near, far=far, step=step, min_weight=min_weight, normals=normals, picture=picture)
            if not inverted:                                    # this window's pose to the frame at +1 is the next window's step
                vs.T.copy_(pose[j])
            vs.started.fill_(True)
        out["flow"], out["flow_valid"], out["flow_canvas"] = HF.pair_flow(pred.expand(self.n, -1, -1), ymap, xmap, K_src, pose,
                                                                          motion=None if rigid_only else motion, max_flow=max_flow, want_canvas=present)
        if present:
            out["canvas"], out["depth"], u16 = HP.depth_present(shown, ymap, xmap, self.vmax, self.gamma, frame=frames[:1], want_depth=True, want_u16=want_u16)
            if want_u16:
                out["depth_u16"] = u16
        if cloud is not None:                                   # the target's cloud, from the depth the pictures show
            out["points"], out["count"] = HC.depth_cloud(shown, ymap, xmap, K_src[:1], *cloud, frame=frames[:1])
        return out

    def _source_intrinsics(self, intrinsics):
        if intrinsics is None:
            raise ValueError("PairPredictor: the flow needs intrinsics (the source-size K [3,3] of the frames)")
        return self._host_K("PairPredictor", intrinsics, 1)[0]          # one K for the whole window

    def _run(self, slot, plan, intrinsics, K_host, present, rigid_only, max_flow, temporal=None, want_u16=False, cloud=None, volume=None, render=None, track=None):
        N = 1 + self.n
        K = self._device_copy(slot, "K", plan.intrinsics(intrinsics), N)
        K_src =self._device_copy(slot, "K_src", K_host, self.n)
        max_flow = float(0.05 * plan.Ws if max_flow is None else max_flow)
        if not max_flow > 0:
            raise ValueError(f"PairPredictor: max_flow must be positive, got {max_flow}")
        key = ("pair", bool(present), bool(rigid_only), max_flow)
        if temporal is None and not want_u16 and cloud is None and volume is None:
            return self._replay(slot, key, lambda: self._chain(plan, slot.frames, K, K_src, bool(present), bool(rigid_only), max_flow))
        key += ((temporal[:2] if temporal is not None else None),) + ((bool(want_u16), cloud) if want_u16 or cloud is not None else ())
        persistent = temporal[2].tensors() if temporal is not None else []
        if volume is not None:                                  # the volume's parameters and addresses are part of what the graph holds; its arrays move on
            vol, vs = volume                                    # with every run, so the eager run before a capture is taken back like the states'
            key += (("volume",) + vol.params(),)
            if render is not None:
                key += (("render",) + render,)
            if track is not None:
                key += (("track",) + track,)
            persistent = persistent + vs.tensors() + [t for t in (vol.tsdf, vol.weight, vol.rgba) if t is not None]
        return self._replay(slot, key, lambda: self._chain(plan, slot.frames, K, K_src, bool(present), bool(rigid_only), max_flow, temporal, bool(want_u16), cloud,
                                                           volume, render, track), persistent=persistent)

    def predict(self, frames, intrinsics, present=True, rigid_only=False, max_flow=None, temporal=None, volume=None, render=None, track=None):
        """frames: the window, a list of 1 + n uint8 [H,W,3] RGB frames of one size -- the target, then the n context frames in the order the dataset
        emits `ctx_img` (self.offsets, ascending, e.g. the frames at -1 and +1).  intrinsics: the source-size K [3,3] of the frames.  Returns a
        dict of device tensors: `depth` [1,H,W], `canvas` [1,2H,W,3], `depth_net` [1,h,w] as DepthPredictor returns them for the target; `pose`
        [n,4,4], target -> context j (p_ctx = R p_target + t); `flow` [n,H,W,2] in pixels of the frame, target -> context j; `flow_valid`
        [n,H,W] uint8 (bit 0: defined, bit 1: lands inside the context frame); `flow_canvas` [n,H,W,3] uint8, the flow on the colour wheel;
        `motion` [n,3,h,w], GoogleMotionNet's per-pixel translation, else None.  rigid_only: the flow of the camera motion alone (`motion` is
        still returned).  max_flow: the flow length, in pixels, that reaches full saturation in `flow_canvas`; default 5 % of the frame's
        width -- a presentation constant, like gamma.  present=False skips the three pictures.  Translations, and with them the flow's share
        that comes from them, are up to the scale of the monocular depth.  No host synchronisation after the first call of a size.  predict keeps
        nothing from call to call: temporal fusion and volume fusion are `stream`'s, and anything but temporal=None, volume=None, render=None,
        track=None is refused."""
        if temporal is not None:
            raise ValueError("PairPredictor.predict is stateless: temporal fusion needs the frames in order, use stream(..., temporal=...)")
        if volume is not None:
            raise ValueError("PairPredictor.predict is stateless: volume fusion chains the poses of frames in order, use stream(..., volume=...)")
        if render is not None:
            raise ValueError("PairPredictor.predict is stateless: render= shows the volume a sequence is fused into, use stream(..., volume=..., render=...)")
        if track is not None:
            raise ValueError("PairPredictor.predict is stateless: track= aligns frames with the volume a sequence is fused into, use stream(..., volume=..., track=...)")
        t = as_window(frames, self.n)
        K_host = self._source_intrinsics(intrinsics)
        plan = self.plan(t.shape[1], t.shape[2])
        slot = self._slot(t.shape[0], plan)
        with torch.cuda.device(self.device):
            self._upload(slot, t)
            out = self._run(slot, plan, intrinsics, K_host, present, rigid_only, max_flow)
            return {k: (v.clone() if v is not None else None) for k, v in out.items()}

    def _result(self, slot, names):
        slot.downloaded.synchronize()
        res = {k: slot.host[k].numpy() for k in names if slot.out[k] is not None}
        for k in ("depth", "canvas", "depth_net", "depth_net_raw", "temporal_state", "depth_u16"):
            if k in res:
                res[k] = res[k][0]
        if "depth_u16" in res:
            res["depth_u16"] = res["depth_u16"].view(np.uint16)
        j, inverted = self.next_context
        res["pose_next"] = invert_pose_np(res["pose"][j]) if inverted else res["pose"][j].copy()
        if "track_state" in res:
            u = unpack_state(res.pop("track_state"))
            res.update(track_delta=u["D"], track_scale=u["scale"], track_count=u["count"], track_rms=u["rms"], track_status=u["status"])
        return res

    def stream(self, frames_iter, intrinsics, present=True, rigid_only=False, max_flow=None, temporal=None, want_u16=False, cloud=None, volume=None,
               render=None, track=None):
        """Generator over host frames of a sequence (uint8 [H,W,3] RGB, one at a time, one size).  Keeps a sliding window and yields, in order, one
        dict of host arrays per target frame that has all its context frames: the outputs of `predict` (`depth` [H,W], `canvas` [2H,W,3], `pose`,
        `flow`, `flow_valid`, `flow_canvas`, `motion`; with present=False `depth_net` instead of the pictures), `index`, the target's position in
        the sequence, and `pose_next` [4,4], the pose target -> next frame: the context at +STRIDE when the model has one; otherwise the inverse of
        the pose to the context at -STRIDE, which is the step previous frame -> target of a model that only looks back.  geometry.pose_utils.accumulate_poses over the yielded `pose_next` is the camera's trajectory, up to the scale of the
        monocular depth.  The arrays are views of pinned buffers and stay valid until the next iteration; uploads, compute and downloads
        overlap as in DepthPredictor.stream.

        temporal=dict(alpha=0.5, tol=0.05): temporally fused depth (see the class).  `depth` and `canvas` then come from the fused map, and every
        record also holds `depth_net` [h,w], the fused map at the network's size, `depth_net_raw` [h,w], the prediction it was fused with, and
        `temporal_state` [h,w] uint8: bits 0-1 the class of the pixel (0 new, 1 fused, 2 / 3 the warped surface lies nearer / farther than the
        prediction, which is kept), bit 2 set where a one-pixel hole of the warp was filled.  alpha in [0, 1) is the weight of the warped
        depth, tol > 0 the relative difference up to which the two count as one surface.  Every call starts from an empty state: its first
        window is the raw prediction, with state 0 everywhere.  ValueError for a model without a context one frame away.

        want_u16 (with present) adds `depth_u16` [H,W] and cloud=dict(min_depth=, max_depth=, step=1) adds `points` [1,cap,16] and `count` [1] of
        the target, as DepthPredictor.stream yields them, from the depth the pictures show (the fused one with temporal).

        volume=vol (a hip.volume.TsdfVolume on this device): every window's depth -- the one the pictures show -- is integrated into the volume
        (sde_tsdf_integrate, with the source-size intrinsics and the target's colours) through the world-to-camera pose chained on the device
        from the model's own step poses (sde_pose_compose); every record then holds `world_to_camera` [4,4], the pose its depth went in with: the
        identity for the first target, which is the world.  Every call, and every change of the frame size, starts a new chain; the volume is the
        caller's and is never reset here, so several sequences may go into one.  ValueError for a model without a context one frame away.

        render=dict(normals=True, picture=True, min_weight=1) (with volume=; also near=, far=, step=, default the volume's min_depth, max_depth
        and voxel): after the window's depth has gone in, the volume is rendered from the window's own camera (sde_tsdf_render, hip.volume.
        TsdfVolume.render: the source-size intrinsics, the chained pose, the frame's size) inside the same graph.  Every record then holds
        `model_depth` [H,W] float32, the z-depth of the fused model's surface along every pixel's ray, 0 where there is none -- the depth that
        is consistent over the whole sequence -- and, unless switched off, `model_normal` [H,W,3] float32 in camera coordinates and
        `model_picture` [H,W,4] uint8.

        track=dict(schedule=None, scale=True, dist_tol=, scale_tol=, min_count=, damping=, min_weight=1, near=, far=, step=) (with volume=; every
        key optional, defaults in hip.align): frame-to-model tracking.  Before a window's depth goes in, the volume is rendered from the pose the
        chain PREDICTS, the depth is aligned with that model (hip.volume.TsdfVolume.track: sde_frame_align, a point-to-plane Gauss-Newton
        iteration per entry of `schedule`, which also fits one depth scale unless scale=False), the pose becomes D^-1 C on the device and the
        depth is integrated -- and rendered, with render= -- times the scale; all inside the same graph, with no read-back: against an empty
        volume (the first window) the kernels leave D = I and the scale at 1 by themselves.  `world_to_camera` is then the CORRECTED pose, and
        every record also holds `track_delta` [4,4] (D: the frame's camera coordinates -> the predicted camera's), `track_scale`, `track_count`
        (the last iteration's inliers), `track_rms` (their root-mean-square point-to-plane distance) and `track_status` (hip.align.OK, TOO_FEW or
        SINGULAR, after which D and the scale are what the iterations before left).  The scale is fitted per window and starts at 1 every time;
        `depth`, the pictures, the cloud and the flow keep the network's scale, and the pose network's next translation is NOT rescaled by it.
        With track=None nothing changes: the same graphs, the same bytes."""
        K_host = self._source_intrinsics(intrinsics)
        fuse = temporal_args(temporal)
        volume = volume_arg(volume, self.device)
        render = render_arg(render, volume)
        track = track_arg(track, volume)
        cloud, _ = DepthPredictor._cloud_args(cloud, K_host, 1)
        want_u16 = bool(want_u16 and present)
        if fuse is not None or volume is not None:
            temporal_context(self.offsets)
        names = [k for k, on in (("depth", present), ("canvas", present), ("depth_net", not present or fuse is not None), ("depth_net_raw", fuse is not None),
                                 ("temporal_state", fuse is not None), ("pose", True), ("flow", True), ("flow_valid", True), ("flow_canvas", present),
                                 ("motion", True), ("depth_u16", want_u16), ("points", cloud is not None), ("count", cloud is not None),
                                 ("world_to_camera", volume is not None), ("model_depth", render is not None),
                                 ("model_normal", render is not None and render[0]), ("model_picture", render is not None and render[1]),
                                 ("track_state", track is not None)) if on]
        live, live_v = [], []                                  # the states this call has reset and is advancing
        lo, hi = min(self.offsets + (0,)), max(self.offsets + (0,))
        targets = []

        def windows():
            held = {}                                          # position in the sequence -> frame, for the span of one window
            for i, frame in enumerate(frames_iter):
                t, _ = self._as_frames(frame)
                if t.is_cuda or t.shape[0] != 1:
                    raise ValueError("PairPredictor.stream takes one host frame [H,W,3] per item")
                held[i] = t[0]
                held.pop(i - (hi - lo) - 1, None)
                target = i - hi
                if target + lo >= 0:
                    targets.append(target)
                    yield as_window([held[target]] + [held[target + o] for o in self.offsets], self.n)

        def result(slot, names):
            res = self._result(slot, names)
            res["index"] = targets.pop(0)
            return res

        def run(slot, plan):
            vol = None
            if volume is not None:
                vs = self._volume_state(plan)
                if not live_v or live_v[0] is not vs:          # the first window of this call, or frames of another size: that target is the world
                    vs.reset()
                    live_v[:] = [vs]
                vol = (volume, vs)
                if render is not None:
                    from ..hip.volume import check_render
                    check_render((plan.Hs, plan.Ws), render[3], render[4], render[5])
            if fuse is None:
                return self._run(slot, plan, intrinsics, K_host, present, rigid_only, max_flow, want_u16=want_u16, cloud=cloud, volume=vol, render=render,
                                 track=track)
            st = self._temporal_state(plan)
            if not live or live[0] is not st:                  # the first window of this call, or frames of another size: an empty state
                st.reset()
                live[:] = [st]
            return self._run(slot, plan, intrinsics, K_host, present, rigid_only, max_flow, temporal=fuse + (st,), want_u16=want_u16, cloud=cloud, volume=vol, render=render,
                             track=track)
        yield from self._pump(windows(), names, run, result)

"""ctypes binding of sde_pair_flow (include/sde_hip.h, csrc/flow.hip): the depth of frame A and the pose A -> B -> dense optical flow at the
restored size, its validity map and its colour picture, one launch per batch; the colour wheel; and the Middlebury .flo file."""
import struct

import numpy as np
import torch

from . import args as A
from . import lib as L
from . import present as HP

WHEEL_SEGMENTS = (15, 6, 4, 11, 13, 6)        # red-yellow, yellow-green, green-cyan, cyan-blue, blue-magenta, magenta-red: 55 entries
FLO_TAG = 202021.25                           # the float32 at the head of a .flo file (the bytes "PIEH")
_wheels = {}


def wheel_u8():
    """The Middlebury colour wheel (Baker et al., "A Database and Evaluation Methodology for Optical Flow") -> uint8 [55,3] host array: along
    each segment one channel ramps as floor(255 * i / n) while the other two stay at 255 / 0."""
    ry, yg, gc, cb, bm, mr = WHEEL_SEGMENTS
    w = np.zeros((sum(WHEEL_SEGMENTS), 3), np.int64)
    ramp = lambda n: np.floor(255 * np.arange(n) / n).astype(np.int64)
    c = 0
    w[c:c + ry, 0], w[c:c + ry, 1] = 255, ramp(ry); c += ry
    w[c:c + yg, 0], w[c:c + yg, 1] = 255 - ramp(yg), 255; c += yg
    w[c:c + gc, 1], w[c:c + gc, 2] = 255, ramp(gc); c += gc
    w[c:c + cb, 1], w[c:c + cb, 2] = 255 - ramp(cb), 255; c += cb
    w[c:c + bm, 2], w[c:c + bm, 0] = 255, ramp(bm); c += bm
    w[c:c + mr, 2], w[c:c + mr, 0] = 255 - ramp(mr), 255
    return w.astype(np.uint8)


def flow_wheel(device):
    """The wheel as a uint8 [55,3] tensor on `device`, built on the host once per device."""
    device = torch.device(device)
    if device not in _wheels:
        _wheels[device] = torch.from_numpy(wheel_u8()).to(device)
    return _wheels[device]


def pair_flow(pred, ymap, xmap, K, T, motion=None, max_flow=10.0, frame=None, want_canvas=True, want_flow=True, want_valid=True, wheel=None, out=None):
    """pred [N,ph,pw] (or [N,1,ph,pw] / [ph,pw]) fp32, ymap [H] / xmap [W] int32 (hip.present's maps: device tensors, or host arrays that are
    validated and uploaded), K [N,3,3] or [3,3] fp32 at the restored size, T [N,4,4] fp32 (the pose A -> B, p_B = R p_A + t), motion [N,3,ph,pw]
    fp32 or None (rigid flow), frame [N,H,W,3] uint8 or None: CUDA tensors.  max_flow > 0: the flow length, in pixels, that reaches full
    saturation.  Returns (flow [N,H,W,2] fp32, valid [N,H,W] uint8 -- bit 0: the flow is defined, bit 1: it lands inside frame B --, canvas
    [N, 2H or H, W, 3] uint8), each None when it was not asked for.  out: optional (flow, valid, canvas) destinations.  No host synchronisation
    (device maps: see depth_present)."""
    if not float(max_flow) > 0:
        raise ValueError(f"pair_flow: max_flow must be positive, got {max_flow!r}")
    if not (want_canvas or want_flow or want_valid):
        raise ValueError("pair_flow: at least one of flow, valid and canvas must be asked for")
    pred = A.as_pred("pair_flow", pred)
    N, ph, pw = pred.shape
    dev = pred.device
    ymap, xmap = HP.ensure_checked(ymap, xmap, ph, pw, dev)
    H, W = ymap.numel(), xmap.numel()
    K = A.as_K("pair_flow", K, N, dev)
    T = A.same_device_tensor("pair_flow", "T", T, torch.float32, (N, 4, 4), dev)
    if motion is not None:
        motion = A.same_device_tensor("pair_flow", "motion", motion, torch.float32, (N, 3, ph, pw), dev).contiguous()
    frame = A.as_frame("pair_flow", frame, N, H, W, dev)
    wheel = A.same_device_tensor("pair_flow", "wheel", flow_wheel(dev) if wheel is None else wheel, torch.uint8, (None, 3), dev)
    if not 0 < wheel.shape[0] <= 256:
        raise L.SdeHipError(f"pair_flow: wheel must have between 1 and 256 rows, got {wheel.shape[0]}")
    rows = 2 * H if frame is not None else H
    flow, valid, canvas = out if out is not None else (None, None, None)
    flow = A.dst("pair_flow", flow, (N, H, W, 2), torch.float32, want_flow, dev)
    valid = A.dst("pair_flow", valid, (N, H, W), torch.uint8, want_valid, dev)
    canvas = A.dst("pair_flow", canvas, (N, rows, W, 3), torch.uint8, want_canvas, dev)
    L.check(L.lib().sde_pair_flow(L.ptr(pred), N, ph, pw, L.ptr(ymap), L.ptr(xmap), H, W, L.ptr(K), L.ptr(T.contiguous()), L.ptr(motion),
                                  L.ptr(wheel.contiguous()), int(wheel.shape[0]), float(max_flow), L.ptr(frame), L.ptr(flow), L.ptr(valid), L.ptr(canvas),
                                  L.stream()), "sde_pair_flow")
    return flow, valid, canvas


def write_flo(path, flow):
    """flow [H,W,2] float32 (array or tensor; a device tensor is copied to the host) -> a Middlebury .flo file: the float32 tag 202021.25, int32
    width, int32 height, then the rows of interleaved (u, v) float32, all little-endian."""
    a = flow.detach().cpu().numpy() if torch.is_tensor(flow) else np.asarray(flow)
    if a.ndim != 3 or a.shape[2] != 2 or a.dtype != np.float32:
        raise ValueError(f"write_flo: flow must be float32 [H,W,2], got {a.dtype} {a.shape}")
    with open(path, "wb") as f:
        f.write(struct.pack("<fii", FLO_TAG, a.shape[1], a.shape[0]))
        np.ascontiguousarray(a, dtype="<f4").tofile(f)


def read_flo(path):
    """A Middlebury .flo file -> flow [H,W,2] float32."""
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) != 12:
            raise ValueError(f"read_flo: {path} is shorter than a .flo header")
        tag, w, h = struct.unpack("<fii", head)
        if tag != FLO_TAG or w <= 0 or h <= 0:
            raise ValueError(f"read_flo: {path} is not a .flo file (tag {tag}, {w} x {h})")
        data = np.fromfile(f, dtype="<f4")
    if data.size != h * w * 2:
        raise ValueError(f"read_flo: {path} holds {data.size} values, {h} x {w} x 2 expected")
    return data.reshape(h, w, 2).astype(np.float32, copy=False)

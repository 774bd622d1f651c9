"""ctypes binding of sde_depth_present (include/sde_hip.h, csrc/present.hip): network outputs -> restored depth, 16-bit depth and the coloured
(optionally frame-stacked) picture of tools/demo.py, one launch per batch."""
from ctypes import c_int, c_void_p

import numpy as np
import torch

from . import args as A
from . import lib as L

_P, _I, _F = c_void_p, c_int, L.c_float
L.register_protos({
    "sde_depth_present": ([_P, _I, _I, _I, _P, _P, _I, _I, _F, _F, _P, _P, _P, _P, _P, _P], c_int),
})

_checked = {}        # (ymap.data_ptr, xmap.data_ptr, ...) -> the pair itself (kept alive, so the pointers cannot be handed out again)
_luts = {}


def check_maps(ymap, xmap, ph, pw, H=None, W=None):
    """Host-side validation of one (ymap, xmap) pair, numpy arrays or host tensors: int32, lengths H / W when given, every entry in [-1, ph) /
    [-1, pw).  The kernel indexes the prediction with whatever the maps hold."""
    for name, m, n, lim in (("ymap", ymap, H, ph), ("xmap", xmap, W, pw)):
        a = m.numpy() if torch.is_tensor(m) else np.asarray(m)
        if a.dtype != np.int32 or a.ndim != 1 or a.size == 0 or (n is not None and a.size != n):
            raise L.SdeHipError(f"depth_present: {name} must be int32 [{n if n is not None else 'n'}], got {a.dtype} {a.shape}")
        if int(a.min()) < -1 or int(a.max()) >= lim:
            raise L.SdeHipError(f"depth_present: {name} entries must lie in [-1, {lim}), got [{int(a.min())}, {int(a.max())}]")


def device_maps(ymap, xmap, ph, pw, device):
    """Validated host maps -> device tensors that depth_present accepts without looking at them again."""
    check_maps(ymap, xmap, ph, pw)
    ym = torch.as_tensor(np.ascontiguousarray(ymap)).to(device)
    xm = torch.as_tensor(np.ascontiguousarray(xmap)).to(device)
    _remember(ym, xm, ph, pw)
    return ym, xm


def _key(ymap, xmap, ph, pw):
    return (ymap.data_ptr(), xmap.data_ptr(), ymap.numel(), xmap.numel(), ymap._version, xmap._version, ph, pw)


def _remember(ymap, xmap, ph, pw):
    if len(_checked) >= 256:
        _checked.clear()
    _checked[_key(ymap, xmap, ph, pw)] = (ymap, xmap)


def ensure_checked(ymap, xmap, ph, pw, device):
    """Maps in any accepted form -> the validated 1-D int32 device pair: host arrays are validated and uploaded; a device pair is validated once
    (one device -> host copy the first time the pair is seen, none after).  Shared by every binding that indexes a prediction through the maps."""
    if not (torch.is_tensor(ymap) and torch.is_tensor(xmap) and ymap.is_cuda and xmap.is_cuda):
        return device_maps(ymap, xmap, ph, pw, device)
    for what, m in (("ymap", ymap), ("xmap", xmap)):
        A.same_device_tensor("the index maps", what, m, torch.int32, (None,), torch.device(device))
    if _key(ymap, xmap, ph, pw) not in _checked:
        check_maps(ymap.cpu(), xmap.cpu(), ph, pw)
        _remember(ymap, xmap, ph, pw)
    return ymap, xmap


def default_lut(device):
    device = torch.device(device)
    if device not in _luts:
        from ..utils.colormap import magma_u8
        _luts[device] = torch.from_numpy(magma_u8()).to(device)
    return _luts[device]


def depth_present(pred, ymap, xmap, vmax, gamma=0.8, lut=None, frame=None, want_depth=True, want_u16=False, out=None):
    """pred [N,ph,pw] (or [N,1,ph,pw] / [ph,pw]) fp32, ymap [H] / xmap [W] int32, lut [256,3] uint8 (default: magma), frame [N,H,W,3] uint8 or None:
    CUDA tensors.  Returns (canvas [N, 2H or H, W, 3] uint8, depth_full [N,H,W] fp32 or None, depth_u16 [N,H,W] int16 bits of uint16 or None).
    Device maps are validated once per distinct pair (one device -> host copy the first time a pair is seen, none after: do that first call
    outside graph capture, or build the pair with device_maps()).  out: optional (canvas, depth_full, depth_u16) destinations.  No host sync."""
    pred = A.as_pred("depth_present", pred)
    N, ph, pw = pred.shape
    dev = pred.device
    ymap, xmap = ensure_checked(ymap, xmap, ph, pw, dev)
    H, W = ymap.numel(), xmap.numel()
    lut = A.same_device_tensor("depth_present", "lut", default_lut(dev) if lut is None else lut, torch.uint8, (256, 3), dev)
    frame = A.as_frame("depth_present", frame, N, H, W, dev)
    rows = 2 * H if frame is not None else H
    canvas, depth, u16 = out if out is not None else (None, None, None)
    canvas = A.dst("depth_present", canvas, (N, rows, W, 3), torch.uint8, True, dev)
    depth = A.dst("depth_present", depth, (N, H, W), torch.float32, want_depth, dev)
    u16 = A.dst("depth_present", u16, (N, H, W), torch.int16, want_u16, dev)          # torch has no arithmetic on uint16: the bits; .cpu().numpy().view(np.uint16) on the host
    L.check(L.lib().sde_depth_present(L.ptr(pred), N, ph, pw, L.ptr(ymap), L.ptr(xmap), H, W, float(vmax), float(gamma), L.ptr(lut.contiguous()),
                                      L.ptr(frame), L.ptr(depth), L.ptr(u16), L.ptr(canvas), L.stream()), "sde_depth_present")
    return canvas, depth, u16

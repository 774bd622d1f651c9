"""The argument checks of the geometry bindings (present, cloud, flow, temporal, lidar), ONE rule: every tensor is on the device of the binding's
primary input (not merely on some GPU: its pointer goes into a launch on that device), destinations are contiguous, and a tensor fault is an
SdeHipError that names the operator and the argument.  Scalar parameters stay with their bindings (ValueError).  Nothing here knows the
library: host memory is refused where the pointer is taken (lib.ptr)."""
import torch

from .lib import SdeHipError


def same_device_tensor(name, what, t, dtype, shape, dev):
    """t must be a `dtype` tensor of `shape` (None: any extent) on `dev`; returns t."""
    if (not torch.is_tensor(t) or t.dtype != dtype or t.dim() != len(shape) or any(s is not None and s != n for s, n in zip(shape, t.shape))
            or t.device != dev):
        want = "[" + ",".join("n" if s is None else str(s) for s in shape) + "]"
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else type(t).__name__
        raise SdeHipError(f"{name}: {what} must be a {dtype} {want} tensor on {dev}, got {got}")
    return t


def as_pred(name, pred):
    """[ph,pw] / [N,1,ph,pw] / [N,ph,pw] fp32 -> contiguous [N,ph,pw]: the primary input, whose device the other arguments must share."""
    if torch.is_tensor(pred) and pred.dim() == 2:
        pred = pred[None]
    elif torch.is_tensor(pred) and pred.dim() == 4 and pred.shape[1] == 1:
        pred = pred[:, 0]
    if not torch.is_tensor(pred) or pred.dim() != 3 or pred.dtype != torch.float32:
        got = f"{pred.dtype} {tuple(pred.shape)}" if torch.is_tensor(pred) else type(pred).__name__
        raise SdeHipError(f"{name}: pred must be a float32 [N,ph,pw] tensor, got {got}")
    return pred.contiguous()


def as_K(name, K, N, dev):
    """K [3,3] (shared by the N frames) or [N,3,3] fp32 on dev -> contiguous [N,3,3]."""
    if torch.is_tensor(K) and K.dim() == 2:
        K = K[None].expand(N, -1, -1)
    return same_device_tensor(name, "K", K, torch.float32, (N, 3, 3), dev).contiguous()


def as_frame(name, frame, N, H, W, dev):
    """None, or uint8 [N,H,W,3] ([H,W,3] for one frame) on dev -> contiguous [N,H,W,3] or None."""
    if frame is None:
        return None
    if torch.is_tensor(frame) and frame.dim() == 3:
        frame = frame[None]
    return same_device_tensor(name, "frame", frame, torch.uint8, (N, H, W, 3), dev).contiguous()


def dst(name, t, shape, dtype, want, dev):
    """A destination: None when not wanted, a new tensor when t is None, else t itself, which must be contiguous `dtype` `shape` on dev."""
    if not want:
        return None
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != dev or not t.is_contiguous():
        raise SdeHipError(f"{name}: destination must be a contiguous {dtype} {tuple(shape)} tensor on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t

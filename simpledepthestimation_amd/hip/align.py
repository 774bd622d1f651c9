"""Frame-to-model alignment: the camera tracked against the TSDF volume (include/sde_hip.h: sde_frame_align, sde_frame_align_reset;
csrc/align.hip).  One `frame_align` call is one Gauss-Newton iteration of a point-to-plane fit of a frame's depth to the model that
`TsdfVolume.render` shows from the predicted pose, together with the update of one depth scale; `AlignState` owns the 40-word state (D, its
inverse, the scale, the last iteration's counts and status), the workspace and the buffers of the rendered model; `TsdfVolume.track` (hip/volume.py)
runs render -> reset -> a schedule of iterations.  `align_terms_host` and `frame_align_host` are the host twins -- the same operations in the same
order in numpy, for machines without a GPU and for the tests, which compare the two bit for bit."""
import numpy as np
import torch

from . import args as A
from . import lib as L
from . import present as HP
from .twins import nearest_pixel_np

POSE, SCALE = 1, 2                                            # the bits of `mode`
OK, TOO_FEW, SINGULAR = 0, 1, 2                               # the status word
STATUS = {OK: "ok", TOO_FEW: "too few", SINGULAR: "singular"}
STATE_WORDS, SUMS = 40, 32
SCALE_AT, SUMSQ_AT, COUNT_AT, SCALE_COUNT_AT, STATUS_AT = 32, 33, 34, 35, 36
TILE_W, TILE_H = 32, 8                                        # pixels per workgroup of the accumulate launch
MAX_PICTURE = 32768

# The defaults of TsdfVolume.track, chosen on the CPU with the twins (DESIGN.md section 31 keeps the measurements): four iterations of pose and
# scale together.  A depth scale and a step along the optical axis explain nearly the same residual, so the two updates overshoot in turn: an
# even number of joint iterations ends on the damped side, and more than four gained nothing on the scenes measured.
DEFAULT_SCHEDULE = (POSE | SCALE,) * 4
DEFAULTS = dict(dist_tol=0.03, scale_tol=0.1, min_count=256, damping=1e-4)


def check_align(dist_tol, scale_tol, min_count, damping, mode, min_depth, max_depth):
    """The scalar argument errors sde_frame_align refuses, raised as ValueError before anything touches the device.  -> the values as the kernel
    receives them (fp32 values as Python floats, ints)."""
    f = lambda x: float(np.float32(x))
    dist_tol, scale_tol, damping, min_depth, max_depth = f(dist_tol), f(scale_tol), f(damping), f(min_depth), f(max_depth)
    if not dist_tol > 0.0 or not scale_tol > 0.0:
        raise ValueError(f"frame_align: dist_tol and scale_tol must be positive, got ({dist_tol!r}, {scale_tol!r})")
    if not damping >= 0.0:
        raise ValueError(f"frame_align: damping must not be negative, got {damping!r}")
    if isinstance(min_count, bool) or int(min_count) != min_count or int(min_count) < 6:
        raise ValueError(f"frame_align: min_count must be an integer of at least 6, got {min_count!r}")
    if isinstance(mode, bool) or not isinstance(mode, (int, np.integer)) or not 1 <= int(mode) <= 3:
        raise ValueError(f"frame_align: mode must be POSE (1), SCALE (2) or POSE | SCALE (3), got {mode!r}")
    if not min_depth < max_depth:
        raise ValueError(f"frame_align: min_depth must lie below max_depth, got ({min_depth}, {max_depth})")
    return dist_tol, scale_tol, int(min_count), damping, int(mode), min_depth, max_depth


def check_size(size):
    try:
        H, W = (int(s) for s in size)
        exact = len(tuple(size)) == 2 and all(int(s) == s for s in size)
    except (TypeError, ValueError):
        exact = False
    if not exact or not (1 <= H <= MAX_PICTURE and 1 <= W <= MAX_PICTURE):
        raise ValueError(f"frame_align: size must be (H, W), integers in [1, {MAX_PICTURE}], got {size!r}")
    return H, W


def slab_rows(H, W):
    """Workgroups of the accumulate launch = rows of 32 partial sums in the workspace."""
    return -(-W // TILE_W) * -(-H // TILE_H)


class AlignState:
    """What one tracked frame needs on the device: `state` (40 fp32 words, layout in include/sde_hip.h), the workspace of the reduction and the
    rendered model (`model_depth` [H,W], `model_normal` [H,W,3]).  `D`, `Dinv` ([4,4]) and `scale` ([1]) are views of `state`: `Dinv` goes into
    `pose_compose(state.Dinv, C)` as it is, `scale` into a device-side multiplication."""

    def __init__(self, size, device="cuda"):
        self.H, self.W = check_size(size)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.SdeHipError("AlignState: the state lives on a GPU; there is no CPU fallback (the host twins are functions of this module)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.state = torch.zeros((STATE_WORDS,), dtype=torch.float32, device=self.device)
        self.workspace = torch.empty((workspace_numel(self.H, self.W),), dtype=torch.float32, device=self.device)
        self.model_depth = torch.empty((self.H, self.W), dtype=torch.float32, device=self.device)
        self.model_normal = torch.empty((self.H, self.W, 3), dtype=torch.float32, device=self.device)
        self.D, self.Dinv, self.scale = self.state[:16].view(4, 4), self.state[16:32].view(4, 4), self.state[SCALE_AT:SCALE_AT + 1]
        self.reset()

    def reset(self):
        """D = Dinv = I, scale = 1, the info words cleared: one launch on the current stream."""
        L.check(L.lib().sde_frame_align_reset(L.ptr(self.state), L.stream()), "sde_frame_align_reset")
        return self

    def info(self):
        """The state read back (synchronises) -> the dict of unpack_state."""
        return unpack_state(self.state.cpu().numpy())


def workspace_numel(H, W):
    """fp32 elements of workspace sde_frame_align asks for."""
    return int(L.lib().sde_frame_align_ws_bytes(int(H), int(W))) // 4


def frame_align(pred, ymap, xmap, K, model_depth, model_normal, state, mode=POSE | SCALE, dist_tol=DEFAULTS["dist_tol"], scale_tol=DEFAULTS["scale_tol"],
                min_count=DEFAULTS["min_count"], damping=DEFAULTS["damping"], min_depth=0.0, max_depth=80.0, workspace=None):
    """One iteration (sde_frame_align).  pred [ph,pw] (or [1,ph,pw] / [1,1,ph,pw]) fp32, ymap [H] / xmap [W] int32 (hip.present's maps), K [3,3]
    fp32 at the restored size, model_depth [H,W] and model_normal [H,W,3] fp32 (TsdfVolume.render's outputs from the predicted pose): CUDA
    tensors on one device.  state: an AlignState, or its 40-word fp32 tensor (then `workspace`, an fp32 tensor of workspace_numel(H, W)
    elements, must be given).  Two launches on the current stream, no host synchronisation.  Returns state."""
    dist_tol, scale_tol, min_count, damping, mode, min_depth, max_depth = check_align(dist_tol, scale_tol, min_count, damping, mode, min_depth, max_depth)
    pred = A.as_pred("frame_align", pred)
    dev = pred.device
    A.same_device_tensor("frame_align", "pred", pred, torch.float32, (1, None, None), dev)
    _, ph, pw = pred.shape
    ymap, xmap = HP.ensure_checked(ymap, xmap, ph, pw, dev)
    H, W = check_size((ymap.numel(), xmap.numel()))
    K = A.as_K("frame_align", K, 1, dev)
    words = state.state if isinstance(state, AlignState) else state
    if workspace is None and isinstance(state, AlignState):
        workspace = state.workspace
    A.same_device_tensor("frame_align", "state", words, torch.float32, (STATE_WORDS,), dev)
    A.same_device_tensor("frame_align", "model_depth", model_depth, torch.float32, (H, W), dev)
    A.same_device_tensor("frame_align", "model_normal", model_normal, torch.float32, (H, W, 3), dev)
    A.same_device_tensor("frame_align", "workspace", workspace, torch.float32, (None,), dev)
    need = workspace_numel(H, W)
    if workspace.numel() < need:
        raise L.SdeHipError(f"frame_align: workspace of {workspace.numel()} elements, {need} are needed for {H} x {W}")
    L.check(L.lib().sde_frame_align(L.ptr(pred), ph, pw, L.ptr(ymap), L.ptr(xmap), H, W, L.ptr(K), L.ptr(model_depth), L.ptr(model_normal), min_depth,
                                    max_depth, dist_tol, scale_tol, min_count, damping, mode, L.ptr(words), L.ptr(workspace), workspace.numel() * 4,
                                    L.stream()), "sde_frame_align")
    return state


# ---- host twins ---------------------------------------------------------------------------------------------------------------------------------
def state_host():
    """The state after sde_frame_align_reset as 40 float32 words (the int32 words are reached through .view(np.int32))."""
    w = np.zeros(STATE_WORDS, np.float32)
    w[[0, 5, 10, 15, 16, 21, 26, 31, SCALE_AT]] = 1
    return w


def unpack_state(words):
    """40 words -> dict(D, Dinv [4,4], scale, sumsq (floats), count, scale_count, status (ints), rms)."""
    w = np.ascontiguousarray(words, dtype=np.float32).reshape(STATE_WORDS)
    i = w.view(np.int32)
    count, sumsq = int(i[COUNT_AT]), float(w[SUMSQ_AT])
    return dict(D=w[:16].reshape(4, 4).copy(), Dinv=w[16:32].reshape(4, 4).copy(), scale=float(w[SCALE_AT]), sumsq=sumsq, count=count,
                scale_count=int(i[SCALE_COUNT_AT]), status=int(i[STATUS_AT]), rms=float(np.sqrt(sumsq / count)) if count > 0 else 0.0)


def align_terms_host(pred, ymap, xmap, K, model_depth, model_normal, D, s, min_depth, max_depth, dist_tol, scale_tol):
    """The per-pixel stage of sde_frame_align with the kernel's bits -> dict: kept, pose, scale (bool [H,W]: the pixel survives step 5, is a pose
    inlier, is a scale inlier), ix, iy (int64 [H,W], 0 where not kept), q [H,W,3], r, rho [H,W], J [H,W,6] and terms [H,W,32] (float32; r, rho, J
    and q hold whatever the arithmetic gave where the pixel is not kept, terms holds 0 there)."""
    f32 = np.float32
    pred, ymap, xmap = np.asarray(pred, dtype=f32), np.asarray(ymap), np.asarray(xmap)
    K, D = np.asarray(K, dtype=f32).reshape(3, 3), np.asarray(D, dtype=f32).reshape(4, 4)
    H, W = ymap.size, xmap.size
    md, mn = np.asarray(model_depth, dtype=f32).reshape(H, W), np.asarray(model_normal, dtype=f32).reshape(H, W, 3)
    lo, hi, dist_tol, scale_tol, s = f32(min_depth), f32(max_depth), f32(dist_tol), f32(scale_tol), f32(s)
    with np.errstate(all="ignore"):
        my, mx = np.broadcast_to(ymap[:, None], (H, W)), np.broadcast_to(xmap[None, :], (H, W))
        keep = (my >= 0) & (mx >= 0)
        d0 = pred[np.where(keep, my, 0), np.where(keep, mx, 0)]
        keep = keep & np.isfinite(d0) & (lo < d0) & (d0 <= hi)
        d = s * d0
        fx, cx, fy, cy = K[0, 0], K[0, 2], K[1, 1], K[1, 2]
        k00, k11, k02, k12 = f32(1) / fx, f32(1) / fy, (f32(-1) * cx) / fx, (f32(-1) * cy) / fy
        rx = lambda u: k00 * u.astype(f32) + k02
        ry = lambda v: k11 * v.astype(f32) + k12
        px, py = d * rx(np.arange(W))[None, :], d * ry(np.arange(H))[:, None]
        q = [D[r, 0] * px + D[r, 1] * py + D[r, 2] * d + D[r, 3] for r in range(3)]
        keep = keep & (q[2] > 0) & (q[2] < np.inf)
        nx_, ny_ = fx * q[0] + cx * q[2], fy * q[1] + cy * q[2]
        den = q[2] + f32(1e-6)
        ok, ix, iy = nearest_pixel_np(nx_ / den, ny_ / den)
        keep = keep & ok & (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        ix, iy = np.where(keep, ix, 0), np.where(keep, iy, 0)
        m = md[iy, ix]
        n = mn[iy, ix]
        keep = keep & (m > 0) & ~((n[..., 0] == 0) & (n[..., 1] == 0) & (n[..., 2] == 0))
        gx, gy = m * rx(ix), m * ry(iy)
        ex, ey, ez = q[0] - gx, q[1] - gy, q[2] - m
        r = n[..., 0] * ex + n[..., 1] * ey + n[..., 2] * ez
        pose = keep & (np.abs(r) <= dist_tol * m)
        J = np.stack([q[1] * n[..., 2] - q[2] * n[..., 1], q[2] * n[..., 0] - q[0] * n[..., 2], q[0] * n[..., 1] - q[1] * n[..., 0],
                      n[..., 0], n[..., 1], n[..., 2]], -1)
        rho = m / q[2]
        scale = keep & (np.abs(rho - f32(1)) <= scale_tol)
        terms = np.zeros((H, W, SUMS), f32)
        k = 0
        for i in range(6):
            for j in range(i, 6):
                terms[..., k] = np.where(pose, J[..., i] * J[..., j], f32(0))
                k += 1
        for i in range(6):
            terms[..., 21 + i] = np.where(pose, J[..., i] * r, f32(0))
        terms[..., 27] = np.where(pose, r * r, f32(0))
        terms[..., 28] = pose
        terms[..., 29] = np.where(scale, rho, f32(0))
        terms[..., 30] = scale
    return dict(kept=keep, pose=pose, scale=scale, ix=ix, iy=iy, q=np.stack(q, -1), r=r, rho=rho, J=J, terms=terms)


def slab_host(terms):
    """terms [H,W,32] float32 -> the slab [rows,32] float32 the accumulate launch writes: per workgroup (32 x 8 pixels) the 64 lanes of each wave
    (8 x 8 pixels, x fastest) as a balanced binary tree, then the four waves in order."""
    H, W, nv = terms.shape
    gy, gx = -(-H // TILE_H), -(-W // TILE_W)
    p = np.zeros((gy * TILE_H, gx * TILE_W, nv), np.float32)
    p[:H, :W] = terms
    v = p.reshape(gy, 8, gx, 4, 8, nv).transpose(0, 2, 3, 1, 4, 5).reshape(gy, gx, 4, 64, nv)
    with np.errstate(all="ignore"):
        while v.shape[3] > 1:
            v = v[:, :, :, 0::2] + v[:, :, :, 1::2]
        v = v[:, :, :, 0]
        out = ((v[:, :, 0] + v[:, :, 1]) + v[:, :, 2]) + v[:, :, 3]
    return np.ascontiguousarray(out.reshape(gy * gx, nv))


def totals_host(slab):
    """The slab's 32 column sums as the finish launch forms them: float64; rows g, g + 32, ... in ascending order, then a balanced tree over g."""
    slab = np.asarray(slab, dtype=np.float32).astype(np.float64)
    S = np.zeros((32, slab.shape[1]), np.float64)
    with np.errstate(all="ignore"):
        for at in range(0, slab.shape[0], 32):
            chunk = slab[at:at + 32]
            S[:chunk.shape[0]] = S[:chunk.shape[0]] + chunk
        while S.shape[0] > 1:
            S = S[0::2] + S[1::2]
    return S[0]


def solve_host(total, damping):
    """Steps 2 and 3 of the finish launch in float64 (Python floats, the kernel's order) -> (T [3,4] float32: the Cayley rotation and the
    translation, xi [6] float64), or (None, None) for SDE_ALIGN_SINGULAR."""
    total = [float(x) for x in total]
    Am = [[0.0] * 6 for _ in range(6)]
    at = 0
    for i in range(6):
        for j in range(i, 6):
            Am[i][j] = Am[j][i] = total[at]
            at += 1
    lm = 1.0 + float(np.float32(damping))
    for i in range(6):
        Am[i][i] = Am[i][i] * lm
    Lm = [[0.0] * 6 for _ in range(6)]
    dg, x = [0.0] * 6, [0.0] * 6
    with np.errstate(all="ignore"):
        f = np.float64                                      # numpy scalars: a division by zero gives inf / nan as on the device, no exception
        for j in range(6):
            s = f(Am[j][j])
            for c in range(j):
                s = s - (f(Lm[j][c]) * f(Lm[j][c])) * f(dg[c])
            dg[j] = s
            if not (s > 0.0 and np.isfinite(s)):
                return None, None
            for i in range(j + 1, 6):
                w = f(Am[i][j])
                for c in range(j):
                    w = w - (f(Lm[i][c]) * f(Lm[j][c])) * f(dg[c])
                Lm[i][j] = w / s
        for i in range(6):
            s = f(-total[21 + i])
            for c in range(i):
                s = s - f(Lm[i][c]) * f(x[c])
            x[i] = s
        for i in range(6):
            x[i] = f(x[i]) / f(dg[i])
        for i in range(4, -1, -1):
            s = f(x[i])
            for c in range(i + 1, 6):
                s = s - f(Lm[c][i]) * f(x[c])
            x[i] = s
        if not all(np.isfinite(np.float32(v)) for v in x):
            return None, None
        a = [f(0.5) * f(x[0]), f(0.5) * f(x[1]), f(0.5) * f(x[2])]
        aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
        den, one = f(1.0) + aa, f(1.0) - aa
        two = f(2.0)
        R = [[(one + two * (a[0] * a[0])) / den, (two * (a[0] * a[1]) - two * a[2]) / den, (two * (a[0] * a[2]) + two * a[1]) / den],
             [(two * (a[0] * a[1]) + two * a[2]) / den, (one + two * (a[1] * a[1])) / den, (two * (a[1] * a[2]) - two * a[0]) / den],
             [(two * (a[0] * a[2]) - two * a[1]) / den, (two * (a[1] * a[2]) + two * a[0]) / den, (one + two * (a[2] * a[2])) / den]]
        T = np.zeros((3, 4), np.float32)
        T[:, :3] = np.array(R, np.float64).astype(np.float32)
        T[:, 3] = np.array(x[3:], np.float64).astype(np.float32)
    return T, np.array(x, np.float64)


def finish_host(words, slab, min_count, damping, mode):
    """The finish launch: words (40 float32, the state on entry) and the slab -> the state it leaves."""
    f32 = np.float32
    w = np.array(words, dtype=f32).reshape(STATE_WORDS).copy()
    info = w.view(np.int32)
    total = totals_host(slab)
    count, count_s = int(total[28]), int(total[30])
    info[COUNT_AT], info[SCALE_COUNT_AT] = count, count_s
    with np.errstate(all="ignore"):
        w[SUMSQ_AT] = f32(total[27])
        if count < int(min_count):
            info[STATUS_AT] = TOO_FEW
            return w
        Dn = None
        if mode & POSE:
            T, _ = solve_host(total, damping)
            if T is None:
                info[STATUS_AT] = SINGULAR
                return w
            D = w[:16].reshape(4, 4)
            Dn = np.zeros((3, 4), f32)
            for r in range(3):
                row = T[r, 0] * D[0] + T[r, 1] * D[1] + T[r, 2] * D[2]
                row[3] = row[3] + T[r, 3]
                Dn[r] = row
        if (mode & SCALE) and count_s >= int(min_count):
            w[SCALE_AT] = w[SCALE_AT] * f32(total[29] / np.float64(count_s))
        if Dn is not None:
            w[:12] = Dn.reshape(-1)
            Di = w[16:32].reshape(4, 4)
            for r in range(3):
                Di[r, :3] = Dn[:, r]
                Di[r, 3] = -((Dn[0, r] * Dn[0, 3] + Dn[1, r] * Dn[1, 3]) + Dn[2, r] * Dn[2, 3])
    info[STATUS_AT] = OK
    return w


def frame_align_host(words, pred, ymap, xmap, K, model_depth, model_normal, mode=POSE | SCALE, dist_tol=DEFAULTS["dist_tol"],
                     scale_tol=DEFAULTS["scale_tol"], min_count=DEFAULTS["min_count"], damping=DEFAULTS["damping"], min_depth=0.0, max_depth=80.0):
    """The host twin of one sde_frame_align call: words (40 float32: state_host() for a fresh state) -> the new 40 words, the kernel's bits."""
    dist_tol, scale_tol, min_count, damping, mode, min_depth, max_depth = check_align(dist_tol, scale_tol, min_count, damping, mode, min_depth, max_depth)
    w = np.asarray(words, dtype=np.float32).reshape(STATE_WORDS)
    t = align_terms_host(pred, ymap, xmap, K, model_depth, model_normal, w[:16].reshape(4, 4), w[SCALE_AT], min_depth, max_depth, dist_tol, scale_tol)
    return finish_host(w, slab_host(t["terms"]), min_count, damping, mode)


def track_host(render, pred, ymap, xmap, K, schedule=DEFAULT_SCHEDULE, min_depth=0.0, max_depth=80.0, **kw):
    """The host twin of TsdfVolume.track given the rendered model: render = (model_depth, model_normal) -> the state after the schedule."""
    w = state_host()
    for mode in schedule:
        w = frame_align_host(w, pred, ymap, xmap, K, render[0], render[1], mode=mode, min_depth=min_depth, max_depth=max_depth, **kw)
    return w

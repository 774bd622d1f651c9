"""What tests/test_predictor.py (CPU) and tests/test_gpu_predictor.py (GPU) share: the cases of the sde_depth_present tests and the numpy
restatement of the kernel's definition (include/sde_hip.h), computed in float64."""
import numpy as np

VMAX, GAMMA = 80.0, 0.8
SLACK = 1e-3                       # a pixel whose float64 t * 256 lies this close to an integer may take either neighbouring index


def _nearest(src, dst):
    return np.minimum(np.floor(np.arange(dst, dtype=np.float64) * (src / dst)).astype(np.int64), src - 1).astype(np.int32)


def case_maps(name):
    """(ph, pw, ymap, xmap) of the three shapes."""
    if name == "paste":            # (5, 7) pasted into (9, 13) at (4, 3): rows of 39 bytes
        ymap = np.full(9, -1, np.int32); ymap[4:9] = np.arange(5)
        xmap = np.full(13, -1, np.int32); xmap[3:10] = np.arange(7)
        return 5, 7, ymap, xmap
    if name == "resize_pad":       # (6, 10) nearest-resized to (11, 23), then top-padded to (15, 23)
        return 6, 10, np.concatenate([np.full(4, -1, np.int32), _nearest(6, 11)]), _nearest(10, 23)
    if name == "identity":         # (64, 96): the one with enough pixels for the boundary statistics
        return 64, 96, np.arange(64, dtype=np.int32), np.arange(96, dtype=np.int32)
    raise KeyError(name)


CASES = ("paste", "resize_pad", "identity")
SEEDS = {"paste": 11, "resize_pad": 12, "identity": 13}


def case_inputs(name, N):
    """pred [N,ph,pw] float32 uniform in [0, 1.25 vmax] with the special values planted, frame [N,H,W,3] uint8, and the maps."""
    ph, pw, ymap, xmap = case_maps(name)
    rng = np.random.default_rng(SEEDS[name] + 100 * N)
    pred = (rng.random((N, ph, pw)) * 1.25 * VMAX).astype(np.float32)
    flat = pred.reshape(N, -1)
    special = np.array([0.0, VMAX, 1e-42, np.nan, np.inf, -3.5], dtype=np.float32)      # exact 0, exact vmax, a denormal, NaN, +inf, a negative value
    for n in range(N):
        flat[n, 3 + n: 3 + n + 6 * 5: 5] = special
    frame = rng.integers(0, 256, (N, ymap.size, xmap.size, 3), dtype=np.uint8)
    return pred, frame, ymap, xmap


def reference(pred, ymap, xmap, lut, vmax=VMAX, gamma=GAMMA):
    """depth_full (float32), depth_u16 (uint16), colour index (int), boundary mask, other admissible index -- from the definition, in float64."""
    r, c = ymap[:, None], xmap[None, :]
    inside = (r >= 0) & (c >= 0)
    full = np.where(inside[None], pred[:, np.maximum(r, 0), np.maximum(c, 0)], np.float32(0)).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = full * np.float32(255)                                   # write_depth: the float32 product, truncated
        u16 = np.where(np.isnan(prod) | (prod <= 0), 0, np.minimum(prod, 65535)).astype(np.float64)
        u16 = np.floor(u16).astype(np.uint16)
        d = full.astype(np.float64)
        d = np.where(np.isnan(d) | (d < 0), 0.0, d)
        s = np.where(np.isinf(d), np.inf, d ** gamma / float(vmax) ** gamma * 256.0)
    fin = np.where(np.isinf(s), 1e9, s)
    idx = np.minimum(255, np.floor(fin)).astype(np.int64)
    lo = np.clip(np.floor(fin - SLACK), 0, 255).astype(np.int64)
    hi = np.clip(np.floor(fin + SLACK), 0, 255).astype(np.int64)
    other = np.where(lo != idx, lo, hi)
    return full, u16, idx, other != idx, other


def boundary_share(name, N, lut):
    pred, _, ymap, xmap = case_inputs(name, N)
    return float(reference(pred, ymap, xmap, lut)[3].mean())

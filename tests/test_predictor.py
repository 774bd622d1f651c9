"""CPU: the inference path's host side -- sde_depth_present's ABI and refusals, the colour table, DepthPredictor's per-size tables against this
package's CPU preprocess chain, the index-map validation and the tool's command line.  The kernel and the predictor itself: test_gpu_predictor.py."""
import ctypes
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import present_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "sde_hip.h")
LIB = os.path.join(ROOT, "simpledepthestimation_amd", "libsde_hip.so")
MAGMA_SHA256 = "e2e7c21b2cdebd6f55d07fae05ea13bb4b4f0908509892384b87c747b9f319f6"      # matplotlib 3.10's magma, 256 x RGB


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_present_is_declared_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    assert re.search(r"\bint\s+sde_depth_present\s*\(", src)
    from simpledepthestimation_amd.hip import lib as L
    import simpledepthestimation_amd.hip.present  # noqa: F401
    args, res = L._PROTOS["sde_depth_present"]
    decl = re.search(r"\bsde_depth_present\s*\(([^;{}]*?)\)\s*;", src, flags=re.S).group(1)
    assert len(args) == decl.count(",") + 1 and res is ctypes.c_int


@pytest.fixture(scope="module")
def present_fn():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(LIB)
    lib.sde_last_error.restype = ctypes.c_char_p
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.sde_depth_present.argtypes = [P, I, I, I, P, P, I, I, F, F, P, P, P, P, P, P]
    lib.sde_depth_present.restype = I
    return lib


GOOD = dict(pred=0x1000, N=1, ph=4, pw=4, ymap=0x2000, xmap=0x3000, H=4, W=4, vmax=80.0, gamma=0.8, lut=0x4000, frame=None, depth=None, u16=None, canvas=0x5000)


@pytest.mark.parametrize("change, word", [
    (dict(N=0), "shape"), (dict(H=0), "shape"), (dict(W=-1), "shape"), (dict(ph=0), "shape"), (dict(pw=0), "shape"),
    (dict(vmax=0.0), "vmax"), (dict(vmax=-1.0), "vmax"), (dict(gamma=0.0), "gamma"),
    (dict(pred=None), "null"), (dict(ymap=None), "null"), (dict(xmap=None), "null"), (dict(lut=None), "null"), (dict(canvas=None), "null")])
def test_present_refusals(present_fn, change, word):
    """Every refusal happens on the host, before any launch: the pointers here are not memory, and there is no GPU."""
    a = dict(GOOD, **change)
    rc = present_fn.sde_depth_present(a["pred"], a["N"], a["ph"], a["pw"], a["ymap"], a["xmap"], a["H"], a["W"], a["vmax"], a["gamma"], a["lut"], a["frame"],
                                      a["depth"], a["u16"], a["canvas"], None)
    msg = present_fn.sde_last_error().decode()
    assert rc < 0 and "sde_depth_present" in msg and word in msg, (rc, msg)


# ---- colour table ------------------------------------------------------------------------------------------------------------------------
def test_magma_table():
    from simpledepthestimation_amd.utils.colormap import magma_u8
    lut = magma_u8()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert hashlib.sha256(lut.tobytes()).hexdigest() == MAGMA_SHA256
    try:
        import matplotlib
    except ImportError:
        return
    assert np.array_equal(lut, matplotlib.colormaps["magma"](np.arange(256), bytes=True)[:, :3])
    lut[0, 0] ^= 1
    assert not np.array_equal(lut, magma_u8())          # callers get copies


def test_boundary_share_of_the_gpu_cases():
    """The GPU test lets pixels whose float64 t * 256 lies within 1e-3 of an integer take either index and asserts that at most 1 % of a case's
    pixels are such pixels; the seeds of present_ref.py are checked here, where no GPU is needed (expected share: 2e-3 / 1 * ~0.8 of the range)."""
    from simpledepthestimation_amd.utils.colormap import magma_u8
    for name in PR.CASES:
        for N in (1, 3):
            assert PR.boundary_share(name, N, magma_u8()) <= 0.01, (name, N)


# ---- forward tables, metadata, backward maps ---------------------------------------------------------------------------------------------
CHAINS = {
    "kbcrop": ([{"NAME": "KBCrop"}], (375, 1242)),
    "crop_resize": ([{"NAME": "CropTopTo", "IMG_H": 72}, {"NAME": "Resize", "IMG_H": 64, "IMG_W": 192}], (80, 200)),
    "resize": ([{"NAME": "Resize", "IMG_H": 64, "IMG_W": 192}], (80, 200)),
    "resize_one_axis": ([{"NAME": "Resize", "IMG_H": 80, "IMG_W": 192}], (80, 200)),
}


def cpu_chain(steps, frame, K=None):
    from simpledepthestimation_amd.data.preprocess import build_preprocess
    import simpledepthestimation_amd.data.preprocess.augmentation, simpledepthestimation_amd.data.preprocess.formating  # noqa: F401,E401
    data = {"img": frame.copy(), "metadata": {}}
    if K is not None:
        data["intrinsics"] = K.copy()
    for s in list(steps) + [{"NAME": "ToTensor"}]:
        data = build_preprocess(s).forward(data)
    return data


def apply_taps(frame, plan):
    """The plan's tables applied to one uint8 [Hs,Ws,3] frame in numpy: the 2-tap 11-bit fixed-point rule of _linear_coefs / resize_linear_u8 read
    through the tables (what sde_image_prep_u8 computes), then ToTensor's division by 255 in float32.  float32 [3,h,w]."""
    src = np.asarray(frame).astype(np.int64)
    y0, y1, b0, b1 = (plan.ytab[:, k].astype(np.int64) for k in range(4))
    x0, x1, a0, a1 = (plan.xtab[:, k].astype(np.int64) for k in range(4))
    rows0 = src[y0][:, x0] * a0[None, :, None] + src[y0][:, x1] * a1[None, :, None]
    rows1 = src[y1][:, x0] * a0[None, :, None] + src[y1][:, x1] * a1[None, :, None]
    out = (((b0[:, None, None] * (rows0 >> 4)) >> 16) + ((b1[:, None, None] * (rows1 >> 4)) >> 16) + 2) >> 2
    out = np.clip(out, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(out.transpose(2, 0, 1)).astype(np.float32) / np.float32(255)


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_forward_tables_match_the_cpu_chain(name):
    from simpledepthestimation_amd.engine.predictor import SizePlan, chain_steps
    from simpledepthestimation_amd.evaluation.depth_evaluation import backward_maps
    steps, (Hs, Ws) = CHAINS[name]
    frame = np.random.default_rng(5).integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
    K = np.array([[721.5, 0, 609.6], [0, 721.5, 172.9], [0, 0, 1]], dtype=np.float32)
    ref = cpu_chain(steps, frame, K)
    plan = SizePlan(chain_steps(None, steps), Hs, Ws)
    got = apply_taps(frame, plan)
    want = ref["img"].numpy()
    assert got.shape == want.shape == (3, plan.h, plan.w) and got.dtype == want.dtype == np.float32
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert plan.meta == ref["metadata"]
    assert plan.xtab.dtype == np.int32 and plan.xtab.shape == (plan.w, 4) and plan.ytab.shape == (plan.h, 4)
    assert plan.ytab[:, :2].min() >= 0 and plan.ytab[:, :2].max() < Hs and plan.xtab[:, :2].min() >= 0 and plan.xtab[:, :2].max() < Ws
    if name == "kbcrop":            # no axis is resized: identity taps behind the crop's offsets
        assert np.array_equal(plan.ytab, np.stack([np.arange(352) + 23, np.arange(352) + 23, np.full(352, 2048), np.zeros(352)], 1))
        assert np.array_equal(plan.xtab[:, 0], np.arange(1216) + 13)
    # intrinsics: what the chain's forward steps leave
    assert np.array_equal(plan.intrinsics(K), ref["intrinsics"])
    assert np.array_equal(plan.intrinsics(np.stack([K, K]))[1], ref["intrinsics"])
    # backward maps: backward_maps of that metadata, by the chain's names
    rows, cols = plan.maps((plan.h, plan.w))
    r2, c2 = backward_maps((plan.h, plan.w), ref["metadata"], [s["NAME"] for s in steps])
    assert rows.dtype == np.int32 and np.array_equal(rows, r2) and np.array_equal(cols, c2) and (rows.size, cols.size) == (Hs, Ws)


def test_chain_defaults_and_errors():
    from simpledepthestimation_amd.config import get_cfg
    from simpledepthestimation_amd.engine.predictor import SizePlan, chain_steps
    cfg = get_cfg()
    assert [n for n, _ in chain_steps(cfg)] == ["KBCrop"]                   # a config without image steps: demo.py's chain
    cfg.merge_from_other_cfg({"DATASETS": {"TEST": {"PREPROCESS": [{"NAME": "LoadImg"}] + CHAINS["crop_resize"][0] + [{"NAME": "ToTensor"}]}}})
    assert chain_steps(cfg) == [("CropTopTo", {"NAME": "CropTopTo", "IMG_H": 72}), ("Resize", {"NAME": "Resize", "IMG_H": 64, "IMG_W": 192})]
    assert chain_steps(cfg, ["Resize"]) == [("Resize", {"NAME": "Resize", "IMG_H": 64, "IMG_W": 192})]      # names take their sizes from the config
    with pytest.raises(ValueError):
        chain_steps(cfg, ["RandomCrop"])
    with pytest.raises(ValueError):
        SizePlan(chain_steps(None, ["KBCrop"]), 300, 1000)                  # smaller than the crop
    with pytest.raises(ValueError):
        SizePlan(chain_steps(cfg), 60, 200)                                 # CropTopTo(72) of 60 rows


# ---- map validation ----------------------------------------------------------------------------------------------------------------------
def test_map_validation():
    from simpledepthestimation_amd.hip.lib import SdeHipError
    from simpledepthestimation_amd.hip.present import check_maps
    ymap, xmap = np.arange(6, dtype=np.int32), np.arange(8, dtype=np.int32)
    check_maps(ymap, xmap, 6, 8, 6, 8)
    check_maps(np.full(6, -1, np.int32), xmap, 6, 8, 6, 8)
    for bad_y, bad_x, H, W in ((np.array([0, 1, 2, 3, 4, 6], np.int32), xmap, 6, 8),            # an entry >= ph
                               (ymap, np.array([0, 1, 2, 3, 4, 5, 6, 8], np.int32), 6, 8),      # ... >= pw
                               (np.array([0, 1, -2, 3, 4, 5], np.int32), xmap, 6, 8),            # < -1
                               (ymap, xmap, 7, 8), (ymap, xmap, 6, 9),                            # wrong lengths
                               (ymap.astype(np.int64), xmap, 6, 8)):                              # wrong type
        with pytest.raises(SdeHipError):
            check_maps(bad_y, bad_x, 6, 8, H, W)


# ---- tool --------------------------------------------------------------------------------------------------------------------------------
def test_demo_help():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "simpledepthestimation_amd.tools.demo", "--help"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for flag in ("--cfg", "--input", "--output", "--opts", "--save-depth", "--no-frame"):
        assert flag in r.stdout
    assert "video" in r.stdout

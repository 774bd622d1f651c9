"""CPU: the float64 restatement of the MotionLearning loss stack (tests/motion_loss_ref.py) against the reference's golden run
(tests/golden/motion_loss.npz, written by scripts/gen_golden_motion_loss.py) and, where the reference checkout is present, against the reference's own
functions in float64; the public names import and refuse CPU tensors.

Golden bound: max(1e-6, 8 x d), d = the reference's own fp32-vs-fp64 difference of the quantity (the golden values are its fp32 run, the restatement
runs in fp64, so the two differ by about d)."""
import importlib
import os
import sys
import types

import numpy as np
import pytest
import torch

import motion_loss_init as MI
import motion_loss_ref as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "motion_loss.npz"))


def ref_rgbd(fA, fB, dA, dB, K, R, t, dl1_w, ssim_w, C1, C2):
    return REF.rgbd_consistency_loss(fA, fB, dA, dB, K, R, t, dl1_w, ssim_w, C1, C2)


@pytest.mark.parametrize("ci", range(len(MI.CASES)))
def test_restatement_reproduces_golden(ci):
    size, C1, C2, dl1_w = MI.CASES[ci]
    res = MI.run_stack(ref_rgbd, REF.motion_consistency_loss, MI.inputs(*MI.SIZES[size]), C1, C2, dl1_w, torch.float64, "cpu")
    bad = MI.compare_with_golden(res, GOLD, ci, 1e-6, 1e-6, exact=True)
    assert not bad, bad


def _reference():
    sys.path.insert(0, ROOT)
    from oracle import ref_harness
    if not ref_harness.available():
        pytest.skip("reference checkout not present")
    ref_harness.load()
    imp = importlib.import_module
    return (imp("detectron2.geometry.camera"), imp("detectron2.modeling.losses.ssim_loss"), imp("detectron2.modeling.losses.motion_loss"),
            imp("detectron2.modeling.meta_arch.MotionLearning"))


def test_restatement_equals_reference_in_float64():
    cam, SS, MLoss, ML = _reference()
    inp = MI.inputs(*MI.SIZES["small"], seed=3)
    for C1, C2 in MI.SSIM_CONSTS + [(1e-4, 9e-4)]:
        def their_rgbd(fA, fB, dA, dB, K, R, t, dl1_w, ssim_w, C1_, C2_):
            ns = types.SimpleNamespace(depth_l1_loss_w=dl1_w, ssim_loss_w=ssim_w, ssim=SS.WeightedSSIM(C1_, C2_))
            return ML.MotionLearningModel.rgbd_consistency_loss(ns, fA, fB, dA, dB, K, R, t)
        a = MI.run_stack(ref_rgbd, REF.motion_consistency_loss, inp, C1, C2, 1.0, torch.float64, "cpu")
        b = MI.run_stack(their_rgbd, MLoss.motion_consistency_loss, inp, C1, C2, 1.0, torch.float64, "cpu")
        for k in a:
            d = float((a[k].double() - b[k].double()).abs().max() / b[k].double().abs().max())
            assert d <= 1e-10, (C1, C2, k, d)
    g = torch.Generator().manual_seed(5)
    f = torch.randn(2, 3, 9, 14, generator=g, dtype=torch.float64)
    assert abs(float(REF.motion_smoothness_loss_fn(f) - MLoss.motion_smoothness_loss_fn(f))) <= 1e-12
    assert abs(float(REF.motion_sparsity_loss_fn(f) - MLoss.motion_sparsity_loss_fn(f))) <= 1e-12
    assert torch.equal(REF.resize_img_avgpool(f, (4, 5)), cam.resize_img_avgpool(f, (4, 5)))
    v = {k: x.double() for k, x in inp.items()}
    for t in (v["t12"], v["t12"][:, :, :1, :1].expand(-1, -1, *v["t12"].shape[-2:])):
        for x, y in zip(REF.view_synthesis(torch.cat([v["frame2"], v["depth2"]], 1), v["depth1"], v["K"], v["R12"], t),
                        cam.view_synthesis(torch.cat([v["frame2"], v["depth2"]], 1), v["depth1"], v["K"], v["R12"], t)):
            assert float((x.double() - y.double()).abs().max()) <= 1e-10


def test_public_names_import_and_refuse_cpu_tensors():
    from simpledepthestimation_amd.geometry import resize_img_avgpool, view_synthesis
    from simpledepthestimation_amd.hip.lib import SdeHipError
    from simpledepthestimation_amd.modeling.losses import (WeightedSSIM, motion_consistency_loss, motion_smoothness_loss_fn, motion_sparsity_loss_fn,
                                                           rgbd_consistency_loss)
    v = MI.inputs(1, 8, 12)
    with pytest.raises(SdeHipError):
        view_synthesis(v["frame2"], v["depth1"], v["K"], v["R12"], v["t12"])
    with pytest.raises(SdeHipError):
        resize_img_avgpool(v["frame1"], (4, 6))
    with pytest.raises(SdeHipError):
        WeightedSSIM(float("inf"), 9e-6)(v["frame1"], v["frame2"], v["depth1"])
    with pytest.raises(SdeHipError):
        rgbd_consistency_loss(v["frame1"], v["frame2"], v["depth1"], v["depth2"], v["K"], v["R12"], v["t12"], depth_l1_w=1.0, ssim_w=3.0, C1=float("inf"), C2=9e-6)
    with pytest.raises(SdeHipError):
        motion_consistency_loss(torch.zeros(1, 8, 12, 2), v["depth1"], v["R12"], v["R21"], v["t12"], v["t21"])
    with pytest.raises(SdeHipError):
        motion_smoothness_loss_fn(v["t12"])
    with pytest.raises(SdeHipError):
        motion_sparsity_loss_fn(v["t12"])


def test_product_does_not_import_oracle():
    import subprocess
    code = ("import sys; import simpledepthestimation_amd.modeling.losses, simpledepthestimation_amd.geometry; "
            "bad=[m for m in sys.modules if m=='oracle' or m.startswith('oracle.')]; sys.exit(1 if bad else 0)")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0

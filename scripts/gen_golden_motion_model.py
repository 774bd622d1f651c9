"""Writes tests/golden/motion_model.npz from the reference's own MotionLearningModel.forward (run on the CPU, unmodified).

Usage: python scripts/gen_golden_motion_model.py   (needs the reference checkout named by oracle.ref_harness; not used on the GPU machine)

The model instance is made without the registries (__new__ + nn.Module.__init__ + attributes, tests/motion_model_ref.make_instance); its depth_net and
pose_net are the stub modules of tests/motion_model_ref.py, whose predictions are parameters filled from the recipe of tests/motion_loss_init.py.  The
occlusion masks are not part of the reference's output: they are read off the return value of its rgbd_consistency_loss through an instance attribute
that forwards to the class's method.  Every case of motion_model_ref.CASES runs in fp32 (the golden values) and in fp64 (their error bars); the
objective is the sum of all loss entries.  Contents (arrays and name lists only):
  {case}_loss_names, {case}_{loss name}      the loss entries the reference produces, fp32
  {case}_g_{depth,rot,trans,motion}          fp32 gradients of the stub networks' parameters, {case}_gn_*: their norms
  {case}_occ{i}, {case}_occ_shapes           np.packbits of the occlusion masks [2B,1,h,w] (1 -> 2 | 2 -> 1) per scale, coarsest first
  {case}_d_*                                 the reference's own fp32-vs-fp64 difference of each of the above (tensors: max |a - b| / max |b|; losses and
                                             norms: |a - b| / |b|)
  state_dict_names, state_dict_shapes        of the reference's MotionLearningModel built from projects/MotionLearning/configs/resnet18.yaml (state_dict_layout)
Asserted here: the occlusion masks of the two runs differ on at most 0.1 % of the pixels, and at most 0.1 % of the elements of a gradient map differ by
more than 3e-3 * max (the caps the tests apply)."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from oracle import ref_harness  # noqa: E402
import motion_model_ref as MM  # noqa: E402


def rel_t(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


def reference_fn(ML, SS, LL, name, dtype):
    s = MM.settings(name)

    def fn(batch, depth_net, pose_net, record):
        model = MM.make_instance(ML.MotionLearningModel, s, depth_net, pose_net, SS.WeightedSSIM(s["C1"], s["C2"]), LL.silog_loss(s["variance_focus"]), dtype, "cpu")

        def recording(*args):
            out = ML.MotionLearningModel.rgbd_consistency_loss(model, *args)
            record.append(out["occlusion_mask"].detach())
            return out
        model.rgbd_consistency_loss = recording
        out = model(batch)
        record[:] = [torch.cat(record[i:i + 2], 0) for i in range(0, len(record), 2)]
        return out
    return fn


class CN(dict):
    __getattr__ = dict.__getitem__


def _merge(a, b):
    for k, v in b.items():
        if isinstance(v, dict) and isinstance(a.get(k), dict):
            _merge(a[k], v)
        else:
            a[k] = v


def state_dict_layout(ML):
    """Names and shapes of the state dict of the reference's own MotionLearningModel, built on the CPU from projects/MotionLearning/configs/resnet18.yaml
    over Base.yaml.  The reference's config package does not import here (no fvcore), so the two files are read with yaml and merged into an attribute
    dict; added are only what its defaults.py supplies (PIXEL_MEAN / PIXEL_STD) and ENCODER_NAME "18" for "18pt" (the same layout, no weight download)."""
    import yaml
    import gen_golden_google
    gen_golden_google.load_ref()                       # the torchvision shims the reference's GoogleResNet needs, as in scripts/gen_golden_google.py
    importlib.import_module("detectron2.modeling.pose_net.GooglePoseNet")      # registers GoogleMotionNet
    d = os.path.join(ref_harness.REF_ROOT, "projects", "MotionLearning", "configs")
    with open(os.path.join(d, "Base.yaml")) as f:
        cfg = yaml.safe_load(f)
    with open(os.path.join(d, "resnet18.yaml")) as f:
        top = yaml.safe_load(f)
    assert top.pop("_BASE_") == "./Base.yaml"
    _merge(cfg, top)
    cfg["MODEL"].update(PIXEL_MEAN=[0.485, 0.456, 0.406], PIXEL_STD=[0.229, 0.224, 0.225])
    assert cfg["MODEL"]["DEPTH_NET"]["ENCODER_NAME"] == "18pt"
    cfg["MODEL"]["DEPTH_NET"]["ENCODER_NAME"] = "18"
    wrap = lambda v: CN({k: wrap(x) for k, x in v.items()}) if isinstance(v, dict) else v
    sd = ML.MotionLearningModel(wrap(cfg)).state_dict()
    return list(sd), [",".join(str(n) for n in v.shape) for v in sd.values()]


def main():
    ref_harness.load()
    SS = importlib.import_module("detectron2.modeling.losses.ssim_loss")
    LL = importlib.import_module("detectron2.modeling.losses.losses")
    ML = importlib.import_module("detectron2.modeling.meta_arch.MotionLearning")
    out = {}
    for name in MM.CASES:
        a = MM.run_case(name, reference_fn(ML, SS, LL, name, torch.float32), torch.float32, "cpu")
        b = MM.run_case(name, reference_fn(ML, SS, LL, name, torch.float64), torch.float64, "cpu")
        p = name + "_"
        out[p + "loss_names"] = np.array(sorted(a["losses"]))
        for k in a["losses"]:
            va, vb = a["losses"][k].item(), b["losses"][k].item()
            out[p + k], out[p + "d_" + k] = np.float64(va), np.float64(abs(va - vb) / abs(vb))
        out[p + "occ_shapes"] = np.array([list(m.shape) for m in a["occ"]])
        flips = 0.0
        for i, (ma, mb) in enumerate(zip(a["occ"], b["occ"])):
            f = float((ma != mb.float()).double().mean())
            flips = max(flips, f)
            assert f <= MM.MAX_OFF, (name, i, f)
            out[p + f"occ{i}"] = np.packbits(ma.numpy().astype(np.uint8).reshape(-1))
        worst = 0.0
        for k, ga in a["grads"].items():
            gb = b["grads"][k]
            off = float(((ga.double() - gb).abs() > MM.GRAD_TOL * gb.abs().max()).double().mean())
            worst = max(worst, off)
            assert off <= MM.MAX_OFF, (name, k, off)
            out[p + "g_" + k], out[p + "d_g_" + k] = ga.numpy(), np.float64(rel_t(ga, gb))
            na, nb = ga.double().norm().item(), gb.norm().item()
            out[p + "gn_" + k], out[p + "d_gn_" + k] = np.float64(na), np.float64(abs(na - nb) / nb)
        print(f"{name}: occ {[round(100 * m.mean().item(), 1) for m in a['occ']]} % flips {flips:.1e} off-tolerance grads {worst:.1e} "
              + " ".join(f"{k} {out[p + k]:.4g} (d {out[p + 'd_' + k]:.1e})" for k in sorted(a["losses"]))
              + " " + " ".join(f"d_g_{k} {out[p + 'd_g_' + k]:.1e}" for k in a["grads"]))
    names, shapes = state_dict_layout(ML)
    out["state_dict_names"], out["state_dict_shapes"] = np.array(names), np.array(shapes)
    path = os.path.join(ROOT, "tests", "golden", "motion_model.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

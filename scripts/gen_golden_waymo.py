"""Generates tests/golden/waymo.npz by RUNNING the reference's own WaymoDepth class (build container only; not needed at test time).

detectron2/data/datasets/waymo.py cannot be imported (its package pulls in cv2, fvcore, ...), so -- as oracle/gen_golden_data.py does for the KITTI
reader, with that module's `_compile` and `Cfg` -- the class definition is compiled, unmodified, from the file's syntax tree into a namespace holding
numpy / os / pickle / torch and stand-ins for the registry decorator and DatasetBase.  The class runs on the synthetic tree of tests/waymo_tree.py for
that module's CASES; stored are the index (metadatas, valid_inds, context_list), every sample's metadata (paths relative to the tree) and intrinsics, and
what batch_collator makes of tests/waymo_tree.fake_samples().  Also written: tests/golden/configs_waymo.json, the parsed mappings of
projects/MotionLearning/configs/{Base_waymo,resnet18_waymo}.yaml (the form oracle/gen_golden_config.py stores the other projects' YAMLs in).  Loading (cv2) is not reachable this way: tests/test_waymo.py pins it by round trips.

    python scripts/gen_golden_waymo.py
"""
import collections
import json
import logging
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.gen_golden_data import REF, Cfg, _compile, _DatasetBase, _Reg  # noqa: E402
from waymo_tree import CASES, fake_samples, make_waymo_tree  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "waymo.npz")


def reference_dataset():
    ns = {"np": np, "os": os, "pickle": pickle, "torch": torch, "defaultdict": collections.defaultdict, "logger": logging.getLogger("ref"),
          "DATASET_REGISTRY": _Reg(), "DatasetBase": _DatasetBase}
    return _compile(os.path.join(REF, "datasets", "waymo.py"), ("WaymoDepth",), ns)["WaymoDepth"]


def _rel(v, tmp):
    if isinstance(v, str):
        return os.path.relpath(v, tmp) if v.startswith(tmp) else v
    if isinstance(v, list):
        return [_rel(x, tmp) for x in v]
    if isinstance(v, dict):
        return {str(k): _rel(x, tmp) for k, x in v.items()}
    return v


def main():
    Ref = reference_dataset()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        image, depth, seg, infos = make_waymo_tree(tmp)
        for tag, kw in CASES.items():
            kw = dict(kw)
            if kw.get("MASK_ROOT"):
                kw["MASK_ROOT"] = seg
            ds = Ref(Cfg(dict(DATA_ROOT=image, DEPTH_ROOT=depth, SPLIT=infos, USE_CAMS=["FRONT"], PREPROCESS=[]), **kw), None)
            out[f"{tag}.metadatas"] = np.array([json.dumps([m[0], m[1], {str(k): v for k, v in m[2].items()}], sort_keys=True) for m in ds.metadatas])
            out[f"{tag}.valid_inds"] = np.array(ds.valid_inds, np.int64)
            out[f"{tag}.context"] = np.array([json.dumps(c) for c in ds.context_list])
            # two cameras: only the first segment has both, so only its samples can be read
            n = len(ds) if "USE_CAMS" not in kw else sum(1 for i in ds.valid_inds if all(c in ds.metadatas[i][2] for c in kw["USE_CAMS"]))
            items = [ds[i] for i in range(n)]
            out[f"{tag}.n_items"] = np.int64(n)
            out[f"{tag}.n_cams"] = np.array([len(it) for it in items], np.int64)
            out[f"{tag}.item_meta"] = np.array([json.dumps(_rel(d["metadata"], tmp), sort_keys=True) for it in items for d in it])
            out[f"{tag}.K"] = np.stack([d["intrinsics"] for it in items for d in it])
        b = ds.batch_collator(fake_samples())
        out["collate.keys"] = np.array(sorted(b.keys()))
        out["collate.types"] = np.array([f"{k}:{type(b[k]).__name__}:{type(b[k][0]).__name__ if isinstance(b[k], list) else ''}" for k in sorted(b.keys())])
        for k in ("img", "img_orig", "intrinsics", "depth", "mask"):
            out[f"collate.{k}"] = b[k].numpy()
        for k in ("ctx_img", "ctx_img_orig", "ctx_depth", "ctx_mask"):
            out[f"collate.{k}.n"] = np.int64(len(b[k]))
            for i, a in enumerate(b[k]):
                out[f"collate.{k}.{i}"] = np.asarray(a)
        out["collate.flip"] = np.array(b["flip"])
        out["collate.metadata"] = np.array([json.dumps(m, sort_keys=True) for m in b["metadata"]])
        out["collate.depth_orig.n"] = np.int64(len(b["depth_orig"]))
    np.savez_compressed(OUT, **out)
    # tests/golden/configs.json holds the MonoDepth2 and Supervised YAMLs; the MotionLearning Waymo pair, parsed the same way, goes beside it
    import yaml
    cfgs = {}
    for name in ("Base_waymo.yaml", "resnet18_waymo.yaml"):
        with open(os.path.join(os.path.dirname(os.path.dirname(REF)), "projects", "MotionLearning", "configs", name)) as f:
            cfgs[f"MotionLearning/{name}"] = yaml.safe_load(f)
    with open(os.path.join(ROOT, "tests", "golden", "configs_waymo.json"), "w") as f:
        json.dump(cfgs, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()

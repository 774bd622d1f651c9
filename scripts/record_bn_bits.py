#!/usr/bin/env python
"""Write tests/golden/bn_stream_bits.json: one SHA-256 per output tensor per case of tests/test_gpu_bn_stream_bits.py's table.

Record with the library whose bits are to be kept -- SDE_HIP_LIB selects another libsde_hip.so of the same ABI, e.g. the parent commit's build:
    SDE_HIP_LIB=/path/to/parent/libsde_hip.so python scripts/record_bn_bits.py
Every case runs twice and must hash alike, and every fused forward launch must equal sde_bn_apply on the bnp it wrote, before anything is written.
--out PATH writes elsewhere (to compare two libraries).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gpu_bn_stream_bits as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=T.GOLDEN)
    args = ap.parse_args()
    from simpledepthestimation_amd.hip import lib as L
    print("library:", L.LIB_PATH)
    rec = {}
    for name in T.CASES:
        rec[name], bad = T.run_case(name)
        again, _ = T.run_case(name)
        if bad:
            sys.exit(f"{name}: the fused launch and sde_bn_apply on its bnp differ in {bad}")
        if again != rec[name]:
            sys.exit(f"{name}: two runs differ in {sorted(k for k in again if again[k] != rec[name][k])}")
        print(f"{name}: {len(rec[name])} tensors")
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

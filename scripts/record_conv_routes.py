#!/usr/bin/env python
"""Record the convolution dispatcher's answers over the grid of tests/conv_route_sweep.py into tests/golden/conv_routes.json.

    SDE_HIP_LIB=/path/to/libsde_hip.so python scripts/record_conv_routes.py             # the library whose answers are the reference
    python scripts/record_conv_routes.py --against /path/to/other/libsde_hip.so        # no file written: first descriptors that differ

Host code only: no GPU is needed (the CU count falls back to 256, an MI355X's).  Record from the commit whose routes are to be kept (before a
refactor of the dispatcher), then tests/test_conv_route_sweep.py holds the result to them."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import conv_route_sweep as S                                  # noqa: E402
from simpledepthestimation_amd.hip import lib as L            # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_routes.json")


def show(d):
    return " ".join(f"{name}={getattr(d, name)}" for name, _ in d._fields_ if name not in ("x0", "x1"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--against", metavar="PATH", help="a second library: print the first descriptors whose answers differ, write nothing")
    ap.add_argument("--show", type=int, default=10, help="differences printed per (option set, dtype)")
    args = ap.parse_args()
    lib = S.bind(L.lib())
    print(f"library: {L.LIB_PATH}")
    if args.against:
        other = S.bind(ctypes.CDLL(args.against))
        bad = 0
        for dt, code in S.DTYPES.items():
            descs = S.descriptors(code)
            a, b = S.sweep(lib, descs), S.sweep(other, descs)
            for name in a:
                diff = [i for i, (x, y) in enumerate(zip(a[name], b[name])) if x != y]
                bad += len(diff)
                for i in diff[:args.show]:
                    d, Cout, ldy = descs[i]
                    print(f"[{name}] [{dt}] #{i} {show(d)} Cout={Cout} ldy={ldy}\n    {dict(zip(S.QUERIES, a[name][i]))}\n    {dict(zip(S.QUERIES, b[name][i]))}")
        print(f"{bad} answers differ" if bad else "every answer is the same")
        return 1 if bad else 0
    digests, defaults = S.digests(lib)
    hist = S.histogram(defaults)
    for name in S.COVER:
        print(f"{hist[name]:6d}  {name}" + ("" if hist[name] >= S.MIN_COVER else f"      < {S.MIN_COVER}: adjust the grid"))
    print(f"{hist['descriptors']:6d}  descriptors, {hist['refused']} refused")
    # queries that disagree with each other at the defaults (kept as they are: see sde_conv_fwd_variant in csrc/conv.hip)
    chalo_split = sum(1 for descs, rows in defaults.values() for t in rows if t[0] // 1000000 == 5 and t[2] > 0)
    print(f"{chalo_split:6d}  descriptors whose variant says chalo while a workspace would split them")
    with open(GOLDEN, "w") as f:
        json.dump({"digests": digests, "histogram": hist}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {GOLDEN}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

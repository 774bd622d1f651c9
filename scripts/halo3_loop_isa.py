"""ISA table of halo3_kernel's steady-state loop (csrc/conv.hip), one row per instantiation (BN 64/32/16 x three sources x bf16/fp16).

Compiles conv.hip device-only for gfx950 and, per instantiation, finds the loop that holds the most MFMAs (a backward branch to an earlier label)
and counts, between its first and its last MFMA: MFMAs, `s_waitcnt vmcnt(0)` (a drained vector-memory wait: the register prefetch hides nothing
past it), every other `s_waitcnt` that names vmcnt, scalar branches, barriers, SALU and VALU instructions; plus the kernel's VGPR count.  Nine
stages (taps) of FM x FN x 2 MFMAs make one channel block.  Only waitcnt, branch, barrier, MFMA and ALU mnemonics are read.

Usage (CPU, about a minute):  python scripts/halo3_loop_isa.py [--source path/to/conv.hip] [--flags "-DSDE_HALO3_WG_PER_CU=3"]
Exits 1 when a loop region holds a vmcnt(0).  profiles/halo3_loop_isa.txt keeps the output for the parent commit and for this tree."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simpledepthestimation_amd", "csrc")
SRC_NAMES = {0: "plain_zero", 1: "plain_reflect", 2: "upcat_reflect"}
NOT_SALU = ("s_waitcnt", "s_branch", "s_cbranch", "s_barrier", "s_nop", "s_load", "s_buffer_load", "s_endpgm", "s_setprio", "s_sleep")


def hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def assembly(source=None, flags=()):
    source = source or os.path.join(CSRC, "conv.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "conv.s")
        subprocess.run([hipcc(), "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{ROOT}/include", f"-I{CSRC}", *flags, "-S", "--cuda-device-only",
                        "-o", out, source], check=True, stderr=subprocess.DEVNULL)
        with open(out) as f:
            return f.read()


def loop_region(lines):
    """(first, last) line index of the MFMAs inside the backward-branch loop that holds the most of them, or None."""
    labels = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"(\.LBB\d+_\d+):", l))}
    mfma = [i for i, l in enumerate(lines) if l.lstrip().startswith("v_mfma")]
    best = None
    for i, l in enumerate(lines):
        m = re.match(r"\s*s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), i) < i:
            inside = [k for k in mfma if labels[m.group(1)] <= k <= i]
            if inside and (best is None or len(inside) > best[0]):
                best = (len(inside), inside[0], inside[-1])
    return None if best is None else best[1:]


def count(lines):
    c = dict(mfma=0, vmcnt0=0, vmcnt_n=0, branch=0, barrier=0, salu=0, valu=0)
    for l in lines:
        op = l.split("//")[0].split(";")[0].strip()
        if not op or op.endswith(":") or op.startswith("."):
            continue
        mn = op.split()[0]
        if mn.startswith("v_mfma"):
            c["mfma"] += 1
        elif mn == "s_waitcnt":
            if re.search(r"vmcnt\(0\)", op):
                c["vmcnt0"] += 1
            elif "vmcnt" in op:
                c["vmcnt_n"] += 1
        elif mn.startswith(("s_branch", "s_cbranch")):
            c["branch"] += 1
        elif mn == "s_barrier":
            c["barrier"] += 1
        elif mn.startswith("s_") and not mn.startswith(NOT_SALU):
            c["salu"] += 1
        elif mn.startswith("v_"):
            c["valu"] += 1
    return c


def analyse(source=None, flags=()):
    """One dict per halo3_kernel instantiation: dtype, bn, src, the loop-region counts, the peeled last block's vmcnt(0) count and the VGPRs."""
    rows = []
    for f in re.split(r"\n(?=_Z\w+:)", assembly(source, flags)):
        m = re.match(r"_Z\w*?12halo3_kernelI(\w+?)Li(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", f)
        if not m:
            continue
        lines = f.split("\n")
        end = next((i for i, l in enumerate(lines) if l.lstrip().startswith("s_endpgm")), len(lines))
        reg = loop_region(lines[:end])
        row = dict(dtype="bf16" if "b" in m.group(1) else "fp16", bn=int(m.group(2)), src=SRC_NAMES.get(int(m.group(5)), m.group(5)))
        row.update(count(lines[reg[0]:reg[1] + 1]) if reg else count([]))
        row["has_loop"] = reg is not None
        v = re.search(r";\s*NumVgprs:\s*(\d+)", f)
        a = re.search(r";\s*NumAgprs:\s*(\d+)", f)
        row["vgpr"] = int(v.group(1)) if v else -1
        row["agpr"] = int(a.group(1)) if a else 0
        sp = re.search(r";\s*ScratchSize:\s*(\d+)", f)
        row["scratch"] = int(sp.group(1)) if sp else 0
        rows.append(row)
    rows.sort(key=lambda r: (r["dtype"], -r["bn"], r["src"]))
    return rows


def table(rows):
    out = [f"{'instantiation':<28} {'stages':>6} {'mfma':>5} {'vmcnt(0)':>8} {'vmcnt(N)':>8} {'branch':>6} {'barrier':>7} {'salu':>5} {'valu':>5} {'vgpr':>5} {'agpr':>5} {'scratch':>7}"]
    for r in rows:
        per_stage = (128 // 16) * (r["bn"] // 16) * 2 // 4       # FM x FN x 2 MFMAs per wave and stage
        name = f"{r['dtype']} BN{r['bn']} {r['src']}"
        out.append(f"{name:<28} {r['mfma'] // per_stage:>6} {r['mfma']:>5} {r['vmcnt0']:>8} {r['vmcnt_n']:>8} {r['branch']:>6} {r['barrier']:>7} {r['salu']:>5} "
                   f"{r['valu']:>5} {r['vgpr']:>5} {r['agpr']:>5} {r['scratch']:>7}")
    return "\n".join(out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--source", default=None, help="another conv.hip (its headers are taken from this tree)")
    ap.add_argument("--flags", default="", help="extra compiler flags, e.g. -DSDE_HALO3_WG_PER_CU=3")
    a = ap.parse_args()
    rows = analyse(a.source, tuple(a.flags.split()))
    print(table(rows))
    bad = [r for r in rows if r["vmcnt0"] or not r["has_loop"]]
    print(f"{len(rows)} instantiations, {len(bad)} with a vmcnt(0) between the first and the last MFMA of the loop")
    sys.exit(1 if bad or len(rows) != 18 else 0)

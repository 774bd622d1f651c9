"""What hipcc made of the fused BatchNorm finalize + apply kernels (csrc/nn.hip), one block per instantiation: registers, scratch, waves per SIMD, and the
order of the vector-memory instructions, waits and barriers from the kernel's entry to its second barrier -- the slab loads must come first, the payload
(global_load_dwordx4 of the 16-bit rows) directly behind them, every wait on the way to the fp64 adds a counted one (vmcnt(N), N >= the payload loads
outstanding), and no payload load below a barrier before the row loop.  Also counts the fp32 arithmetic of the kernel (v_fma / v_mul / v_sub / v_add / v_max),
to compare contraction between two sources.  Only load, store, waitcnt, barrier, branch and ALU mnemonics are read.

Usage (CPU):  python scripts/bn_stream_isa.py [--source path/to/nn.hip] [--flags "-DSDE_BNFA_U=2"]      profiles/bn_stream_isa.txt keeps the output."""
import argparse
import collections
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simpledepthestimation_amd", "csrc")


def assembly(source, flags):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "nn.s")
        subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{ROOT}/include", f"-I{CSRC}", *flags, "-S", "--cuda-device-only", "-o", out, source],
                       check=True)
        with open(out) as f:
            return f.read()


def mnemonic(line):
    op = line.split(";")[0].split("//")[0].strip()
    return (op.split()[0], op) if op and not op.endswith(":") and not op.startswith(".") else (None, None)


def prologue(lines):
    """Run-length summary of loads / waits / barriers / branches up to the second s_barrier."""
    seq, barriers = [], 0
    for l in lines:
        mn, op = mnemonic(l)
        if mn is None:
            continue
        if mn.startswith(("global_load", "global_store", "buffer_load")):
            item = mn
        elif mn == "s_waitcnt" and "vmcnt" in op:
            item = re.search(r"vmcnt\(\d+\)", op).group(0)
        elif mn == "s_barrier":
            item = "s_barrier"
            barriers += 1
        elif mn.startswith("s_cbranch") or mn == "s_branch":
            item = "branch"
        elif mn == "v_add_f64":
            item = "v_add_f64"
        else:
            continue
        if seq and seq[-1][0] == item:
            seq[-1][1] += 1
        else:
            seq.append([item, 1])
        if barriers == 2:
            break
    return " | ".join(f"{n}x {i}" if n > 1 else i for i, n in seq)


def analyse(source, flags):
    out = []
    for f in re.split(r"\n(?=_Z\w+:)", assembly(source, flags)):
        m = re.match(r"(_Z\w*?\d\d(bn_(?:bwd_)?finalize_apply_kernel)I(DF16[b_])(Lb[01]E)?E\w*):", f)
        if not m:
            continue
        lines = f.split("\n")
        end = next((i for i, l in enumerate(lines) if l.lstrip().startswith("s_endpgm")), len(lines))
        get = lambda k: int(re.search(rf";\s*{k}:\s*(\d+)", f).group(1))
        alu = collections.Counter(mn for mn, _ in map(mnemonic, lines[:end]) if mn and re.match(r"v_(fma|fmac|mul|sub|add|max|mad)\w*_f32", mn))
        out.append(dict(kernel=m.group(2), dtype=("bf16" if m.group(3) == "DF16b" else "fp16") + {None: "", "Lb1E": ", residual", "Lb0E": ", no residual"}[m.group(4)], vgpr=get("NumVgprs"), scratch=get("ScratchSize"),
                        waves=get("Occupancy"), lds=get("LDSByteSize"), alu=dict(sorted(alu.items())), prologue=prologue(lines[:end])))
    return sorted(out, key=lambda r: (r["kernel"], r["dtype"]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--source", default=os.path.join(CSRC, "nn.hip"), help="another nn.hip (its headers are taken from this tree)")
    ap.add_argument("--flags", default="", help="extra compiler flags")
    a = ap.parse_args()
    for r in analyse(a.source, tuple(a.flags.split())):
        print(f"{r['kernel']}<{r['dtype']}>: {r['vgpr']} VGPRs, scratch {r['scratch']} B, LDS {r['lds']} B, {r['waves']} waves per SIMD")
        print(f"  fp32 arithmetic in the kernel: {r['alu']}")
        print(f"  entry .. second barrier: {r['prologue']}")

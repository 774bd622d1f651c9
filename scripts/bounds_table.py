"""Turn an SDE_BOUNDS_LOG file (tests/conv_bounds.py: one "<dtype> <assertion> <error / limit>" line per assertion) into the table kept under profiles/:
the worst ratio and the number of assertions per name and storage type.

    SDE_BOUNDS_LOG=run.log python -m pytest -m gpu tests/test_gpu_norm_bounds.py
    python scripts/bounds_table.py run.log header.txt > profiles/norm_bounds.txt

header.txt (optional) is copied in front of the table."""
import sys
from collections import OrderedDict

TYPES = ["f32", "bf16", "fp16"]


def main(argv):
    rows = OrderedDict()
    with open(argv[1]) as f:
        for line in f:
            parts = line.split()
            if len(parts) < 3:
                continue
            dt, name, ratio = parts[0], " ".join(parts[1:-1]), float(parts[-1])
            worst, n = rows.setdefault(name, {}).get(dt, (0.0, 0))
            rows[name][dt] = (max(worst, ratio), n + 1)
    if len(argv) > 2:
        sys.stdout.write(open(argv[2]).read().rstrip("\n") + "\n\n")
    width = max(len(n) for n in rows) + 2
    print("assertion".ljust(width) + "".join(f"{t + ' worst':>12}  {'(n)':>5}" for t in TYPES))
    over = 0
    for name in sorted(rows):
        cells = ""
        for t in TYPES:
            if t in rows[name]:
                worst, n = rows[name][t]
                over += worst > 1.0
                cells += f"{worst:12.4f}  {n:5d}"
            else:
                cells += f"{'-':>12}  {'':>5}"
        print(name.ljust(width) + cells)
    print(f"\n{sum(n for r in rows.values() for _, n in r.values())} assertions, {len(rows)} names, {over} ratios above 1")


if __name__ == "__main__":
    main(sys.argv)

"""Writes simpledepthestimation_amd/utils/magma_u8.txt: matplotlib's `magma` colour map as 256 lines of RRGGBB hex digits (768 bytes of table, kept
as text), which utils/colormap.py:magma_u8() loads.  Run once; matplotlib is not needed at run time.

    python scripts/gen_magma_lut.py
"""
import os

import matplotlib
import numpy as np

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "simpledepthestimation_amd", "utils", "magma_u8.txt")

if __name__ == "__main__":
    lut = np.ascontiguousarray(matplotlib.colormaps["magma"](np.arange(256), bytes=True)[:, :3], dtype=np.uint8)
    assert lut.shape == (256, 3)
    with open(OUT, "w") as f:
        f.write("".join(bytes(row).hex() + "\n" for row in lut))
    print(f"{OUT}: {lut.shape[0]} entries, matplotlib {matplotlib.__version__}")

"""Colour tables for presenting depth maps.  `magma_u8()` is matplotlib's `magma` map sampled at its 256 entries (what plt.imshow(..., cmap='magma')
of the reference's tools/demo.py:L77 looks up), stored beside this file as 256 lines of RRGGBB hex digits by scripts/gen_magma_lut.py so that
matplotlib is not needed at run time."""
import os

import numpy as np

_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "magma_u8.txt")
_magma = None


def magma_u8():
    """[256, 3] uint8, RGB.  A fresh copy per call."""
    global _magma
    if _magma is None:
        with open(_PATH) as f:
            raw = np.frombuffer(bytes.fromhex("".join(f.read().split())), dtype=np.uint8)
        if raw.size != 768:
            raise RuntimeError(f"{_PATH}: expected 256 RRGGBB entries, found {raw.size} bytes (regenerate with scripts/gen_magma_lut.py)")
        _magma = raw.reshape(256, 3)
    return _magma.copy()

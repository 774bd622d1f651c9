"""CPU: hip.nn.twin_eligible, the one rule that decides whether a convolution's forward operand may be a view of the Adam kernel's 16-bit twin
of the flat parameter buffer (exact cast of the master slot, 16-byte aligned for the GEMM loaders) or stays on the per-step pack."""
import pytest

from simpledepthestimation_amd.hip.nn import TWIN_ALIGN, twin_eligible

# (Cout, Cin, cin_pad, ldy, ohwi, slot offset in elements, expected, why)
CASES = [
    (64, 64, 64, 64, True, 0, True, "1x1 / 3x3 64->64 at the start of the buffer"),
    (128, 64, 64, 128, True, 9408 + 64 + 64, True, "offset a multiple of 8 elements = 16 bytes"),
    (64, 192, 192, 64, True, 8, True, "192 input channels: a multiple of 8, no padding"),
    (64, 64, 64, 64, True, 4, False, "slot behind a one-element bias: offset = 4 mod 8 elements is 8 bytes mod 16"),
    (64, 64, 64, 64, True, 8 * 1000 + 4, False, "offset = 4 mod 8 further up"),
    (1, 64, 64, 8, True, 0, False, "Cout = 1: the operand is padded to ldy = 8 rows"),
    (64, 3, 8, 64, True, 0, False, "Cin = 3: the stem's operand is padded to 8 input channels"),
    (64, 64, 64, 64, False, 0, False, "OIHW master: the slot is not in operand order"),
    (64, 64, 72, 64, True, 0, False, "wider virtual input than the weight (cin_pad != Cin)"),
    (60, 64, 64, 64, True, 0, False, "ldy != Cout"),
    (60, 64, 64, 60, True, 0, False, "Cout no multiple of 8: the transposing pack moves 8 output channels at a time"),
]


@pytest.mark.parametrize("Cout,Cin,cin_pad,ldy,ohwi,off,want,why", CASES, ids=[c[-1] for c in CASES])
def test_twin_eligible(Cout, Cin, cin_pad, ldy, ohwi, off, want, why):
    assert twin_eligible(Cout, Cin, cin_pad, ldy, ohwi, off) is want, why


def test_alignment_is_of_the_address_not_of_the_offset():
    """A twin whose base is itself 8 bytes off the boundary flips which offsets qualify; fp32 operands have no twin."""
    assert TWIN_ALIGN == 16
    assert not twin_eligible(64, 64, 64, 64, True, 0, base_align=8)
    assert twin_eligible(64, 64, 64, 64, True, 4, base_align=8)
    assert not twin_eligible(64, 64, 64, 64, True, 0, esize=4)

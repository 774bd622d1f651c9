"""CPU: the ISA of halo3_kernel's steady-state loop (csrc/conv.hip), read by scripts/halo3_loop_isa.py from a device-only compile for gfx950.

A `s_waitcnt vmcnt(0)` between the first and the last MFMA of the loop drains the weight prefetch that was issued three stages ahead (the state the
kernel was in while the stage number was decoded at run time: 6-16 such waits per three stages); a spill or a 169th VGPR in the plain-source
64-wide kernel costs the third wave per SIMD.  One compile (about a minute) serves every test here; skipped where hipcc is absent."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rows():
    spec = importlib.util.spec_from_file_location("halo3_loop_isa", os.path.join(ROOT, "scripts", "halo3_loop_isa.py"))
    isa = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(isa)
    if isa.hipcc() is None:
        pytest.skip("hipcc not found")
    return isa.analyse()


def test_all_eighteen_instantiations_have_a_loop(rows):
    assert sorted((r["dtype"], r["bn"], r["src"]) for r in rows) == sorted((d, bn, s) for d in ("bf16", "fp16") for bn in (64, 32, 16)
                                                                           for s in ("plain_zero", "plain_reflect", "upcat_reflect"))
    assert all(r["has_loop"] for r in rows)


def test_no_drained_wait_between_the_first_and_the_last_mfma_of_the_loop(rows):
    bad = [(r["dtype"], r["bn"], r["src"], r["vmcnt0"]) for r in rows if r["vmcnt0"]]
    assert not bad, f"s_waitcnt vmcnt(0) inside the loop: {bad}"


def test_one_trip_is_a_whole_channel_block_with_the_taps_unrolled(rows):
    """Nine stages of FM x FN x 2 MFMAs per trip, and no scalar branch in the 64- and 32-wide kernels (the 16-wide one keeps the EXEC-mask skips
    around its half-empty weight store passes: one per stage at the most)."""
    for r in rows:
        assert r["mfma"] == 9 * r["bn"] // 4, (r["dtype"], r["bn"], r["src"], r["mfma"])
        assert r["branch"] <= (9 if r["bn"] == 16 else 0), (r["dtype"], r["bn"], r["src"], r["branch"])


def test_register_budget(rows):
    """No spills anywhere; the plain-source kernels fit three waves per SIMD (512 / 3 -> 168 VGPRs).  (The up-sample + concat loader at BN 64 does
    not: it holds two sets of halo loads and runs two waves per SIMD.)"""
    for r in rows:
        assert r["scratch"] == 0 and r["agpr"] == 0, (r["dtype"], r["bn"], r["src"], r["scratch"], r["agpr"])
        if r["src"] != "upcat_reflect" or r["bn"] < 64:
            assert 0 < r["vgpr"] <= 168, (r["dtype"], r["bn"], r["src"], r["vgpr"])

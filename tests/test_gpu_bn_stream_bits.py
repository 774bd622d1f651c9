"""Bit-for-bit record of the fused BatchNorm finalize + apply launches (csrc/nn.hip: bn_finalize_apply_kernel, bn_bwd_finalize_apply_kernel), hashed,
against tests/golden/bn_stream_bits.json.

The JSON is written by scripts/record_bn_bits.py from this module's case table with a library of the same ABI (SDE_HIP_LIB): the commit before the
kernels began to keep slab and row loads in flight.  A change to how these kernels schedule their loads must reproduce it unchanged: no sum may change
its order and no element its expression.  One SHA-256 per tensor over its bytes as stored (a -0.0 in an output would be a finding, none is canonicalised).
The kernels are called through the C ABI (sde_bn_finalize_apply, sde_bn_bwd, sde_bn_bwd_from_part) on slabs the case builds from seeded CPU generators.

Cases, the smallest that reach every branch of the kernels:
  slab rows 1, 8, 9, 57, 64, 65, 255, 256: a thread owns rows rl, rl + 8, ...; groups of eight of them (64 slab rows) alternate between two accumulators, the
      rest goes to the first one; the loads are issued eight per thread at a time (64 slab rows);
  M 1, 31, 32, 33: fewer rows than one 32-row pass, one pass exactly, one more; at C = 64 the grid helper gives 32 rows per workgroup (rpw) up to M = 32 768,
      so 31 / 32 / 33 are also rpw - 1 / rpw / rpw + 1 and every M > 32 has two or more row ranges per strip;
  C = 192, M = 54 719 / 54 720 / 54 721: 342 row ranges of rpw = 160 (five passes: one unrolled block of four and one pass of the next) minus one row, exactly,
      and -- rpw 192, 286 ranges -- one row into the last range;
  C = 192, M = 10 945: rpw = 64, two passes, 172 ranges, the last with one row;
  with and without residual, with and without ReLU, running statistics null and not, accumulate_params 0 and 1, bf16 and fp16.
Forward self-consistency: `out` of the fused launch equals, bit for bit, sde_bn_apply fed the bnp that launch wrote.
"""
import functools
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bn_stream_bits.json")
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
EPS, MOM = 1e-5, 0.1
REDUCE_ROWS = 64                     # spare slab rows the reduce helpers may use (sde_hip.h: SDE_REDUCE_ROWS)
TARGET_WGS, PASS_ROWS = 1024, 32     # the grid helper's rule, restated to place M against rows-per-workgroup


def rows_per_wg(M, C):
    strips = C // 64
    chunks = -(-TARGET_WGS // strips)
    rpw = -(-M // chunks)
    return max(PASS_ROWS, -(-rpw // PASS_ROWS) * PASS_ROWS)


# (C, slab rows, M)
SMALL = [(64, 1, 1), (64, 8, 31), (64, 9, 32), (64, 57, 33), (64, 64, 1), (64, 65, 33), (64, 255, 31), (64, 256, 32), (192, 129, 33), (192, 256, 10945)]
BIG = [(192, 200, 54719), (192, 16, 54720), (192, 128, 54721)]
assert rows_per_wg(32, 64) == 32 and rows_per_wg(33, 64) == 32 and rows_per_wg(10945, 192) == 64
assert rows_per_wg(54719, 192) == 160 and rows_per_wg(54720, 192) == 160 and rows_per_wg(54721, 192) == 192


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def _gen(*key):
    return torch.Generator().manual_seed(int(hashlib.sha256(repr(key).encode()).hexdigest()[:8], 16))


@functools.lru_cache(maxsize=4)
def _maps(M, C):
    """Three fp32 maps [M, C] on the CPU (y, residual / dz, a second gradient), shared by the storage types and left unchanged."""
    g = _gen("maps", M, C)
    return tuple(torch.randn(M, C, generator=g) for _ in range(3))


def _slab(rows, C, M, key):
    """[rows + REDUCE_ROWS][C][2]: per-row (sum, sum of squares) of about M / rows values of variance near 1.5, so that no variance is clamped."""
    g = _gen("slab", rows, C, M, key)
    per = M / rows
    s = torch.zeros(rows + REDUCE_ROWS, C, 2)
    s[:rows, :, 0] = torch.randn(rows, C, generator=g) * 0.3 * per
    s[:rows, :, 1] = (torch.rand(rows, C, generator=g) + 1.0) * per
    return s


def _api():
    from simpledepthestimation_amd.hip import lib as L, nn as HN      # (hip.nn registers the BatchNorm prototypes)
    return L, HN


def _call(L, name, *args):
    L.check(getattr(L.lib(), name)(*args, L.stream()), name)


def run_forward(C, rows, M, kind, variants):
    """sde_bn_finalize_apply for each (residual, relu, running statistics) variant -> ({name: sha256}, self-consistency failures)."""
    L, HN = _api()
    dtype, code = DTYPES[kind], HN.dtype_code(DTYPES[kind])
    assert L.lib().sde_bn_finalize_apply_ok(rows, C, code)
    y32, r32, _ = _maps(M, C)
    g = _gen("fwd", C, rows, M)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(DEV), torch.randn(C, generator=g).to(DEV)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    slab = _slab(rows, C, M, "fwd").to(DEV)
    y, res = y32.to(dtype).to(DEV), r32.to(dtype).to(DEV)
    rec, bad = {}, []
    for with_res, relu, running in variants:
        tag = f"{'res' if with_res else 'nores'}_{'relu' if relu else 'lin'}_{'run' if running else 'norun'}"
        bnp, out, again = torch.empty(4, C, device=DEV), torch.empty(M, C, dtype=dtype, device=DEV), torch.empty(M, C, dtype=dtype, device=DEV)
        rm, rv = (rm0.to(DEV), rv0.to(DEV)) if running else (None, None)
        rd = res if with_res else None
        _call(L, "sde_bn_finalize_apply", L.ptr(slab), rows, C, M, L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), MOM, EPS, L.ptr(bnp), L.ptr(y), L.ptr(rd),
              int(relu), code, L.ptr(out))
        _call(L, "sde_bn_apply", L.ptr(y), L.ptr(bnp), L.ptr(rd), int(relu), M, C, code, L.ptr(again))
        torch.cuda.synchronize()
        rec[f"{tag}.out"], rec[f"{tag}.bnp"] = sha(out), sha(bnp)
        if running:
            rec[f"{tag}.rmean"], rec[f"{tag}.rvar"] = sha(rm), sha(rv)
        if not torch.equal(out.view(torch.int16), again.view(torch.int16)):
            bad.append(tag)
    return rec, bad


def _bnp(C, key):
    """[4][C] mean, rstd, scale, shift from a seeded generator (the backward kernels only read them)."""
    g = _gen("bnp", C, key)
    return torch.stack([torch.randn(C, generator=g) * 0.2, torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2])


def run_from_part(C, rows, M, kind):
    """sde_bn_bwd_from_part on a host-built (sum gm, sum gm * xhat) slab, accumulate_params 0 and 1."""
    L, HN = _api()
    dtype, code = DTYPES[kind], HN.dtype_code(DTYPES[kind])
    y32, d32, _ = _maps(M, C)
    bnp = _bnp(C, "part").to(DEV)
    slab = _slab(rows, C, M, "bwd")
    slab[:rows, :, 1] -= 1.5 * M / rows          # (sum gm * xhat has no sign)
    slab = slab.to(DEV)
    y, gm = y32.to(dtype).to(DEV), d32.to(dtype).to(DEV)
    g = _gen("prior", C)
    prior = torch.randn(2, C, generator=g)
    rec = {}
    for acc in (0, 1):
        dy, coef = torch.empty(M, C, dtype=dtype, device=DEV), torch.zeros(2, C, device=DEV)
        dgamma, dbeta = prior[0].to(DEV), prior[1].to(DEV)
        _call(L, "sde_bn_bwd_from_part", L.ptr(slab), rows, L.ptr(gm), L.ptr(y), L.ptr(bnp), M, C, code, L.ptr(coef), L.ptr(dgamma), L.ptr(dbeta), acc, L.ptr(dy))
        torch.cuda.synchronize()
        rec.update({f"acc{acc}.dy": sha(dy), f"acc{acc}.dgamma": sha(dgamma), f"acc{acc}.dbeta": sha(dbeta)})
    return rec


def run_bwd(C, M, kind):
    """sde_bn_bwd: its own reduce pass in front of the fused launch; a plain gradient, and two summed gradients under the re-derived ReLU mask."""
    L, HN = _api()
    dtype, code = DTYPES[kind], HN.dtype_code(DTYPES[kind])
    y32, d32, e32 = _maps(M, C)
    bnp = _bnp(C, "bwd").to(DEV)
    gamma = torch.ones(C, device=DEV)
    y, d0, d1 = y32.to(dtype).to(DEV), d32.to(dtype).to(DEV), e32.to(dtype).to(DEV)
    nblk = L.lib().sde_reduce_num_blocks(M, C)
    g = _gen("prior", C)
    prior = torch.randn(2, C, generator=g)
    rec = {}
    for masked, acc in ((0, 0), (1, 1)):
        part, coef = torch.zeros(nblk + REDUCE_ROWS, C, 2, device=DEV), torch.zeros(2, C, device=DEV)
        dy, gm = torch.empty(M, C, dtype=dtype, device=DEV), torch.empty(M, C, dtype=dtype, device=DEV)
        dgamma, dbeta = prior[0].to(DEV), prior[1].to(DEV)
        _call(L, "sde_bn_bwd", L.ptr(d0), L.ptr(d1 if masked else None), L.ptr(None), L.ptr(None), L.ptr(y), L.ptr(bnp), L.ptr(gamma), masked, M, C, code,
              L.ptr(part), L.ptr(coef), L.ptr(dgamma), L.ptr(dbeta), acc, L.ptr(gm if masked else None), L.ptr(dy))
        torch.cuda.synchronize()
        tag = "masked_acc1" if masked else "plain_acc0"
        rec.update({f"{tag}.dy": sha(dy), f"{tag}.dgamma": sha(dgamma), f"{tag}.dbeta": sha(dbeta)})
    return rec


ALL_VARIANTS = [(0, 1, 1), (1, 1, 1), (1, 0, 0), (0, 0, 0)]      # (residual, relu, running statistics)
BIG_VARIANTS = [(1, 1, 1), (0, 0, 0)]


def _cases():
    c = {}
    for kind in DTYPES:
        for C, rows, M in SMALL + BIG:
            v = BIG_VARIANTS if (C, rows, M) in BIG else ALL_VARIANTS
            c[f"fwd_{kind}_C{C}_R{rows}_M{M}"] = functools.partial(run_forward, C, rows, M, kind, v)
            c[f"from_part_{kind}_C{C}_R{rows}_M{M}"] = functools.partial(run_from_part, C, rows, M, kind)
        # slab rows from sde_bn_bwd's own reduce pass: 1, 1, 235, and 79 behind the 1024-thread reduce workgroups (313 of the narrow ones would be too many).
        # C = 64 only: at C = 192 (24 channel groups, no divisor of 256) that pass adds with LDS float atomics and two runs of one library differ.
        for C, M in [(64, 1), (64, 33), (64, 30000), (64, 40000)]:
            c[f"bwd_{kind}_C{C}_M{M}"] = functools.partial(run_bwd, C, M, kind)
    return c


CASES = _cases()


def run_case(name):
    """({output name: sha256}, forward variants whose output differs from sde_bn_apply's)."""
    r = CASES[name]()
    return r if isinstance(r, tuple) else (r, [])


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_table_and_record_agree(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_bn_stream_bits(golden, name):
    got, inconsistent = run_case(name)
    assert not inconsistent, f"the fused launch and sde_bn_apply on its bnp differ: {inconsistent}"
    assert got == golden[name], sorted(k for k in got if got[k] != golden[name].get(k))

"""GPU: BatchNorm and GroupNorm (csrc/nn.hip) and the random layer norm (csrc/google.hip), element by element against the fp64 references and limits of
tests/norm_bounds.py, in fp32, bf16 and fp16 (the random layer norm: fp32 and bf16, the types it is built for).

The kernels are called through the C ABI on partial-sum slabs the test builds -- no GEMM stands in front of them -- with every result carved out of a
sentinel-filled buffer (stream_bounds.guarded): afterwards no element may still be the sentinel and the 256 bytes before and after are untouched.  Every
case computes the route it is meant to hit from the exported predicates (sde_bn_finalize_apply_ok, sde_reduce_num_blocks, the sde_bn_set_fuse state) and
the rule in the source (norm_bounds.bn_reduce_route, bn_finalize_fused, gn_path, rln_layout) and asserts it BEFORE it runs: a case that lands on another
route fails.  Where an autograd wrapper exists (hip/nn.py batch_norm_act, group_norm_relu; hip/google.py rand_layer_norm) it must agree with the direct
call bit for bit.  tests/test_norm_bounds.py shows on the CPU that these same assertions reject single planted faults.

Backward operands are what the forward kernels left (bnp, gnp, rlnp, the stored output), each checked against its own limit first; the reduced
gradients are built from the masked gradient the kernel stored (norm_bounds' docstring says why)."""
import types

import pytest
import torch

import norm_bounds as NB

pytestmark = pytest.mark.gpu
dev = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
NAME = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "fp16"}
INF = float("inf")
EPS, MOM = 1e-5, 0.1
f32 = torch.float32


@pytest.fixture(scope="module")
def K():
    from simpledepthestimation_amd.hip import google, lib, nn
    return types.SimpleNamespace(L=lib, HN=nn, HG=google)


def up(t, dtype=f32):
    return None if t is None else t.to(dtype).to(dev).contiguous()


def call(K, name, *args):
    K.L.check(getattr(K.L.lib(), name)(*args, K.L.stream()), name)


def result(guard, name, written=True):
    """The guarded result on the CPU (fp32), after the guard-band check.  written=False: a scratch slab the kernel fills only in part -- bands only."""
    buf, out = guard
    torch.cuda.synchronize()
    if written:
        NB.assert_guards(buf, out, name)
    else:
        n = out.numel() * out.element_size()
        b = buf.cpu()
        assert bool((b[:NB.GUARD] == NB.SENTINEL).all()) and bool((b[NB.GUARD + n:] == NB.SENTINEL).all()), f"{name}: written outside the buffer"
    return out.float().cpu()


def untouched(guard, name):
    torch.cuda.synchronize()
    assert bool((guard[0].cpu() == NB.SENTINEL).all()), f"{name}: written although this route does not produce it"


def filled(shape, dtype, value):
    """A guarded buffer that holds `value` (a slot the kernel accumulates into)."""
    g = NB.guarded(shape, dtype, dev)
    g[1].copy_(value.to(dev))
    return g


def same_bits(a, b, name):
    a, b = a.detach().contiguous().reshape(-1), b.detach().contiguous().reshape(-1)
    assert a.dtype == b.dtype and a.numel() == b.numel() and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"{name}: the wrapper and the C ABI call differ"


def agree(a, b, bound, dtype, name, exact=True):
    """The wrapper against the direct call: the same bits, or -- where the kernel adds with LDS float atomics, whose order changes from launch to
    launch -- both inside the limit, so no further apart than twice it (conv_bounds.assert_two_kernels)."""
    if exact:
        return same_bits(a, b, name)
    NB.CB.assert_two_kernels(a.detach().float().cpu().reshape(bound.ref.shape), b.detach().float().cpu().reshape(bound.ref.shape), bound, dtype, name + ": wrapper | C ABI")


def within(got, bound, dtype, name):
    NB.assert_within(got, bound, dtype, name, l2_tol=INF)


class fuse_state:
    """sde_bn_set_fuse(state) and hip.nn.FUSE_BN_FINALIZE for the block, restored on exit."""

    def __init__(self, K, state):
        self.K, self.state = K, state

    def __enter__(self):
        self.old = self.K.L.lib().sde_bn_set_fuse(self.state)
        self.old_py, self.K.HN.FUSE_BN_FINALIZE = self.K.HN.FUSE_BN_FINALIZE, bool(self.state)

    def __exit__(self, *exc):
        self.K.L.lib().sde_bn_set_fuse(self.old)
        self.K.HN.FUSE_BN_FINALIZE = self.old_py


# ---------------------------------------------------------------------------------------------------------------------------------------
# BatchNorm forward
# ---------------------------------------------------------------------------------------------------------------------------------------
def ragged(rows):
    return 37 * rows + 11


# route, C, slab rows, M, storage types, fuse state
BN_FWD_CASES = [("fused", 64, r, m, "16", 1) for r, m in ((1, 1), (8, 31), (9, 33), (57, ragged(57)), (64, 31), (65, ragged(65)), (256, ragged(256)))] + [
    ("separate", 64, 9, ragged(9), "f32", 1),                # fp32 has no fused launch
    ("separate", 40, 9, ragged(9), "16", 1),                 # C % 64 != 0
    ("separate", 64, 257, ragged(257), "16", 1),             # one slab row too many
    ("separate", 64, 9, ragged(9), "16", 0),                 # fused launches switched off
    ("pre_reduce", 8, 4097, 4500, "all", 1),                 # rows_reduce_kernel in front of the finalize
]


@pytest.mark.parametrize("case", BN_FWD_CASES, ids=lambda c: f"{c[0]}-C{c[1]}-R{c[2]}-M{c[3]}-{c[4]}-fuse{c[5]}")
def test_batchnorm_forward(K, case):
    route, C, rows, M, kinds, fuse = case
    for dtype in NB.dtypes_of(kinds):
        code = K.HN.dtype_code(dtype)
        with fuse_state(K, fuse):
            fused = bool(K.HN.FUSE_BN_FINALIZE) and bool(K.L.lib().sde_bn_finalize_apply_ok(rows, C, code))
            assert fused == NB.bn_finalize_fused(rows, C, dtype, fuse) == (route == "fused"), f"{case}: not on the {route} route"
            assert (NB.pre_reduce_chunk(rows) > 0) == (route == "pre_reduce")
            y, gamma, beta = NB.bn_input(M, C, dtype, 3 + rows)
            res = NB.draw((M, C), dtype, 4)
            part = NB.host_slab(y, rows)
            g = torch.Generator().manual_seed(5)
            rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
            ref = NB.BNForward(part, M, gamma, beta, EPS, MOM)
            brm, brv = ref.running(rm0, rv0)
            slab = torch.zeros(rows + NB.REDUCE_ROWS, C, 2)
            slab[:rows] = part
            yd, gd, bd = up(y, dtype), up(gamma), up(beta)
            for r, relu in ((None, True), (res, True), (res, False)):
                tag = f"bn {route}{' +res' if r is not None else ''}{' relu' if relu else ''}"
                rd, sd = up(r, dtype), slab.to(dev)
                bnp, out = NB.guarded((4, C), f32, dev), NB.guarded((M, C), dtype, dev)
                rm, rv = filled((C,), f32, rm0), filled((C,), f32, rv0)
                if fused:
                    call(K, "sde_bn_finalize_apply", K.L.ptr(sd), rows, C, M, K.L.ptr(gd), K.L.ptr(bd), K.L.ptr(rm[1]), K.L.ptr(rv[1]), MOM, EPS, K.L.ptr(bnp[1]),
                         K.L.ptr(yd), K.L.ptr(rd), int(relu), code, K.L.ptr(out[1]))
                else:
                    call(K, "sde_bn_finalize", K.L.ptr(sd), rows, C, M, K.L.ptr(gd), K.L.ptr(bd), K.L.ptr(rm[1]), K.L.ptr(rv[1]), MOM, EPS, K.L.ptr(bnp[1]))
                    call(K, "sde_bn_apply", K.L.ptr(yd), K.L.ptr(bnp[1]), K.L.ptr(rd), int(relu), M, C, code, K.L.ptr(out[1]))
                got_bnp = result(bnp, tag + " bnp")
                within(got_bnp, ref.bnp, dtype, f"bn {route} bnp")
                within(result(rm, tag + " running mean"), brm, dtype, f"bn {route} running mean")
                within(result(rv, tag + " running var"), brv, dtype, f"bn {route} running var")
                got = result(out, tag)
                within(got, ref.out(y, r, relu, dtype), dtype, f"bn {route} out")
                within(got, NB.bn_apply(y, got_bnp, r, relu, dtype), dtype, f"bn {route} out | its own bnp")
                # the wrapper picks the launch by the same rule and must give the same bits
                wm, wv = rm0.to(dev), rv0.to(dev)
                with torch.no_grad():
                    ow = K.HN.batch_norm_act(yd.view(1, 1, M, C), slab.to(dev), gd, bd, wm, wv, residual=None if rd is None else rd.view(1, 1, M, C), relu=relu,
                                             momentum=MOM, eps=EPS)
                same_bits(ow, out[1], tag)
                same_bits(wm, rm[1], tag + " running mean")
                same_bits(wv, rv[1], tag + " running var")


@pytest.mark.parametrize("dtype", DTYPES, ids=list(NAME.values()))
def test_batchnorm_eval_mode(K, dtype):
    M, C = 75, 40
    code = K.HN.dtype_code(dtype)
    y, gamma, beta = NB.bn_input(M, C, dtype, 9)
    g = torch.Generator().manual_seed(10)
    rm, rv = torch.randn(C, generator=g) * 3.0, torch.rand(C, generator=g) + 0.01
    res = NB.draw((M, C), dtype, 11)
    bnp, out = NB.guarded((4, C), f32, dev), NB.guarded((M, C), dtype, dev)
    yd, rd, gd, bd, rmd, rvd = up(y, dtype), up(res, dtype), up(gamma), up(beta), up(rm), up(rv)
    call(K, "sde_bn_eval_params", K.L.ptr(gd), K.L.ptr(bd), K.L.ptr(rmd), K.L.ptr(rvd), EPS, C, K.L.ptr(bnp[1]))
    call(K, "sde_bn_apply", K.L.ptr(yd), K.L.ptr(bnp[1]), K.L.ptr(rd), 1, M, C, code, K.L.ptr(out[1]))
    got_bnp = result(bnp, "eval bnp")
    within(got_bnp, NB.bn_eval_params(gamma, beta, rm, rv, EPS), dtype, "bn eval bnp")
    within(result(out, "eval out"), NB.bn_apply(y, got_bnp, res, True, dtype), dtype, "bn eval out | its own bnp")
    with torch.no_grad():
        ow = K.HN.batch_norm_act(yd.view(1, 1, M, C), None, gd, bd, rmd, rvd, residual=rd.view(1, 1, M, C), relu=True, eps=EPS, training=False)
    same_bits(ow, out[1], "eval out")
    assert torch.equal(rmd.cpu(), rm) and torch.equal(rvd.cpu(), rv), "eval mode touched the running statistics"


# ---------------------------------------------------------------------------------------------------------------------------------------
# BatchNorm backward
# ---------------------------------------------------------------------------------------------------------------------------------------
def gpu_bnp(K, y, gamma, beta, M, C):
    """bnp of a one-row slab from sde_bn_finalize (checked in test_batchnorm_forward): the operand of the backward kernels, and what the wrapper's
    forward leaves (one slab row: one order of summation, the fused and the separate finalize agree to the bit)."""
    slab = torch.zeros(1 + NB.REDUCE_ROWS, C, 2)
    slab[:1] = NB.host_slab(y, 1)
    bnp = torch.empty(4, C, device=dev)
    sd, gd, bd = slab.to(dev), up(gamma), up(beta)            # (named: a temporary would be freed, and its memory reused, before the launch)
    call(K, "sde_bn_finalize", K.L.ptr(sd), 1, C, M, K.L.ptr(gd), K.L.ptr(bd), K.L.ptr(None), K.L.ptr(None), MOM, EPS, K.L.ptr(bnp))
    torch.cuda.synchronize()
    return bnp, slab


def bn_bwd_ids(c):
    return f"C{c[0]}-M{c[1]}-{c[2]}-g{c[3]}-mode{c[4]}-acc{c[5]}-{c[6]}"


@pytest.mark.parametrize("fuse", [1, 0], ids=["fused", "separate"])
@pytest.mark.parametrize("case", NB.BN_BWD_CASES, ids=bn_bwd_ids)
def test_batchnorm_backward(K, case, fuse):
    C, M, kinds, n_grads, relu_mode, acc, want = case
    for dtype in NB.dtypes_of(kinds):
        code = K.HN.dtype_code(dtype)
        with fuse_state(K, fuse):
            nblk0 = K.L.lib().sde_reduce_num_blocks(M, C)
            route, nblk, n_part = NB.bn_reduce_route(M, C, dtype, nblk0, fuse)
            expect = "fast256" if (want == "wide1024" and not fuse) else want
            assert route == expect, f"{case} {NAME[dtype]} fuse={fuse}: the reduce pass takes {route}, not {expect}"
            if want == "wide1024":
                # (more than 256 reduce workgroups start at M = 32 769 for C = 64: one workgroup per 128 rows)
                assert nblk0 > NB.BNFA_MAX_ROWS and K.L.lib().sde_reduce_num_blocks(32768, C) == NB.BNFA_MAX_ROWS
            fused = NB.bn_finalize_fused(nblk, C, dtype, fuse)
            assert fused == (bool(fuse) and dtype != f32 and C % 64 == 0 and nblk <= 256)
            y, _, res, grads, gamma, beta = NB.bn_bwd_operands(C, M, dtype, n_grads, relu_mode, 100 + C + M)
            bnp_d, slab = gpu_bnp(K, y, gamma, beta, M, C)
            bnp = bnp_d.cpu()
            yd, rd = up(y, dtype), up(res, dtype)
            out_d, out = None, None
            if relu_mode == 1:
                og = NB.guarded((M, C), dtype, dev)
                call(K, "sde_bn_apply", K.L.ptr(yd), K.L.ptr(bnp_d), K.L.ptr(rd), 1, M, C, code, K.L.ptr(og[1]))
                out = result(og, "bn out")
                within(out, NB.bn_apply(y, bnp, res, True, dtype), dtype, "bn bwd: the stored output")
                out_d = og[1]
            mask, und = NB.bn_mask(y, bnp, res, relu_mode, dtype)
            NB.assert_decided(und, f"{case} {NAME[dtype]}")
            if relu_mode == 1:
                assert torch.equal((out > 0)[~und], mask.bool()[~und]), "the stored output disagrees with the sign of the fp64 value on a decided element"
            gds = [up(t, dtype) for t in grads] + [None, None]
            need_gm = bool(relu_mode) or n_grads > 1
            gm = NB.guarded((M, C), dtype, dev) if need_gm else None
            dy, coef = NB.guarded((M, C), dtype, dev), NB.guarded((2, C), f32, dev)
            g = torch.Generator().manual_seed(7)
            prior = (torch.randn(C, generator=g) * 3.0, torch.randn(C, generator=g) * 3.0) if acc else None
            dgamma = filled((C,), f32, prior[0]) if acc else NB.guarded((C,), f32, dev)
            dbeta = filled((C,), f32, prior[1]) if acc else NB.guarded((C,), f32, dev)
            part = torch.empty(nblk0 + NB.REDUCE_ROWS, C, 2, device=dev)
            gmd = up(gamma)
            call(K, "sde_bn_bwd", K.L.ptr(gds[0]), K.L.ptr(gds[1]), K.L.ptr(gds[2]), K.L.ptr(out_d), K.L.ptr(yd), K.L.ptr(bnp_d), K.L.ptr(gmd), int(bool(relu_mode)),
                 M, C, code, K.L.ptr(part), K.L.ptr(coef[1]), K.L.ptr(dgamma[1]), K.L.ptr(dbeta[1]), acc, K.L.ptr(gm[1] if gm else None), K.L.ptr(dy[1]))
            tag = f"bn bwd {route}{' fused' if fused else ''}"
            if need_gm:
                got_gm = result(gm, tag + " gm")
                within(got_gm, NB.bn_gm(grads, mask, und, dtype), dtype, tag + " gm")
            else:
                got_gm = grads[0]
            s = NB.bn_sums(got_gm, y, bnp, n_part, nblk, prior=prior)
            within(result(dbeta, tag + " dbeta"), s["dbeta"], dtype, tag + " dbeta")
            within(result(dgamma, tag + " dgamma"), s["dgamma"], dtype, tag + " dgamma")
            if fused:
                untouched(coef, tag + " coef")
            else:
                within(result(coef, tag + " coef"), s["coef"], dtype, tag + " coef")
            b_dy = NB.bn_dy(got_gm, y, bnp, s["k"], s["ek"], dtype)
            within(result(dy, tag + " dy"), b_dy, dtype, tag + " dy")
            if acc:
                continue
            # the autograd wrapper: the same forward (one slab row), the same backward launch
            yw = yd.clone().view(1, 1, M, C).requires_grad_(True)
            rw = rd.clone().view(1, 1, M, C).requires_grad_(True) if relu_mode == 1 else None
            gw, bw = up(gamma).requires_grad_(True), up(beta).requires_grad_(True)
            o = K.HN.batch_norm_act(yw, slab.to(dev), gw, bw, torch.zeros(C, device=dev), torch.ones(C, device=dev), residual=rw, relu=bool(relu_mode),
                                    momentum=MOM, eps=EPS, n_out=n_grads)
            o = o if isinstance(o, tuple) else (o,)
            torch.autograd.backward(list(o), [t.view(1, 1, M, C) for t in gds[:n_grads]])
            exact = route != "atomics"
            agree(yw.grad, dy[1], b_dy, dtype, tag + " dy", exact)
            agree(gw.grad, dgamma[1], s["dgamma"], dtype, tag + " dgamma", exact)
            agree(bw.grad, dbeta[1], s["dbeta"], dtype, tag + " dbeta", exact)
            if rw is not None:
                same_bits(rw.grad, gm[1], tag + " dres")


@pytest.mark.parametrize("rows", NB.BN_FROM_PART_ROWS)
@pytest.mark.parametrize("dtype", DTYPES, ids=list(NAME.values()))
def test_batchnorm_backward_from_a_host_slab(K, dtype, rows):
    """sde_bn_bwd_from_part: 1 and 256 rows take the fused launch in the 16-bit types, 257 the separate one, 4097 go through rows_reduce_kernel first."""
    C = 64 if dtype != f32 else 8
    M = 300 if rows <= 257 else 4200
    code = K.HN.dtype_code(dtype)
    fused = NB.bn_finalize_fused(rows, C, dtype, 1)
    assert fused == (dtype != f32 and rows <= 256) and (NB.pre_reduce_chunk(rows) > 0) == (rows == 4097)
    y, _, _, grads, gamma, beta = NB.bn_bwd_operands(C, M, dtype, 1, 0, 13)
    with fuse_state(K, 1):
        bnp_d, _ = gpu_bnp(K, y, gamma, beta, M, C)
        bnp = bnp_d.cpu()
        gmv = grads[0]
        xh = (y - bnp[0]) * bnp[1]
        part = torch.stack([NB.host_slab(gmv, rows)[..., 0], NB.host_slab(gmv * xh, rows)[..., 0]], 2)
        slab = torch.zeros(rows + NB.REDUCE_ROWS, C, 2)
        slab[:rows] = part
        g = torch.Generator().manual_seed(7)
        prior = (torch.randn(C, generator=g), torch.randn(C, generator=g))
        dy, coef = NB.guarded((M, C), dtype, dev), NB.guarded((2, C), f32, dev)
        dgamma, dbeta = filled((C,), f32, prior[0]), filled((C,), f32, prior[1])
        sd = slab.to(dev)
        gmd, yd = up(gmv, dtype), up(y, dtype)
        call(K, "sde_bn_bwd_from_part", K.L.ptr(sd), rows, K.L.ptr(gmd), K.L.ptr(yd), K.L.ptr(bnp_d), M, C, code, K.L.ptr(coef[1]), K.L.ptr(dgamma[1]),
             K.L.ptr(dbeta[1]), 1, K.L.ptr(dy[1]))
    s = NB.bn_sums(None, y, bnp, 0, rows, prior=prior, part=part)
    tag = f"bn from_part{' fused' if fused else ''}{' pre_reduce' if rows > 4096 else ''}"
    within(result(dgamma, tag + " dgamma"), s["dgamma"], dtype, tag + " dgamma")
    within(result(dbeta, tag + " dbeta"), s["dbeta"], dtype, tag + " dbeta")
    if fused:
        untouched(coef, tag + " coef")
    else:
        within(result(coef, tag + " coef"), s["coef"], dtype, tag + " coef")
    within(result(dy, tag + " dy"), NB.bn_dy(gmv, y, bnp, s["k"], s["ek"], dtype), dtype, tag + " dy")


# ---------------------------------------------------------------------------------------------------------------------------------------
# GroupNorm
# ---------------------------------------------------------------------------------------------------------------------------------------
ACT_NAME = {NB.ACT_NONE: "none", NB.ACT_RELU: "relu", NB.ACT_ELU: "elu"}


@pytest.mark.parametrize("dtype", DTYPES, ids=list(NAME.values()))
@pytest.mark.parametrize("case", NB.GN_CASES, ids=lambda c: f"C{c[0]}-G{c[1]}-HW{c[2]}-{ACT_NAME[c[3]]}{'-res' if c[4] else ''}-{c[5]}")
def test_groupnorm(K, dtype, case):
    C, G, HW, act, with_res, path = case
    assert NB.gn_path(C, dtype) == path, f"C = {C} in {NAME[dtype]} takes the {NB.gn_path(C, dtype)} order, not {path}"
    B = 2
    code = K.HN.dtype_code(dtype)
    x, res, gamma, beta, dout = NB.gn_operands(B, HW, C, dtype, with_res, C + HW)
    ref = NB.GNForward(x, res, gamma, beta, G, EPS, act, dtype)
    xd, rd, gd, bd, dd = up(x, dtype), up(res, dtype), up(gamma), up(beta), up(dout, dtype)
    part, gnp, out = NB.guarded((B, NB.GN_CHUNKS, C, 2), f32, dev), NB.guarded((B, G, 2), f32, dev), NB.guarded((B, HW, C), dtype, dev)
    call(K, "sde_gn_relu_res_fwd", K.L.ptr(xd), K.L.ptr(rd), K.L.ptr(gd), K.L.ptr(bd), B, HW, C, G, EPS, act, code, K.L.ptr(part[1]), K.L.ptr(gnp[1]), K.L.ptr(out[1]))
    tag = f"gn {path} {ACT_NAME[act]}{' +res' if with_res else ''}"
    within(result(part, tag + " part"), ref.part, dtype, f"gn {path} part")
    got_gnp = result(gnp, tag + " gnp")
    within(got_gnp, ref.gnp, dtype, f"gn {path} gnp")
    got_out = result(out, tag + " out")
    within(got_out, ref.out, dtype, tag + " out")
    # backward on what forward left
    g = torch.Generator().manual_seed(7)
    prior = (torch.randn(C, generator=g), torch.randn(C, generator=g))
    for acc in (0, 1):
        coef, dx = NB.guarded((B, G, 2), f32, dev), NB.guarded((B, HW, C), dtype, dev)
        dgamma = filled((C,), f32, prior[0]) if acc else NB.guarded((C,), f32, dev)
        dbeta = filled((C,), f32, prior[1]) if acc else NB.guarded((C,), f32, dev)
        bpart = NB.guarded((B, NB.GN_CHUNKS, C, 2), f32, dev)
        call(K, "sde_gn_relu_res_bwd", K.L.ptr(dd), K.L.ptr(out[1]), K.L.ptr(xd), K.L.ptr(rd), K.L.ptr(gnp[1]), K.L.ptr(gd), B, HW, C, G, act, code, K.L.ptr(bpart[1]),
             K.L.ptr(coef[1]), K.L.ptr(dgamma[1]), K.L.ptr(dbeta[1]), acc, K.L.ptr(dx[1]))
        b = NB.gn_backward(dout, got_out, x, res, got_gnp, gamma, G, act, dtype, prior=prior if acc else None)
        result(bpart, tag + " bwd part")
        within(result(coef, tag + " coef"), b["coef"], dtype, tag + " coef")
        within(result(dgamma, tag + " dgamma"), b["dgamma"], dtype, tag + " dgamma")
        within(result(dbeta, tag + " dbeta"), b["dbeta"], dtype, tag + " dbeta")
        within(result(dx, tag + " dx"), b["dx"], dtype, tag + " dx")
    # the autograd wrapper (fresh parameter gradients: the accumulate = 0 call above)
    xw = xd.clone().view(B, 1, HW, C).requires_grad_(True)
    rw = rd.clone().view(B, 1, HW, C).requires_grad_(True) if with_res else None
    gw, bw = gd.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    ow = K.HN.group_norm_relu(xw, gw, bw, G, EPS, ACT_NAME[act], residual=rw)
    exact = path != "atomics"
    agree(ow, out[1], ref.out, dtype, tag + " out", exact)
    sv = ow.grad_fn.saved_tensors           # x, out, gnp, gamma, res as the wrapper's forward left them
    ow.backward(dd.view(B, 1, HW, C))
    coef0, dx0 = NB.guarded((B, G, 2), f32, dev), NB.guarded((B, HW, C), dtype, dev)
    dg0, db0 = NB.guarded((C,), f32, dev), NB.guarded((C,), f32, dev)
    bp0 = torch.empty(B, NB.GN_CHUNKS, C, 2, device=dev)
    call(K, "sde_gn_relu_res_bwd", K.L.ptr(dd), K.L.ptr(out[1]), K.L.ptr(xd), K.L.ptr(rd), K.L.ptr(gnp[1]), K.L.ptr(gd), B, HW, C, G, act, code, K.L.ptr(bp0),
         K.L.ptr(coef0[1]), K.L.ptr(dg0[1]), K.L.ptr(db0[1]), 0, K.L.ptr(dx0[1]))
    torch.cuda.synchronize()
    if exact:
        same_bits(xw.grad, dx0[1], tag + " dx")
        same_bits(gw.grad, dg0[1], tag + " dgamma")
        same_bits(bw.grad, db0[1], tag + " dbeta")
    else:       # the wrapper's backward read ITS forward's output and statistics, a few atomics-ordered bits from the direct call's: its own reference
        bw_ = NB.gn_backward(dout, sv[1].float().cpu().view(B, HW, C), x, res, sv[2].cpu(), gamma, G, act, dtype)
        within(xw.grad.float().cpu().view(B, HW, C), bw_["dx"], dtype, tag + " dx (wrapper)")
        within(gw.grad.cpu(), bw_["dgamma"], dtype, tag + " dgamma (wrapper)")
        within(bw.grad.cpu(), bw_["dbeta"], dtype, tag + " dbeta (wrapper)")
    if with_res:
        same_bits(rw.grad, xw.grad, tag + " dres")


@pytest.mark.parametrize("dtype", DTYPES, ids=list(NAME.values()))
def test_groupnorm_refusals(K, dtype):
    """C below the 16-byte group (the only C that would reach the fixed-channel order of the statistics kernels) and a residual off the vector path are
    refused by the host before anything is launched."""
    V = NB.VEC[dtype]
    code = K.HN.dtype_code(dtype)
    for C, G, with_res in ((V // 2, 1, False), (48, 16, True)):
        assert NB.gn_path(C, dtype) == ("channel" if C < V else "atomics")
        x = torch.zeros(1, 4, C, dtype=dtype, device=dev)
        p = torch.zeros(C, device=dev)
        part, gnp, out = NB.guarded((1, NB.GN_CHUNKS, C, 2), f32, dev), NB.guarded((1, G, 2), f32, dev), NB.guarded((1, 4, C), dtype, dev)
        with pytest.raises(K.L.SdeHipError):
            call(K, "sde_gn_relu_res_fwd", K.L.ptr(x), K.L.ptr(x if with_res else None), K.L.ptr(p), K.L.ptr(p), 1, 4, C, G, EPS, 1, code, K.L.ptr(part[1]), K.L.ptr(gnp[1]),
                 K.L.ptr(out[1]))
        with pytest.raises(K.L.SdeHipError):
            call(K, "sde_gn_relu_res_bwd", K.L.ptr(x), K.L.ptr(x), K.L.ptr(x), K.L.ptr(x if with_res else None), K.L.ptr(gnp[1]), K.L.ptr(p), 1, 4, C, G, 1, code,
                 K.L.ptr(part[1]), K.L.ptr(gnp[1]), K.L.ptr(p), K.L.ptr(p), 0, K.L.ptr(out[1]))
        for gd in (part, gnp, out):
            untouched(gd, "a refused GroupNorm call")


# ---------------------------------------------------------------------------------------------------------------------------------------
# random layer norm
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", NB.dtypes_of("rln"), ids=["f32", "bf16"])
@pytest.mark.parametrize("case", NB.RLN_CASES, ids=lambda c: f"C{c[0]}-Cr{c[1]}-HW{c[2]}-train{c[3]}-s{c[4]}{'-res' if c[5] else ''}{'-relu' if c[6] else ''}-g{c[7]}")
def test_rand_layer_norm(K, dtype, case):
    C, Cr, HW, train, s, with_res, relu, n_grads = case
    B = 2
    cch, TX, TY, per_thread = NB.rln_layout(C, dtype)
    if C == 192:
        assert 256 % cch != 0 and TX * TY < 256                     # idle threads in the workgroup
    if C == 2048:
        assert per_thread == (2 if dtype == f32 else 1) and TY == 1
    nch = NB.rln_chunks(HW)
    assert nch == K.L.lib().sde_randln_chunks(HW) == {2: 1, 63: 1, 64: 1, 200: 3, 5000: 32}[HW]
    code = K.HN.dtype_code(dtype)
    y, res, gamma, beta, z, grads = NB.rln_operands(B, HW, C, Cr, dtype, with_res, n_grads, C + HW)
    ref = NB.RLNForward(y, res, gamma, beta, z, s, train, NB.RLN_EPS, relu, dtype)
    yd, rd, gd, bd, zd = up(y, dtype), up(res, dtype), up(gamma), up(beta), up(z)
    sd = torch.tensor([s], dtype=f32, device=dev)
    part, rlnp, out = NB.guarded((B, NB.RLN_CHUNKS, C, 2), f32, dev), NB.guarded((B, C, 2), f32, dev), NB.guarded((B, HW, C), dtype, dev)
    call(K, "sde_randln_fwd", K.L.ptr(yd), K.L.ptr(rd), K.L.ptr(gd), K.L.ptr(bd), K.L.ptr(zd), K.L.ptr(sd), train, B, HW, C, Cr, NB.RLN_EPS, int(relu), code,
         K.L.ptr(part[1]), K.L.ptr(rlnp[1]), K.L.ptr(out[1]))
    tag = f"rln{' train' if train and s else ''}{' +res' if with_res else ''}{' relu' if relu else ''}"
    within(result(part, tag + " part", written=False)[:, :nch], ref.part, dtype, "rln part")
    got_rlnp = result(rlnp, tag + " rlnp")
    within(got_rlnp, ref.rlnp, dtype, "rlnp")
    got_out = result(out, tag + " out")
    within(got_out, ref.out, dtype, tag + " out")
    assert float(got_out[..., Cr:].abs().sum()) == 0.0 and float(got_rlnp[:, Cr:].abs().sum()) == 0.0
    # backward on what forward left
    gds = [up(t, dtype) for t in grads] + [None, None]
    g = torch.Generator().manual_seed(7)
    prior = (torch.randn(Cr, generator=g), torch.randn(Cr, generator=g))
    for acc in (0, 1):
        gm, dx = NB.guarded((B, HW, C), dtype, dev), NB.guarded((B, HW, C), dtype, dev)
        dgamma = filled((Cr,), f32, prior[0]) if acc else NB.guarded((Cr,), f32, dev)
        dbeta = filled((Cr,), f32, prior[1]) if acc else NB.guarded((Cr,), f32, dev)
        bpart = NB.guarded((B, NB.RLN_CHUNKS, C, 2), f32, dev)
        call(K, "sde_randln_bwd", K.L.ptr(gds[0]), K.L.ptr(gds[1]), K.L.ptr(gds[2]), K.L.ptr(out[1] if relu else None), K.L.ptr(yd), K.L.ptr(rlnp[1]), K.L.ptr(gd), int(relu),
             B, HW, C, Cr, code, K.L.ptr(bpart[1]), K.L.ptr(dgamma[1]), K.L.ptr(dbeta[1]), acc, K.L.ptr(gm[1]), K.L.ptr(dx[1]))
        b = NB.rln_backward(grads, got_out, y, got_rlnp, gamma, relu, dtype, prior=prior if acc else None)
        result(bpart, tag + " bwd part", written=False)
        within(result(gm, tag + " gm"), b["gm"], dtype, tag + " gm")
        got_dx = result(dx, tag + " dx")
        within(got_dx, b["dx"], dtype, tag + " dx")
        assert float(got_dx[..., Cr:].abs().sum()) == 0.0
        within(result(dgamma, tag + " dgamma"), b["dgamma"], dtype, tag + " dgamma")
        within(result(dbeta, tag + " dbeta"), b["dbeta"], dtype, tag + " dbeta")
        if acc == 0:
            keep = (dx[1], dgamma[1], dbeta[1], gm[1])
    # the autograd wrapper
    yw = yd.clone().view(B, 1, HW, C).requires_grad_(True)
    rw = rd.clone().view(B, 1, HW, C).requires_grad_(True) if with_res else None
    gw, bw = gd.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    o = K.HG.rand_layer_norm(yw, gw, bw, zd if train else None, sd if train else None, eps=NB.RLN_EPS, train=bool(train), residual=rw, relu=relu, n_out=n_grads)
    o = o if isinstance(o, tuple) else (o,)
    same_bits(o[0], out[1], tag + " out")
    torch.autograd.backward(list(o), [t.view(B, 1, HW, C) for t in gds[:n_grads]])
    same_bits(yw.grad, keep[0], tag + " dx")
    same_bits(gw.grad, keep[1], tag + " dgamma")
    same_bits(bw.grad, keep[2], tag + " dbeta")
    if with_res:
        same_bits(rw.grad, keep[3] if (relu or n_grads > 1) else gds[0], tag + " dres")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the seam to conv_bounds: the slab a convolution's epilogue hands to BatchNorm
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["persistent GEMM", "halo"])
def test_conv_slab_totals(K, kernel):
    """conv2d(..., bn_stats=True) on 2 x 15 x 31 x 64 -> 64 in bf16 (tests/conv_variant_table.py: the persistent LDS-DMA GEMM by default, the LDS-halo
    kernel when its workgroup threshold is lifted): the slab's column totals against the fp64 sums of the output AS STORED -- the epilogues sum the
    rounded values (norm_bounds.conv_slab_totals quotes them), so the convolution's own error, conv_bounds' subject, is not part of this limit."""
    import ctypes
    import math
    NN = K.HN
    g = torch.Generator().manual_seed(9)
    B, H, W, C = 2, 15, 31, 64
    x = (torch.randn(B, H, W, C, generator=g) + 0.3).to(torch.bfloat16).to(dev)
    w = (torch.randn(C, C, 3, 3, generator=g) / math.sqrt(C * 9)).to(torch.bfloat16).float().to(dev)
    old = K.L.lib().sde_conv_set_halo_min_blocks(0) if kernel == "halo" else None
    try:
        d = NN._desc(x, None, NN.SRC_PLAIN, 3, 3, 1, 1, False, H, W, H, W)
        variant = K.L.lib().sde_conv_fwd_variant(ctypes.byref(d), C)
        assert (variant == 3128064) if kernel == "halo" else (variant // 1000000 == 7), f"{kernel}: variant {variant}"
        with torch.no_grad():
            y, stats = NN.conv2d(x, w, None, stride=1, pad=1, bn_stats=True)
        torch.cuda.synchronize()
    finally:
        if old is not None:
            K.L.lib().sde_conv_set_halo_min_blocks(old)
    rows = stats.shape[0] - NN.REDUCE_ROWS
    tot = stats[:rows].double().sum(0).cpu()
    within(tot, NB.conv_slab_totals(y.float().cpu().view(-1, C)), torch.bfloat16, f"conv slab totals ({kernel})")

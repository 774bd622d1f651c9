"""CPU self-test of tests/norm_bounds.py: BatchNorm, GroupNorm and the random layer norm restated in fp32 torch, with the kernels' roundings and (where
it matters) their summation order, stay inside the helper's assertions; single planted faults -- the ones a whole-tensor relative L2 lets through -- are
rejected by the same assertion functions the GPU tests call; and every input of tests/test_gpu_norm_bounds.py keeps its undecided ReLU masks below
1 in 1000.

The emulations are written from the kernels (csrc/nn.hip, csrc/google.hip), in fp32 with explicit roundings, not from the helper's fp64 expressions, so
the two are independent statements of each operator."""
import pytest
import torch

import norm_bounds as NB

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "fp16"]
bydtype = pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
INF = float("inf")
EPS = 1e-5
f32 = torch.float32


def st(t, dtype):
    """(T)v: the value after the store in the activation type"""
    return t.to(dtype).float()


def within(got, bound, dtype, name):
    NB.assert_within(got, bound, dtype, name, l2_tol=INF)


def Bound_last(b, c):
    """index of the largest reference value of channel c of a [M, C] bound"""
    return int(b.ref[:, c].abs().argmax()), c


def rejects(got, bound, dtype, name):
    with pytest.raises(AssertionError):
        NB.assert_within(got, bound, dtype, name, l2_tol=INF)


def two_ulps(got, bound, dtype, idx=None):
    """got with one element (default: the largest reference value) moved by two units in the last place of the 16-bit storage type.  In fp32 the counted
    roundings of these kernels -- and the n u of the statistics every output inherits -- are themselves worth more than two ulps, so a correct limit
    cannot reject two: there the element is moved to the first ulp step beyond its limit."""
    bad = got.clone().double()
    if idx is None:
        i = int(bound.ref.abs().flatten().argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), bound.ref.shape))
    ulp = float(NB.ulp_of(bound.ref[idx].reshape(1), dtype))
    steps = 2 if dtype != torch.float32 else int((float(bound.lim[idx]) + abs(float(bad[idx]) - float(bound.ref[idx]))) // ulp) + 2
    bad[idx] = bad[idx] + steps * ulp
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------------
# BatchNorm
# ---------------------------------------------------------------------------------------------------------------------------------------
def emu_bn_finalize(part, n, gamma, beta, eps, rm, rv, mom, fault=None):
    """bn_finalize_kernel: fp64 fold (behind the fp32 chunk sums of rows_reduce_kernel for tall slabs), fp64 variance, fp32 parameters."""
    p = part
    chunk = NB.pre_reduce_chunk(p.shape[0])
    if chunk:
        p = torch.stack([p[i:i + chunk].sum(0, dtype=f32) for i in range(0, p.shape[0], chunk)])
    if fault == "row left out":
        p = p[1:]
    s = p.double().sum(0)
    mean = s[:, 0] / n
    var = (s[:, 1] / n - mean * mean).clamp(min=0)
    epsf = NB.f32(eps)
    rstd = (1.0 / (torch.sqrt(var) + epsf) if fault == "eps outside the root" else 1.0 / torch.sqrt(var + epsf)).float()
    sc = gamma * rstd
    bnp = torch.stack([mean.float(), rstd, sc, beta - mean.float() * sc])
    unb = var if (n <= 1 or fault == "biased running variance") else var * n / (n - 1.0)
    m = torch.tensor(mom, dtype=f32)
    return bnp, (1.0 - m) * rm + m * mean.float(), (1.0 - m) * rv + m * unb.float()


def emu_bn_apply(y, bnp, res, relu, dtype):
    t = NB.emu_fma(y, bnp[2], bnp[3])
    if res is not None:
        t = t + res
    return st(t.clamp(min=0) if relu else t, dtype), t


@bydtype
@pytest.mark.parametrize("rows,M,C", [(1, 33, 8), (9, 344, 64), (257, 600, 40), (4097, 4500, 8)])
def test_batchnorm_forward(dtype, rows, M, C):
    y, gamma, beta = NB.bn_input(M, C, dtype, 3)
    res = NB.draw((M, C), dtype, 4)
    part = NB.host_slab(y, rows)
    rm, rv = torch.randn(C, generator=torch.Generator().manual_seed(5)), torch.rand(C, generator=torch.Generator().manual_seed(6)) + 0.5
    ref = NB.BNForward(part, M, gamma, beta, EPS)
    brm, brv = ref.running(rm, rv)
    bnp, nrm, nrv = emu_bn_finalize(part, M, gamma, beta, EPS, rm, rv, 0.1)
    within(bnp, ref.bnp, f32, "bnp")
    within(nrm, brm, f32, "running mean")
    within(nrv, brv, f32, "running var")
    for r, relu in ((None, True), (res, True), (res, False)):
        out, _ = emu_bn_apply(y, bnp, r, relu, dtype)
        b = ref.out(y, r, relu, dtype)
        within(out, b, dtype, "bn out")
        within(out, NB.bn_apply(y, bnp, r, relu, dtype), dtype, "bn apply")
        sel = Bound_last(b, C - 1)
        rejects(two_ulps(out, b, dtype, sel), b, dtype, "bn out, one element two ulps off")
    # the planted faults
    if rows > 1:
        fb, _, _ = emu_bn_finalize(part, M, gamma, beta, EPS, rm, rv, 0.1, "row left out")
        rejects(fb, ref.bnp, f32, "bnp, one slab row left out")
    if rows <= NB.PRE_REDUCE_ABOVE:        # (behind the fp32 chunk sums of a taller slab the statistics carry 128 u, more than eps moves rstd at var ~ 2)
        fb, _, _ = emu_bn_finalize(part, M, gamma, beta, EPS, rm, rv, 0.1, "eps outside the root")
        rejects(fb, ref.bnp, f32, "bnp, eps outside the root")
    _, _, fv = emu_bn_finalize(part, M, gamma, beta, EPS, rm, rv, 0.1, "biased running variance")
    rejects(fv, brv, f32, "running var, biased")


def test_batchnorm_eval_params():
    g = torch.Generator().manual_seed(8)
    C = 40
    gamma, beta, rm, rv = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g), torch.randn(C, generator=g) * 3, torch.rand(C, generator=g) + 0.01
    b = NB.bn_eval_params(gamma, beta, rm, rv, EPS)
    rstd = 1.0 / torch.sqrt(rv + NB.f32(EPS))
    sc = gamma * rstd
    within(torch.stack([rm, rstd, sc, beta - rm * sc]), b, f32, "eval bnp")
    bad = 1.0 / (torch.sqrt(rv) + NB.f32(EPS))
    rejects(torch.stack([rm, bad, gamma * bad, beta - rm * gamma * bad]), b, f32, "eval bnp, eps outside the root")


def emu_bn_bwd(grads, out, y, bnp, relu_mode, dtype, nblk, fault=None, pre=None):
    """bn_bwd_reduce_kernel (per-workgroup fp32 partials over contiguous row ranges, fp64 fold) and the apply pass.  -> gm, dbeta, dgamma, coef, dy"""
    d = grads[0]
    use = grads[:1] if fault == "second gradient ignored" else grads[:2] if fault == "third gradient ignored" else grads
    for t in use[1:]:
        d = d + t
    if relu_mode == 1:
        d = torch.where((pre if fault == "mask before the residual" else out) > 0, d, torch.zeros_like(d))
    elif relu_mode == 2:
        d = torch.where(NB.emu_fma(y, bnp[2], bnp[3]) > 0, d, torch.zeros_like(d))
    gm = st(d, dtype)
    xh = (y - bnp[0]) * bnp[1]
    M = y.shape[0]
    part = NB.host_slab(torch.zeros(M, y.shape[1]), nblk)
    edges = [round(i * M / nblk) for i in range(nblk + 1)]
    for i in range(nblk):
        part[i, :, 0] = gm[edges[i]:edges[i + 1]].sum(0, dtype=f32)
        part[i, :, 1] = (gm * xh)[edges[i]:edges[i + 1]].sum(0, dtype=f32)
    s = part.double().sum(0)
    coef = torch.stack([s[:, 0] / M, s[:, 1] / M]).float()
    k1, k2 = (coef[1], coef[0]) if fault == "k1 and k2 swapped" else (coef[0], coef[1])
    inner = gm - k1 if fault == "xhat k2 dropped" else gm - k1 - xh * k2
    return gm, s[:, 0].float(), s[:, 1].float(), coef, st(bnp[2] * inner, dtype)


BWD_FAULTS = ["k1 and k2 swapped", "xhat k2 dropped", "second gradient ignored", "third gradient ignored", "mask before the residual"]


@bydtype
@pytest.mark.parametrize("M,C,n_grads,relu_mode", [(37, 64, 3, 1), (300, 24, 2, 2), (1, 8, 1, 0), (3000, 64, 3, 1)])
def test_batchnorm_backward(dtype, M, C, n_grads, relu_mode):
    y, bnp, res, grads, _, _ = NB.bn_bwd_operands(C, M, dtype, n_grads, relu_mode, 11)
    out, _ = emu_bn_apply(y, bnp, res, bool(relu_mode), dtype)
    pre = NB.emu_fma(y, bnp[2], bnp[3])
    mask, und = NB.bn_mask(y, bnp, res, relu_mode, dtype)
    NB.assert_decided(und, "bn backward")
    if relu_mode == 1:
        assert torch.equal((out > 0)[~und], mask.bool()[~und])
    nblk = max(1, M // 100)
    n_part = -(-M // nblk) + 1

    def run(fault=None):
        return emu_bn_bwd(grads, out, y, bnp, relu_mode, dtype, nblk, fault, pre)

    def check(r, expect_fail=()):
        gm, dbeta, dgamma, coef, dy = r
        s = NB.bn_sums(gm, y, bnp, n_part, nblk)
        got = {"gm": (gm, NB.bn_gm(grads, mask, und, dtype), dtype), "dbeta": (dbeta, s["dbeta"], f32), "dgamma": (dgamma, s["dgamma"], f32),
               "coef": (coef, s["coef"], f32), "dy": (dy, NB.bn_dy(gm, y, bnp, s["k"], s["ek"], dtype), dtype)}
        failed = set()
        for name, (g, b, dt) in got.items():
            try:
                within(g, b, dt, "bn " + name)
            except AssertionError:
                failed.add(name)
        return failed, got

    failed, got = check(run())
    assert not failed, failed
    dy, b, _ = got["dy"]
    if M > 1:
        rejects(two_ulps(dy, b, dtype, Bound_last(b, C - 1)), b, dtype, "dy, one element two ulps off")
        for fault in BWD_FAULTS:
            if ("second" in fault and n_grads < 2) or ("third" in fault and n_grads < 3) or ("mask" in fault and relu_mode != 1):
                continue
            failed, _ = check(run(fault))
            assert failed, f"'{fault}' passed every assertion"
        # a prior value in the slot (accumulate)
        prior = (torch.full((C,), 3.0), torch.full((C,), -2.0))
        gm, dbeta, dgamma, coef, _ = run()
        s = NB.bn_sums(gm, y, bnp, n_part, nblk, prior=prior)
        within(prior[0] + dgamma, s["dgamma"], f32, "dgamma accumulated")
        rejects(dgamma, s["dgamma"], f32, "dgamma, the slot overwritten")


@pytest.mark.parametrize("rows", NB.BN_FROM_PART_ROWS)
def test_batchnorm_backward_from_a_host_slab(rows):
    dtype, C = torch.bfloat16, 8
    M = 300 if rows <= 257 else 4200
    y, bnp, _, grads, _, _ = NB.bn_bwd_operands(C, M, dtype, 1, 0, 13)
    gm = grads[0]
    xh = (y - bnp[0]) * bnp[1]
    part = torch.stack([NB.host_slab(gm, rows)[..., 0], NB.host_slab(gm * xh, rows)[..., 0]], 2)
    s = NB.bn_sums(None, y, bnp, 0, rows, part=part)
    p = part
    chunk = NB.pre_reduce_chunk(rows)
    if chunk:
        p = torch.stack([p[i:i + chunk].sum(0, dtype=f32) for i in range(0, rows, chunk)])
    tot = p.double().sum(0)
    coef = (tot / M).float().t()
    within(coef, s["coef"], f32, "coef")
    within(tot[:, 1].float(), s["dgamma"], f32, "dgamma")
    dy = st(bnp[2] * (gm - coef[0] - xh * coef[1]), dtype)
    within(dy, NB.bn_dy(gm, y, bnp, s["k"], s["ek"], dtype), dtype, "dy")
    if rows > 1:
        tot2 = p[1:].double().sum(0)
        rejects((tot2 / M).float().t(), s["coef"], f32, "coef, one slab row left out")


@pytest.mark.parametrize("case", NB.BN_BWD_CASES, ids=lambda c: f"C{c[0]}-M{c[1]}-{c[2]}-mode{c[4]}")
def test_undecided_share_of_the_gpu_batchnorm_inputs(case):
    C, M, kinds, n_grads, relu_mode, _, _ = case
    for dtype in NB.dtypes_of(kinds):
        y, bnp, res, _, _, _ = NB.bn_bwd_operands(C, M, dtype, n_grads, relu_mode, 100 + C + M)
        mask, und = NB.bn_mask(y, bnp, res, relu_mode, dtype)
        NB.assert_decided(und, f"C={C} M={M} {dtype}")
        if relu_mode and C > 3:
            assert not und[:, 2].any() and not und[:, 3].any(), "the planted exact zeros are decided"
            if relu_mode == 2:
                assert float(mask[:, 2].sum()) == 0 and float(mask[0, 3]) == 0


def test_assert_decided_rejects_a_tensor_of_ties():
    und = torch.zeros(10, 100, dtype=torch.bool)
    und[0, :2] = True
    with pytest.raises(AssertionError):
        NB.assert_decided(und, "two in a thousand")
    und[0, 1] = False
    NB.assert_decided(und, "one in a thousand")


# ---------------------------------------------------------------------------------------------------------------------------------------
# GroupNorm
# ---------------------------------------------------------------------------------------------------------------------------------------
def emu_act(o, act):
    return o.clamp(min=0) if act == NB.ACT_RELU else torch.where(o > 0, o, torch.expm1(o)) if act == NB.ACT_ELU else o


def emu_gn_fwd(x, res, gamma, beta, G, eps, act, dtype, fault=None):
    B, HW, C = x.shape
    cpg = C // G
    v = x + res if res is not None else x
    part = torch.zeros(B, NB.GN_CHUNKS, C, 2)
    for q, (p0, p1) in enumerate(NB.chunk_ranges(HW, NB.GN_CHUNKS)):
        if fault == "pixel left out" and q == 0:
            p0 += 1
        if p1 > p0:
            part[:, q, :, 0], part[:, q, :, 1] = v[:, p0:p1].sum(1, dtype=f32), (v[:, p0:p1] * v[:, p0:p1]).sum(1, dtype=f32)
    s = part.double().sum(1).view(B, G, cpg, 2).sum(2)
    n = float(HW * cpg)
    mean = s[..., 0] / n
    var = (s[..., 1] / n - mean * mean).clamp(min=0)
    gnp = torch.stack([mean.float(), (1.0 / torch.sqrt(var + NB.f32(eps))).float()], 2)
    m, r = gnp[..., 0].repeat_interleave(cpg, 1).view(B, 1, C), gnp[..., 1].repeat_interleave(cpg, 1).view(B, 1, C)
    return part, gnp, st(emu_act((v - m) * r * gamma + beta, act), dtype)


def emu_gn_bwd(dout, out, x, res, gnp, gamma, G, act, dtype, fault=None):
    B, HW, C = x.shape
    cpg = C // G
    v = x + res if (res is not None and fault != "residual left out") else x
    src = x if fault == "derivative from x" else out
    de = torch.where(src > 0, dout, torch.zeros_like(dout)) if act == NB.ACT_RELU else torch.where(src > 0, dout, dout * (src + 1.0)) if act == NB.ACT_ELU else dout
    m, r = gnp[..., 0].repeat_interleave(cpg, 1).view(B, 1, C), gnp[..., 1].repeat_interleave(cpg, 1).view(B, 1, C)
    xh = (v - m) * r
    part = torch.zeros(B, NB.GN_CHUNKS, C, 2)
    for q, (p0, p1) in enumerate(NB.chunk_ranges(HW, NB.GN_CHUNKS)):
        if p1 > p0:
            part[:, q, :, 0], part[:, q, :, 1] = de[:, p0:p1].sum(1, dtype=f32), (de * xh)[:, p0:p1].sum(1, dtype=f32)
    pd = part.double()
    dbeta, dgamma = pd[..., 0].sum((0, 1)).float(), pd[..., 1].sum((0, 1)).float()
    n = float(HW * cpg)
    co = ((pd.sum(1) * gamma.double().view(1, C, 1)).view(B, G, cpg, 2).sum(2) / n).float()
    c1, c2 = co[..., 0].repeat_interleave(cpg, 1).view(B, 1, C), co[..., 1].repeat_interleave(cpg, 1).view(B, 1, C)
    return co, dgamma, dbeta, st(r * (gamma * de - c1 - xh * c2), dtype)


@bydtype
@pytest.mark.parametrize("C,G,HW,act,with_res", [(64, 16, 63, NB.ACT_ELU, True), (48, 48, 10, NB.ACT_ELU, False), (96, 16, 130, NB.ACT_RELU, False), (64, 16, 1, NB.ACT_NONE, True)])
def test_groupnorm(dtype, C, G, HW, act, with_res):
    B = 2
    x, res, gamma, beta, dout = NB.gn_operands(B, HW, C, dtype, with_res, 21)
    ref = NB.GNForward(x, res, gamma, beta, G, EPS, act, dtype)
    part, gnp, out = emu_gn_fwd(x, res, gamma, beta, G, EPS, act, dtype)
    within(part, ref.part, f32, "gn part")
    within(gnp, ref.gnp, f32, "gnp")
    within(out, ref.out, dtype, "gn out")
    rejects(two_ulps(out, ref.out, dtype), ref.out, dtype, "gn out, one element two ulps off")
    if HW > 1:
        fp, fg, _ = emu_gn_fwd(x, res, gamma, beta, G, EPS, act, dtype, "pixel left out")
        rejects(fp, ref.part, f32, "gn part, one pixel left out")
        rejects(fg, ref.gnp, f32, "gnp, one pixel left out")
    b = NB.gn_backward(dout, out, x, res, gnp, gamma, G, act, dtype)

    def failing(r):
        bad = set()
        for name, g, dt in zip(("coef", "dgamma", "dbeta", "dx"), r, (f32, f32, f32, dtype)):
            try:
                within(g, b[name], dt, "gn " + name)
            except AssertionError:
                bad.add(name)
        return bad
    good = emu_gn_bwd(dout, out, x, res, gnp, gamma, G, act, dtype)
    assert not failing(good)
    if HW > 1:
        rejects(two_ulps(good[3], b["dx"], dtype), b["dx"], dtype, "gn dx, one element two ulps off")
    if with_res and HW > 1:
        assert failing(emu_gn_bwd(dout, out, x, res, gnp, gamma, G, act, dtype, "residual left out"))
    if act == NB.ACT_ELU:
        assert failing(emu_gn_bwd(dout, out, x, res, gnp, gamma, G, act, dtype, "derivative from x"))


def test_groupnorm_paths_by_channel_count():
    """The rule of gn_stats_kernel, restated: which C reaches which order.  The fixed-channel order needs C < the 16-byte group (refused by the host)."""
    for dtype in DTYPES:
        assert NB.gn_path(64, dtype) == NB.gn_path(512, dtype) == "vector"
        assert NB.gn_path(48, dtype) == NB.gn_path(96, dtype) == NB.gn_path(192, dtype) == "atomics"
        assert NB.gn_path(768, dtype) == NB.gn_path(1536, dtype) == "slots"
        V = NB.VEC[dtype]
        assert all(NB.gn_path(c, dtype) != "channel" for c in range(V, 4097, V))
        assert NB.gn_path(V // 2, dtype) == "channel"
    for C, G, HW, act, with_res, path in NB.GN_CASES:
        assert all(NB.gn_path(C, dt) == path for dt in DTYPES) and (not with_res or path == "vector")


# ---------------------------------------------------------------------------------------------------------------------------------------
# random layer norm
# ---------------------------------------------------------------------------------------------------------------------------------------
def emu_rln_fwd(y, res, gamma, beta, z, s, train, eps, relu, dtype, fault=None):
    B, HW, C = y.shape
    Cr = gamma.numel()
    nch = NB.rln_chunks(HW)
    k = y[:, :1]
    d = y - k
    part = torch.zeros(B, nch, C, 2)
    for q, (p0, p1) in enumerate(NB.chunk_ranges(HW, nch)):
        part[:, q, :, 0], part[:, q, :, 1] = d[:, p0:p1].sum(1, dtype=f32), (d[:, p0:p1] * d[:, p0:p1]).sum(1, dtype=f32)
    sd = part.double().sum(1)
    n = float(HW)
    mean = (0.0 if fault == "no shift on the mean" else k[:, 0].double()) + sd[..., 0] / n
    var = ((sd[..., 1] - sd[..., 0] * sd[..., 0] / n) / (n - 1.0)).clamp(min=0)
    fm = fv = torch.ones(B, Cr)
    sf = torch.tensor(s, dtype=f32)
    if train and float(sf) != 0.0:
        f = 1.0 + torch.fmod(z * sf, sf * 2.0)
        fm, fv = f[0], f[1]
    m = mean[:, :Cr].float() * fm
    r = (1.0 / torch.sqrt((var[:, :Cr].float() * fv).double() + NB.f32(eps))).float()
    rlnp = torch.zeros(B, C, 2)
    rlnp[:, :Cr, 0], rlnp[:, :Cr, 1] = m, r
    o = gamma * ((y[..., :Cr] - m.unsqueeze(1)) * r.unsqueeze(1)) + beta
    if res is not None:
        o = o + res[..., :Cr]
    if relu:
        o = o.clamp(min=0)
    out = y.clone() if fault == "padding not zeroed" else torch.zeros(B, HW, C)
    out[..., :Cr] = o
    return part, rlnp, st(out, dtype)


def emu_rln_bwd(grads, out, y, rlnp, gamma, relu, dtype, fault=None):
    B, HW, C = y.shape
    Cr = gamma.numel()
    nch = NB.rln_chunks(HW)
    use = grads[:1] if fault == "second gradient ignored" else grads
    gv = use[0]
    for t in use[1:]:
        gv = gv + t
    if relu:
        gv = torch.where(out > 0, gv, torch.zeros_like(gv))
    m, r = rlnp[..., 0].unsqueeze(1), rlnp[..., 1].unsqueeze(1)
    k = torch.ones(B, 1, C) if fault == "padding not zeroed" else torch.zeros(B, 1, C)
    k[..., :Cr] = gamma * r[..., :Cr]
    t2 = gv * ((y - m) * r)
    part = torch.zeros(B, nch, C, 2)
    for q, (p0, p1) in enumerate(NB.chunk_ranges(HW, nch)):
        part[:, q, :, 0], part[:, q, :, 1] = gv[:, p0:p1].sum(1, dtype=f32), t2[:, p0:p1].sum(1, dtype=f32)
    pd = part.double().sum((0, 1))
    return st(gv, dtype), st(gv * k, dtype), pd[:Cr, 1].float(), pd[:Cr, 0].float()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C,Cr,HW,train,s,with_res,relu,n_grads", [(64, 61, 63, 1, NB.RLN_STDDEV, True, True, 2), (64, 61, 200, 1, 0.0, True, False, 1),
                                                                   (192, 190, 130, 0, NB.RLN_STDDEV, False, True, 3), (64, 61, 2, 1, NB.RLN_STDDEV, False, False, 1)])
def test_rand_layer_norm(dtype, C, Cr, HW, train, s, with_res, relu, n_grads):
    B = 2
    y, res, gamma, beta, z, grads = NB.rln_operands(B, HW, C, Cr, dtype, with_res, n_grads, 31)
    ref = NB.RLNForward(y, res, gamma, beta, z, s, train, NB.RLN_EPS, relu, dtype)
    part, rlnp, out = emu_rln_fwd(y, res, gamma, beta, z, s, train, NB.RLN_EPS, relu, dtype)
    within(part, ref.part, f32, "rln part")
    within(rlnp, ref.rlnp, f32, "rlnp")
    within(out, ref.out, dtype, "rln out")
    rejects(two_ulps(out, ref.out, dtype), ref.out, dtype, "rln out, one element two ulps off")
    _, fr, fo = emu_rln_fwd(y, res, gamma, beta, z, s, train, NB.RLN_EPS, relu, dtype, "no shift on the mean")
    rejects(fr, ref.rlnp, f32, "rlnp, no shift on the mean")
    rejects(fo, ref.out, dtype, "rln out, no shift on the mean")
    _, _, fo = emu_rln_fwd(y, res, gamma, beta, z, s, train, NB.RLN_EPS, relu, dtype, "padding not zeroed")
    rejects(fo, ref.out, dtype, "rln out, padding not zeroed")
    if train and s:
        # the factors are not 1: a kernel that forgets the noise is outside the limits
        _, fr, _ = emu_rln_fwd(y, res, gamma, beta, z, 0.0, train, NB.RLN_EPS, relu, dtype)
        rejects(fr, ref.rlnp, f32, "rlnp, noise factors left out")
    b = NB.rln_backward(grads, out, y, rlnp, gamma, relu, dtype)

    def failing(r):
        bad = set()
        for name, g, dt in zip(("gm", "dx", "dgamma", "dbeta"), r, (dtype, dtype, f32, f32)):
            try:
                within(g, b[name], dt, "rln " + name)
            except AssertionError:
                bad.add(name)
        return bad
    assert not failing(emu_rln_bwd(grads, out, y, rlnp, gamma, relu, dtype))
    if not relu:            # (behind a ReLU the zero padding of the stored output masks the padding gradients anyway)
        assert "dx" in failing(emu_rln_bwd(grads, out, y, rlnp, gamma, relu, dtype, "padding not zeroed"))
    if n_grads > 1:
        assert failing(emu_rln_bwd(grads, out, y, rlnp, gamma, relu, dtype, "second gradient ignored"))


def test_rand_layer_norm_layouts_and_chunks():
    """google.hip's Layout and chunk rule, restated for the cases of the GPU file."""
    assert [NB.rln_chunks(hw) for hw in (2, 63, 64, 127, 128, 200, 5000)] == [1, 1, 1, 1, 2, 3, 32]
    assert NB.rln_layout(192, torch.bfloat16) == (24, 24, 10, 1) and 256 % 24 != 0          # 16 threads of the workgroup stay idle
    assert NB.rln_layout(192, torch.float32) == (48, 48, 5, 1)
    assert NB.rln_layout(2048, torch.float32) == (512, 256, 1, 2)                           # two channel groups per thread
    assert NB.rln_layout(2048, torch.bfloat16) == (256, 256, 1, 1)

"""GPU parity of the concat-free dense-block operators (csrc/dense.hip, hip/dense.py): relu(BatchNorm2d(torch.cat(pieces, 1))) with the
gradients of every piece gathered per piece, and the transitions' AvgPool2d(2, 2).

Everything is compared with
  * torch on the CPU (cat -> BatchNorm2d in training mode -> ReLU) in fp32 from operands rounded to the storage type (relative L2: 6e-3 for the
    output and 1.5 x that for gradients in bf16 = 16-bit output rounding; 1e-3 in fp32: the limits of tests/test_gpu_gconv.py; running statistics
    within the output limit), and
  * the composed route -- hip.bts.cat + hip.bts.channel_stats + HipBatchNorm2d -- on the same device buffers (hip.dense.DENSE_DIRECT = False):
    fp32 arithmetic both, so at most one 16-bit ulp apart (close16 of tests/test_gpu_gconv.py); in fp32 2e-5 of the maximum.

Inputs are standard normal except in the two-pixel case, which draws them at 0.005: with two values per channel xhat is +-sqrt(var / (var + eps)),
so BatchNorm's input gradient is the incoming one times eps / (var + eps) -- at unit scale 1e-5 of it, the float32 cancellation noise of any
implementation (torch's included); at that scale var ~ eps and the gradient is a well-conditioned number again.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
dev = "cuda"

CASES = {  # name: (B, H, W, piece widths, input scale)
    "two_values_per_channel": (2, 1, 1, (8, 8), 0.005),
    "ragged": (2, 3, 5, (16, 8, 8, 8), 1.0),
    "several_reduce_rows": (2, 33, 47, (64, 32, 32), 1.0),
    "densenet161_widest_transition": (2, 2, 3, (96,) + (48,) * 36, 1.0),
}
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
POOLS = [(2, 2, 2, 8), (2, 5, 7, 16), (2, 32, 46, 64)]


def close16(a, b, dt, what):
    """16-bit tensors that may differ by summation order only: <= 1 ulp + a small absolute term (tests/test_gpu_gconv.py)."""
    a, b = a.float(), b.float()
    ulp = 2.0 ** -7 if dt == torch.bfloat16 else 2.0 ** -10
    err = (a - b).abs()
    bad = (err > ulp * torch.maximum(a.abs(), b.abs()) + 2e-3).sum().item()
    assert bad == 0, f"{what}: {bad} of {a.numel()} elements differ by more than one ulp (max {err.max().item():.3e})"


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def limits(dt):
    lim = 6e-3 if dt == torch.bfloat16 else 1e-3
    return lim, (1.5 * lim if dt == torch.bfloat16 else lim)


def nhwc(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().to(dt).to(dev)


def nchw(t):
    return t.detach().float().cpu().permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def reference(name, dtype):
    """Operands (rounded to the storage type) and the CPU fp32 result: computed once per case, shared by the tests, never modified."""
    B, H, W, widths, scale = CASES[name]
    dt = DT[dtype]
    g = torch.Generator().manual_seed(len(name) * 7 + B)
    C = sum(widths)
    pieces = [(torch.randn(B, c, H, W, generator=g) * scale + 0.3 * scale).to(dt).float() for c in widths]
    gamma, beta = 1 + 0.5 * torch.randn(C, generator=g), 0.5 * torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    gy = torch.randn(B, C, H, W, generator=g).to(dt).float()
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    leaves = [p.clone().requires_grad_(True) for p in pieces]
    y = F.relu(bn.train()(torch.cat(leaves, 1)))
    y.backward(gy)
    with torch.no_grad():
        ev = torch.nn.BatchNorm2d(C).eval()
        ev.weight.copy_(gamma); ev.bias.copy_(beta); ev.running_mean.copy_(rm); ev.running_var.copy_(rv)
        y_eval = F.relu(ev(torch.cat(pieces, 1)))
    return dict(pieces=pieces, gamma=gamma, beta=beta, rm=rm, rv=rv, gy=gy, y=y.detach(), dp=[p.grad for p in leaves], dgamma=bn.weight.grad, dbeta=bn.bias.grad,
                rm_out=bn.running_mean.clone(), rv_out=bn.running_var.clone(), y_eval=y_eval)


def make_norm(ref, training=True):
    from simpledepthestimation_amd.layers.hip_modules import HipBatchNorm2d
    norm = HipBatchNorm2d(ref["gamma"].numel())
    with torch.no_grad():
        norm.weight.copy_(ref["gamma"]); norm.bias.copy_(ref["beta"]); norm.running_mean.copy_(ref["rm"]); norm.running_var.copy_(ref["rv"])
    return norm.to(dev).train(training)


def run_device(name, dtype, direct, backwards=1):
    from simpledepthestimation_amd.hip import bts as HB
    from simpledepthestimation_amd.hip import dense as HD
    ref, dt = reference(name, dtype), DT[dtype]
    old = HD.DENSE_DIRECT
    HD.DENSE_DIRECT = direct
    try:
        norm = make_norm(ref)
        leaves = [nhwc(p, dt).requires_grad_(True) for p in ref["pieces"]]
        gy = nhwc(ref["gy"], dt)
        for _ in range(backwards):
            blk = HD.DenseBlock(sum(p.shape[-1] for p in leaves))
            for p in leaves:
                HD.dense_piece(p, blk, HB.channel_stats(p))
            y = HD.dense_bn_relu(blk, norm)
            y.backward(gy)
        torch.cuda.synchronize()
    finally:
        HD.DENSE_DIRECT = old
    return dict(y=y.detach().cpu(), dp=[p.grad.cpu() for p in leaves], dgamma=norm.weight.grad.cpu(), dbeta=norm.bias.grad.cpu(),
                rm=norm.running_mean.cpu(), rv=norm.running_var.cpu(), batches=int(norm.state_dict()["num_batches_tracked"]))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_dense_bn_relu(name, dtype):
    B, H, W, widths, _ = CASES[name]
    dt = DT[dtype]
    ref = reference(name, dtype)
    on = run_device(name, dtype, True)
    off = run_device(name, dtype, False)
    lim, glim = limits(dt)
    assert tuple(on["y"].shape) == (B, H, W, sum(widths)) and on["y"].dtype == dt and on["batches"] == 1
    errs = {"y": rel(nchw(on["y"]), ref["y"]), "running_mean": rel(on["rm"], ref["rm_out"]), "running_var": rel(on["rv"], ref["rv_out"]),
            "dgamma": rel(on["dgamma"], ref["dgamma"]), "dbeta": rel(on["dbeta"], ref["dbeta"]),
            "dpieces": rel(torch.cat([nchw(p) for p in on["dp"]], 1), torch.cat(ref["dp"], 1))}
    worst_piece = max(rel(nchw(p), r) for p, r in zip(on["dp"], ref["dp"]))
    print("  " + name, dtype, " ".join(f"{k} {v:.2e}" for k, v in errs.items()), f"worst piece {worst_piece:.2e}")
    for k in ("y", "running_mean", "running_var"):
        assert errs[k] < lim, f"{k} vs fp32 CPU: relative L2 error {errs[k]:.3e}"
    for k in ("dgamma", "dbeta", "dpieces"):
        assert errs[k] < glim, f"{k} vs fp32 CPU: relative L2 error {errs[k]:.3e}"
    assert worst_piece < glim, f"gradient of one piece vs fp32 CPU: relative L2 error {worst_piece:.3e}"
    # ... and against the composed route on the same buffers
    pairs = [("y", on["y"], off["y"])] + [(f"dpiece{k}", a, b) for k, (a, b) in enumerate(zip(on["dp"], off["dp"]))]
    for what, a, b in pairs:
        if dt == torch.float32:
            assert (a - b).abs().max() <= 2e-5 * b.abs().max(), f"{what}: direct vs composed {(a - b).abs().max():.3e} of {b.abs().max():.3e}"
        else:
            close16(a, b, dt, what + " direct vs composed")
    for what in ("dgamma", "dbeta", "rm", "rv"):
        assert (on[what] - off[what]).abs().max() <= 2e-5 * off[what].abs().max() + 1e-6, what


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_two_runs_are_bit_identical(dtype):
    a = run_device("several_reduce_rows", dtype, True)
    b = run_device("several_reduce_rows", dtype, True)
    for k in ("y", "dgamma", "dbeta", "rm", "rv"):
        assert torch.equal(a[k], b[k]), k
    assert all(torch.equal(p, q) for p, q in zip(a["dp"], b["dp"]))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_second_backward_accumulates_into_existing_grads(dtype):
    one = run_device("ragged", dtype, True)
    two = run_device("ragged", dtype, True, backwards=2)
    assert two["batches"] == 2
    for k in ("dgamma", "dbeta"):          # the second pass adds into the fp32 .grad of the first, inside the kernel
        assert (two[k] - 2 * one[k]).abs().max() <= 1e-6 * one[k].abs().max(), k
    lim, glim = limits(DT[dtype])
    for p, q in zip(two["dp"], one["dp"]):  # the pieces' .grad (storage type) is summed by autograd
        assert rel(p.float(), 2 * q.float()) < glim


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_gather_sums_three_consumers_and_an_outside_gradient(dtype):
    """Pieces p0..p3; three norms read (p0,p1), (p0,p1,p2), (p0..p3): p1 has three readers inside the block, and its alias is read outside it too."""
    from simpledepthestimation_amd.hip import bts as HB
    from simpledepthestimation_amd.hip import dense as HD
    from simpledepthestimation_amd.layers.hip_modules import HipBatchNorm2d
    dt = DT[dtype]
    g = torch.Generator().manual_seed(5)
    B, H, W, widths = 2, 5, 7, (16, 8, 8, 8)
    pieces = [torch.randn(B, c, H, W, generator=g).to(dt).float() for c in widths]
    readers = [2, 3, 4]
    params = [(1 + 0.5 * torch.randn(sum(widths[:n]), generator=g), 0.5 * torch.randn(sum(widths[:n]), generator=g)) for n in readers]
    cots = [torch.randn(B, sum(widths[:n]), H, W, generator=g).to(dt).float() for n in readers]
    outside = torch.randn(B, widths[1], H, W, generator=g).to(dt).float()
    leaves = [p.clone().requires_grad_(True) for p in pieces]
    loss = (leaves[1] * outside).sum()
    for n, (ga, be), c in zip(readers, params, cots):
        loss = loss + (F.relu(F.batch_norm(torch.cat(leaves[:n], 1), None, None, ga, be, True)) * c).sum()
    loss.backward()
    dl = [nhwc(p, dt).requires_grad_(True) for p in pieces]
    blk = HD.DenseBlock(sum(widths))
    outs, alias = [], None
    for k, p in enumerate(dl):
        a = HD.dense_piece(p, blk, HB.channel_stats(p))
        alias = a if k == 1 else alias
        if k + 1 in readers:
            norm = HipBatchNorm2d(blk.width).to(dev)
            with torch.no_grad():
                norm.weight.copy_(params[readers.index(k + 1)][0]); norm.bias.copy_(params[readers.index(k + 1)][1])
            outs.append(HD.dense_bn_relu(blk, norm))
    torch.autograd.backward(outs + [alias], [nhwc(c, dt) for c in cots] + [nhwc(outside, dt)])
    torch.cuda.synchronize()
    lim, glim = limits(dt)
    errs = [rel(nchw(d.grad), p.grad) for d, p in zip(dl, leaves)]
    print("  gather", dtype, " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < glim, errs


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", POOLS)
def test_avg_pool_2x2(shape, dtype):
    from simpledepthestimation_amd.hip import dense as HD
    B, H, W, C = shape
    dt = DT[dtype]
    g = torch.Generator().manual_seed(H * W)
    x = torch.randn(B, C, H, W, generator=g).to(dt).float()
    gy = torch.randn(B, C, H // 2, W // 2, generator=g).to(dt).float()
    xr = x.clone().requires_grad_(True)
    y = F.avg_pool2d(xr, 2, 2)
    y.backward(gy)
    xd = nhwc(x, dt).requires_grad_(True)
    yd = HD.avg_pool_2x2(xd)
    yd.backward(nhwc(gy, dt))
    torch.cuda.synchronize()
    lim, glim = limits(dt)
    assert tuple(yd.shape) == (B, H // 2, W // 2, C) and yd.dtype == dt
    assert rel(nchw(yd), y.detach()) < lim and rel(nchw(xd.grad), xr.grad) < glim
    if H % 2:
        assert float(xd.grad[:, H - 1].abs().max()) == 0.0       # the odd last row lies outside every window


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_eval_mode_uses_the_running_statistics(dtype):
    from simpledepthestimation_amd.hip import dense as HD
    ref, dt = reference("ragged", dtype), DT[dtype]
    norm = make_norm(ref, training=False)
    blk = HD.DenseBlock(norm.num_features, track=False)
    with torch.no_grad():
        for p in ref["pieces"]:
            HD.dense_piece(nhwc(p, dt), blk)
        y = HD.dense_bn_relu(blk, norm)
    torch.cuda.synchronize()
    assert rel(nchw(y), ref["y_eval"]) < limits(dt)[0]
    assert torch.equal(norm.running_mean.cpu(), ref["rm"]) and int(norm.state_dict()["num_batches_tracked"]) == 0


@pytest.mark.parametrize("what", ["fp16", "width12", "41pieces"])
def test_refusals(what):
    from simpledepthestimation_amd.hip import dense as HD
    from simpledepthestimation_amd.hip.lib import SdeHipError
    from simpledepthestimation_amd.layers.hip_modules import HipBatchNorm2d
    dt, width, n = (torch.float16, 8, 2) if what == "fp16" else (torch.bfloat16, 12, 2) if what == "width12" else (torch.bfloat16, 8, 41)
    norm = HipBatchNorm2d(width * n).to(dev).eval()
    blk = HD.DenseBlock(width * n, track=False)
    for _ in range(n):
        HD.dense_piece(torch.zeros(2, 3, 3, width, device=dev, dtype=dt), blk)
    with pytest.raises(SdeHipError, match={"fp16": "fp32 and bf16 only", "width12": "multiple of 8", "41pieces": "1..40 pieces"}[what]):
        HD.dense_bn_relu(blk, norm)
    if what == "fp16":
        with pytest.raises(SdeHipError, match="fp32 and bf16 only"):
            HD.avg_pool_2x2(torch.zeros(2, 4, 4, 8, device=dev, dtype=dt))

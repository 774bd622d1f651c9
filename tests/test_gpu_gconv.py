"""GPU parity of the grouped 3x3 convolution (csrc/gconv.hip, hip.nn.grouped_conv3x3): Conv2d(C, C, 3, stride 1 | 2, padding 1, groups=G, bias=False),
the 3x3 of a ResNeXt bottleneck.

Forward and both gradients are compared with
  * F.conv2d(groups=G) on the CPU in fp32 from the operands rounded to the storage type, as tests/test_gpu_deconv.py does (relative L2: 6e-3 for y and
    1.5 x that for gradients in bf16 = 16-bit output rounding; 1e-3 in fp32), and
  * the composed route -- a dense block-diagonal weight through hip.nn.conv2d -- on the same device buffers (hip.nn.GCONV_DIRECT = False): fp32
    accumulation both, so at most one 16-bit ulp apart (close16 of that file); in fp32 2e-5 of the maximum, and
  * element by element, an fp64 reference with the a-priori limits of tests/conv_bounds.py (Conv3x3Case): y, dX and dW of both routes, and the two
    routes against each other.
"""
import functools
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_bounds as CB

pytestmark = pytest.mark.gpu
dev = "cuda"

CASES = {  # name: (B, H, W, C, G, stride)
    "1x1_every_neighbour_out_of_range": (1, 1, 1, 32, 8, 1),
    "odd_sizes_stride2_cg8": (2, 3, 5, 64, 8, 2),
    "ragged_tiles_cg16": (3, 13, 9, 64, 4, 1),
    "cg32_even_sizes_stride2": (2, 6, 10, 64, 2, 2),
    "cg64": (2, 5, 7, 128, 2, 1),
    "resnext50_layer1_cg4": (2, 4, 4, 128, 32, 1),
    "three_super_groups_c48_stride2": (2, 5, 7, 48, 12, 2),
    "many_pixel_tiles": (2, 33, 47, 32, 8, 1),        # weight-gradient partials of several workgroups, several statistics rows
}
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
REF_DT = dict(DT, fp16=torch.float16)       # the references also in fp16, for the CPU self-test of their bounds (tests/test_conv_bounds.py)


def close16(a, b, dt, what):
    """16-bit tensors that may differ by summation order only: <= 1 ulp + a small absolute term (tests/test_gpu_conv_small.py)."""
    a, b = a.float(), b.float()
    ulp = 2.0 ** -7 if dt == torch.bfloat16 else 2.0 ** -10
    err = (a - b).abs()
    bad = (err > ulp * torch.maximum(a.abs(), b.abs()) + 2e-3).sum().item()
    assert bad == 0, f"{what}: {bad} of {a.numel()} elements differ by more than one ulp (max {err.max().item():.3e})"


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@functools.lru_cache(maxsize=None)
def reference(name, dtype):
    """Operands (rounded to the storage type) and the CPU fp32 result: computed once per case, shared by the tests, never modified."""
    B, H, W, C, G, stride = CASES[name]
    dt = REF_DT[dtype]
    g = torch.Generator().manual_seed(len(name) * 13 + B)
    x = torch.randn(B, C, H, W, generator=g).to(dt).float()
    w = torch.randn(C, C // G, 3, 3, generator=g) / math.sqrt(C // G * 2.25)
    w[:, :, 0, 2] *= 3                                 # a flipped or transposed tap shows
    w = w.to(dt).float()
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, None, stride, 1, groups=G)
    gy = torch.randn(y.shape, generator=g).to(dt).float()
    y.backward(gy)
    return dict(x=x, w=w, gy=gy, y=y.detach(), dx=xr.grad, dw=wr.grad)


@functools.lru_cache(maxsize=None)
def bounds(name, dtype):
    """(Conv3x3Case, its gradient bounds) of reference(name, dtype): fp64, computed once per case."""
    B, H, W, C, G, stride = CASES[name]
    ref = reference(name, dtype)
    case = CB.Conv3x3Case(ref["x"], ref["w"], REF_DT[dtype], groups=G, stride=stride)
    return case, case.backward(ref["gy"])


def nchw(t):
    return t.float().permute(0, 3, 1, 2)


def nhwc(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().to(dt).to(dev)


def run_device(name, dtype, direct, backwards=1, ohwi=False, stats=False):
    from simpledepthestimation_amd.hip import nn as NN
    B, H, W, C, G, stride = CASES[name]
    ref, dt = reference(name, dtype), DT[dtype]
    old = NN.GCONV_DIRECT
    NN.GCONV_DIRECT = direct
    try:
        xd = nhwc(ref["x"], dt).requires_grad_(True)
        if ohwi:      # HipTrainer's layout: channels-last memory under the usual shape, for the weight and its gradient slot
            wd = ref["w"].permute(0, 2, 3, 1).contiguous().to(dev).permute(0, 3, 1, 2).requires_grad_(True)
            wd.grad = torch.zeros(C, 3, 3, C // G, device=dev).permute(0, 3, 1, 2)
        else:
            wd = ref["w"].clone().to(dev).requires_grad_(True)
        gyd = nhwc(ref["gy"], dt)
        st = None
        for _ in range(backwards):
            y = NN.grouped_conv3x3(xd, wd, G, stride, bn_stats=stats)
            if stats:
                y, st = y
            y.backward(gyd)
        torch.cuda.synchronize()
    finally:
        NN.GCONV_DIRECT = old
    return dict(y=y.detach().cpu(), dx=xd.grad.cpu(), dw=wd.grad.cpu(), stats=st.cpu() if st is not None else None)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_grouped_conv3x3(name, dtype):
    B, H, W, C, G, stride = CASES[name]
    dt = DT[dtype]
    ref = reference(name, dtype)
    on = run_device(name, dtype, True)
    off = run_device(name, dtype, False)
    lim = 6e-3 if dt == torch.bfloat16 else 1e-3
    glim = 1.5 * lim if dt == torch.bfloat16 else lim
    y = on["y"]
    assert tuple(y.shape) == (B, (H - 1) // stride + 1, (W - 1) // stride + 1, C) and y.dtype == dt
    errs = {"y": rel(y.float().permute(0, 3, 1, 2), ref["y"]), "dx": rel(on["dx"].float().permute(0, 3, 1, 2), ref["dx"]), "dW": rel(on["dw"], ref["dw"])}
    print("  " + name, dtype, " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["y"] < lim, f"y vs fp32 CPU: relative L2 error {errs['y']:.3e}"
    for k in ("dx", "dW"):
        assert errs[k] < glim, f"{k} vs fp32 CPU: relative L2 error {errs[k]:.3e}"
    # every element of both routes against the fp64 reference, and the two routes against each other (the relative-L2 lines are the ones above)
    case, bw = bounds(name, dtype)
    for route, out in (("kernels", on), ("composed", off)):
        CB.assert_within(nchw(out["y"]), case.y, dt, f"{dtype} gconv y ({route})", l2_tol=float("inf"))
        CB.assert_within(nchw(out["dx"]), bw["dX"], dt, f"{dtype} gconv dX ({route})", l2_tol=float("inf"))
        CB.assert_within(out["dw"], bw["dW"], torch.float32, f"{dtype} gconv dW ({route})", l2_tol=float("inf"))
    CB.assert_two_kernels(nchw(on["y"]), nchw(off["y"]), case.y, dt, f"{dtype} gconv y (kernels vs composed)")
    CB.assert_two_kernels(nchw(on["dx"]), nchw(off["dx"]), bw["dX"], dt, f"{dtype} gconv dX (kernels vs composed)")
    CB.assert_two_kernels(on["dw"], off["dw"], bw["dW"], torch.float32, f"{dtype} gconv dW (kernels vs composed)")
    # the grouped kernels against the dense block-diagonal route on the same buffers
    if dt == torch.bfloat16:
        close16(y, off["y"], dt, "y (grouped kernels vs dense block-diagonal weight)")
        close16(on["dx"], off["dx"], dt, "dx")
    else:
        for k in ("y", "dx", "dw"):
            e = float((on[k].double() - off[k].double()).abs().max() / off[k].double().abs().max())
            print(f"    {k}: kernels vs composed {e:.2e}")
            assert e <= 2e-5, f"{k}: grouped kernels vs composed route {e:.2e}"


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name,ohwi", [("odd_sizes_stride2_cg8", False), ("ragged_tiles_cg16", True)])
def test_second_backward_accumulates_into_existing_grads(name, ohwi, dtype):
    """The first backward returns fresh gradients (or adds into the zeroed slot the weight already owns: `ohwi`, HipTrainer's channels-last layout of the
    weight and its gradient); from then on the parameter owns an fp32 .grad and the reduce launch adds into it in place."""
    dt = DT[dtype]
    ref = reference(name, dtype)
    two = run_device(name, dtype, True, backwards=2, ohwi=ohwi)
    glim = 1.5 * 6e-3 if dt == torch.bfloat16 else 1e-3
    assert rel(two["dw"], 2 * ref["dw"]) < glim
    assert rel(two["dx"].float().permute(0, 3, 1, 2), 2 * ref["dx"]) < glim
    assert rel(two["y"].float().permute(0, 3, 1, 2), ref["y"]) < (6e-3 if dt == torch.bfloat16 else 1e-3)
    # element by element: two gradients, each within its bound, and the rounding of their stored sum (dX: autograd's add in the activation dtype; dW: the
    # reduce launch's add into the fp32 slot)
    case, bw = bounds(name, dtype)
    CB.assert_within(nchw(two["y"]), case.y, dt, f"{dtype} gconv y (second backward)", l2_tol=float("inf"))
    CB.assert_within(nchw(two["dx"]), CB.accumulated(bw["dX"], 2, dt), dt, f"{dtype} gconv dX (second backward)", l2_tol=float("inf"))
    CB.assert_within(two["dw"], CB.accumulated(bw["dW"], 2, torch.float32), torch.float32, f"{dtype} gconv dW (second backward)", l2_tol=float("inf"))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_weight_gradient_is_bit_reproducible(dtype):
    a = run_device("many_pixel_tiles", dtype, True)
    b = run_device("many_pixel_tiles", dtype, True)
    assert torch.equal(a["dw"], b["dw"]) and torch.equal(a["dx"], b["dx"]) and torch.equal(a["y"], b["y"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["many_pixel_tiles", "odd_sizes_stride2_cg8"])
def test_statistics_slab(name, dtype):
    """(sum, sum of squares) of the STORED outputs.  Bound per channel: M * 2^-23 * sum|y| (sum y^2 for the squares), the worst case of any fp32 summation
    order of M terms, computed from the stored y alone."""
    from simpledepthestimation_amd.hip import nn as NN
    out = run_device(name, dtype, True, stats=True)
    y = out["y"].double().flatten(0, 2)
    M = y.shape[0]
    got = out["stats"][:-NN.REDUCE_ROWS].double().sum(0)
    assert out["stats"].shape[1:] == (y.shape[1], 2) and out["stats"].shape[0] > NN.REDUCE_ROWS
    if name == "many_pixel_tiles":
        assert out["stats"].shape[0] - NN.REDUCE_ROWS > 1, "this case is meant to span several statistics rows"
    e1 = (got[:, 0] - y.sum(0)).abs()
    e2 = (got[:, 1] - (y * y).sum(0)).abs()
    b1 = M * 2.0 ** -23 * y.abs().sum(0)
    b2 = M * 2.0 ** -23 * (y * y).sum(0)
    print(f"  {name} {dtype}: sum err/bound {float((e1 / b1).max()):.2e}, squares err/bound {float((e2 / b2).max()):.2e}")
    assert (e1 <= b1).all() and (e2 <= b2).all()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["many_pixel_tiles", "odd_sizes_stride2_cg8"])
def test_conv_norm_matches_torch(name, dtype):
    """conv_norm(HipGroupedConv2d, HipBatchNorm2d, x) in training mode against torch's relu(bn(conv(x))) on the CPU, forward and backward.
    BatchNorm's operand is the STORED convolution output, so the reference rounds it to the storage type too (value only, gradient straight through), as
    it does x, w and gy: without that the bf16 reference's ReLU mask differs from any bf16 run's on the elements whose bn(y) lies within a rounding step of
    zero, and two CPU references that differ in nothing else are 1.4e-2 (dx), 1.7e-2 (dW) and 1.8e-2 (dbeta) apart on the many-tile case."""
    from simpledepthestimation_amd.layers.hip_modules import HipBatchNorm2d, HipGroupedConv2d, conv_norm
    B, H, W, C, G, stride = CASES[name]
    dt = DT[dtype]
    ref = reference(name, dtype)
    g = torch.Generator().manual_seed(5)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    conv_t, bn_t = nn.Conv2d(C, C, 3, stride, 1, groups=G, bias=False), nn.BatchNorm2d(C)
    with torch.no_grad():
        conv_t.weight.copy_(ref["w"]); bn_t.weight.copy_(gamma); bn_t.bias.copy_(beta)
    xr = ref["x"].clone().requires_grad_(True)
    y_t = conv_t(xr)
    out_t = F.relu(bn_t(y_t + (y_t.to(dt).float() - y_t).detach()))
    out_t.backward(ref["gy"])
    conv_d, bn_d = HipGroupedConv2d(C, G, stride).to(dev), HipBatchNorm2d(C).to(dev)
    with torch.no_grad():
        conv_d.weight.copy_(ref["w"]); bn_d.weight.copy_(gamma); bn_d.bias.copy_(beta)
    xd = nhwc(ref["x"], dt).requires_grad_(True)
    out_d = conv_norm(conv_d, bn_d, xd)
    out_d.backward(nhwc(ref["gy"], dt))
    torch.cuda.synchronize()
    lim = 6e-3 if dt == torch.bfloat16 else 1e-3
    glim = 1.5 * lim if dt == torch.bfloat16 else lim
    errs = {"out": rel(out_d.detach().cpu().float().permute(0, 3, 1, 2), out_t.detach()), "dx": rel(xd.grad.cpu().float().permute(0, 3, 1, 2), xr.grad),
            "dW": rel(conv_d.weight.grad.cpu(), conv_t.weight.grad), "dgamma": rel(bn_d.weight.grad.cpu(), bn_t.weight.grad),
            "dbeta": rel(bn_d.bias.grad.cpu(), bn_t.bias.grad), "running_var": rel(bn_d.running_var.cpu(), bn_t.running_var)}
    print("  " + name, dtype, " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["out"] < lim and errs["running_var"] < lim
    for k in ("dx", "dW", "dgamma", "dbeta"):
        assert errs[k] < glim, f"{k}: relative L2 error {errs[k]:.3e}"


def test_unsupported_arguments_raise():
    from simpledepthestimation_amd.hip import nn as NN
    from simpledepthestimation_amd.hip.lib import SdeHipError
    x = torch.zeros(1, 2, 2, 32, device=dev)
    with pytest.raises(SdeHipError, match="fp32 or bf16"):
        NN.grouped_conv3x3(x.half(), torch.zeros(32, 8, 3, 3, device=dev), 4)
    with pytest.raises(SdeHipError, match="3x3"):
        NN.grouped_conv3x3(x, torch.zeros(32, 8, 5, 5, device=dev), 4)
    with pytest.raises(SdeHipError, match=r"channels per group in \(4, 8, 16, 32, 64\)"):
        NN.grouped_conv3x3(x, torch.zeros(32, 2, 3, 3, device=dev), 16)
    with pytest.raises(SdeHipError, match="channel mismatch"):
        NN.grouped_conv3x3(x, torch.zeros(64, 8, 3, 3, device=dev), 8)
    # ... and the C entry points themselves, before any launch
    lib = NN.L.lib()
    assert lib.sde_gconv3x3_stats_rows(1, 2, 2, 32, 16, 1, NN.L.BF16) == -1 and b"not supported" in lib.sde_last_error()
    assert lib.sde_gconv3x3_fwd(NN.L.ptr(x), NN.L.ptr(x), 0, 1, 2, 2, 32, 4, 3, NN.L.F32, NN.L.ptr(x), None, NN.L.stream()) < 0
    assert lib.sde_gconv3x3_wgrad_ws_bytes(1, 2, 2, 32, 4, 1, NN.L.F16) == 0

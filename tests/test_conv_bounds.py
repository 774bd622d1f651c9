"""CPU self-test of tests/conv_bounds.py: an honest fp32 convolution stays inside the per-element bounds, seeded kernel-bug lookalikes do not.

Each storage dtype is emulated on the CPU: fp32 F.conv2d (autograd for the gradients) on operands rounded to the dtype, the result rounded to the
dtype."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import conv_bounds as CB

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "fp16"]
SHAPES = {"2x96x160_64_128": (2, 96, 160, 64, 128), "2x24x40_64_64": (2, 24, 40, 64, 64), "1x6x10_2048_64": (1, 6, 10, 2048, 64)}


def old_check(a, b, dtype, name, f32_tol=2e-5, bf16_tol=1.5e-2):
    """test_gpu_nn.check() as it stood before the per-element bound (relative L2 + max-abs against 50 tol of the largest value)."""
    e = ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()
    tol = f32_tol if dtype == torch.float32 else bf16_tol
    assert e < tol, f"{name}: relative L2 error {e:.3e} > {tol}"
    mx = (a.double() - b.double()).abs().max().item()
    scale = b.abs().max().item() + 1e-30
    assert mx / scale < tol * 50, f"{name}: max abs error {mx:.3e} (scale {scale:.3e})"


@functools.lru_cache(maxsize=None)
def forward_case(shape, dtype, reflect=False):
    """(ConvCase, emulated output, operands) of a 3x3 stride-1 layer; computed once per (shape, dtype, padding) and left unchanged."""
    B, H, W, Cin, Cout = SHAPES[shape]
    g = torch.Generator().manual_seed(Cin + Cout + H)
    x = CB.rounded(torch.randn(B, Cin, H, W, generator=g), dtype)
    w = CB.rounded(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9), dtype)
    case = CB.ConvCase(x, w, None, dtype, stride=1, pad=1, reflect=reflect)
    xin = F.pad(x, (1, 1, 1, 1), mode="reflect") if reflect else x
    y = F.conv2d(xin, w, None, 1, 0 if reflect else 1).to(dtype).float()
    return case, y, (x, w)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_emulated_forward_is_inside_the_bound(shape, dtype):
    case, y, _ = forward_case(shape, dtype)
    worst = CB.assert_within(y, case.y, dtype, f"y {shape}")
    print(f"{shape} {CB.DT_NAME[dtype]}: worst error / limit {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["zero_bias", "refl_elu_two_consumers", "upcat_refl_elu", "s2_zero"])
def test_emulated_layer_with_gradients_is_inside_the_bounds(kind, dtype):
    """Every output of ConvCase (y, dX, dSkip, dW, dbias) for the source kinds of the engine, small shapes: fp32 autograd on the rounded operands."""
    g = torch.Generator().manual_seed(len(kind))
    upcat, reflect, act = kind.startswith("upcat"), "refl" in kind, (1 if "elu" in kind else 0)
    stride = 2 if kind == "s2_zero" else 1
    B, H, W, C0, C1, Cout = 2, 7, 11, 24, (16 if upcat else 0), 20
    x0 = CB.rounded(torch.randn(B, C0, H, W, generator=g), dtype).requires_grad_(True)
    x1 = CB.rounded(torch.randn(B, C1, 2 * H, 2 * W, generator=g), dtype).requires_grad_(True) if C1 else None
    w = CB.rounded(torch.randn(Cout, C0 + C1, 3, 3, generator=g) / math.sqrt((C0 + C1) * 9), dtype).requires_grad_(True)
    b = (torch.randn(Cout, generator=g) * 0.1).requires_grad_(True)
    case = CB.ConvCase(x0.detach(), w.detach(), b.detach(), dtype, stride=stride, pad=1, reflect=reflect, act=act, x1=x1.detach() if C1 else None, upcat=upcat)
    xin = F.interpolate(x0, scale_factor=2, mode="nearest") if upcat else x0
    xin = torch.cat([xin, x1], 1) if C1 else xin
    xin = F.pad(xin, (1, 1, 1, 1), mode="reflect") if reflect else xin
    y = F.conv2d(xin, w, b, stride, 0 if reflect else 1)
    y = F.elu(y) if act else y
    gys = [CB.rounded(torch.randn(y.shape, generator=g), dtype) for _ in range(2 if "two" in kind else 1)]
    y.backward(sum(gys))
    CB.assert_within(y.detach().to(dtype).float(), case.y, dtype, "y")
    bounds = case.backward(gys)
    assert set(bounds) == {"dX", "dW", "dbias"} | ({"dSkip"} if C1 else set())
    CB.assert_within(x0.grad.to(dtype).float(), bounds["dX"], dtype, "dX")
    if C1:
        CB.assert_within(x1.grad.to(dtype).float(), bounds["dSkip"], dtype, "dSkip")
    CB.assert_within(w.grad, bounds["dW"], torch.float32, "dW")
    CB.assert_within(b.grad, bounds["dbias"], torch.float32, "dbias")
    # and the bound is not vacuous: the limits are a small fraction of the typical magnitude
    for k, bd in bounds.items():
        assert float(bd.lim.median()) < (0.1 if act else 0.02) * float(bd.ref.abs().median() + bd.ref.abs().mean()), k


def test_seeded_corruptions_are_rejected():
    """Three kernel-bug lookalikes in the bf16 output of 2 x 96 x 160, 64 -> 128 (test_gpu_nn's 3x3_bigM_64_128), each rejected by assert_within:
      1. one output pixel (all 128 channels) swapped with its neighbour,
      2. one corner of the last, ragged 64-row tile zeroed (4 pixels x 4 channels),
      3. one reflected border column computed with zero padding instead.
    The regression this module exists for: check() of test_gpu_nn.py as it stood (relative L2 < 1.5e-2, max-abs < 0.75 of the largest value; kept
    above as old_check) ACCEPTS the first corruption, and the second -- it is asserted here, so putting the old check back in place of the bound
    makes them pass again.  One element off by four unit roundoffs (y * (1 + 4 * 2^-8)) passes the old check as well and fails the bound.  (A whole
    border column of every image and row is 1 / 160 of the tensor: relative L2 4.6e-2, which the old check does see.)"""
    dtype = torch.bfloat16
    case, y, _ = forward_case("2x96x160_64_128", dtype)
    CB.assert_within(y, case.y, dtype, "clean")

    def rejected(bad, bound, what, old_accepts=True):
        if old_accepts:
            old_check(bad, bound.ref, dtype, what)                  # the old assertion lets it through ...
        with pytest.raises(AssertionError, match="exceed the per-element bound"):
            CB.assert_within(bad, bound, dtype, what)               # ... the bound does not

    # (a typical pixel pair: the one of row 50 whose largest channel difference is the median of the row's -- a pair with an outlier channel
    # above 0.75 of the tensor's maximum would trip the old max-abs line)
    diff = (y[1, :, 50, 1:] - y[1, :, 50, :-1]).abs().amax(0)
    c = int(diff.argsort()[diff.numel() // 2])
    swap = y.clone()
    swap[1, :, 50, c], swap[1, :, 50, c + 1] = y[1, :, 50, c + 1], y[1, :, 50, c]
    rejected(swap, case.y, "pixel swapped with its neighbour")
    corner = y.clone()
    corner[1, -4:, -1, -4:] = 0          # NCHW view of the last 4 rows x last 4 columns of the [M, Cout] GEMM
    rejected(corner, case.y, "ragged-tile corner zeroed")
    one = y.clone()
    i = (0, 5, 17, 33)
    assert abs(float(y[i])) > 0.05
    one[i] = y[i] * (1 + 4 * 2.0 ** -8)
    rejected(one, case.y, "one element off by four unit roundoffs")
    rcase, ry, (x, w) = forward_case("2x96x160_64_128", dtype, True)
    CB.assert_within(ry, rcase.y, dtype, "clean (reflect)")
    col = ry.clone()
    col[:, :, :, 0] = F.conv2d(x, w, None, 1, 1).to(dtype).float()[:, :, :, 0]
    rejected(col, rcase.y, "reflected border column computed with zero padding", old_accepts=False)


def test_failure_message_names_count_index_error_and_limit():
    case, y, _ = forward_case("2x24x40_64_64", torch.float16)
    bad = y.clone()
    bad[1, 3, 5, 7] += 0.25
    bad[0, 0, 0, 0] += 0.002
    with pytest.raises(AssertionError) as ei:
        CB.assert_within(bad, case.y, torch.float16, "y")
    msg = str(ei.value)
    assert "2 of 122880 elements" in msg and "worst at (1, 3, 5, 7)" in msg and "error 2.5" in msg and "limit" in msg
    nan = y.clone()
    nan[0, 1, 2, 3] = float("nan")
    with pytest.raises(AssertionError, match="1 of 122880"):
        CB.assert_within(nan, case.y, torch.float16, "y")


def test_two_kernel_limit():
    """|a - b| <= lim_a + lim_b: two different fp32 summation orders of the same operands pass, a one-pixel difference does not; an extra limit
    (`also`) can only tighten it."""
    dtype = torch.bfloat16
    case, y, (x, w) = forward_case("2x24x40_64_64", dtype)
    parts = [F.conv2d(x[:, c:c + 16], w[:, c:c + 16], None, 1, 1) for c in (48, 0, 32, 16)]      # split-K in another order
    y2 = sum(parts).to(dtype).float()
    assert not torch.equal(y2, y)
    CB.assert_two_kernels(y, y2, case.y, dtype, "two orders")
    CB.assert_two_kernels(y, y2, case.y, dtype, "two orders", also=2.0 ** -7 * torch.maximum(y.abs(), y2.abs()) + 2e-3)
    y3 = y2.clone()
    y3[0, :, 3, 4] = y2[0, :, 3, 5]
    with pytest.raises(AssertionError, match="differ by more than"):
        CB.assert_two_kernels(y, y3, case.y, dtype, "pixel")
    with pytest.raises(AssertionError):
        CB.assert_two_kernels(y, y2, case.y, dtype, "tightened", also=torch.zeros_like(y))

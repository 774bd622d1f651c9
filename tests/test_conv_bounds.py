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


# ---------------------------------------------------------------------------------------------------------------------------------------
# The convolutions outside the engine: grouped 3x3, transposed 3x3 stride 2, dilated 3x3, Conv3d(1 -> 8) pack.  The cases are the GPU tests' own (their
# cached references: operands rounded to the storage type, an fp32 CPU result, the fp64 bounds), here also in fp16.
# ---------------------------------------------------------------------------------------------------------------------------------------
import test_gpu_bts as TB          # noqa: E402  (importable without a GPU: the device is touched inside the tests only)
import test_gpu_deconv as TD       # noqa: E402
import test_gpu_gconv as TG        # noqa: E402
import test_gpu_nn as TN           # noqa: E402

NAMES = ["fp32", "bf16", "fp16"]
DILATED = [(d, (2, 5, 7, 37, 21)) for d in (1, 3, 6, 12, 18, 24)] + [(d, (2, 13, 19, 40, 24)) for d in (3, 6)]
CONV3D = [(2, 16, 5, 7), (1, 64, 9, 12), (2, 256, 3, 4), (2, 64, 40, 36), (1, 192, 47, 50), (3, 128, 26, 33)]


def not_vacuous(bounds, frac=0.02):
    for k, bd in bounds.items():
        assert float(bd.lim.median()) < frac * float(bd.ref.abs().median() + bd.ref.abs().mean()), k


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def old_rel_l2(a, b, dt, gradient, what):
    """The whole-tensor assertion of test_gpu_gconv.py and test_gpu_deconv.py: relative L2 against the fp32 CPU result, 6e-3 (gradients 9e-3) in 16
    bits, 1e-3 in fp32."""
    lim = 1e-3 if dt == torch.float32 else (9e-3 if gradient else 6e-3)
    assert rel(a, b) < lim, f"{what}: relative L2 error {rel(a, b):.3e}"


def old_max_abs(a, b, dt, what):
    """test_gpu_bts.py's: max-abs error over max-abs value < 2e-2 in 16 bits, 2e-5 in fp32."""
    e = float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-12))
    assert e < (2e-5 if dt == torch.float32 else 2e-2), f"{what}: {e:.3e}"


def rejected(bad, bound, dt, what, old, old_accepts=True):
    if old_accepts:
        old(bad)                                                      # the assertion the bound replaces lets it through ...
    else:
        with pytest.raises(AssertionError):
            old(bad)
    with pytest.raises(AssertionError, match="exceed the per-element bound"):
        CB.assert_within(bad, bound, dt, what, l2_tol=float("inf"))   # ... the bound does not


@pytest.mark.parametrize("dtype", NAMES)
@pytest.mark.parametrize("name", list(TG.CASES))
def test_emulated_grouped_conv_is_inside_the_bounds(name, dtype):
    dt, ref = TG.REF_DT[dtype], TG.reference(name, dtype)
    case, bw = TG.bounds(name, dtype)
    CB.assert_within(CB.rounded(ref["y"], dt), case.y, dt, "y")
    CB.assert_within(CB.rounded(ref["dx"], dt), bw["dX"], dt, "dX")
    CB.assert_within(ref["dw"], bw["dW"], torch.float32, "dW")
    # a second backward: two stored data gradients added in the storage type, two weight gradients in fp32
    dx = CB.rounded(ref["dx"], dt)
    CB.assert_within(CB.rounded(dx + dx, dt), CB.accumulated(bw["dX"], 2, dt), dt, "dX twice")
    CB.assert_within(ref["dw"] + ref["dw"], CB.accumulated(bw["dW"], 2, torch.float32), torch.float32, "dW twice")
    if ref["y"].numel() > 2048:          # (the 1x1 image's medians are those of a handful of border sums)
        not_vacuous({"y": case.y, **bw})


@pytest.mark.parametrize("dtype", NAMES)
@pytest.mark.parametrize("full", [True, False], ids=["bias_relu", "plain"])
@pytest.mark.parametrize("name", list(TD.CASES))
def test_emulated_conv_transpose_is_inside_the_bounds(name, full, dtype):
    """... and the condition on the ReLU masks: at most 0.1 % of a case's elements undecided by the fp64 reference."""
    dt, ref = TD.REF_DT[dtype], TD.reference(name, full, dtype)
    case, bw = TD.bounds(name, full, dtype)
    print(f"{name} {dtype}: {int(case.undecided.sum())} of {case.undecided.numel()} ReLU masks undecided")
    assert case.undecided_share <= 1e-3
    assert full or not case.undecided.any()
    CB.assert_within(CB.rounded(ref["y"], dt), case.y, dt, "y")
    CB.assert_within(CB.rounded(ref["dx"], dt), bw["dX"], dt, "dX")
    CB.assert_within(ref["dw"], bw["dW"], torch.float32, "dW")
    assert ("dbias" in bw) == full
    if full:
        CB.assert_within(ref["db"], bw["dbias"], torch.float32, "dbias")
        # the other admissible mask: every undecided element flipped, the gradients recomputed in fp32
        x, w, b = (ref[k].clone().requires_grad_(True) for k in ("x", "w", "bias"))
        pre = F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1)
        pre.backward(ref["gy"] * ((pre.detach() > 0) ^ case.undecided).float())
        CB.assert_within(CB.rounded(x.grad, dt), bw["dX"], dt, "dX, undecided masks flipped", l2_tol=float("inf"))
        CB.assert_within(w.grad, bw["dW"], torch.float32, "dW, undecided masks flipped", l2_tol=float("inf"))
        CB.assert_within(b.grad, bw["dbias"], torch.float32, "dbias, undecided masks flipped", l2_tol=float("inf"))
    if ref["y"].numel() > 2048:
        not_vacuous({"y": case.y, **bw}, 0.1 if full else 0.02)


@pytest.mark.parametrize("dtype", NAMES)
@pytest.mark.parametrize("d,shape", DILATED)
def test_emulated_dilated_conv_is_inside_the_bounds(d, shape, dtype):
    dt, ref = TB.REF_DT[dtype], TB.dilated_reference(dtype, d, shape)
    x, w = ref["x"].clone().requires_grad_(True), ref["w"].clone().requires_grad_(True)
    y = F.conv2d(x, w, padding=d, dilation=d)
    y.backward(ref["gy"])
    CB.assert_within(CB.rounded(y.detach(), dt), ref["case"].y, dt, "y")
    CB.assert_within(CB.rounded(x.grad, dt), ref["bw"]["dX"], dt, "dX")
    CB.assert_within(w.grad, ref["bw"]["dW"], torch.float32, "dW")
    if d < min(shape[1:3]):              # (a dilation past the image leaves the centre tap alone: sums of Cin terms)
        not_vacuous({"y": ref["case"].y, **ref["bw"]})


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", CONV3D, ids=["x".join(map(str, s)) for s in CONV3D])
def test_emulated_conv3d_pack_is_inside_the_bounds(shape, dtype):
    ref = TN.conv3d_reference(dtype, *shape)
    case, bw = ref["case"], ref["bw"]
    CB.assert_within(CB.rounded(ref["o"], dtype), case.y, dtype, "y")
    CB.assert_within(CB.rounded(ref["dx"], dtype), bw["dX"], dtype, "dX")
    CB.assert_within(ref["dw"], bw["dW"], torch.float32, "dW")
    CB.assert_within(ref["db"], bw["dbias"], torch.float32, "dbias")
    not_vacuous({"y": case.y, "dX": bw["dX"]})
    # dW and dbias sum K = B D H W terms.  The worst case of an fp32 sum grows like K * 2^-24 * K E|a b|, the sum itself like sqrt(K): their ratio,
    # about 0.64 K^1.5 2^-24, passes 1 % near K = 4096.  Beyond that the bound still holds but says little, and test_gpu_nn.py's relative-L2 line
    # (2e-5) is the one that binds.
    B, D, H, W = shape
    if B * D * H * W <= 4096:
        not_vacuous({"dW": bw["dW"], "dbias": bw["dbias"]})


def typical(t):
    """flat index of the element of median magnitude"""
    return int(t.abs().flatten().argsort()[t.numel() // 2])


def test_grouped_weight_gradient_entry_off_by_half_is_rejected():
    """resnext50_layer1_cg4 (C = 128, G = 32: 4608 weight-gradient entries), bf16: one entry of typical size off by half its value moves the relative
    L2 error by about 0.5 / sqrt(4608); test_gpu_gconv.py's 9e-3 -- its only assertion on a bf16 weight gradient -- accepts that."""
    dt = torch.bfloat16
    ref, (case, bw) = TG.reference("resnext50_layer1_cg4", "bf16"), TG.bounds("resnext50_layer1_cg4", "bf16")
    assert ref["dw"].numel() == 4608
    bad = ref["dw"].clone()
    bad.view(-1)[typical(bad)] *= 1.5
    rejected(bad, bw["dW"], torch.float32, "dW entry off by half", lambda t: old_rel_l2(t, ref["dw"], dt, True, "dW"))


def test_grouped_stride2_parity_block_shifted_is_rejected():
    """cg32_even_sizes_stride2, bf16: the first 16-pixel block of the data gradient's (even row, even column) parity class takes each pixel from the
    next one of the class.  16 of the 120 pixels: relative L2 0.5, which the old assertion sees as well (old_accepts=False) -- at a shape where
    it would not, 16 pixels in 400 000, the fp64 reference no longer fits a test of a few seconds."""
    dt = torch.bfloat16
    ref, (case, bw) = TG.reference("cg32_even_sizes_stride2", "bf16"), TG.bounds("cg32_even_sizes_stride2", "bf16")
    dx = CB.rounded(ref["dx"], dt)
    B, C, H, W = dx.shape
    cls = [(b, i, j) for b in range(B) for i in range(0, H, 2) for j in range(0, W, 2)]
    bad = dx.clone()
    for (b, i, j), (b1, i1, j1) in zip(cls[:16], cls[1:17]):
        bad[b, :, i, j] = dx[b1, :, i1, j1]
    rejected(bad, bw["dX"], dt, "parity block shifted", lambda t: old_rel_l2(t, ref["dx"], dt, True, "dX"), old_accepts=False)


def test_conv_transpose_neighbour_tap_dropped_at_the_tile_column_is_rejected():
    """second_tile_column_one_pixel_wide (W = 17), bf16, plain: output column 2 * 15 + 1 computed without its x[i, 16] tap, the halo column of the first
    8 x 16 tile.  One output column in 34: relative L2 0.1, so the old assertion rejects it too (old_accepts=False); what it lacked was a case
    with W > 16 -- every earlier case fits one tile column."""
    dt = torch.bfloat16
    name = "second_tile_column_one_pixel_wide"
    ref, (case, bw) = TD.reference(name, False, "bf16"), TD.bounds(name, False, "bf16")
    assert all(c[2] <= 10 for n, c in TD.CASES.items() if n not in ("second_tile_column_one_pixel_wide", "exact_tile_halo_out_of_range", "three_tile_columns_ragged_channels"))
    x0 = ref["x"].clone()
    x0[..., 16] = 0
    bad = CB.rounded(ref["y"], dt)
    bad[..., 31] = CB.rounded(F.conv_transpose2d(x0, ref["w"], None, stride=2, padding=1, output_padding=1), dt)[..., 31]
    rejected(bad, case.y, dt, "halo tap dropped", lambda t: old_rel_l2(t, ref["y"], dt, False, "y"), old_accepts=False)


def test_dilated_partial_subgrid_row_dropped_is_rejected():
    """small_odd (H = 5), d = 3, bf16: the sub-grids' second row exists for two of the three row residues only (rows 3 and 4); a merge that sizes the
    sub-grids by H // d leaves those output rows zero.  test_gpu_bts.py's max-abs line sees zeroed rows (old_accepts=False).  What that line does
    let through, and the bound does not: one element off by 1.5 % of the tensor's largest value."""
    dt = torch.bfloat16
    ref = TB.dilated_reference("bf16", 3, (2, 5, 7, 37, 21))
    y = CB.rounded(ref["y"].float(), dt)
    CB.assert_within(y, ref["case"].y, dt, "clean")
    old = lambda t: old_max_abs(t, ref["y"], dt, "y")
    bad = y.clone()
    bad[:, :, 3:, :] = 0
    rejected(bad, ref["case"].y, dt, "partial sub-grid row dropped", old, old_accepts=False)
    one = y.clone()
    one.view(-1)[typical(y)] += 0.015 * float(y.abs().max())
    rejected(one, ref["case"].y, dt, "one element off by 1.5 % of the maximum", old)


def test_conv3d_channel_group_boundary_element_is_rejected():
    """1 x 64 x 9 x 12, bf16: the first element of a 16-byte channel group (channel 8 of feature 3) taken from its neighbour in the previous group
    (channel 7) at one pixel -- the pixel where that changes the value by the median amount.  check() of test_gpu_nn.py without a bound
    (old_check above) accepts it: one element in 55 296."""
    dt = torch.bfloat16
    ref = TN.conv3d_reference(dt, 1, 64, 9, 12)
    y = CB.rounded(ref["o"], dt)
    ch = 3 * 64 + 8
    diff = (y[0, ch] - y[0, ch - 1]).abs()
    i, j = divmod(typical(diff), diff.shape[1])
    assert float(diff[i, j]) > 0
    bad = y.clone()
    bad[0, ch, i, j] = y[0, ch - 1, i, j]
    rejected(bad, ref["case"].y, dt, "group boundary element", lambda t: old_check(t, ref["o"], dt, "conv3d out"))

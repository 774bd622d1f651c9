"""GPU parity of the transposed-convolution operator (csrc/deconv.hip, hip.nn.conv_transpose2d): ConvTranspose2d(3, stride 2, padding 1,
output_padding 1) [+ bias + ReLU], GoogleResNetv2's up-sampling layer (GoogleResNetv2.py:L42-44, L127-138).

Forward and every gradient are compared with
  * F.conv_transpose2d on the CPU in fp32 from the 16-bit-rounded operands, as tests/test_gpu_conv_small.py does (relative L2: 6e-3 for y and 1.5 x
    that for gradients in bf16 = 16-bit output rounding; 1e-3 in fp32), and
  * the zero-insertion route through the convolution engine on the same device buffers (hip.nn.DECONV_DIRECT = False): fp32 accumulation both, so
    at most one 16-bit ulp apart (close16 of that file); in fp32 2e-5 of the maximum (the TOL of tests/test_gpu_google_resnet.py), and
  * element by element, an fp64 reference with the a-priori limits of tests/conv_bounds.py (DeconvCase): y, dX, dW and dbias of both routes, and
    the two routes against each other.  tests/test_conv_bounds.py checks on the CPU that at most 0.1 % of any case's ReLU masks are undecided.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import conv_bounds as CB

pytestmark = pytest.mark.gpu
dev = "cuda"

CASES = {  # name: (B, H, W, Cin, Cout)
    "1x1_every_neighbour_out_of_range": (1, 1, 1, 16, 16),
    "odd_sizes_halo_on_both_edges": (2, 3, 5, 64, 32),
    "ragged_tiles_narrow_output": (3, 13, 9, 32, 16),
    "small_even_map": (2, 4, 4, 128, 64),
    "long_k": (2, 6, 10, 512, 256),
    "ragged_channel_tiles": (2, 5, 7, 40, 24),
    "padded_channels_on_both_sides": (2, 5, 7, 20, 12),        # bf16: 24 stored input channels, 16 stored output channels (4 exact zeros)
    # the kernel's 8 x 16 pixel tile crossed both ways
    "second_tile_column_one_pixel_wide": (1, 9, 17, 16, 16),   # ... and the first tile's halo column read from the neighbour tile
    "exact_tile_halo_out_of_range": (2, 8, 16, 24, 12),
    "three_tile_columns_ragged_channels": (1, 17, 33, 40, 24),
}
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
REF_DT = dict(DT, fp16=torch.float16)       # the references also in fp16, for the CPU self-test of their bounds (tests/test_conv_bounds.py)
# conv_bounds.DeconvCase cannot decide the ReLU mask of an element whose fp64 pre-activation lies within its own limit of zero, and at most 0.1 % of a
# case's elements may be like that.  With K = 9 * 512 + 1 the limit near zero is about 5e-3 against pre-activations of unit variance: zero-mean
# operands leave 0.4 % of long_k undecided whatever the seed (every other case: <= 0.06 %).  Its bias is therefore drawn away from zero, |bias| >= 2:
# 0.05 %, and all but the channels with the largest |bias| keep pixels on both sides of the ReLU.
BIAS_AWAY = {"long_k": 2.0}


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
def reference(name, full, dtype):
    """Operands (rounded to the storage type) and the CPU fp32 result: computed once per case, shared by the tests, never modified."""
    B, H, W, Cin, Cout = CASES[name]
    dt = REF_DT[dtype]
    g = torch.Generator().manual_seed(len(name) * 13 + B + 7 * full)
    x = torch.randn(B, Cin, H, W, generator=g).to(dt).float()
    w = (torch.randn(Cin, Cout, 3, 3, generator=g) / math.sqrt(Cin * 2.25)).to(dt).float()
    bias = torch.randn(Cout, generator=g) * 0.3 if full else None
    if full and name in BIAS_AWAY:
        bias = bias + BIAS_AWAY[name] * torch.sign(bias)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = bias.clone().requires_grad_(True) if full else None
    y = F.conv_transpose2d(xr, wr, br, stride=2, padding=1, output_padding=1)
    if full:
        y = F.relu(y)
    gy = torch.randn(y.shape, generator=g).to(dt).float()
    y.backward(gy)
    return dict(x=x, w=w, bias=bias, gy=gy, y=y.detach(), dx=xr.grad, dw=wr.grad, db=br.grad if full else None)


@functools.lru_cache(maxsize=None)
def bounds(name, full, dtype):
    """(DeconvCase, its gradient bounds) of reference(name, full, dtype): fp64, computed once per case."""
    ref = reference(name, full, dtype)
    case = CB.DeconvCase(ref["x"], ref["w"], ref["bias"], REF_DT[dtype], act=CB.ACT_RELU if full else CB.ACT_NONE)
    return case, case.backward(ref["gy"])


def nchw(t, C):
    return t[..., :C].float().permute(0, 3, 1, 2)


def nhwc(t, dt):
    """NCHW fp32 -> NHWC `dt` on the device, channels zero-padded to the 16-byte group."""
    V = 4 if dt == torch.float32 else 8
    t = t.permute(0, 2, 3, 1)
    return F.pad(t, (0, -t.shape[3] % V)).contiguous().to(dt).to(dev)


def run_device(ref, dt, full, direct, backwards=1):
    from simpledepthestimation_amd.hip import nn as NN
    old = NN.DECONV_DIRECT, NN.DECONV_RULE
    NN.DECONV_DIRECT, NN.DECONV_RULE = direct, False          # (rule off: `direct` runs the kernel on every case, the long-K one included)
    try:
        xd = nhwc(ref["x"], dt).requires_grad_(True)
        wd = ref["w"].clone().to(dev).requires_grad_(True)
        bd = ref["bias"].clone().to(dev).requires_grad_(True) if full else None
        gyd = nhwc(ref["gy"], dt)
        for _ in range(backwards):
            y = NN.conv_transpose2d(xd, wd, bd, act=NN.ACT_RELU if full else NN.ACT_NONE)
            y.backward(gyd)
        torch.cuda.synchronize()
    finally:
        NN.DECONV_DIRECT, NN.DECONV_RULE = old
    return dict(y=y.detach().cpu(), dx=xd.grad.cpu(), dw=wd.grad.cpu(), db=bd.grad.cpu() if full else None)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("full", [True, False], ids=["bias_relu", "plain"])
@pytest.mark.parametrize("name", list(CASES))
def test_conv_transpose2d(name, full, dtype):
    B, H, W, Cin, Cout = CASES[name]
    dt = DT[dtype]
    ref = reference(name, full, dtype)
    on = run_device(ref, dt, full, True)
    off = run_device(ref, dt, full, False)
    lim = 6e-3 if dt == torch.bfloat16 else 1e-3
    glim = 1.5 * lim if dt == torch.bfloat16 else lim
    y = on["y"]
    assert tuple(y.shape[:3]) == (B, 2 * H, 2 * W) and y.shape[3] >= Cout and y.dtype == dt
    if y.shape[3] > Cout:
        assert (y[..., Cout:] == 0).all() and (off["y"][..., Cout:] == 0).all(), "padded output channels must be exact zeros"
    errs = {"y": rel(y[..., :Cout].float().permute(0, 3, 1, 2), ref["y"]), "dx": rel(on["dx"][..., :Cin].float().permute(0, 3, 1, 2), ref["dx"]),
            "dW": rel(on["dw"], ref["dw"])}
    if full:
        errs["dbias"] = rel(on["db"], ref["db"])
    print("  " + name, dtype, " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["y"] < lim, f"y vs fp32 CPU: relative L2 error {errs['y']:.3e}"
    for k in ("dx", "dW", "dbias"):
        assert errs.get(k, 0.0) < glim, f"{k} vs fp32 CPU: relative L2 error {errs[k]:.3e}"
    if on["dx"].shape[3] > Cin:
        assert (on["dx"][..., Cin:] == 0).all(), "padded input-gradient channels must be exact zeros"
    # every element of both routes against the fp64 reference, and the two routes against each other (the relative-L2 lines are the ones above)
    case, bw = bounds(name, full, dtype)
    for route, out in (("kernel", on), ("zero insertion", off)):
        CB.assert_within(nchw(out["y"], Cout), case.y, dt, f"{dtype} deconv y ({route})", l2_tol=float("inf"))
        CB.assert_within(nchw(out["dx"], Cin), bw["dX"], dt, f"{dtype} deconv dX ({route})", l2_tol=float("inf"))
        CB.assert_within(out["dw"], bw["dW"], torch.float32, f"{dtype} deconv dW ({route})", l2_tol=float("inf"))
        if full:
            CB.assert_within(out["db"], bw["dbias"], torch.float32, f"{dtype} deconv dbias ({route})", l2_tol=float("inf"))
    CB.assert_two_kernels(nchw(on["y"], Cout), nchw(off["y"], Cout), case.y, dt, f"{dtype} deconv y (kernel vs zero insertion)")
    CB.assert_two_kernels(nchw(on["dx"], Cin), nchw(off["dx"], Cin), bw["dX"], dt, f"{dtype} deconv dX (kernel vs zero insertion)")
    CB.assert_two_kernels(on["dw"], off["dw"], bw["dW"], torch.float32, f"{dtype} deconv dW (kernel vs zero insertion)")
    if full:
        CB.assert_two_kernels(on["db"], off["db"], bw["dbias"], torch.float32, f"{dtype} deconv dbias (kernel vs zero insertion)")
    # the parity-split kernel against the zero-insertion route on the same buffers
    if dt == torch.bfloat16:
        close16(y, off["y"], dt, "y (direct vs zero insertion)")
        close16(on["dx"], off["dx"], dt, "dx")
    else:
        for k in ("y", "dx", "dw"):
            e = float((on[k].double() - off[k].double()).abs().max() / off[k].double().abs().max())
            assert e <= 2e-5, f"{k}: direct vs zero insertion {e:.2e}"


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["odd_sizes_halo_on_both_edges", "padded_channels_on_both_sides"])
def test_second_backward_accumulates_into_existing_grads(name, dtype):
    """The first backward returns fresh gradients; from then on the parameters own fp32 .grad tensors and the kernels add into them in place."""
    dt = DT[dtype]
    ref = reference(name, True, dtype)
    Cin = CASES[name][3]
    two = run_device(ref, dt, True, True, backwards=2)
    glim = 1.5 * 6e-3 if dt == torch.bfloat16 else 1e-3
    assert rel(two["dw"], 2 * ref["dw"]) < glim and rel(two["db"], 2 * ref["db"]) < glim
    assert rel(two["dx"][..., :Cin].float().permute(0, 3, 1, 2), 2 * ref["dx"]) < glim
    # element by element: two gradients, each within its bound, and the rounding of their stored sum (dX: autograd's add in the activation dtype; dW and
    # dbias: the kernels' add into the fp32 slot)
    case, bw = bounds(name, True, dtype)
    INF = float("inf")
    CB.assert_within(nchw(two["dx"], Cin), CB.accumulated(bw["dX"], 2, dt), dt, f"{dtype} deconv dX (second backward)", l2_tol=INF)
    CB.assert_within(two["dw"], CB.accumulated(bw["dW"], 2, torch.float32), torch.float32, f"{dtype} deconv dW (second backward)", l2_tol=INF)
    CB.assert_within(two["db"], CB.accumulated(bw["dbias"], 2, torch.float32), torch.float32, f"{dtype} deconv dbias (second backward)", l2_tol=INF)


def test_unsupported_arguments_raise():
    from simpledepthestimation_amd.hip import nn as NN
    from simpledepthestimation_amd.hip.lib import SdeHipError
    x = torch.zeros(1, 2, 2, 16, device=dev)
    with pytest.raises(SdeHipError, match="3x3"):
        NN.conv_transpose2d(x, torch.zeros(16, 16, 4, 4, device=dev))
    with pytest.raises(SdeHipError, match="fp32 or bf16"):
        NN.conv_transpose2d(x.half(), torch.zeros(16, 16, 3, 3, device=dev))
    with pytest.raises(SdeHipError, match="input channels"):
        NN.conv_transpose2d(x, torch.zeros(32, 16, 3, 3, device=dev))

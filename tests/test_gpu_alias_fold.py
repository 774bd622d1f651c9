"""GPU: an operator with more consumers than its backward kernel has gradient slots (hip.nn.fan_in folds the surplus into the last slot with torch adds).

No network of the package reaches this path (their largest n_out is 3, the norm kernels take 3 gradients; convolution, max-pool 2 and at most 2 aliases),
so it is driven here directly.  Every alias receives a gradient of small integers (|v| <= 4): all partial sums are then exact in fp32 and in bf16, in
any order, and the gradients must EQUAL those of the same operator with one output fed the pre-summed gradient."""
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])


def _ints(g, shape, dtype):
    return torch.randint(-4, 5, shape, generator=g).to(dtype).to(dev)


def _leaf(g, shape, dtype=torch.float32):
    return torch.randn(shape, generator=g).to(dtype).to(dev).requires_grad_(True)


def _folded_equals_presummed(op, leaves, n_out, g, dtype):
    """op(n_out) -> output alias(es) over `leaves`; the gradients of the leaves with n_out aliases fed douts[k] against one output fed sum(douts)."""
    outs = op(n_out)
    assert len(outs) == n_out and all(t.data_ptr() == outs[0].data_ptr() for t in outs)
    douts = [_ints(g, outs[0].shape, dtype) for _ in range(n_out)]
    folded = torch.autograd.grad(outs, leaves, douts)
    total = douts[0]
    for d in douts[1:]:
        total = total + d
    single = torch.autograd.grad([op(1)], leaves, [total])
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(folded, single)):
        assert torch.isfinite(b).all() and b.abs().sum() > 0, k
        assert torch.equal(a, b), (k, (a.float() - b.float()).abs().max().item())


@DTYPES
@pytest.mark.parametrize("norm", ["BN", "randLN"])
def test_norm_with_four_consumers(norm, dtype):
    from simpledepthestimation_amd.hip import google as HG
    from simpledepthestimation_amd.hip import nn as NN
    g = torch.Generator().manual_seed(11)
    B, H, W, C = 2, 4, 6, 16                                   # 16 channels: BatchNorm's fused hand-overs (C % 64 == 0) stay out of it
    x = torch.randn(B, H, W, C, generator=g).to(dtype).to(dev)
    w = (torch.randn(C, C, 1, 1, generator=g) / 4).to(dev)
    y, stats = NN.conv2d(x, w, None, bn_stats=True)             # BatchNorm reads its statistics from the producing convolution's slab
    y = y.detach().requires_grad_(True)
    gamma, beta, res = _leaf(g, (C,)), _leaf(g, (C,)), _leaf(g, (B, H, W, C), dtype)
    z = torch.randn(2, B, C, generator=g).to(dev)
    stddev = torch.full((1,), 0.5, device=dev)

    def op(n):
        if norm == "BN":
            return NN.batch_norm_act(y, stats, gamma, beta, torch.zeros(C, device=dev), torch.ones(C, device=dev), residual=res, relu=True, n_out=n)
        return HG.rand_layer_norm(y, gamma, beta, z, stddev, residual=res, relu=True, n_out=n)
    _folded_equals_presummed(op, [y, gamma, beta, res], 4, g, dtype)        # dx, dgamma, dbeta, dres


@DTYPES
def test_max_pool_with_three_consumers(dtype):
    from simpledepthestimation_amd.hip import nn as NN
    g = torch.Generator().manual_seed(12)
    x = _leaf(g, (1, 5, 7, 8), dtype)
    _folded_equals_presummed(lambda n: NN.max_pool_3x3_s2(x, n_out=n), [x], 3, g, dtype)


@DTYPES
def test_conv_with_three_consumers(dtype):
    from simpledepthestimation_amd.hip import nn as NN
    g = torch.Generator().manual_seed(13)
    x = _leaf(g, (1, 6, 6, 8), dtype)
    w, b = _leaf(g, (8, 8, 3, 3)), _leaf(g, (8,))
    _folded_equals_presummed(lambda n: NN.conv2d(x, w, b, stride=1, pad=1, n_out=n), [x, w, b], 3, g, dtype)     # dx, weight and bias gradients

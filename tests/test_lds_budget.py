"""LDS budget of the kernels that share a compute unit during the backward pass ("co-residency").

The data-gradient chain runs on one queue, the weight gradients on a second one beside it.  A compute unit has 160 KiB of LDS; a workgroup of the persistent
GEMM (the chain's main kernel) takes 49 920 B and the chain needs at least two of them per compute unit to run near its stand-alone speed (three fit
when nothing else is resident).  So every side-queue kernel that can run beside the persistent GEMM must leave room for two of its workgroups:
LDS(side kernel) + 2 x LDS(pgemm) <= 160 KiB.  sde_kernel_lds_bytes is a host-only query: no GPU needed.
"""
import pytest

CU_LDS = 160 * 1024


@pytest.fixture(scope="module")
def NN():
    from simpledepthestimation_amd.hip import nn, lib as L
    if not L.available():
        pytest.fail("libsde_hip.so is not built")
    return nn


def test_pgemm_ring_is_what_the_budget_assumes(NN):
    assert NN.kernel_lds_bytes(NN.KERNEL_PGEMM, 3) == 3 * (128 * 128 + 64 * 4) == 49920
    assert CU_LDS // NN.kernel_lds_bytes(NN.KERNEL_PGEMM, 3) == 3          # alone: three per compute unit


def test_wgrad_dma_rings(NN):
    assert [NN.kernel_lds_bytes(NN.KERNEL_WGRAD_DMA, r) for r in (0, 1, 2)] == [3 * 24576, 4 * 12288, 3 * 12288]
    two = 2 * NN.kernel_lds_bytes(NN.KERNEL_PGEMM, 3)
    for ring in (1, 2):      # the slim rings exist for this
        assert NN.kernel_lds_bytes(NN.KERNEL_WGRAD_DMA, ring) + two <= CU_LDS
    assert NN.kernel_lds_bytes(NN.KERNEL_WGRAD_DMA, 0) + two > CU_LDS      # ... and the wide one leaves room for ONE (why a forked launch must not take it)
    with pytest.raises(Exception):
        NN.kernel_lds_bytes(NN.KERNEL_WGRAD_DMA, 3)
    with pytest.raises(Exception):
        NN.kernel_lds_bytes(99, 0)


def test_forked_weight_gradients_leave_room_for_two_pgemm_workgroups(NN):
    """Shipped defaults: the ring that the bottleneck-ResNet family (the flagship workload's) gives a weight-gradient GEMM forked beside the chain, and
    the other side-queue kernels.  (The halo kernel of the narrow decoder layers runs beside the narrow-input halo kernels' data gradients, not beside
    the persistent GEMM: reported in DESIGN 6.4, not part of this budget.  The basic-block and PackNet families keep ring 0 until an A/B of their own
    says otherwise: a family that moves to a slim ring is held to the budget too.)"""
    from simpledepthestimation_amd.hip import lib as L
    two = 2 * NN.kernel_lds_bytes(NN.KERNEL_PGEMM, 3)
    assert L.WGRAD_DMA_RINGS["resnet"] != 0
    side = {f"wgrad_dma ring of family {fam}": NN.kernel_lds_bytes(NN.KERNEL_WGRAD_DMA, ring) for fam, ring in L.WGRAD_DMA_RINGS.items() if ring != 0}
    side["wgrad_kernel (16-bit, single stage buffer)"] = NN.kernel_lds_bytes(NN.KERNEL_WGRAD_STAGED)
    side["wgrad_sum_batched"] = NN.kernel_lds_bytes(NN.KERNEL_WGRAD_SUM)
    side["wgrad_reduce_batched"] = NN.kernel_lds_bytes(NN.KERNEL_WGRAD_REDUCE)
    for name, lds in side.items():
        assert lds > 0 and lds + two <= CU_LDS, (name, lds, two)

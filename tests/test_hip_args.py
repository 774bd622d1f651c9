"""The argument checker the geometry bindings share (hip/args.py), on CPU tensors: what it normalises, and that every refusal is an SdeHipError
that carries the caller's name and the argument's.  "Another device" is the meta device here: the rule compares devices, whatever they are."""
import pytest
import torch

from simpledepthestimation_amd.hip import args as A
from simpledepthestimation_amd.hip.lib import SdeHipError

CPU, OTHER = torch.device("cpu"), torch.device("meta")


def refused(call, *words):
    with pytest.raises(SdeHipError) as e:
        call()
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_pred_is_normalised_from_its_three_ranks():
    base = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    for given, want in ((base, base), (base[:, None], base), (base[0], base[:1])):
        got = A.as_pred("op", given)
        assert tuple(got.shape) == tuple(want.shape) and got.is_contiguous() and torch.equal(got, want)
    strided = A.as_pred("op", base.transpose(1, 2))
    assert strided.is_contiguous() and torch.equal(strided, base.transpose(1, 2))
    assert A.as_pred("op", base).data_ptr() == base.data_ptr()                       # nothing is copied without need
    refused(lambda: A.as_pred("my_op", base.double()), "my_op", "pred", "float32")
    refused(lambda: A.as_pred("my_op", base[0, 0]), "my_op", "pred")                 # rank 1
    refused(lambda: A.as_pred("my_op", base[:, None].expand(2, 2, 3, 4)), "my_op", "pred")      # [N,2,ph,pw]
    refused(lambda: A.as_pred("my_op", base.numpy()), "my_op", "pred")


def test_K_is_broadcast_and_checked():
    K = torch.tensor([[2.0, 0, 1], [0, 3.0, 1], [0, 0, 1]])
    got = A.as_K("op", K, 3, CPU)
    assert tuple(got.shape) == (3, 3, 3) and got.is_contiguous() and all(torch.equal(got[n], K) for n in range(3))
    per_frame = torch.stack([K, 2 * K])
    assert A.as_K("op", per_frame, 2, CPU).data_ptr() == per_frame.data_ptr()
    refused(lambda: A.as_K("my_op", per_frame, 3, CPU), "my_op", "K", "[3,3,3]")              # N
    refused(lambda: A.as_K("my_op", K[:2], 1, CPU), "my_op", "K")                             # shape
    refused(lambda: A.as_K("my_op", K[0], 1, CPU), "my_op", "K")                              # rank
    refused(lambda: A.as_K("my_op", K.double(), 1, CPU), "my_op", "K", "float32")             # dtype
    refused(lambda: A.as_K("my_op", K, 1, OTHER), "my_op", "K", "meta")                       # device
    refused(lambda: A.as_K("my_op", K.to(OTHER), 1, CPU), "my_op", "K", "cpu")


def test_frame():
    f = torch.zeros(2, 4, 5, 3, dtype=torch.uint8)
    assert A.as_frame("op", None, 2, 4, 5, CPU) is None
    assert A.as_frame("op", f, 2, 4, 5, CPU).data_ptr() == f.data_ptr()
    assert tuple(A.as_frame("op", f[0], 1, 4, 5, CPU).shape) == (1, 4, 5, 3)
    refused(lambda: A.as_frame("my_op", f, 2, 5, 4, CPU), "my_op", "frame", "[2,5,4,3]")
    refused(lambda: A.as_frame("my_op", f.float(), 2, 4, 5, CPU), "my_op", "frame", "uint8")
    refused(lambda: A.as_frame("my_op", f[..., 0], 2, 4, 5, CPU), "my_op", "frame")
    refused(lambda: A.as_frame("my_op", f, 2, 4, 5, OTHER), "my_op", "frame", "meta")


def test_same_device_tensor():
    t = torch.zeros(2, 4, 4)
    assert A.same_device_tensor("op", "T", t, torch.float32, (2, 4, 4), CPU) is t
    assert A.same_device_tensor("op", "T", t, torch.float32, (None, 4, None), CPU) is t
    refused(lambda: A.same_device_tensor("my_op", "T", t, torch.float32, (2, 3, 4), CPU), "my_op: T must be", "[2,3,4]")
    refused(lambda: A.same_device_tensor("my_op", "T", t, torch.float32, (2, 4), CPU), "my_op: T must be")
    refused(lambda: A.same_device_tensor("my_op", "T", t, torch.float32, (None, 4, 4, None), CPU), "my_op: T must be", "[n,4,4,n]")
    refused(lambda: A.same_device_tensor("my_op", "T", t, torch.int32, (2, 4, 4), CPU), "my_op: T must be", "int32")
    refused(lambda: A.same_device_tensor("my_op", "T", t, torch.float32, (2, 4, 4), OTHER), "my_op: T must be", "meta")
    refused(lambda: A.same_device_tensor("my_op", "T", None, torch.float32, (2, 4, 4), CPU), "my_op: T must be", "NoneType")


def test_destinations():
    assert A.dst("op", None, (2, 3), torch.uint8, False, CPU) is None
    assert A.dst("op", torch.zeros(5), (2, 3), torch.uint8, False, CPU) is None          # not wanted: not looked at
    new = A.dst("op", None, (2, 3), torch.uint8, True, CPU)
    assert tuple(new.shape) == (2, 3) and new.dtype == torch.uint8 and new.device == CPU
    t = torch.zeros(2, 3, dtype=torch.uint8)
    assert A.dst("op", t, (2, 3), torch.uint8, True, CPU) is t
    refused(lambda: A.dst("my_op", t, (3, 2), torch.uint8, True, CPU), "my_op: destination must be")
    refused(lambda: A.dst("my_op", t, (2, 3), torch.int16, True, CPU), "my_op: destination must be", "int16")
    refused(lambda: A.dst("my_op", t, (2, 3), torch.uint8, True, OTHER), "my_op: destination must be", "meta")
    refused(lambda: A.dst("my_op", torch.zeros(3, 2, dtype=torch.uint8).t(), (2, 3), torch.uint8, True, CPU), "my_op: destination must be", "contiguous")

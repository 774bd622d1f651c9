"""CPU: the streaming kernel files refuse a dtype outside their type list on the host, before any launch, and keep their grid sizes.

Every call here hands HOST pointers to an entry point that must return SDE_ERR_ARG without launching.  Without a GPU a regression only turns
the -1 into the launch error -2; with one it would launch on host memory, so the whole module is skipped where a GPU is present."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="a regression would launch kernels on host pointers")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "simpledepthestimation_amd", "libsde_hip.so")
SDE_ERR_ARG = -1
SDE_F16 = 2
NOT_A_DTYPE = 7


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(LIB)
    lib.sde_last_error.restype = ctypes.c_char_p
    return lib


_BUF = ctypes.create_string_buffer(1 << 16)
P = ctypes.c_void_p(ctypes.addressof(_BUF))
NULL = ctypes.c_void_p(None)
L = ctypes.c_long

# one entry point per converted file: (name, arguments with valid sizes and pointers, given the dtype)
ALL_TYPES = [          # files instantiated for fp32, bf16 and fp16
    ("sde_bn_apply", lambda dt: (P, P, NULL, 0, L(4), 8, dt, P, NULL)),                       # nn.hip
    ("sde_space_to_depth", lambda dt: (P, 1, 2, 2, 8, dt, P, NULL)),                          # packnet.hip
    ("sde_dilate_split", lambda dt: (P, 1, 2, 2, 8, 1, dt, P, NULL)),                         # bts.hip
    ("sde_conv3d_fwd", lambda dt: (P, P, NULL, 1, 2, 2, 8, dt, P, NULL)),                     # conv3d.hip
]
NO_FP16 = [            # files instantiated for fp32 and bf16 only
    ("sde_bilinear2_fwd", lambda dt: (P, 1, 2, 2, 8, dt, P, NULL)),                           # google.hip
    ("sde_prep_input_bwd", lambda dt: (P, NULL, 1, 3, 2, 2, 8, dt, P, NULL)),                 # motion.hip
    ("sde_avgpool2x2_fwd", lambda dt: (P, 1, 2, 2, 8, dt, P, NULL)),                          # dense.hip
]
CASES = [(n, a, NOT_A_DTYPE) for n, a in ALL_TYPES + NO_FP16] + [(n, a, SDE_F16) for n, a in NO_FP16]


@pytest.mark.parametrize("name,args,dtype", CASES, ids=[f"{n}-dtype{d}" for n, _, d in CASES])
def test_unlisted_dtype_is_an_argument_error(built, name, args, dtype):
    fn = getattr(built, name)
    fn.restype = ctypes.c_int
    rc = fn(*args(dtype))
    msg = built.sde_last_error().decode()
    assert rc == SDE_ERR_ARG, (rc, msg)
    assert name in msg and f"dtype {dtype}" in msg, msg


def test_depth_head_bias_blocks_keeps_its_grid(built):
    """sde_depth_head_bias_blocks is the grid of the depth head's backward, and sizes the Python-side partial buffer: 256 items per
    workgroup, at least one workgroup, at most 8192."""
    f = built.sde_depth_head_bias_blocks
    f.restype = ctypes.c_int
    assert f(1, 1, 1) == 1
    assert f(12, 192, 640) == 5760          # below the cap
    assert f(64, 384, 1280) == 8192         # above it

"""Host side of the HIP ConvNeXt block: the validator, the workspace query, the refusals and the trainer's flag, without a GPU;
and a gradcheck of the float64 restatement the GPU tests compare against."""
import ctypes

import pytest
import torch

import convnext_ref as R


def _args(C, **over):
    x, params, _ = R.inputs((1, C, 3, 4), seed=1)
    args = dict(zip(["x"] + list(R.SHAPES), [x] + params))
    args.update(over)
    return args


@pytest.mark.parametrize("name,args", [
    ("x", _args(12)), ("x", _args(72)), ("w1", _args(16, w1=torch.zeros(16, 64))),
    ("x", _args(16, x=torch.zeros(1, 16, 3, 4, dtype=torch.float64))), ("gamma", _args(16, gamma=None))],
    ids=["C=12", "C=72", "w1 shape", "float64 x", "no gamma"])
def test_validator_names_the_argument(name, args):
    from neuroquant_amd import ops
    with pytest.raises(ValueError, match=rf"convnext_block: {name}\b"):
        ops.convnext_block_args("convnext_block", **args)
    assert ops.convnext_block_args("convnext_block", **_args(16)) == (1, 16, 3, 4)


def test_workspace_formula_and_refusals():
    from neuroquant_amd import _lib
    lib = _lib.lib()
    for N, C, H, W in [(1, 64, 128, 256), (2, 16, 2, 4), (3, 24, 17, 33)]:
        P = N * H * W
        Q = -(-(-(-P // 16)) // 4)
        G, S, T = min(Q, 256), min(Q, 16), N * -(-H // 8) * -(-W // 32)
        assert lib.nq_convnext_block_ws_bytes(N, C, H, W) == 4 * (P * C + 4 * G * C + 4 * S * (8 * C * C + 4 * C) + 50 * T * C)
    p = ctypes.c_void_p(4096)
    for C in (12, 72, 0):
        assert lib.nq_convnext_block_ws_bytes(1, C, 4, 4) == 0
        assert lib.nq_convnext_block_forward(*[p] * 13, 1, C, 4, 4, None) == -1
        assert lib.nq_convnext_block_backward(*[p] * 23, 1 << 30, 1, C, 4, 4, None) == -1
    assert lib.nq_convnext_block_forward(*[p] * 12, None, 1, 16, 4, 4, None) == -1       # a null output
    assert lib.nq_convnext_block_backward(*[p] * 23, 16, 1, 16, 4, 4, None) == -1          # a workspace below the query


def test_regress_flag():
    from neuroquant_amd.methods import regress
    assert regress.parse_args([]).enc_kernels == "torch"
    assert regress.parse_args(["--enc_kernels", "hip"]).enc_kernels == "hip"
    with pytest.raises(SystemExit):
        regress.parse_args(["--enc_kernels", "triton"])


def test_restatement_passes_gradcheck():
    x, params, _ = R.inputs((1, 8, 3, 4), seed=0)
    leaves = [t.double().requires_grad_(True) for t in [x] + params]
    assert torch.autograd.gradcheck(R.block, leaves)

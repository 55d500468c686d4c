"""Host side of the HIP encoder stages: the validator, the workspace query, the refusals, the trainer's flag and the module's
construction, without a GPU; and a gradcheck of the float64 restatement the GPU tests compare against."""
import ctypes

import pytest
import torch

import patchify_ref as R


def _args(shape, order, **over):
    x, params, _ = R.inputs(shape, order, seed=1)
    args = dict(zip(["x", "conv_w", "conv_b", "ln_w", "ln_b"], [x] + params), order=order)
    args.update(over)
    return args


@pytest.mark.parametrize("name,args", [
    ("conv_w", _args((1, 8, 12, 12, 8, 6), "pre")), ("conv_w", _args((1, 8, 4, 4, 12, 2), "pre")),
    ("x", _args((1, 3, 4, 4, 8, 2), "pre")), ("x", _args((1, 8, 4, 4, 8, 2), "pre", x=torch.zeros(1, 8, 4, 4, dtype=torch.float64))),
    ("conv_w", _args((1, 8, 4, 4, 8, 2), "pre", conv_w=torch.zeros(8, 16, 2, 2))), ("x", _args((1, 8, 3, 9, 8, 4), "pre"))],
    ids=["s=6", "C_out=12", "pre with C_in=3", "float64 x", "conv_w shape", "H < s"])
def test_validator_names_the_argument(name, args):
    from neuroquant_amd import ops
    with pytest.raises(ValueError, match=rf"patchify_ln: {name}\b"):
        ops.patchify_ln_args("patchify_ln", **args)
    assert ops.patchify_ln_args("patchify_ln", **_args((2, 3, 11, 20, 16, 5), "post")) == (2, 3, 11, 20, 16, 5)


def test_workspace_formula_and_refusals():
    from neuroquant_amd import _lib
    lib = _lib.lib()
    for N, Cin, H, W, Cout, s, order in [(2, 3, 640, 1280, 64, 5, 0), (2, 64, 128, 256, 64, 4, 1), (1, 24, 7, 11, 40, 3, 1)]:
        K, P = Cin * s * s, N * (H // s) * (W // s)
        T = -(-P // 16)
        if order == 0:
            A, Lw, G = P * Cout, Cout, min(T if T < 1024 and Cin >= 16 else -(-T // 4), 256)
        else:
            A, Lw, G = 0, Cin, min(-(-T * s // 4), 256)
        S = min(-(-T // 4), 32, max(1, 2 ** 19 // (Cout * (K + 1))))
        assert lib.nq_patchify_ln_ws_bytes(N, Cin, H, W, Cout, s, order) == 4 * (A + 2 * G * Lw + 4 * S * Cout * (K + 1))
    p = ctypes.c_void_p(4096)
    for N, Cin, H, W, Cout, s, order in [(1, 8, 12, 12, 8, 6, 1), (1, 8, 4, 4, 12, 2, 1), (1, 3, 4, 4, 8, 2, 1), (1, 8, 3, 9, 8, 4, 1),
                                         (1, 8, 4, 4, 8, 2, 2), (0, 8, 4, 4, 8, 2, 0)]:
        assert lib.nq_patchify_ln_ws_bytes(N, Cin, H, W, Cout, s, order) == 0
        assert lib.nq_patchify_ln_forward(*[p] * 8, N, Cin, H, W, Cout, s, order, None) == -1
        assert lib.nq_patchify_ln_backward(*[p] * 14, 1 << 30, N, Cin, H, W, Cout, s, order, None) == -1
    assert lib.nq_patchify_ln_forward(*[p] * 5, None, p, p, 1, 8, 4, 4, 8, 2, 1, None) == -1            # a null output
    assert lib.nq_patchify_ln_backward(*[p] * 9, None, *[p] * 4, 1 << 30, 1, 8, 4, 4, 8, 2, 1, None) == -1   # a null d conv_w
    assert lib.nq_patchify_ln_backward(*[p] * 14, 16, 1, 8, 4, 4, 8, 2, 1, None) == -1                   # a workspace below the query


def test_regress_flag_and_module_construction():
    from neuroquant_amd.methods import regress
    from neuroquant_amd.models._layers import ConvNeXt
    assert regress.parse_args([]).enc_kernels == "torch"
    assert regress.parse_args(["--enc_kernels", "hip_all"]).enc_kernels == "hip_all"
    with pytest.raises(SystemExit):
        regress.parse_args(["--enc_kernels", "triton"])
    with pytest.raises(ValueError):
        ConvNeXt(stage_blocks=1, strds=[5, 2], dims=[16, 12], kernels='hip_all')      # an unserved width
    hip, ref = (ConvNeXt(stage_blocks=1, strds=[5, 2], dims=[16, 8], kernels=k) for k in ('hip_all', 'torch'))
    assert hip.state_dict().keys() == ref.state_dict().keys()


@pytest.mark.parametrize("order", ["post", "pre"])
def test_restatement_passes_gradcheck(order):
    x, params, _ = R.inputs((1, 8, 5, 7, 8, 2), order, seed=0)
    leaves = [t.double().requires_grad_(True) for t in [x] + params]
    assert torch.autograd.gradcheck(lambda *t: R.stage(*t, order), leaves)

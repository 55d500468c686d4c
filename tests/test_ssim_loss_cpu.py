"""CPU-side checks of the SSIM training loss: the header's closed-form gradient against float64 autograd
through the restatement of pytorch_msssim.ssim (tests/ssim_loss_ref.py), the trainer's loss table, and the two C entries, whose
argument checks run before the device is touched."""
import ctypes
import os

import pytest
import torch

import ssim_loss_ref as SR
from conftest import ROOT, TINY_HNERV

WEIGHTS = ((0.0, 1.0), (1.0, 0.0), (0.3, 0.7), (0.7, 0.3))


@pytest.mark.parametrize("B,C,H,W", [(1, 1, 11, 11), (2, 3, 12, 21), (1, 3, 19, 130)], ids=str)
def test_closed_form_gradient_equals_float64_autograd(B, C, H, W):
    g = torch.Generator().manual_seed(100 * H + W)
    tgt = torch.rand(B, C, H, W, generator=g, dtype=torch.float64)
    pred = (tgt + 0.1 * torch.randn(B, C, H, W, generator=g, dtype=torch.float64)).clamp(0, 1)
    for w_mse, w_ssim in WEIGHTS:
        loss3, grad, _ = SR.loss_autograd(pred, tgt, w_mse, w_ssim)
        closed3, closed_grad = SR.loss_closed(pred, tgt, w_mse, w_ssim)
        assert float((loss3 - closed3).abs().max()) <= 1e-12
        assert float((grad - closed_grad).abs().max()) <= 1e-12
        assert float(grad.abs().max()) > 1e-6                        # and there is a gradient to compare


def test_trainer_loss_table():
    from neuroquant_amd.methods import regress
    args = regress.parse_args(["--arch", "hnerv", "--synthetic", "8"])
    table = {"ssim": (0.0, 1.0), "Fusion1": (0.3, 0.7), "Fusion3": (0.5, 0.5), "Fusion5": (0.7, 0.3)}
    for name, (w_mse, w_ssim) in table.items():
        assert regress.loss_params(args, dict(TINY_HNERV, loss=name)) == dict(w_mse=w_mse, w_ssim=w_ssim)
        assert getattr(args, "loss_domain", "rgb") == "rgb"          # evaluations log what they logged
    assert regress.loss_params(args, dict(TINY_HNERV, loss="l2")) is None
    for name in ("l1", "Fusion6", "Fusion10", "nonsense"):
        with pytest.raises(NotImplementedError):
            regress.loss_params(args, dict(TINY_HNERV, loss=name))


def test_entries_are_declared_and_exported():
    from neuroquant_amd import _lib
    header = open(os.path.join(ROOT, "include", "nq_hip.h")).read()
    lib = _lib.lib()
    for name in ("nq_ssim_loss_ws_floats", "nq_ssim_loss"):
        assert f" {name}(" in header and name in _lib.EXPORTS
        assert getattr(lib, name).argtypes                            # bound with a signature
    assert lib.nq_abi_version() == 7


def test_c_entries_reject_bad_arguments_without_a_gpu():
    from neuroquant_amd import _lib
    lib = _lib.lib()
    p, n = ctypes.c_void_p(16), None
    INVALID, UNSUPPORTED = -1, -2

    def call(pred=p, tgt=p, loss3=p, grad=p, ws=p, B=2, C=3, H=12, W=21, w_mse=0.7, w_ssim=0.3, gscale=1.0):
        return lib.nq_ssim_loss(pred, tgt, loss3, grad, ws, B, C, H, W, w_mse, w_ssim, gscale, n)

    for kw in (dict(pred=n), dict(tgt=n), dict(loss3=n), dict(ws=n)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(B=0), dict(B=-1), dict(C=0), dict(H=10), dict(W=10), dict(H=0), dict(W=-11)):
        assert call(**kw) == INVALID, kw
        assert lib.nq_ssim_loss_ws_floats(kw.get("B", 2), kw.get("C", 3), kw.get("H", 12), kw.get("W", 21)) == 0
    nan, inf = float("nan"), float("inf")
    for kw in (dict(w_mse=-1.0), dict(w_ssim=-0.5), dict(w_mse=nan), dict(w_ssim=inf), dict(w_ssim=-inf), dict(gscale=nan)):
        assert call(**kw) == INVALID, kw
    big = dict(B=2 ** 31 - 1, C=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1)                  # the element count past int64
    assert call(**big) == INVALID and lib.nq_ssim_loss_ws_floats(*big.values()) == 0
    assert call(B=65536, C=1) == UNSUPPORTED                                                 # planes past grid.y
    # the workspace: B frame values, two partial sums per forward tile and plane, three maps of the valid region
    for B, C, H, W in [(1, 1, 11, 11), (2, 3, 12, 21), (1, 3, 19, 130), (2, 3, 640, 1280)]:
        tiles = -(-(H - 10) // 8) * -(-(W - 10) // 118)
        assert lib.nq_ssim_loss_ws_floats(B, C, H, W) == B + 2 * B * C * tiles + 3 * B * C * (H - 10) * (W - 10)


def test_ops_check_arguments_before_any_launch():
    from neuroquant_amd import ops
    x = torch.zeros(1, 3, 12, 12)
    with pytest.raises(ValueError):
        ops.ssim_loss_raw(torch.zeros(1, 3, 10, 12), torch.zeros(1, 3, 10, 12), 0.0, 1.0)
    with pytest.raises(ValueError):
        ops.ssim_loss_raw(x, torch.zeros(1, 3, 12, 13), 0.0, 1.0)
    for w in ((-1.0, 1.0), (float("nan"), 1.0), (0.0, 0.0), (1.0, float("inf")), (None, 1.0)):
        with pytest.raises(ValueError):
            ops.ssim_loss_raw(x, x, *w)
    with pytest.raises(RuntimeError):
        ops.ssim_loss_raw(x, x, 0.0, 1.0)                              # CPU tensors: no fallback
    with pytest.raises(RuntimeError):
        ops.ssim(x, x)
    assert ops.SSIM_LOSS_TILE == (8, 118)

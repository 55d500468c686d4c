"""CPU-side checks of the calibration's MSE + SSIM objective: the head-mode closed form against float64
autograd through the tanh (tests/ssim_head_ref.py), the C entry's argument checks (they run before the device is touched), the
driver's flags and the engine's keyword."""
import ctypes
import os

import pytest
import torch

import ssim_head_ref as HR
from conftest import ROOT, TINY_HNERV

WEIGHTS = ((0.0, 1.0), (1.0, 0.0), (0.3, 0.7), (0.7, 0.3))


@pytest.mark.parametrize("B,C,H,W", [(1, 1, 11, 11), (2, 3, 12, 21), (1, 3, 19, 130)], ids=str)
def test_head_closed_form_equals_float64_autograd_through_the_tanh(B, C, H, W):
    g = torch.Generator().manual_seed(100 * H + W)
    z = 1.5 * torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    pred = 0.5 * torch.tanh(z) + 0.5
    tgt = (pred + 0.1 * torch.randn(B, C, H, W, generator=g, dtype=torch.float64)).clamp(0, 1)
    for w_mse, w_ssim in WEIGHTS:
        loss3, gz, db = HR.head_autograd(z, tgt, w_mse, w_ssim, float(C))
        closed3, g_img, g_head, closed_db, _ = HR.head_closed(pred, tgt, w_mse, w_ssim, float(C))
        assert float((loss3 - closed3).abs().max()) <= 1e-12
        assert float((gz - g_head).abs().max()) <= 1e-12
        assert float((db - closed_db).abs().max()) <= 1e-12
        assert float(gz.abs().max()) > 1e-6                          # and there is a gradient to compare
        # the factor as the kernel spells it
        assert float((g_head - g_img * 0.5 * (1 - (2 * pred - 1) ** 2)).abs().max()) <= 1e-15


def test_entries_are_declared_and_exported():
    from neuroquant_amd import _lib
    header = open(os.path.join(ROOT, "include", "nq_hip.h")).read()
    lib = _lib.lib()
    for name in ("nq_ssim_loss_head_ws_floats", "nq_ssim_loss_head"):
        assert f" {name}(" in header and name in _lib.EXPORTS
        assert getattr(lib, name).argtypes                            # bound with a signature
    assert lib.nq_abi_version() == 7


def test_c_entry_rejects_bad_arguments_without_a_gpu():
    from neuroquant_amd import _lib
    lib = _lib.lib()
    p, n = ctypes.c_void_p(16), None
    INVALID, UNSUPPORTED = -1, -2

    def call(pred=p, tgt=p, cache=n, idx=n, loss3=p, grad=p, db=p, ws=p, B=2, C=3, H=12, W=21, w_mse=0.7, w_ssim=0.3, scale=3.0):
        return lib.nq_ssim_loss_head(pred, tgt, cache, idx, loss3, grad, db, ws, B, C, H, W, w_mse, w_ssim, scale, n)

    # what nq_ssim_loss refuses
    for kw in (dict(pred=n), dict(loss3=n), dict(ws=n)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(B=0), dict(B=-1), dict(C=0), dict(H=10), dict(W=10), dict(H=0), dict(W=-11)):
        assert call(**kw) == INVALID, kw
        assert lib.nq_ssim_loss_head_ws_floats(kw.get("B", 2), kw.get("C", 3), kw.get("H", 12), kw.get("W", 21)) == 0
    nan, inf = float("nan"), float("inf")
    for kw in (dict(w_mse=-1.0), dict(w_ssim=-0.5), dict(w_mse=nan), dict(w_ssim=inf), dict(w_ssim=-inf), dict(scale=nan)):
        assert call(**kw) == INVALID, kw
    big = dict(B=2 ** 31 - 1, C=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1)                  # the element count past int64
    assert call(**big) == INVALID and lib.nq_ssim_loss_head_ws_floats(*big.values()) == 0
    assert call(B=65536, C=1) == UNSUPPORTED                                                 # planes past grid.y
    # the target: both, neither, a cache without indices; the bias gradient without the gradient it sums
    assert call(tgt=p, cache=p, idx=p) == INVALID
    assert call(tgt=n, cache=n, idx=n) == INVALID
    assert call(tgt=n, cache=n, idx=p) == INVALID
    assert call(tgt=n, cache=p, idx=n) == INVALID
    assert call(grad=n, db=p) == INVALID
    # the workspace: that of nq_ssim_loss and one partial sum per backward workgroup (8 x 118 tiles of the H x W image)
    for B, C, H, W in [(1, 1, 11, 11), (2, 3, 12, 21), (1, 3, 19, 130), (2, 3, 640, 1280)]:
        tiles = -(-H // 8) * -(-W // 118)
        assert lib.nq_ssim_loss_head_ws_floats(B, C, H, W) == lib.nq_ssim_loss_ws_floats(B, C, H, W) + B * C * tiles


def test_ops_check_arguments_before_any_launch():
    from neuroquant_amd import ops
    x = torch.zeros(1, 3, 12, 12)
    before = ops.ssim_loss_head_launches
    with pytest.raises(ValueError):
        ops.ssim_loss_head_grad(torch.zeros(1, 3, 10, 12), tgt=torch.zeros(1, 3, 10, 12))
    with pytest.raises(ValueError):
        ops.ssim_loss_head_grad(x, tgt=torch.zeros(1, 3, 12, 13))
    with pytest.raises(ValueError):
        ops.ssim_loss_head_grad(x)                                                           # neither target
    with pytest.raises(ValueError):
        ops.ssim_loss_head_grad(x, tgt=x, cache_u8=torch.zeros(5, 3, 12, 12, dtype=torch.uint8), idx=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.ssim_loss_head_grad(x, cache_u8=torch.zeros(5, 3, 12, 12, dtype=torch.uint8))    # no indices
    with pytest.raises(ValueError):
        ops.ssim_loss_head_grad(x, cache_u8=torch.zeros(5, 3, 12, 13, dtype=torch.uint8), idx=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.ssim_loss_head_grad(x, cache_u8=torch.zeros(5, 3, 12, 12), idx=torch.zeros(1, dtype=torch.int64))   # not uint8
    with pytest.raises(ValueError):
        ops.ssim_loss_head_grad(x, cache_u8=torch.zeros(5, 3, 12, 12, dtype=torch.uint8), idx=torch.zeros(2, dtype=torch.int64))
    for w in ((-1.0, 1.0), (float("nan"), 1.0), (0.0, 0.0), (1.0, float("inf")), (None, 1.0)):
        with pytest.raises(ValueError):
            ops.ssim_loss_head_grad(x, tgt=x, w_mse=w[0], w_ssim=w[1])
    with pytest.raises(RuntimeError):
        ops.ssim_loss_head_grad(x, tgt=x, w_mse=0.0, w_ssim=1.0)                             # CPU tensors: no fallback
    assert ops.ssim_loss_head_launches == before


def test_driver_flags_and_the_shared_weight_table():
    from neuroquant_amd.methods import calibrate_network as cn
    from neuroquant_amd.methods import regress
    table = {"ssim": (0.0, 1.0), "Fusion1": (0.3, 0.7), "Fusion3": (0.5, 0.5), "Fusion5": (0.7, 0.3)}
    assert cn.SSIM_LOSSES == table and regress.SSIM_LOSSES is cn.SSIM_LOSSES
    dflt = cn.parse_args(["--arch", "hnerv"])
    assert dflt.rec_loss == "l2" and dflt.rec_weights is None and cn.rec_loss_params(dflt) is None
    assert cn.rec_loss_params(cn.parse_args(["--arch", "hnerv", "--rec_loss", "l2"])) is None
    for name, (w_mse, w_ssim) in table.items():
        args = cn.parse_args(["--arch", "hnerv", "--rec_loss", name])
        assert cn.rec_loss_params(args) == dict(w_mse=w_mse, w_ssim=w_ssim)
    args = cn.parse_args(["--arch", "hnerv", "--rec_weights", "0.25", "2"])
    assert cn.rec_loss_params(args) == dict(w_mse=0.25, w_ssim=2.0)
    with pytest.raises(SystemExit):                                   # argparse: not allowed with
        cn.parse_args(["--arch", "hnerv", "--rec_loss", "Fusion5", "--rec_weights", "0.7", "0.3"])
    with pytest.raises(SystemExit):
        cn.parse_args(["--arch", "hnerv", "--rec_loss", "l1"])
    for bad in (["-1", "1"], ["0", "0"], ["nan", "1"]):
        with pytest.raises(ValueError):
            cn.rec_loss_params(cn.parse_args(["--arch", "hnerv", "--rec_weights"] + bad))
    with pytest.raises(ValueError):
        cn.rec_loss_params(cn.parse_args(["--arch", "hnerv", "--rec_loss", "Fusion1", "--loss_domain", "yuv420"]))
    # the trainer's table is where it was and refuses what it refused
    rargs = regress.parse_args(["--arch", "hnerv", "--synthetic", "8"])
    assert regress.loss_params(rargs, dict(TINY_HNERV, loss="Fusion5")) == dict(w_mse=0.7, w_ssim=0.3)
    with pytest.raises(NotImplementedError):
        regress.loss_params(rargs, dict(TINY_HNERV, loss="l1"))


def test_engine_keyword_is_checked_before_the_first_iteration():
    from neuroquant_amd.quantization import model_reconstruction
    from neuroquant_amd.quantization.calib_model import LossFunction
    ok = dict(w_mse=0.7, w_ssim=0.3)
    with pytest.raises(ValueError):
        model_reconstruction(None, cali_data=None, gt=[], loss_domain="yuv420", ssim=ok)
    for bad in (dict(w_mse=0.7), dict(w_mse=0.7, w_ssim=0.3, w_l1=1.0), dict(w_mse=-1.0, w_ssim=1.0), dict(w_mse=0.0, w_ssim=0.0),
                dict(w_mse=float("nan"), w_ssim=1.0), dict(w_mse=None, w_ssim=1.0), (0.7, 0.3)):
        with pytest.raises(ValueError):
            model_reconstruction(None, cali_data=None, gt=[], ssim=bad)
    lf = LossFunction(None, rec_loss="ssim", ssim=ok)
    assert lf.rec == "ssim" and lf.ssim == ok

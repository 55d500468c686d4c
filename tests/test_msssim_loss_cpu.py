"""CPU-side checks of the MS-SSIM training loss: the header's closed-form gradient against float64 autograd
through the restatement (tests/msssim_loss_ref.py), its forward value against tests/msssim_ref.py, the C entries (whose
argument checks run before the device is touched), the flags of both drivers and the engine's keyword."""
import ctypes
import os

import pytest
import torch

import msssim_loss_ref as MR
import msssim_ref as M
from conftest import ROOT, TINY_HNERV

WEIGHTS = ((0.0, 1.0), (1.0, 0.0), (0.3, 0.7), (0.7, 0.3))


def _pair(B, C, H, W, sigma=0.1):
    g = torch.Generator().manual_seed(100 * H + W)
    tgt = torch.rand(B, C, H, W, generator=g, dtype=torch.float64)
    # smooth the target a little so that every scale has structure to compare (no plane near the clamp)
    tgt = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(tgt, (2, 2, 2, 2), mode="replicate"), 5, 1)
    pred = (tgt + sigma * torch.randn(B, C, H, W, generator=g, dtype=torch.float64)).clamp(0, 1)
    return pred, tgt


def test_closed_form_gradient_equals_float64_autograd():
    pred, tgt = _pair(2, 2, 161, 170)
    for w_mse, w_ms in WEIGHTS:
        loss3, grad, _, v = MR.loss_autograd(pred, tgt, w_mse, w_ms)
        closed3, closed_grad = MR.loss_closed(pred, tgt, w_mse, w_ms)
        assert float(v.min()) > 0.01                                  # no plane is clamped here
        assert float((loss3 - closed3).abs().max()) <= 1e-12
        assert float((grad - closed_grad).abs().max()) <= 1e-12
        assert float(grad.abs().max()) > 1e-7                         # and there is a gradient to compare


def test_forward_value_is_the_ms_ssim_yardstick():
    for pred, tgt in (_pair(2, 2, 161, 170), (torch.rand(1, 3, 162, 175, generator=torch.Generator().manual_seed(1)),
                                              torch.rand(1, 3, 162, 175, generator=torch.Generator().manual_seed(2)))):
        loss3, _, ms_b, _ = MR.loss_autograd(pred, tgt, 0.0, 1.0)
        ref = M.ms_ssim_f64(pred, tgt)
        assert float((ms_b - ref).abs().max()) <= 1e-15
        assert abs(float(loss3[0]) - (1.0 - float(ref.mean()))) <= 1e-15


def test_clamped_planes_give_a_zero_and_finite_gradient():
    """independent uniform images: some v_s <= 0 on every plane; autograd meets no 0^w, the closed form agrees"""
    g = torch.Generator().manual_seed(1000 * 162 + 175)               # the GPU tests' clamp case A
    pred, tgt = torch.rand(1, 3, 162, 175, generator=g), torch.rand(1, 3, 162, 175, generator=g)
    loss3, grad, ms_b, v = MR.loss_autograd(pred, tgt, 0.0, 1.0)
    assert bool(((v <= 0).any(0)).all()) and ms_b.tolist() == [0.0] and float(loss3[0]) == 1.0
    assert abs(float(v.min()) + 0.0075) < 1e-4                        # far from fp32 doubt
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) == 0.0
    closed3, closed_grad = MR.loss_closed(pred, tgt, 0.3, 0.7)
    loss3, grad, _, _ = MR.loss_autograd(pred, tgt, 0.3, 0.7)
    assert float((loss3 - closed3).abs().max()) <= 1e-12 and float((grad - closed_grad).abs().max()) <= 1e-12


def test_up_is_the_adjoint_of_the_pooling():
    g = torch.Generator().manual_seed(3)
    for h, w in ((161, 176), (162, 175), (11, 22), (21, 21)):
        x = torch.rand(1, 2, h, w, generator=g, dtype=torch.float64)
        y = torch.rand(1, 2, (h + 1) // 2, (w + 1) // 2, generator=g, dtype=torch.float64)
        assert MR.pool(x).shape == y.shape
        assert abs(float((MR.pool(x) * y).sum()) - float((x * MR.up(y, h, w)).sum())) <= 1e-10


def test_entries_are_declared_and_exported():
    from neuroquant_amd import _lib
    header = open(os.path.join(ROOT, "include", "nq_hip.h")).read()
    lib = _lib.lib()
    for name in ("nq_msssim_loss_ws_floats", "nq_msssim_loss"):
        assert f" {name}(" in header and name in _lib.EXPORTS
        assert getattr(lib, name).argtypes                            # bound with a signature
    assert lib.nq_abi_version() == 7


def _ws_formula(B, C, H, W):
    """the header's workspace formula"""
    n, h, w = B + 5 * B * C, H, W
    for s in range(5):
        tiles = -(-(h - 10) // 8) * -(-(w - 10) // 118)
        n += B * C * tiles * (2 if s == 0 else 1) + 3 * B * C * (h - 10) * (w - 10) + (3 * B * C * h * w if s else 0)
        h, w = (h + 1) // 2, (w + 1) // 2
    return n


def test_c_entries_reject_bad_arguments_without_a_gpu():
    from neuroquant_amd import _lib
    lib = _lib.lib()
    p, n = ctypes.c_void_p(16), None
    INVALID, UNSUPPORTED = -1, -2

    def call(pred=p, tgt=p, loss3=p, grad=p, ws=p, B=2, C=3, H=161, W=176, w_mse=0.7, w_ms=0.3, gscale=1.0):
        return lib.nq_msssim_loss(pred, tgt, loss3, grad, ws, B, C, H, W, w_mse, w_ms, gscale, n)

    for kw in (dict(pred=n), dict(tgt=n), dict(loss3=n), dict(ws=n)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(B=0), dict(B=-1), dict(C=0), dict(C=-3), dict(H=160), dict(W=160), dict(H=0), dict(W=-161), dict(H=11, W=11)):
        assert call(**kw) == INVALID, kw
        assert lib.nq_msssim_loss_ws_floats(kw.get("B", 2), kw.get("C", 3), kw.get("H", 161), kw.get("W", 176)) == 0
    nan, inf = float("nan"), float("inf")
    for kw in (dict(w_mse=-1.0), dict(w_ms=-0.5), dict(w_mse=nan), dict(w_ms=inf), dict(w_ms=-inf), dict(gscale=nan),
               dict(gscale=inf), dict(w_mse=0.0, w_ms=0.0)):
        assert call(**kw) == INVALID, kw
    big = dict(B=2 ** 31 - 1, C=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1)                  # the element count past int64
    assert call(**big) == INVALID and lib.nq_msssim_loss_ws_floats(*big.values()) == 0
    assert call(B=65536, C=1) == UNSUPPORTED and lib.nq_msssim_loss_ws_floats(65536, 1, 161, 176) == 0   # planes past grid.y
    for shape in [(1, 1, 161, 161), (2, 3, 161, 176), (1, 3, 162, 175), (2, 3, 640, 1280)]:
        assert lib.nq_msssim_loss_ws_floats(*shape) == _ws_formula(*shape)


def test_ops_check_arguments_before_any_launch():
    from neuroquant_amd import ops
    x = torch.zeros(1, 3, 161, 161)
    low = torch.zeros(1, 3, 160, 200)
    with pytest.raises(ValueError):
        ops.ms_ssim_loss_raw(low, low, 0.0, 1.0)
    with pytest.raises(ValueError):
        ops.ms_ssim_loss(low, low)
    with pytest.raises(ValueError):
        ops.ms_ssim_loss_raw(x, torch.zeros(1, 3, 161, 162), 0.0, 1.0)
    for w in ((-1.0, 1.0), (float("nan"), 1.0), (0.0, 0.0), (1.0, float("inf")), (None, 1.0)):
        with pytest.raises(ValueError):
            ops.ms_ssim_loss_raw(x, x, *w)
        with pytest.raises(ValueError):
            ops.msssim_loss_head_grad(x, tgt=x, w_mse=w[0], w_ms=w[1])
    before = ops.msssim_loss_head_launches
    u8, idx = torch.zeros(4, 3, 161, 161, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError):
        ops.msssim_loss_head_grad(x)                                   # neither target
    with pytest.raises(ValueError):
        ops.msssim_loss_head_grad(x, tgt=x, cache_u8=u8, idx=idx)      # both
    with pytest.raises(ValueError):
        ops.msssim_loss_head_grad(x, cache_u8=u8.float(), idx=idx)     # not a uint8 cache
    with pytest.raises(ValueError):
        ops.msssim_loss_head_grad(x, cache_u8=u8[:, :, :160], idx=idx)
    with pytest.raises(ValueError):
        ops.msssim_loss_head_grad(low, tgt=low)
    with pytest.raises(RuntimeError):
        ops.ms_ssim_loss_raw(x, x, 0.0, 1.0)                           # CPU tensors: no fallback
    with pytest.raises(RuntimeError):
        ops.msssim_loss_head_grad(x, tgt=x)
    with pytest.raises(RuntimeError):
        ops.msssim_loss_head_grad(x, cache_u8=u8, idx=idx)
    assert ops.msssim_loss_head_launches == before
    assert ops.MSSSIM_LOSS_LAUNCHES == 11


def test_driver_flags_and_exclusions():
    from neuroquant_amd.methods import calibrate_network as cn
    from neuroquant_amd.methods import regress
    base = ["--arch", "hnerv"]
    dflt = cn.parse_args(base)
    assert dflt.rec_ms_weights is None and cn.rec_msssim_params(dflt) is None
    for name in ("l2", "ssim", "Fusion5"):
        assert cn.rec_msssim_params(cn.parse_args(base + ["--rec_loss", name])) is None
    args = cn.parse_args(base + ["--rec_loss", "msssim"])
    assert cn.rec_msssim_params(args) == dict(w_mse=0.0, w_ms=1.0) and cn.rec_loss_params(args) is None
    args = cn.parse_args(base + ["--rec_ms_weights", "0.25", "2"])
    assert cn.rec_msssim_params(args) == dict(w_mse=0.25, w_ms=2.0) and cn.rec_loss_params(args) is None
    for both in (["--rec_loss", "msssim", "--rec_ms_weights", "0.7", "0.3"], ["--rec_weights", "1", "1", "--rec_ms_weights", "1", "1"],
                 ["--rec_loss", "Fusion5", "--rec_ms_weights", "0.7", "0.3"]):
        with pytest.raises(SystemExit):                               # argparse: not allowed with
            cn.parse_args(base + both)
    with pytest.raises(SystemExit):
        cn.parse_args(base + ["--rec_loss", "l1"])                    # still refused
    for bad in (["-1", "1"], ["0", "0"], ["nan", "1"]):
        with pytest.raises(ValueError):
            cn.rec_msssim_params(cn.parse_args(base + ["--rec_ms_weights"] + bad))
    for flags in (["--rec_loss", "msssim"], ["--rec_ms_weights", "0.5", "0.5"]):
        with pytest.raises(ValueError):
            cn.rec_msssim_params(cn.parse_args(base + flags + ["--loss_domain", "yuv420"]))
    # the trainer: `loss: msssim`, optional `loss_weights`; the SSIM table is the four-entry table it was
    assert list(cn.SSIM_LOSSES) == ["ssim", "Fusion1", "Fusion3", "Fusion5"] and regress.SSIM_LOSSES is cn.SSIM_LOSSES
    rargs = regress.parse_args(["--arch", "hnerv", "--synthetic", "8"])
    assert regress.loss_params(rargs, dict(TINY_HNERV, loss="msssim")) == dict(w_mse=0.0, w_ms=1.0)
    assert regress.loss_params(rargs, dict(TINY_HNERV, loss="msssim", loss_weights=[0.5, 0.5])) == dict(w_mse=0.5, w_ms=0.5)
    assert getattr(rargs, "loss_domain", "rgb") == "rgb"
    for bad in ([0.5], [0.0, 0.0], [-1.0, 1.0], "0.5 0.5", [float("nan"), 1.0]):
        with pytest.raises(ValueError):
            regress.loss_params(rargs, dict(TINY_HNERV, loss="msssim", loss_weights=bad))
    for name in ("l1", "Fusion6", "Fusion10", "nonsense"):
        with pytest.raises(NotImplementedError):
            regress.loss_params(rargs, dict(TINY_HNERV, loss=name))


def test_engine_keyword_is_checked_before_the_first_iteration():
    from neuroquant_amd.quantization import model_reconstruction
    from neuroquant_amd.quantization.calib_model import LossFunction
    ok = dict(w_mse=0.7, w_ms=0.3)
    with pytest.raises(ValueError):
        model_reconstruction(None, cali_data=None, gt=[], loss_domain="yuv420", msssim=ok)
    with pytest.raises(ValueError):
        model_reconstruction(None, cali_data=None, gt=[], ssim=dict(w_mse=0.7, w_ssim=0.3), msssim=ok)
    for bad in (dict(w_mse=0.7), dict(w_mse=0.7, w_ssim=0.3), dict(w_mse=0.7, w_ms=0.3, w_l1=1.0), dict(w_mse=-1.0, w_ms=1.0),
                dict(w_mse=0.0, w_ms=0.0), dict(w_mse=float("nan"), w_ms=1.0), dict(w_mse=None, w_ms=1.0), (0.7, 0.3)):
        with pytest.raises(ValueError):
            model_reconstruction(None, cali_data=None, gt=[], msssim=bad)
    with pytest.raises(ValueError):                                   # the ssim keyword keeps its exact key check
        model_reconstruction(None, cali_data=None, gt=[], ssim=ok)
    lf = LossFunction(None, rec_loss="msssim", msssim=ok)
    assert lf.rec == "msssim" and lf.msssim == ok

"""CPU-side checks of the YUV 4:2:0 objective: the float64 yardstick (tests/yuv_loss_ref.py) against torch's
float64 autograd and against the player's conversion (tests/yuv_ref.py), and the C entries' argument checks, which run before
the device is touched."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import yuv_loss_ref as LR
import yuv_ref as R

MATRICES = ("bt601", "bt709")
WEIGHTS = ((6, 1, 1), (1, 1, 1), (1, 0, 0), (0, 1, 2))


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


@pytest.mark.parametrize("matrix,full_range,weights", list(itertools.product(MATRICES, (False, True), WEIGHTS)))
def test_closed_form_gradient_equals_float64_autograd(matrix, full_range, weights):
    pred, tgt, _ = LR.images(2, 6, 10, seed=3)
    loss4, g, _ = LR.loss_f64(pred, tgt, matrix, full_range, weights)
    p = torch.from_numpy(pred).double().requires_grad_(True)
    L, mse = LR.loss_torch(p, torch.from_numpy(tgt).double(), matrix, full_range, weights)
    (gt,) = torch.autograd.grad(L, p)
    assert _rel(g, gt.numpy()) <= 1e-12
    want = np.array([float(L.detach())] + [float(m.detach()) for m in mse])
    np.testing.assert_allclose(loss4, want, rtol=1e-12, atol=0)
    # tanh-head form: pred = tanh(x) * 0.5 + 0.5, the gradient at x and its channel sums
    x = torch.atanh(torch.from_numpy(np.clip(pred, 0.02, 0.98)).double() * 2 - 1).requires_grad_(True)
    ph = torch.tanh(x) * 0.5 + 0.5
    Lh, _ = LR.loss_torch(ph, torch.from_numpy(tgt).double(), matrix, full_range, weights)
    (gx,) = torch.autograd.grad(Lh, x)
    _, gh, dbh = LR.loss_f64(ph.detach().numpy(), tgt, matrix, full_range, weights, head=True)
    assert _rel(gh, gx.numpy()) <= 1e-12
    np.testing.assert_allclose(dbh, gx.sum(dim=(0, 2, 3)).numpy(), rtol=0, atol=1e-12 * float(gx.abs().sum()))
    # gscale multiplies the gradient, nothing else
    l2, g2, _ = LR.loss_f64(pred, tgt, matrix, full_range, weights, gscale=0.25)
    np.testing.assert_array_equal(l2, loss4)
    np.testing.assert_allclose(g2, 0.25 * g, rtol=1e-15, atol=0)


@pytest.mark.parametrize("matrix,full_range", list(itertools.product(MATRICES, (False, True))))
def test_plane_mse_is_the_players_metric_before_rounding(matrix, full_range):
    """255^2 MSE_plane = the mean squared difference of the unrounded 8-bit codes of pred and tgt, per plane"""
    pred, tgt, _ = LR.images(2, 8, 12, seed=5)
    H, W = pred.shape[-2:]
    loss4, _, _ = LR.loss_f64(pred, tgt, matrix, full_range)
    a, b = R.rgb_to_yuv420_f64(pred, matrix, full_range), R.rgb_to_yuv420_f64(tgt, matrix, full_range)
    d2 = (a - b) ** 2
    HW = H * W
    want = [d2[:, :HW].mean(), d2[:, HW:HW + HW // 4].mean(), d2[:, HW + HW // 4:].mean()]
    np.testing.assert_allclose(255.0 ** 2 * loss4[1:], want, rtol=1e-9, atol=0)
    wy, wu, wv = 6.0, 1.0, 1.0
    np.testing.assert_allclose(loss4[0], 3 * (wy * loss4[1] + wu * loss4[2] + wv * loss4[3]) / 8, rtol=1e-14)


@pytest.mark.parametrize("matrix", MATRICES)
def test_grey_differences_carry_no_chroma_error(matrix):
    pred, tgt, _ = LR.images(1, 4, 6, seed=7)
    grey = np.random.default_rng(1).normal(0, 0.05, size=(1, 1, 4, 6))
    loss4, g, _ = LR.loss_f64(tgt.astype(np.float64) + grey, tgt, matrix, False)
    assert loss4[1] > 1e-5
    assert loss4[2] <= 1e-28 * loss4[1] and loss4[3] <= 1e-28 * loss4[1]      # Kr + Kg + Kb = 1 up to rounding


def _entry():
    from neuroquant_amd import _lib
    return _lib.lib()


def test_c_entries_reject_bad_arguments_without_a_gpu():
    lib = _entry()
    p, n = ctypes.c_void_p(16), None
    INVALID, UNSUPPORTED = -1, -2

    def call(pred=p, tgt=p, cache=n, idx=n, loss=p, grad=p, db=n, ws=p, B=2, H=4, W=8, matrix=1, full=0, wy=6.0, wu=1.0, wv=1.0):
        return lib.nq_yuv420_loss(pred, tgt, cache, idx, loss, grad, db, ws, B, H, W, matrix, full, wy, wu, wv, 1.0, n)

    for kw in (dict(pred=n), dict(loss=n), dict(grad=n), dict(ws=n)):                       # null pointers
        assert call(**kw) == INVALID, kw
    assert call(tgt=p, cache=p, idx=p) == INVALID                                            # both targets
    assert call(tgt=n) == INVALID                                                            # neither
    assert call(tgt=n, cache=p, idx=n) == INVALID                                            # a cache without indices
    for kw in (dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(H=-2), dict(W=-4), dict(H=3), dict(W=7)):
        assert call(**kw) == INVALID, kw
        assert lib.nq_yuv420_loss_ws_floats(kw.get("B", 2), kw.get("H", 4), kw.get("W", 8)) == 0
    for kw in (dict(matrix=2), dict(matrix=-1), dict(full=2), dict(full=-1)):
        assert call(**kw) == INVALID, kw
    nan, inf = float("nan"), float("inf")
    for kw in (dict(wy=-1.0), dict(wu=-0.5), dict(wv=-6.0), dict(wy=nan), dict(wu=inf), dict(wv=-inf),
               dict(wy=0.0, wu=0.0, wv=0.0)):
        assert call(**kw) == INVALID, kw
    big = dict(B=2 ** 31 - 1, H=2 ** 31 - 2, W=2 ** 31 - 2)                                   # B * 3 * H * W past int64
    assert call(**big) == INVALID and lib.nq_yuv420_loss_ws_floats(*big.values()) == 0
    grid = dict(B=2 ** 20, H=2 ** 11, W=2 ** 11)                                              # 2^32 workgroups
    assert call(**grid) == UNSUPPORTED and lib.nq_yuv420_loss_ws_floats(*grid.values()) == 0
    assert call(tgt=n, cache=p, idx=p, db=p, **grid) == UNSUPPORTED


def test_workspace_size():
    lib = _entry()
    for B, H, W in [(1, 2, 2), (2, 6, 10), (1, 34, 516), (2, 640, 1280), (2, 960, 1920)]:
        got = lib.nq_yuv420_loss_ws_floats(B, H, W)
        assert got == 6 * -(-(B * (H // 2) * (W // 2)) // 256) > 0        # six sums per workgroup of the one-block-per-thread launch


def test_ops_check_arguments_before_any_launch():
    from neuroquant_amd import ops
    x = torch.zeros(1, 3, 4, 4)
    with pytest.raises(ValueError):
        ops.yuv420_loss_raw(x, tgt=x, matrix="bt2020")
    for w in ((1, 1), (-1, 1, 1), (0, 0, 0), (float("nan"), 1, 1), (1, 1, float("inf")), None):
        with pytest.raises(ValueError):
            ops.yuv420_loss_raw(x, tgt=x, weights=w)
    with pytest.raises(ValueError):
        ops.yuv420_loss_raw(torch.zeros(1, 3, 3, 4), tgt=torch.zeros(1, 3, 3, 4))
    with pytest.raises(RuntimeError):
        ops.yuv420_loss_raw(x, tgt=x)                                      # CPU tensors: no fallback
    assert ops.yuv420_loss_launches == 0

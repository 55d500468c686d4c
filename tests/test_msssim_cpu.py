"""MS-SSIM without a GPU: the float64 yardstick (tests/msssim_ref.py) against an independent restatement and against known
answers, and the boundary of the new C entry points / ops / utils names."""
import ctypes

import numpy as np
import pytest
import torch

import msssim_ref as R


def _independent_ms_ssim(X, Y):
    """The definition once more with other tools: scipy's correlate1d for the window, reshape-mean for the pooling
    (even sizes only), numpy float64 throughout."""
    from scipy.ndimage import correlate1d
    g = R.window(torch.float64).numpy()

    def filt(a):
        a = correlate1d(a, g, axis=-2, mode="constant")[..., 5:-5, :]
        return correlate1d(a, g, axis=-1, mode="constant")[..., :, 5:-5]

    X, Y = X.double().numpy(), Y.double().numpy()
    vals = []
    for s in range(5):
        mu1, mu2 = filt(X), filt(Y)
        s1, s2, s12 = filt(X * X) - mu1 * mu1, filt(Y * Y) - mu2 * mu2, filt(X * Y) - mu1 * mu2
        cs_map = (2 * s12 + R.C2) / (s1 + s2 + R.C2)
        if s < 4:
            vals.append(np.maximum(cs_map.mean((-2, -1)), 0))
            f, c, h, w = X.shape
            assert h % 2 == 0 and w % 2 == 0
            X = X.reshape(f, c, h // 2, 2, w // 2, 2).mean((3, 5))
            Y = Y.reshape(f, c, h // 2, 2, w // 2, 2).mean((3, 5))
        else:
            ssim_map = (2 * mu1 * mu2 + R.C1) / (mu1 * mu1 + mu2 * mu2 + R.C1) * cs_map
            vals.append(np.maximum(ssim_map.mean((-2, -1)), 0))
    v = np.stack(vals, 0) ** np.array(R.WEIGHTS).reshape(-1, 1, 1)
    return v.prod(0).mean(1)


def test_restatement_agrees_with_an_independent_one():
    pytest.importorskip("scipy")
    Y = R.bunny_frames(2)
    X = R.noisy(Y, 0.014)
    a, b = R.ms_ssim_f64(X, Y).numpy(), _independent_ms_ssim(X, Y)
    print("ms_ssim_f64", a, "independent", b, "max diff", np.abs(a - b).max())
    assert a.shape == (2,) and np.all((a > 0.98) & (a < 0.999))
    assert np.abs(a - b).max() <= 1e-12


def test_identical_and_inverted_inputs():
    Y = R.bunny_frames(2)
    for dtype in (torch.float64, torch.float32):
        assert torch.equal(R.ms_ssim_f64(Y, Y, dtype=dtype), torch.ones(2, dtype=dtype))
        assert torch.equal(R.ms_ssim_f64(1 - Y, Y, dtype=dtype), torch.zeros(2, dtype=dtype))     # relu and 0^w = 0


def _pool_padded_by_hand(a):
    """avg_pool2d(kernel 2, stride 2, padding (h % 2, w % 2)) written out: explicit zeros on both sides, divisor 4."""
    f, c, h, w = a.shape
    ph, pw = h % 2, w % 2
    p = torch.zeros(f, c, h + 2 * ph, w + 2 * pw, dtype=a.dtype)
    p[:, :, ph:ph + h, pw:pw + w] = a
    oh, ow = (h + 2 * ph - 2) // 2 + 1, (w + 2 * pw - 2) // 2 + 1
    p = p[:, :, :2 * oh, :2 * ow]
    return (p[:, :, 0::2, 0::2] + p[:, :, 0::2, 1::2] + p[:, :, 1::2, 0::2] + p[:, :, 1::2, 1::2]) / 4


def test_odd_sizes_pool_with_zero_padding_and_divisor_four():
    Y = R.bunny_frames(1)[:, :, 100:423, 200:845].contiguous()          # 323 x 645: odd at scales 1, 3 (H) and 1, 2, 4 (W)
    X = R.noisy(Y, 0.014)
    g = R.window()
    Xs, Ys, vals = X.double(), Y.double(), []
    sizes = []
    for s in range(5):
        sizes.append(tuple(Xs.shape[-2:]))
        ssim, cs = R.ssim_cs(Xs, Ys, g)
        vals.append(torch.relu(cs if s < 4 else ssim))
        if s < 4:
            Xs, Ys = _pool_padded_by_hand(Xs), _pool_padded_by_hand(Ys)
    assert sizes == [(323, 645), (162, 323), (81, 162), (41, 81), (21, 41)]
    want = torch.prod(torch.stack(vals) ** torch.tensor(R.WEIGHTS, dtype=torch.float64).view(-1, 1, 1), 0).mean(1)
    got = R.ms_ssim_f64(X, Y)
    print("odd size", got, want)
    assert (got - want).abs().max() <= 1e-14


def test_c_entry_points_reject_bad_arguments_without_a_gpu():
    from neuroquant_amd import _lib
    lib = _lib.lib()
    assert "nq_ms_ssim" in _lib.EXPORTS and "nq_ms_ssim_ws_floats" in _lib.EXPORTS
    assert lib.nq_abi_version() == 7
    p, n = ctypes.c_void_p(16), None
    assert lib.nq_ms_ssim(n, p, p, p, 1, 3, 640, 1280, n) == -1
    assert lib.nq_ms_ssim(p, n, p, p, 1, 3, 640, 1280, n) == -1
    assert lib.nq_ms_ssim(p, p, n, p, 1, 3, 640, 1280, n) == -1
    assert lib.nq_ms_ssim(p, p, p, n, 1, 3, 640, 1280, n) == -1
    assert lib.nq_ms_ssim(p, p, p, p, 0, 3, 640, 1280, n) == -1
    assert lib.nq_ms_ssim(p, p, p, p, 1, 0, 640, 1280, n) == -1
    assert lib.nq_ms_ssim(p, p, p, p, 1, 3, 160, 640, n) == -1          # the package's assert: min(H, W) > 160
    assert lib.nq_ms_ssim(p, p, p, p, 1, 3, 640, 160, n) == -1
    assert lib.nq_ms_ssim_ws_floats(1, 3, 160, 640) == 0
    # both pooled pyramids (4 scales x 2 images) + one partial sum per 8 x 118 tile of every scale's valid region
    pyr = 2 * 3 * (320 * 640 + 160 * 320 + 80 * 160 + 40 * 80)
    tiles = sum(-(-(h - 10) // 8) * -(-(w - 10) // 118) for h, w in [(640, 1280), (320, 640), (160, 320), (80, 160), (40, 80)])
    assert lib.nq_ms_ssim_ws_floats(1, 3, 640, 1280) == pyr + 3 * tiles
    assert lib.nq_ms_ssim_ws_floats(8, 3, 640, 1280) == 8 * (pyr + 3 * tiles)


def test_ops_and_utils_names():
    from neuroquant_amd import ops, utils
    with pytest.raises(RuntimeError):
        ops.ms_ssim(torch.zeros(1, 3, 161, 161), torch.zeros(1, 3, 161, 161))      # CPU tensors: no fallback
    assert callable(utils.msssim_fn_single) and callable(utils.msssim_fn_batch)
    from neuroquant_amd.methods import calibrate_network as cn
    assert cn.METRIC_NAMES == ['pred_seen_psnr', 'pred_seen_ssim', 'pred_unseen_psnr', 'pred_unseen_ssim']

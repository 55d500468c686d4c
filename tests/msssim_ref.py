"""Yardstick of the MS-SSIM tests: a restatement of pytorch_msssim.ms_ssim(X, Y, data_range=1, size_average=False) with
torch CPU ops, in float64 by default (`dtype=torch.float32` runs the same code in fp32, which gives the tests the error
that the number format alone costs).  Test code: the package does not import it.

The definition (include/nq_hip.h, nq_ms_ssim): 11-tap Gaussian window (sigma 1.5) whose taps are evaluated in float32,
separable valid filtering along H then along W per channel; cs / ssim = means of the maps; five scales with
avg_pool2d(kernel 2, stride 2, padding (h % 2, w % 2)) between them; relu, the powers (0.0448, 0.2856, 0.3001, 0.2363,
0.1333), their product, the mean over channels.  pytorch_msssim itself is not available where this project is built and
tested, so parity with the package's last bits is not pinned by anything here."""
import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window(dtype=torch.float64):
    """the package's _fspecial_gauss_1d(11, 1.5): built as a float32 tensor, then used in `dtype`."""
    coords = torch.arange(11, dtype=torch.float32) - 11 // 2
    g = torch.exp(-(coords ** 2) / (2 * 1.5 ** 2))
    return (g / g.sum()).to(dtype)


def _filter(x, g):
    """valid separable filter of (F, C, h, w), along H then along W, each channel on its own."""
    c = x.shape[1]
    x = F.conv2d(x, g.view(1, 1, -1, 1).expand(c, 1, -1, 1), groups=c)
    return F.conv2d(x, g.view(1, 1, 1, -1).expand(c, 1, 1, -1), groups=c)


def ssim_cs(X, Y, g):
    """-> (ssim, cs), each (F, C): the means of the two maps over the valid region."""
    mu1, mu2 = _filter(X, g), _filter(Y, g)
    s1 = _filter(X * X, g) - mu1 * mu1
    s2 = _filter(Y * Y, g) - mu2 * mu2
    s12 = _filter(X * Y, g) - mu1 * mu2
    cs_map = (2 * s12 + C2) / (s1 + s2 + C2)
    ssim_map = (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs_map
    return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)


def ms_ssim_f64(X, Y, dtype=torch.float64):
    """(F, C, H, W) CPU tensors -> (F,) `dtype`."""
    X, Y = X.detach().cpu().to(dtype), Y.detach().cpu().to(dtype)
    assert X.dim() == 4 and X.shape == Y.shape
    assert min(X.shape[-2:]) > (11 - 1) * 2 ** 4
    g = window(dtype)
    vals = []
    for s in range(5):
        ssim, cs = ssim_cs(X, Y, g)
        if s < 4:
            vals.append(torch.relu(cs))
            pad = (X.shape[2] % 2, X.shape[3] % 2)
            X = F.avg_pool2d(X, kernel_size=2, padding=pad)
            Y = F.avg_pool2d(Y, kernel_size=2, padding=pad)
    vals.append(torch.relu(ssim))
    v = torch.stack(vals, 0)                                              # (5, F, C)
    w = torch.tensor(WEIGHTS, dtype=dtype).view(-1, 1, 1)
    return torch.prod(v ** w, 0).mean(1)


# ---- the inputs the tests share: real frames and four ways of spoiling them ----
def bunny_frames(n=2):
    """the first n frames of tests/golden/bunny8_640x1280.npz as (n, 3, 640, 1280) float32 in [0, 1]."""
    import os
    import numpy as np
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bunny8_640x1280.npz"))
    return torch.from_numpy(z["frames"][:n].copy()).float() / 255.0


def noisy(Y, sigma, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (Y + sigma * torch.randn(Y.shape, generator=g)).clamp(0, 1)


def posterised(Y):
    return torch.round(7 * Y) / 7


def box_blurred(Y):
    """3 x 3 box blur, edges replicated."""
    c = Y.shape[1]
    k = torch.full((c, 1, 3, 3), 1.0 / 9.0)
    return F.conv2d(F.pad(Y, (1, 1, 1, 1), mode="replicate"), k, groups=c)

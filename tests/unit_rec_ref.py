"""Plain torch restatement of the unit-wise reconstruction tail: the three losses of the reference's
calib_block.LossFunction (round_loss aside), their gradient by autograd, the GELU' multiply and F.pixel_unshuffle; and the QDrop
mask from tests/qat_ref.philox4x32_10."""
import numpy as np
import torch
import torch.nn.functional as F

import qat_ref


def loss(pred, tgt, mode, p=2.0, fisher=None):
    """the reference's rec_loss (calib_block.py:63-71, quantizer.lp_loss) in the dtype of its arguments"""
    if mode == "lp":
        return (pred - tgt).abs().pow(p).sum(1).mean()
    if mode == "fisher_diag":
        return ((pred - tgt).pow(2) * fisher.pow(2)).sum(1).mean()
    a, g = (pred - tgt).abs(), fisher.abs()
    return (torch.sum(a * g, (1, 2, 3)).view(-1, 1, 1, 1) * a * g).mean() / 100


def tail(pred, tgt, mode, p=2.0, fisher=None, z=None, r=1, dtype=torch.float64):
    """-> (loss (1,), dconv = pixel_unshuffle(dL/dpred * z, r)) in `dtype`"""
    x = pred.to(dtype).requires_grad_(True)
    l = loss(x, tgt.to(dtype), mode, p, None if fisher is None else fisher.to(dtype))
    (g,) = torch.autograd.grad(l, x)
    if z is not None:
        g = g * z.to(dtype)
    return l.detach().view(1), F.pixel_unshuffle(g, r)


def qdrop_take(shape, prob, seed, step):
    """True where x takes xq: u < prob, u = (word >> 8) * 2^-24 of counter {i >> 2 low, i >> 2 high, b, step}, word i & 3"""
    B, n = shape[0], int(np.prod(shape[1:]))
    i, b = np.tile(np.arange(n, dtype=np.uint64), B), np.repeat(np.arange(B, dtype=np.uint64), n)
    q = i >> np.uint64(2)
    words = qat_ref.philox4x32_10(q & qat_ref.M32, q >> np.uint64(32), b, np.zeros_like(i) + np.uint64(step),
                                  np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))
    word = np.choose((i & np.uint64(3)).astype(np.int64), words)
    u = (word >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return torch.from_numpy((u < np.float32(prob)).reshape(shape))

"""The YUV 4:2:0 objective of include/nq_hip.h (nq_yuv420_loss) stated twice:

`loss_f64`   float64 numpy, the closed form: loss4 = (L, MSE_Y, MSE_U, MSE_V), dL/dpred, and the tanh-head form of the gradient
             with its channel sums.  The yardstick of the kernel.
`loss_torch` the same loss in torch ops (avg_pool2d for the box), in the dtype of its inputs, for autograd.

Both use yuv_ref.constants(matrix, np.float64): unrounded constants."""
import numpy as np
import torch
import torch.nn.functional as F

import yuv_ref

S_LIMITED = (219.0 / 255.0, 224.0 / 255.0)     # (sY, sC); (1, 1) in full range


def scales(full_range):
    return (1.0, 1.0) if full_range else S_LIMITED


def _box(c):
    """mean over 2 x 2 blocks of (B, H, W), row 0 first, left before right"""
    return ((c[:, 0::2, 0::2] + c[:, 0::2, 1::2]) + (c[:, 1::2, 0::2] + c[:, 1::2, 1::2])) * 0.25


def _up(c):
    return c.repeat(2, axis=1).repeat(2, axis=2)


def loss_f64(pred, tgt, matrix="bt709", full_range=False, weights=(6, 1, 1), head=False, gscale=1.0):
    """-> (loss4 (4,), grad (B, 3, H, W), db (3,) or None), all float64.  head: grad is multiplied by 0.5 (1 - (2 pred - 1)^2)
    and db holds its sums over frames and pixels."""
    k = yuv_ref.constants(matrix, np.float64)
    p, t = np.asarray(pred, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    B, _, H, W = p.shape
    wy, wu, wv = (float(w) for w in weights)
    wsum = wy + wu + wv
    sY, sC = scales(full_range)
    d = p - t
    dr, dg, db_ = d[:, 0], d[:, 1], d[:, 2]
    dy = (k["kr"] * dr + k["kg"] * dg) + k["kb"] * db_
    mu, mv = _box((db_ - dy) * k["icb"]), _box((dr - dy) * k["icr"])
    n = float(B * H * W)
    mse = np.array([((sY * dy) ** 2).sum() / n, ((sC * mu) ** 2).sum() / (n / 4), ((sC * mv) ** 2).sum() / (n / 4)])
    L = 3.0 * (wy * mse[0] + wu * mse[1] + wv * mse[2]) / wsum
    # dL/d(dy) from the luma term, dL/d(dcb), dL/d(dcr) of every pixel from its block's chroma terms (a quarter each)
    a_y = 6.0 * wy * sY * sY / (wsum * n) * dy
    a_cb = _up(6.0 * wu * sC * sC / (wsum * n) * mu)
    a_cr = _up(6.0 * wv * sC * sC / (wsum * n) * mv)
    gy = a_y - a_cb * k["icb"] - a_cr * k["icr"]            # dcb and dcr depend on dy with factor -icb, -icr
    g = np.stack([k["kr"] * gy + a_cr * k["icr"], k["kg"] * gy, k["kb"] * gy + a_cb * k["icb"]], axis=1) * gscale
    dbias = None
    if head:
        g = g * 0.5 * (1.0 - (2.0 * p - 1.0) ** 2)
        dbias = g.sum(axis=(0, 2, 3))
    return np.concatenate([[L], mse]), g, dbias


def loss_torch(pred, tgt, matrix="bt709", full_range=False, weights=(6, 1, 1)):
    """-> (L, (MSE_Y, MSE_U, MSE_V)) as torch scalars in pred's dtype; differentiable"""
    k = {n: float(v) for n, v in yuv_ref.constants(matrix, np.float64).items()}
    wy, wu, wv = (float(w) for w in weights)
    sY, sC = scales(full_range)
    d = pred - tgt
    dr, dg, db_ = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    dy = (k["kr"] * dr + k["kg"] * dg) + k["kb"] * db_
    eu = sC * F.avg_pool2d((db_ - dy) * k["icb"], 2)
    ev = sC * F.avg_pool2d((dr - dy) * k["icr"], 2)
    mse = ((sY * dy).pow(2).mean(), eu.pow(2).mean(), ev.pow(2).mean())
    return 3.0 * (wy * mse[0] + wu * mse[1] + wv * mse[2]) / (wy + wu + wv), mse


def images(B, H, W, seed):
    """pred strictly inside (0, 1) with a few values at exactly 0 and 1, tgt on the 8-bit grid (so that a uint8 cache holds it
    exactly): float32 (B, 3, H, W) each, and the uint8 codes of tgt"""
    rng = np.random.default_rng(seed)
    tgt_u8 = rng.integers(0, 256, size=(B, 3, H, W), dtype=np.uint8)
    tgt = tgt_u8.astype(np.float32) / np.float32(255)
    pred = np.clip(tgt + rng.normal(0, 0.08, size=tgt.shape).astype(np.float32), 0.02, 0.98).astype(np.float32)
    flat = pred.reshape(-1)
    pick = rng.permutation(flat.size)[:min(4, flat.size)]
    flat[pick] = np.array([0.0, 1.0, 1.0, 0.0], dtype=np.float32)[:pick.size]
    return pred, tgt, tgt_u8

"""Yardstick of the absolute-error loss tests (include/nq_hip.h: nq_lp_loss): the definition, restated plainly.

  loss   A = mean |d|^p, M = mean d^2, L = w_abs A + w_mse M, d = pred - tgt  ->  (scale L, A, M), scale dL/dpred in closed form
         (sign(0) = 0), and with head=True that gradient times 0.5 (1 - (2 pred - 1)^2) with its per-channel sums db.
         float64 by default; `dtype=torch.float32` runs the same code in fp32: what the number format alone costs.

Test code: the package does not import it."""
import torch


def loss(pred, tgt, p, w_abs, w_mse, scale=1.0, head=False, dtype=torch.float64):
    """(B, C, H, W) tensors -> (loss3, grad, db or None) as `dtype` CPU tensors"""
    X, Y = pred.detach().cpu().to(dtype), tgt.detach().cpu().to(dtype)
    d = X - Y
    A, M = d.abs().pow(p).mean(), (d * d).mean()
    grad = scale * (w_abs * p * d.abs().pow(p - 1) * d.sign() + w_mse * 2 * d) / d.numel()
    db = None
    if head:
        t = 2 * X - 1
        grad = grad * 0.5 * (1 - t * t)
        db = grad.sum((0, 2, 3))
    return torch.stack([scale * (w_abs * A + w_mse * M), A, M]), grad, db

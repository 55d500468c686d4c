"""Yardstick of the SSIM-loss tests (include/nq_hip.h: nq_ssim_loss), built on the restatement of
pytorch_msssim that the MS-SSIM tests use (tests/msssim_ref.py: window, _filter, ssim_cs), stated twice:

  loss_autograd   L = mean_b [w_mse * MSE_b + w_ssim * (1 - SSIM_b)] and dL/dX by torch autograd, in float64 by default;
                  `dtype=torch.float32` runs the same code in fp32: what the number format alone costs.
  loss_closed     the closed-form gradient of the header (P, Q, R filtered by the adjoint of the valid filter), float64.

Test code: the package does not import it."""
import torch
import torch.nn.functional as F

import msssim_ref as M


def loss_autograd(pred, tgt, w_mse, w_ssim, dtype=torch.float64):
    """(B, C, H, W) tensors -> (loss3, grad, ssim_b): loss3 = (L, mean MSE, mean SSIM) and ssim_b (B,) as `dtype` tensors,
    grad = dL/dpred (B, C, H, W) by autograd."""
    X = pred.detach().cpu().to(dtype).requires_grad_(True)
    Y = tgt.detach().cpu().to(dtype)
    ssim_b = M.ssim_cs(X, Y, M.window(dtype))[0].mean(1)
    mse_b = ((X - Y) ** 2).flatten(1).mean(1)
    L = (w_mse * mse_b + w_ssim * (1 - ssim_b)).mean()
    (grad,) = torch.autograd.grad(L, X)
    return torch.stack([L, mse_b.mean(), ssim_b.mean()]).detach(), grad, ssim_b.detach()


def _adjoint(m, g):
    """gT*: the same (symmetric) window over the map zero-extended by 10 on every side"""
    return M._filter(F.pad(m, (10, 10, 10, 10)), g)


def loss_closed(pred, tgt, w_mse, w_ssim):
    """the header's closed form in float64 -> (loss3, grad)"""
    X, Y = pred.detach().cpu().double(), tgt.detach().cpu().double()
    B, C, H, W = X.shape
    N = (H - 10) * (W - 10)
    g = M.window()
    mx, my = M._filter(X, g), M._filter(Y, g)
    sxx, syy, sxy = M._filter(X * X, g), M._filter(Y * Y, g), M._filter(X * Y, g)
    A1, A2 = 2 * mx * my + M.C1, 2 * (sxy - mx * my) + M.C2
    B1, B2 = mx * mx + my * my + M.C1, (sxx - mx * mx) + (syy - my * my) + M.C2
    S = A1 * A2 / (B1 * B2)
    P = 2 * my * (A2 - A1) / (B1 * B2) + 2 * mx * S * (1 / B2 - 1 / B1)
    Q = -S / B2
    R = 2 * A1 / (B1 * B2)
    ssim_b = S.flatten(2).mean(-1).mean(1)
    mse_b = ((X - Y) ** 2).flatten(1).mean(1)
    L = (w_mse * mse_b + w_ssim * (1 - ssim_b)).mean()
    grad = w_mse * 2 * (X - Y) / (B * C * H * W) - w_ssim / (B * C * N) * (_adjoint(P, g) + 2 * X * _adjoint(Q, g) + Y * _adjoint(R, g))
    return torch.stack([L, mse_b.mean(), ssim_b.mean()]), grad

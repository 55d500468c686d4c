"""Yardstick of the tests of nq_ssim_loss_head (include/nq_hip.h): the quantities a calibration iteration takes
from the MSE + SSIM loss behind a tanh head, built on tests/ssim_loss_ref.py (and through it tests/msssim_ref.py), stated twice:

  head_autograd   z -> p = 0.5 tanh(z) + 0.5 -> scale * L(p, tgt): loss3 = (scale L, mean MSE, mean SSIM), dL/dz by torch
                  autograd through the tanh, db[c] = the sum of dL/dz over frames and pixels.  float64.
  head_closed     from the image p itself: g_img = scale dL/dp (autograd of the restatement), g_head = g_img * 2 p (1 - p)
                  (= g_img * 0.5 (1 - (2 p - 1)^2), the tanh backward written in p), db.  float64 by default;
                  `dtype=torch.float32` runs the same code in fp32: what the number format alone costs.

Test code: the package does not import it."""
import torch

import ssim_loss_ref as SR
import msssim_ref as M


def head_autograd(z, tgt, w_mse, w_ssim, scale):
    """z, tgt (B, C, H, W) -> (loss3, dL/dz, db) in float64, everything by autograd"""
    z = z.detach().cpu().double().requires_grad_(True)
    Y = tgt.detach().cpu().double()
    p = 0.5 * torch.tanh(z) + 0.5
    ssim_b = M.ssim_cs(p, Y, M.window(torch.float64))[0].mean(1)
    mse_b = ((p - Y) ** 2).flatten(1).mean(1)
    L = scale * (w_mse * mse_b + w_ssim * (1 - ssim_b)).mean()
    (gz,) = torch.autograd.grad(L, z)
    return torch.stack([L, mse_b.mean(), ssim_b.mean()]).detach(), gz, gz.sum((0, 2, 3))


def head_closed(pred, tgt, w_mse, w_ssim, scale, dtype=torch.float64):
    """pred, tgt (B, C, H, W) -> (loss3, g_img, g_head, db, ssim_b) as `dtype` tensors: loss3 = (scale L, mean MSE, mean SSIM),
    g_img = scale dL/dpred, g_head = g_img * 2 pred (1 - pred), db = its sums over frames and pixels"""
    loss3, grad, ssim_b = SR.loss_autograd(pred, tgt, w_mse, w_ssim, dtype=dtype)
    p = pred.detach().cpu().to(dtype)
    s = torch.tensor(scale, dtype=dtype)
    g_img = s * grad
    g_head = g_img * (2 * p * (1 - p))
    return torch.stack([s * loss3[0], loss3[1], loss3[2]]), g_img, g_head, g_head.sum((0, 2, 3)), ssim_b

"""Yardstick of the MS-SSIM-loss tests (include/nq_hip.h: nq_msssim_loss), built on the restatement of
pytorch_msssim that the MS-SSIM tests use (tests/msssim_ref.py: window, _filter, ssim_cs), stated twice:

  loss_autograd   L = mean_b [w_mse * MSE_b + w_ms * (1 - MS_b)] and dL/dX by torch autograd, in float64 by default;
                  `dtype=torch.float32` runs the same code in fp32: what the number format alone costs.
  loss_closed     the closed-form gradient of the header (derivative maps per scale, the adjoint of the valid filter, the
                  adjoint `up` of the pooling), float64.

The clamp rule is explicit in both: a plane with any v_s <= 0 has M = 0 and contributes a detached zero, so 0^w never meets
autograd (which would give 0 * inf = NaN there).

Test code: the package does not import it."""
import torch
import torch.nn.functional as F

import msssim_ref as M
from ssim_loss_ref import _adjoint


def pool(X):
    """the next scale: 2 x 2 averages, divisor 4, padding (h % 2, w % 2)"""
    return F.avg_pool2d(X, kernel_size=2, padding=(X.shape[2] % 2, X.shape[3] % 2))


def scale_values(X, Y, g):
    """-> v (5, B, C): mean cs of scales 1 .. 4, mean ssim of scale 5 (differentiable)"""
    vals = []
    for s in range(5):
        ssim, cs = M.ssim_cs(X, Y, g)
        if s < 4:
            vals.append(cs)
            X, Y = pool(X), pool(Y)
    vals.append(ssim)
    return torch.stack(vals, 0)


def plane_products(v):
    """v (5, B, C) -> (M (B, C), live (B, C)): M = prod_s v_s^w_s where every v_s > 0, a detached exact zero elsewhere"""
    live = (v > 0).all(0)
    w = torch.tensor(M.WEIGHTS, dtype=v.dtype).view(-1, 1, 1)
    safe = torch.where(live.unsqueeze(0), v, torch.ones_like(v))      # the clamped planes never reach the power
    return torch.where(live, torch.prod(safe ** w, 0), torch.zeros_like(v[0])), live


def loss_autograd(pred, tgt, w_mse, w_ms, dtype=torch.float64):
    """(B, C, H, W) tensors -> (loss3, grad, ms_b, v): loss3 = (L, mean MSE, mean MS-SSIM), ms_b (B,) and v (5, B, C) as `dtype`
    tensors, grad = dL/dpred (B, C, H, W) by autograd."""
    X = pred.detach().cpu().to(dtype).requires_grad_(True)
    Y = tgt.detach().cpu().to(dtype)
    v = scale_values(X, Y, M.window(dtype))
    ms_b = plane_products(v)[0].mean(1)
    mse_b = ((X - Y) ** 2).flatten(1).mean(1)
    L = (w_mse * mse_b + w_ms * (1 - ms_b)).mean()
    (grad,) = torch.autograd.grad(L, X)
    return torch.stack([L, mse_b.mean(), ms_b.mean()]).detach(), grad, ms_b.detach(), v.detach()


def up(G, h, w):
    """the adjoint of pool() for an h x w scale: up(G)[i, j] = G[(i + h % 2) // 2, (j + w % 2) // 2] / 4"""
    i = (torch.arange(h) + h % 2) // 2
    j = (torch.arange(w) + w % 2) // 2
    return G[:, :, i][:, :, :, j] / 4


def loss_closed(pred, tgt, w_mse, w_ms):
    """the header's closed form in float64 -> (loss3, grad)"""
    X, Y = pred.detach().cpu().double(), tgt.detach().cpu().double()
    B, C, H, W = X.shape
    g = M.window()
    X1, Y1 = X, Y
    vals, units, counts = [], [], []
    for s in range(5):
        mx, my = M._filter(X, g), M._filter(Y, g)
        sxx, syy, sxy = M._filter(X * X, g), M._filter(Y * Y, g), M._filter(X * Y, g)
        A2 = 2 * (sxy - mx * my) + M.C2
        B2 = (sxx - mx * mx) + (syy - my * my) + M.C2
        cs = A2 / B2
        if s < 4:   # the luminance factor dropped
            m, P, Q, R = cs, 2 * (mx * cs - my) / B2, -cs / B2, 2 / B2
        else:       # P, Q, R of nq_ssim_loss
            A1, B1 = 2 * mx * my + M.C1, mx * mx + my * my + M.C1
            m = A1 * A2 / (B1 * B2)
            P = 2 * my * (A2 - A1) / (B1 * B2) + 2 * mx * m * (1 / B2 - 1 / B1)
            Q, R = -m / B2, 2 * A1 / (B1 * B2)
        vals.append(m.flatten(2).mean(-1))
        counts.append(m.shape[2] * m.shape[3])
        units.append(_adjoint(P, g) + 2 * X * _adjoint(Q, g) + Y * _adjoint(R, g))      # d(sum of the map) / dX_s
        if s < 4:
            X, Y = pool(X), pool(Y)
    v = torch.stack(vals, 0)
    live = (v > 0).all(0)
    w = torch.tensor(M.WEIGHTS, dtype=torch.float64)
    Mp = torch.where(live, torch.prod(torch.where(live.unsqueeze(0), v, torch.ones_like(v)) ** w.view(-1, 1, 1), 0),
                     torch.zeros_like(v[0]))
    G = None
    for s in range(4, -1, -1):
        dv = torch.where(live, -(w_ms / (B * C)) * w[s] * Mp / torch.where(live, v[s], torch.ones_like(v[s])),
                         torch.zeros_like(Mp))
        own = (dv / counts[s])[:, :, None, None] * units[s]
        G = own if G is None else own + up(G, units[s].shape[2], units[s].shape[3])
    ms_b = Mp.mean(1)
    mse_b = ((X1 - Y1) ** 2).flatten(1).mean(1)
    L = (w_mse * mse_b + w_ms * (1 - ms_b)).mean()
    grad = G + w_mse * 2 * (X1 - Y1) / (B * C * H * W)
    return torch.stack([L, mse_b.mean(), ms_b.mean()]), grad

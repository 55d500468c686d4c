"""Restatement of the level-rate definition (include/nq_hip.h above nq_level_rate) in torch: the yardstick of
tests/test_rate_cpu.py and tests/test_rate_gpu.py.  Test code, not imported by the package.

The LEVELS are taken in float32 with the kernel's expression (floor(x / delta), then (f + 0) + zp and (f + 1) + zp, clamped), so
that they are the kernel's levels; the counts are exact integers; the cost table is log2((n + K) / (c + 1)) in float64 rounded
once to float32 (the definition); R_soft, R_hard and the gradient are evaluated in `dtype`: float64 for the reference, float32
for e32, what the number format alone costs."""
import numpy as np
import torch

ZETA, GAMMA = 1.1, -0.1


def levels(x, delta, zp, K):
    """x (rows, row_len) float32, delta / zp (rows,) or (1,) float32 -> (lo, hi) int64, the kernel's float32 expressions"""
    x, d, z = x.float(), delta.float().reshape(-1, 1), zp.float().reshape(-1, 1)
    f = torch.floor(x / d)
    lo = torch.clamp((f + 0.0) + z, 0, K - 1)
    hi = torch.clamp((f + 1.0) + z, 0, K - 1)
    return lo.long(), hi.long()


def hard_levels(x, alpha, delta, zp, K):
    lo, hi = levels(x, delta, zp, K)
    return torch.where(alpha >= 0, hi, lo)


def cost_table(counts, n, K):
    """-> (float64 values, the float32 table)"""
    c64 = torch.log2((float(n) + float(K)) / (counts.double() + 1.0))
    return c64, c64.float()


def soft_parts(alpha, dtype):
    """h and h' in `dtype` (the expressions of nq_adaround_backward) and lin = 1.2 sigmoid(alpha) - 0.1"""
    s = torch.sigmoid(alpha.to(dtype))
    lin = s * (ZETA - GAMMA) + GAMMA
    h = lin.clamp(0, 1)
    hp = torch.where((lin >= 0) & (lin <= 1), (ZETA - GAMMA) * (s * (1 - s)), torch.zeros_like(s))
    return h, hp, lin


def rate(x, alpha, delta, zp, K, scale=1.0, gate=1.0, dtype=torch.float64):
    """-> dict(counts int64 (K,), cost float32 (K,), cost64, r_soft, r_hard (0-d `dtype`), grad (`dtype`, shaped like alpha))"""
    lo, hi = levels(x, delta, zp, K)
    lv = torch.where(alpha >= 0, hi, lo)
    counts = torch.bincount(lv.flatten(), minlength=K)
    cost64, cost32 = cost_table(counts, x.numel(), K)
    cost = cost32.to(dtype)
    h, hp, _ = soft_parts(alpha, dtype)
    r_soft = ((1 - h) * cost[lo] + h * cost[hi]).sum()
    r_hard = (counts.to(dtype) * cost).sum()
    g = torch.as_tensor(gate, dtype=dtype) * torch.as_tensor(scale, dtype=dtype)
    grad = (g * (cost[hi] - cost[lo])) * hp
    return dict(counts=counts, cost=cost32, cost64=cost64, r_soft=r_soft, r_hard=r_hard, grad=grad)


def rate_autograd(x, alpha, delta, zp, K, scale=1.0):
    """float64 autograd of scale * R_soft w.r.t. alpha with the table detached -> (r_soft, grad)"""
    lo, hi = levels(x, delta, zp, K)
    counts = torch.bincount(torch.where(alpha >= 0, hi, lo).flatten(), minlength=K)
    cost = cost_table(counts, x.numel(), K)[1].double().detach()
    a = alpha.double().clone().requires_grad_(True)
    h = (torch.sigmoid(a) * (ZETA - GAMMA) + GAMMA).clamp(0, 1)
    r = ((1 - h) * cost[lo] + h * cost[hi]).sum()
    (g,) = torch.autograd.grad(r * scale, a)
    return r.detach(), g


def entropy_bits(lv, K):
    """the zeroth-order entropy of the levels in bits (export._entropy_bits)"""
    hist = torch.bincount(lv.flatten().long(), minlength=K).double()
    p = hist[hist > 0] / hist.sum()
    return float(-(p * torch.log2(p)).sum() * lv.numel())


def make_tensor(rows, row_len, K, per_row, seed, kind="generic"):
    """-> dict(x, alpha, delta, zp, K, per_row) float32 CPU tensors.  kind 'generic': x / delta at least 0.05 away from an integer
    and spread past both ends of the grid, alpha with 1.2 sigmoid - 0.1 at least 1e-4 away from 0 and 1 on either side of both;
    the explicit edge cases are 'one_level', 'clamped', 'alpha_zero', 'alpha_30'."""
    g = torch.Generator().manual_seed(seed)
    ns = rows if per_row else 1
    delta = (0.01 + 0.05 * torch.rand(ns, generator=g)).float()
    zp = torch.randint(0, K, (ns,), generator=g).float()
    zc = zp.reshape(-1, 1)
    n = rows * row_len
    if kind == "one_level":
        u = torch.full((rows, row_len), 1.5) - zc + float(K // 2)             # f + zp = K / 2 + 1 everywhere
    elif kind == "clamped":
        below = torch.rand(rows, row_len, generator=g) < 0.5
        u = torch.where(below, -zc - 7.5, float(K) - zc + 6.5) + torch.zeros(rows, row_len)
    else:
        span = K + 4
        u = torch.randint(0, span, (rows, row_len), generator=g).float() - 2.0 - zc + 0.05 + 0.9 * torch.rand(rows, row_len, generator=g)
    x = (u * delta.reshape(-1, 1)).float()
    if kind == "alpha_zero":
        alpha = torch.zeros(rows, row_len)
    elif kind == "alpha_30":
        alpha = torch.where(torch.rand(rows, row_len, generator=g) < 0.5, -30.0, 30.0) + torch.zeros(rows, row_len)
    elif kind == "one_level":
        alpha = 0.2 + 2.0 * torch.rand(rows, row_len, generator=g)
    else:
        inner = -2.3 + 4.6 * torch.rand(rows, row_len, generator=g)
        outer = (2.6 + 3.4 * torch.rand(rows, row_len, generator=g)) * torch.where(torch.rand(rows, row_len, generator=g) < 0.5, -1.0, 1.0)
        alpha = torch.where(torch.rand(rows, row_len, generator=g) < 0.7, inner, outer)
    return dict(x=x.contiguous(), alpha=alpha.float().contiguous(), delta=delta, zp=zp, K=K, per_row=int(per_row), kind=kind)


def margins(t):
    """(distance of x / delta from the nearest integer, distance of 1.2 sigmoid(alpha) - 0.1 from {0, 1}) in float64: what the
    generated cases keep away from the discontinuities"""
    u = t["x"].double() / t["delta"].double().reshape(-1, 1)
    du = float((u - u.round()).abs().min())
    lin = soft_parts(t["alpha"], torch.float64)[2]
    dl = float(torch.minimum(lin.abs(), (lin - 1).abs()).min())
    return du, dl


def seq_sum_f32(values):
    """((0 + v_0) + v_1) + ... in float32: the totals of nq_level_rate"""
    s = np.float32(0.0)
    for v in values:
        s = np.float32(s + np.float32(v))
    return float(s)

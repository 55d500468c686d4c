"""The ConvNeXt block (include/nq_hip.h: nq_convnext_block_forward) as plain torch ops.  In float64 with autograd it is the
reference of tests/test_convnext_gpu.py, in float32 on the CPU the yardstick of its bound."""
import torch
import torch.nn.functional as F

SHAPES = dict(dw_w=lambda C: (C, 1, 7, 7), dw_b=lambda C: (C,), ln_w=lambda C: (C,), ln_b=lambda C: (C,), w1=lambda C: (4 * C, C),
              b1=lambda C: (4 * C,), w2=lambda C: (C, 4 * C), b2=lambda C: (C,), gamma=lambda C: (C,))


def block(x, dw_w, dw_b, ln_w, ln_b, w1, b1, w2, b2, gamma, dtype=torch.float64):
    x, dw_w, dw_b, ln_w, ln_b, w1, b1, w2, b2, gamma = (t.to(dtype) for t in (x, dw_w, dw_b, ln_w, ln_b, w1, b1, w2, b2, gamma))
    C = x.shape[1]
    u = F.conv2d(x, dw_w, dw_b, padding=3, groups=C).permute(0, 2, 3, 1)
    a = F.layer_norm(u, (C,), ln_w, ln_b, 1e-6)
    m = F.linear(F.gelu(F.linear(a, w1, b1)), w2, b2)
    return x + (gamma * m).permute(0, 3, 1, 2)


def inputs(shape, seed, init=False):
    """x, the nine parameters and an upstream gradient, fp32 on the CPU.  Parameters of order one (a wrong MLP would hide under
    the residual at the module's init), or with init=True exactly that init: gamma 1e-6, weights of std 0.02, zero biases."""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    p = {k: torch.randn(s(C), generator=g) for k, s in SHAPES.items()}
    if init:
        p = {k: v * 0.02 if k in ("dw_w", "w1", "w2") else torch.zeros_like(v) for k, v in p.items()}
        p["ln_w"], p["gamma"] = torch.ones(C), torch.full((C,), 1e-6)
    else:
        p["dw_w"], p["w1"], p["w2"] = p["dw_w"] / 7.0, p["w1"] / C ** 0.5, p["w2"] / (4 * C) ** 0.5   # outputs of order one
    return torch.randn(N, C, H, W, generator=g), [p[k] for k in SHAPES], torch.randn(N, C, H, W, generator=g)


def out_and_grads(tensors, dy, dtype):
    """[out, dx, nine parameter gradients] of block() in `dtype` on the CPU"""
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in tensors]
    out = block(*leaves, dtype=dtype)
    return [out.detach()] + list(torch.autograd.grad(out, leaves, dy.to(dtype)))


def within_bound(name, got, ref64, ref32):
    """the project's bound: max|T_hip - T_64| <= 4 max|T_32 - T_64| + 8 eps_fp32 max|T_64|; prints the seen
    fraction of it"""
    err = float((got.double().cpu() - ref64).abs().max())
    bound = 4.0 * float((ref32.double() - ref64).abs().max()) + 8.0 * torch.finfo(torch.float32).eps * float(ref64.abs().max())
    print(f"{name}: |hip - f64| {err:.3e}, bound {bound:.3e}, fraction {err / bound if bound else float('inf'):.3f}")
    return err <= bound

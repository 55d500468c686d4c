"""A downsampling stage of the HNeRV encoder (include/nq_hip.h: nq_patchify_ln_forward) as plain torch ops.  In float64 with
autograd it is the reference of tests/test_patchify_gpu.py, in float32 on the CPU the yardstick of its bound
(convnext_ref.within_bound)."""
import torch
import torch.nn.functional as F

NAMES = ["out", "dx", "d_conv_w", "d_conv_b", "d_ln_w", "d_ln_b"]


def ln_cf(x, w, b, eps=1e-6):
    """models/_layers.py LayerNorm.forward, channels_first"""
    u = x.mean(1, keepdim=True)
    s = (x - u).pow(2).mean(1, keepdim=True)
    return w[:, None, None] * ((x - u) / torch.sqrt(s + eps)) + b[:, None, None]


def stage(x, conv_w, conv_b, ln_w, ln_b, order):
    s = conv_w.shape[-1]
    if order == "post":
        return ln_cf(F.conv2d(x, conv_w, conv_b, stride=s), ln_w, ln_b)
    return F.conv2d(ln_cf(x, ln_w, ln_b), conv_w, conv_b, stride=s)


def inputs(shape, order, seed):
    """x, [conv_w, conv_b, ln_w, ln_b] and an upstream gradient, fp32 on the CPU: parameters of order one, conv_w scaled so that
    the outputs are of order one"""
    N, Cin, H, W, Cout, s = shape
    g = torch.Generator().manual_seed(seed)
    Cl = Cout if order == "post" else Cin
    params = [torch.randn(Cout, Cin, s, s, generator=g) / (Cin * s * s) ** 0.5, torch.randn(Cout, generator=g),
              torch.randn(Cl, generator=g), torch.randn(Cl, generator=g)]
    return torch.randn(N, Cin, H, W, generator=g), params, torch.randn(N, Cout, H // s, W // s, generator=g)


def out_and_grads(tensors, dy, order, dtype):
    """[out, dx, d conv_w, d conv_b, d ln_w, d ln_b] of stage() in `dtype` on the CPU"""
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in tensors]
    out = stage(*leaves, order)
    return [out.detach()] + list(torch.autograd.grad(out, leaves, dy.to(dtype)))

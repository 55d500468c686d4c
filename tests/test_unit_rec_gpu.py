"""Unit-wise reconstruction on the GPU: ops.unit_rec_loss and ops.qdrop_mix against the float64 restatement
(tests/unit_rec_ref.py).  Bounds: _bound of test_lp_loss_gpu.py, e32 the error of the SAME restatement run in float32:
    |loss - ref| <= 4 e32 + 8 * 2^-24 |ref|,   max|dconv - ref| <= 4 e32_dconv + 8 * 2^-24 max|dconv_ref|
Worst observed error / bound per case is printed (run with -s) and recorded in DESIGN.md §33."""
import functools

import pytest
import torch
import torch.nn.functional as F

import unit_rec_ref as UR
from test_lp_loss_gpu import _bound

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = [("lp", 2.0), ("lp", 1.0), ("lp", 2.4), ("fisher_diag", 2.0), ("fisher_full", 2.0)]
# (B, C, H, W, r) of the conv output: odd widths, rows longer than a tile, several bands, every r; the last four take the 16-byte forms
SHAPES = [(1, 1, 1, 1, 2), (2, 3, 5, 7, 1), (2, 3, 5, 7, 2), (2, 3, 5, 7, 3), (1, 2, 3, 5, 4), (1, 2, 2, 3, 5), (2, 5, 3, 67, 2),
          (1, 1, 40, 9, 2), (2, 2, 3, 260, 2), (1, 1, 2, 260, 5), (1, 1, 2, 12, 3), (1, 2, 5, 1032, 1)]


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """-> pred, cache of 3 targets, cache of Fisher weights |g| + 1, idx, z on the CPU; a tenth of pred exactly equal to its target"""
    B, C, H, W, r = shape
    full = (B, C, H * r, W * r)
    g = torch.Generator().manual_seed(sum(shape) + 31 * r)
    cache = torch.randn((3,) + full[1:], generator=g)
    fisher = torch.randn((3,) + full[1:], generator=g).abs() + 1
    idx = torch.tensor([2, 0][:B])
    equal = torch.rand(full, generator=g) < 0.1
    pred = torch.where(equal, cache[idx], torch.randn(full, generator=g))
    return pred, cache, fisher, idx, torch.rand(full, generator=g) * 1.2 - 0.1


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode,p", MODES)
def test_kernel_against_float64(mode, p, shape):
    from neuroquant_amd import _lib as L, ops
    r = shape[4]
    pred, cache, fisher, idx, z = _inputs(shape)
    tgt, fsh = cache[idx], fisher[idx] if mode != "lp" else None
    x, worst = pred.to(DEV), {}
    for with_z in (False, True):
        r64, r32 = (UR.tail(pred, tgt, mode, p, fsh, z if with_z else None, r, dt) for dt in (torch.float64, torch.float32))
        zd = z.to(DEV) if with_z else None
        plain, again = (ops.unit_rec_loss(x, tgt.to(DEV), mode, p, fisher=None if fsh is None else fsh.to(DEV), z=zd, r=r) for _ in "ab")
        cached = ops.unit_rec_loss(x, cache.to(DEV), mode, p, fisher=fisher.to(DEV), z=zd, r=r, idx=idx.to(DEV))
        assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(plain, again, cached))   # a second call, and from the cache
        loss, dconv = plain
        assert dconv.shape == r64[1].shape
        worst[with_z] = (_bound(loss, r64[0], r32[0]), _bound(dconv, r64[1], r32[1], float(r64[1].abs().max())))
        zero = F.pixel_unshuffle((pred == tgt).float(), r).bool()
        assert bool((dconv.cpu()[zero] == 0).all())                       # pred == tgt: exactly 0
        if (mode, p) == ("lp", 2.0):   # nq_ps_gelu_backward of nq_lp_loss's image-mode gradient, bit for bit
            g = ops.lp_loss_raw(x, tgt=tgt.to(DEV), p=2.0, scale=float(shape[1]))[1]
            zz, chain = (zd if with_z else torch.ones_like(x)), torch.empty_like(dconv)
            L.check(L.lib().nq_ps_gelu_backward(ops._p(g), ops._p(zz), ops._p(chain), shape[0], shape[1], shape[2], shape[3], r,
                                                ops._stream()))
            assert torch.equal(chain, dconv)
    print(f"unit_rec {mode} p={p} {shape}: (loss, dconv) error / bound without z {worst[False]}, with z {worst[True]}")
    assert max(max(w) for w in worst.values()) <= 1.0, worst


@pytest.mark.parametrize("elems", [(2, 3, 7), (4, 33, 65)])
def test_qdrop_mix(elems):
    from neuroquant_amd import ops
    g = torch.Generator().manual_seed(5)
    xq, xfp = torch.rand((5,) + elems, generator=g) + 0.5, -torch.rand((5,) + elems, generator=g) - 0.5   # no value in both
    idx = torch.tensor([4, 0, 4])
    q, f, i = xq.to(DEV), xfp.to(DEV), idx.to(DEV)
    seed, step = 0x1234567890ABCDEF, 7
    x, take = ops.qdrop_mix(q, f, i, 0.5, seed, step).cpu(), UR.qdrop_take((3,) + elems, 0.5, seed, step)
    assert torch.equal(x, torch.where(take, xq[idx], xfp[idx])) and 0.4 < float(take.float().mean()) < 0.6
    assert bool(((x == xq[idx]) ^ (x == xfp[idx])).all())                 # every element from exactly one source
    assert torch.equal(ops.qdrop_mix(q, f, i, 0.5, seed, torch.tensor([step], dtype=torch.int32, device=DEV)).cpu(), x)
    assert not torch.equal(ops.qdrop_mix(q, f, i, 0.5, seed, step + 1).cpu(), x)
    assert torch.equal(ops.qdrop_mix(q, None, i, 1.0).cpu(), xq[idx]) and torch.equal(ops.qdrop_mix(q, f, i, 0.0).cpu(), xfp[idx])


@pytest.mark.parametrize("cin,cout,k,r", [(4, 12, 3, 2), (5, 4, 1, 1)])
def test_unit_step_against_autograd(cin, cout, k, r):
    """d(alpha) of weight and bias of one block_reconstruction iteration (calib_unit.UnitStep: AdaRound forward, convolution, the
    tail, weight gradient, AdaRound backward) against autograd of the restated unit: a block with PixelShuffle + GELU, a bare layer"""
    from types import SimpleNamespace as NS
    from neuroquant_amd.quantization import QuantModule, QuantNeRVBlock, calib_unit
    from oracle import nq_oracle as O
    torch.manual_seed(k)
    conv, qp = torch.nn.Conv2d(cin, cout, k, padding=k // 2), dict(n_bits=4, channel_wise=True, scale_method="max")
    unit = (QuantNeRVBlock(NS(conv=[conv, torch.nn.PixelShuffle(r)], act=torch.nn.GELU()), False, qp) if r > 1
            else QuantModule(conv, False, qp)).to(DEV)
    m = calib_unit.prepare_unit(NS(set_quant_state=lambda s: None), unit)
    inps, outs, idx = torch.randn(3, cin, 6, 9), torch.randn(3, cout // r ** 2, 6 * r, 9 * r), torch.tensor([2, 0])
    got = calib_unit.UnitStep(unit, inps.to(DEV), None, outs.to(DEV), None, "mse", 2.0, 1.0).gradients(idx.to(DEV))

    def ref(dt):
        qs = [(q.alpha.detach().cpu().to(dt).requires_grad_(True), q.delta.detach().cpu().to(dt), q.zero_point.cpu().to(dt), q.n_levels)
              for q in (m.weight_quantizer, m.bias_quantizer)]
        W, b = (O.adaround_fake_quant(x.detach().cpu().to(dt), *q, True)[0] for x, q in zip((m.weight, m.bias), qs))
        y = F.conv2d(inps[idx].to(dt), W, b, padding=k // 2)
        loss = UR.loss(F.gelu(F.pixel_shuffle(y, r)) if r > 1 else y, outs[idx].to(dt), "lp", 2.0)
        return (loss.detach().view(1),) + torch.autograd.grad(loss, [qs[0][0], qs[1][0]])
    r64, r32 = ref(torch.float64), ref(torch.float32)
    worst = [_bound(got[0], r64[0], r32[0])] + [_bound(a, b, c, float(b.abs().max())) for a, b, c in zip(got[1:], r64[1:], r32[1:])]
    print(f"unit step {cin}->{cout} k={k} r={r}: (loss, d alpha_w, d alpha_b) error / bound {worst}")
    assert max(worst) <= 1.0, worst

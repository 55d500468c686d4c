"""The absolute-error loss on the GPU: nq_lp_loss through ops.lp_loss_raw against the float64 restatement
(tests/lp_loss_ref.py), then the layers above it: the L1 term behind the SSIM and MS-SSIM losses, and the calibration engine.

Bounds (the convention of test_ssim_loss_gpu.py).  e32 is the error of the SAME restatement run in float32 on the same inputs:
    |loss3 - ref| <= 4 e32 + 8 * 2^-24 |ref|                     per entry
    max|grad - ref| <= 4 e32_grad + 8 * 2^-24 max|grad_ref|
    |db_c - ref| <= 4 e32_db + 8 * 2^-24 sum_{b,h,w} |grad_ref|   (every term of the sum carries its own rounding)
Worst observed error / bound per case is printed (run with -s) and recorded in DESIGN.md §32."""
import functools

import numpy as np
import pytest
import torch

import lp_loss_ref as LR
import msssim_loss_ref as MR
import ssim_loss_ref as SR
from conftest import BITS, T, TINY_HNERV, state_dict_from_npz

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULPS = 8 * 2.0 ** -24
K = 4096                                  # ops.LP_LOSS_CHUNK, asserted below
# H*W (odd: every plane after the first starts misaligned), p, (w_abs, w_mse), head mode, target from the uint8 cache
CASES = [(1, 1.0, (1.0, 0.0), False, False), (3, 1.5, (0.3, 0.7), True, True),
         (K - 1, 1.0, (0.3, 0.7), True, False), (K - 1, 3.5, (1.0, 0.0), False, True),
         (K + 5, 1.0, (1.0, 0.0), True, True), (K + 5, 1.5, (1.0, 0.0), True, False),
         (2 * K + 3, 3.5, (0.3, 0.7), True, False), (2 * K + 3, 1.0, (0.3, 0.7), False, True),
         (2 * K + 3, 1.5, (0.3, 0.7), False, False), (0, 1.0, (1.0, 0.0), True, False)]   # 0: the (1, 1, 1, 1) image


@functools.lru_cache(maxsize=None)
def _inputs(hw, cached):
    """-> (pred, tgt, cache or None, idx or None, equal mask) on the CPU: values in (0, 1), a tenth of pred exactly equal to tgt"""
    shape = (2, 3, 1, hw) if hw else (1, 1, 1, 1)
    g = torch.Generator().manual_seed(7 * hw + cached)
    cache = idx = None
    if cached:
        cache = torch.randint(0, 256, (3,) + shape[1:], generator=g, dtype=torch.uint8)
        idx = torch.tensor([1, 1])
        tgt = cache[idx].float() / 255.0                    # k / 255 as the kernel computes it
    else:
        tgt = torch.rand(shape, generator=g) * 0.98 + 0.01
    equal = torch.rand(shape, generator=g) < 0.1
    pred = torch.where(equal, tgt, torch.rand(shape, generator=g) * 0.98 + 0.01)
    return pred, tgt, cache, idx, equal | (pred == tgt)


def _bound(got, r64, r32, scale=None):
    """-> worst |got - r64| / bound with bound = 4 e32 + ULPS * scale: per entry with e32 = |r32 - r64| and scale |r64| (or the
    per-entry `scale` array); for a float `scale` (a gradient) over the whole tensor, e32 = max |r32 - r64|"""
    r64 = r64.double().numpy()
    e32 = np.abs(r32.double().numpy() - r64)
    err = np.abs(got.double().cpu().numpy() - r64)
    if isinstance(scale, float):
        return float(err.max() / (4 * e32.max() + ULPS * scale))
    return float((err / np.maximum(4 * e32 + ULPS * (np.abs(r64) if scale is None else scale), 1e-300)).max())


@pytest.mark.parametrize("hw,p,weights,head,cached", CASES)
def test_kernel_against_float64(hw, p, weights, head, cached):
    from neuroquant_amd import _lib as L, ops
    assert ops.LP_LOSS_CHUNK == K
    pred, tgt, cache, idx, equal = _inputs(hw, cached)
    C, scale = pred.shape[1], 3.0
    target = dict(cache_u8=cache.to(DEV), idx=idx.to(DEV)) if cached else dict(tgt=tgt.to(DEV))
    kw = dict(p=p, w_abs=weights[0], w_mse=weights[1], scale=scale)
    r64, r32 = (LR.loss(pred, tgt, p, *weights, scale=scale, head=head, dtype=dt) for dt in (torch.float64, torch.float32))
    x = pred.to(DEV)
    before = ops.lp_loss_launches
    loss3, grad, db = ops.lp_loss_raw(x, **target, **kw, head=head)
    assert ops.lp_loss_launches == before + 1 and (db is None) == (not head)
    present = [0] + [i for i, w in ((1, weights[0]), (2, weights[1])) if w > 0]
    worst = dict(loss=_bound(loss3[present], r64[0][present], r32[0][present]),
                 grad=_bound(grad, r64[1], r32[1], float(r64[1].abs().max())))
    assert all(float(loss3[i]) == 0.0 for i in (1, 2) if i not in present)          # an absent term is not computed: it reads 0
    if head:
        worst["db"] = _bound(db, r64[2], r32[2], r64[1].abs().sum((0, 2, 3)).numpy())
    print(f"lp_loss hw={hw} p={p} w={weights} head={head} cached={cached}: error / bound {worst}")
    assert max(worst.values()) <= 1.0, worst
    assert bool((grad.cpu()[equal] == 0).all()) and (hw < 16 or bool(equal.any()))   # pred == tgt: exactly 0
    # bit-identical from call to call; forward only gives the same loss bits
    again = ops.lp_loss_raw(x, **target, **kw, head=head)
    assert all(torch.equal(a, b) for a, b in zip((loss3, grad) + ((db,) if head else ()), again))
    assert torch.equal(ops.lp_loss_raw(x, **target, **kw, want_grad=False)[0], loss3)
    if head:   # the head mode is nq_tanh_out_backward of the image mode's result, bit for bit
        img_grad, dconv = ops.lp_loss_raw(x, **target, **kw)[1], torch.empty_like(x)
        L.check(L.lib().nq_tanh_out_backward(ops._p(img_grad), ops._p(x), ops._p(dconv), x.numel(), ops._stream()))
        assert torch.equal(dconv, grad)
    # accumulate: one more rounding on top of what is there, and loss3[1:] left alone
    g = torch.Generator().manual_seed(3)
    filled = [torch.randn(3, generator=g).to(DEV), (torch.randn(pred.shape, generator=g) * 1e-4).to(DEV),
              torch.randn(C, generator=g).to(DEV) if head else None]
    into = tuple(None if t is None else t.clone() for t in filled)
    assert ops.lp_loss_raw(x, **target, **kw, into=into)[0] is into[0]
    assert torch.equal(into[0], torch.cat([filled[0][:1] + loss3[:1], filled[0][1:]])) and torch.equal(into[1], filled[1] + grad)
    assert not head or torch.equal(into[2], filled[2] + db)


@pytest.mark.parametrize("name,shape", [("Fusion6", (2, 3, 8 + 11, 118 + 11)), ("Fusion10", (1, 3, 161, 161))])
def test_l1_term_behind_ssim_and_msssim(name, shape):
    """0.7 L1 + 0.3 (1 - SSIM) resp. (1 - MS-SSIM) with its gradient, from the float64 helpers of those losses plus the L1 restatement;
    w_l1 = 0 is what it always was, bit for bit, and launches no nq_lp_loss"""
    from neuroquant_amd import ops
    fn, ref = (ops.ssim_loss, SR.loss_autograd) if name == "Fusion6" else (ops.ms_ssim_loss, MR.loss_autograd)
    g = torch.Generator().manual_seed(11)
    tgt = torch.rand(shape, generator=g)
    pred = (tgt + 0.05 * torch.randn(shape, generator=g)).clamp(0.0, 1.0)
    r = {dt: (ref(pred, tgt, 0.0, 0.3, dtype=dt)[:2], LR.loss(pred, tgt, 1.0, 0.7, 0.0, dtype=dt)[:2]) for dt in (torch.float64, torch.float32)}
    l64, l32 = (r[dt][0][0][0] + r[dt][1][0][0] for dt in r)
    g64, g32 = (r[dt][0][1] + r[dt][1][1] for dt in r)
    q, t = pred.to(DEV).requires_grad_(True), tgt.to(DEV)
    before = ops.lp_loss_launches
    base = fn(q, t, 0.0, 0.3)
    zero = fn(q, t, 0.0, 0.3, w_l1=0.0)
    assert torch.equal(base, zero) and torch.equal(*(torch.autograd.grad(v, q)[0] for v in (base, zero)))
    assert ops.lp_loss_launches == before
    loss = fn(q, t, 0.0, 0.3, w_l1=0.7)
    (grad,) = torch.autograd.grad(loss, q)
    assert ops.lp_loss_launches == before + 1
    worst = dict(loss=_bound(loss.detach().view(1), l64.view(1), l32.view(1)), grad=_bound(grad, g64, g32, float(g64.abs().max())))
    print(f"{name} {shape}: error / bound {worst}")
    assert max(worst.values()) <= 1.0, worst


def test_calibration_on_norm_p_1(golden):
    """4 iterations (two of each phase) of model_reconstruction(p=1) on the tiny HNeRV: every logged loss is lp_loss(p=1) =
    C * mean |out - img| of the frames the decoder produced, in float64; p = 2 launches no nq_lp_loss"""
    from neuroquant_amd import ops
    from neuroquant_amd.models import HNeRV
    from neuroquant_amd.quantization import QuantModel, model_reconstruction
    z = golden("traj_hnerv.npz")
    emb = T(z["emb"]).to(DEV)
    frames = (T(golden("frames_320x640.npz")["frames"]).float() / 255.0).to(DEV)
    batches = [dict(img=frames[i:i + 2], idx=torch.arange(i, i + 2), norm_idx=torch.arange(i, i + 2).float() / 8) for i in (0, 2)]
    seen = []

    def run(p):
        model = HNeRV(TINY_HNERV)
        model.load_state_dict(state_dict_from_npz(z, "sd:"))
        qnn = QuantModel(model.to(DEV).eval(), hadamard=False, weight_quant_params=dict(n_bits=8, channel_wise=True, scale_method="max"))
        qnn.set_bitwidth(BITS)
        qnn.eval()
        qnn.set_quant_state(True)
        with torch.no_grad():
            qnn(emb[:2])

        def probe(phase, layers, grads):   # the engine's weights are still in place: the frames of this iteration once more
            b = batches[len(seen) % 2]
            with torch.no_grad():
                out = qnn(emb[b["idx"].to(DEV)])[0]
            seen.append([LR.loss(out, b["img"], 1.0, 1.0, 0.0, scale=3.0, dtype=dt)[0][:1] for dt in (torch.float64, torch.float32)])

        rec, before = [], ops.lp_loss_launches
        model_reconstruction(qnn, cali_data=emb, gt=batches, arch="hnerv", batch_size=2, iters=40, weight=0.01, hadamard=False,
                             b_range=(20, 2), warmup=0.2, lr=0.003, recorder=rec, max_steps=4, probe=probe, p=p)
        return rec, ops.lp_loss_launches - before

    rec, launches = run(1.0)
    assert len(rec) == 4 and launches == 4 and len(seen) == 4
    for (total, round_loss, _, _), (r64, r32) in zip(rec, seen):
        assert round_loss == 0.0 and _bound(torch.tensor([total], dtype=torch.float64), r64, r32) <= 1.0, (total, float(r64))
    assert run(2.0)[1] == 0

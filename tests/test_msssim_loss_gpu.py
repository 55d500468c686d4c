"""The MS-SSIM training loss on the GPU: nq_msssim_loss against the float64 restatement
(tests/msssim_loss_ref.py), then the layers above it: ops, autograd, the hand-over into a calibration iteration, the trainer's
step and the calibration driver.

Bounds.  e32 is the error of the SAME restatement run in float32 against float64 on the same inputs: what the number format
alone costs.  The kernel is held to 4 * e32 (the project's convention for "same format, other summation order") plus
8 * 2^-24 of the value's scale (a few fp32 ulps, so a lucky restatement cannot make the bound zero):
    |loss3 - ref| <= 4 e32 + 8 * 2^-24 |ref|                     per entry
    max|grad - ref| <= 4 e32_grad + 8 * 2^-24 max|grad_ref|
Worst observed error / bound per shape is printed (run with -s) and recorded in DESIGN.md §22."""
import ctypes
import functools
import logging
import os

import numpy as np
import pytest
import torch

import msssim_loss_ref as MR
import msssim_ref as M
from conftest import BITS, T, TINY_HNERV, state_dict_from_npz

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULPS = 8 * 2.0 ** -24
WEIGHTS = ((0.0, 1.0), (1.0, 0.0), (0.3, 0.7), (0.7, 0.3))
SENTINEL = -77.25
SHAPES = [(1, 1, 161, 161),          # scale 5 is 11 x 11, one valid pixel; every scale pads
          (2, 3, 161, 176),          # odd height, even width
          (1, 3, 162, 175),          # 162 -> 81 -> 41 -> 21 -> 11 and 175 -> 88 -> 44 -> 22 -> 11: the padding differs per scale and axis
          (2, 3, 176, 300),          # scale 1 spans several 8 x 118 tiles both ways; scale 2 crosses one tile edge
          (1, 3, 340, 161)]          # tall and narrow
CLAMP_ALL, CLAMP_SOME = (1, 3, 162, 175), (2, 3, 161, 176)


@functools.lru_cache(maxsize=None)
def _frames():
    return M.bunny_frames(2)


def _crop(shape):
    """the real frames' pixels from (301, 517) on, the first C channels"""
    B, C, H, W = shape
    return _frames()[:B, :C, 301:301 + H, 517:517 + W].contiguous()


@functools.lru_cache(maxsize=None)
def _cases(shape):
    """-> [(name, pred, tgt)] float32 CPU tensors; in float64 every v_s of every plane is >= 0.12 (no plane near the clamp)"""
    B, C, H, W = shape
    crop = _crop(shape)
    rnd = torch.rand(shape, generator=torch.Generator().manual_seed(1000 * H + W + B))
    return [("noisy0.02", M.noisy(crop, 0.02), crop), ("noisy0.2", M.noisy(crop, 0.2), crop),
            ("posterised", M.posterised(crop), crop), ("box_blurred", M.box_blurred(crop), crop),
            ("random", M.noisy(rnd, 0.1), rnd)]


@functools.lru_cache(maxsize=None)
def _uniform(shape):
    """two independent uniform images: the clamp cases (CLAMP_ALL: every plane clamped; CLAMP_SOME: planes 0 and 1 of frame 0)"""
    g = torch.Generator().manual_seed(1000 * shape[2] + shape[3])
    return torch.rand(shape, generator=g), torch.rand(shape, generator=g)


def _inputs(shape, name):
    return _uniform(shape) if name == "uniform" else next((p, t) for n, p, t in _cases(shape) if n == name)


@functools.lru_cache(maxsize=None)
def _reference(shape, name, weights):
    """-> (ref3, ref_grad, bound3, bound_grad, ms_b, live, min v_s) as float64 / bool numpy: computed once, shared, never written to"""
    pred, tgt = _inputs(shape, name)
    l64, g64, ms64, v64 = MR.loss_autograd(pred, tgt, *weights)
    l32, g32, _, v32 = MR.loss_autograd(pred, tgt, *weights, dtype=torch.float32)
    live = (v64 > 0).all(0)
    assert torch.equal(live, (v32 > 0).all(0)) and float(v64.abs().min()) > 1e-4        # no plane in fp32 doubt about the clamp
    l64, g64 = l64.numpy(), g64.numpy()
    e3 = np.abs(l32.double().numpy() - l64)
    eg = float(np.abs(g32.double().numpy() - g64).max())
    out = (l64, g64, 4 * e3 + ULPS * np.abs(l64), 4 * eg + ULPS * float(np.abs(g64).max()), ms64.numpy(), live.numpy(),
           float(v64.min()))
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _guarded(n):
    g = 4
    buf = torch.full((n + 2 * g,), SENTINEL, device=DEV, dtype=torch.float32)
    return buf, buf[g:g + n]


def _intact(buf, view):
    g = (buf.numel() - view.numel()) // 2
    return bool((buf[:g] == SENTINEL).all()) and bool((buf[g + view.numel():] == SENTINEL).all())


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _run(pred, tgt, weights, want_grad=True, scale=1.0):
    """one nq_msssim_loss call on guarded buffers -> (loss3, grad or None, per-frame MS-SSIM) as tensors on the GPU"""
    from neuroquant_amd import _lib as L
    lib = L.lib()
    B, C, H, W = pred.shape
    pred, tgt = pred.to(DEV).contiguous(), tgt.to(DEV).contiguous()
    nws = lib.nq_msssim_loss_ws_floats(B, C, H, W)
    assert nws > 0
    bufs = {k: _guarded(m) for k, m in (("loss3", 3), ("grad", pred.numel()), ("ws", nws))}
    rc = lib.nq_msssim_loss(_ptr(pred), _ptr(tgt), _ptr(bufs["loss3"][1]), _ptr(bufs["grad"][1]) if want_grad else None,
                            _ptr(bufs["ws"][1]), B, C, H, W, weights[0], weights[1], scale,
                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert _intact(buf, view), f"{k}: a sentinel next to the buffer was overwritten"
    if not want_grad:
        assert bool((bufs["grad"][1] == SENTINEL).all())
    return bufs["loss3"][1].clone(), bufs["grad"][1].clone().view_as(pred) if want_grad else None, bufs["ws"][1][:B].clone()


def _ratios(got3, got_grad, ref):
    ref3, ref_grad, bound3, bound_grad = ref[:4]
    e3 = np.abs(got3.double().cpu().numpy() - ref3)
    with np.errstate(divide="ignore", invalid="ignore"):             # a zero bound (an exactly zero value) asks for equality
        r3 = np.where(bound3 > 0, e3 / bound3, np.where(e3 == 0, 0.0, np.inf))
    rg = float(np.abs(got_grad.double().cpu().numpy() - ref_grad).max()) / bound_grad
    return r3, rg


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_kernel_against_float64(shape):
    """1: every case and weight pair of one shape, values and gradient; two calls agree bit for bit"""
    worst3, worst_g, where = np.zeros(3), 0.0, None
    for name, pred, tgt in _cases(shape):
        for weights in WEIGHTS:
            loss3, grad, _ = _run(pred, tgt, weights)
            again3, again_grad, _ = _run(pred, tgt, weights)
            assert torch.equal(loss3, again3) and torch.equal(grad, again_grad)
            ref = _reference(shape, name, weights)
            assert ref[5].all() and ref[6] >= 0.12                    # no plane is near the clamp
            r3, rg = _ratios(loss3, grad, ref)
            print(f"msssim_loss {shape} {name} {weights}: error / bound  L {r3[0]:.3f}  MSE {r3[1]:.3f}  MS-SSIM {r3[2]:.3f}  "
                  f"grad {rg:.3f}")
            if rg > worst_g:
                worst_g, where = rg, (name, weights)
            worst3 = np.maximum(worst3, r3)
            assert r3.max() <= 1.0 and rg <= 1.0, (name, weights, r3, rg)
    print(f"msssim_loss {shape}: worst error / bound  loss3 {worst3.max():.3f}  grad {worst_g:.3f} at {where}")


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_identical_images(shape):
    """2: pred == tgt gives loss3 == [0, 0, 1], MS_b == 1 exactly and (at most) a few ulps of gradient"""
    for img in (_crop(shape), _cases(shape)[4][2], _uniform(shape)[0]):
        for weights in WEIGHTS:
            loss3, grad, frame = _run(img, img.clone(), weights)
            assert loss3.tolist() == [0.0, 0.0, 1.0]
            assert frame.tolist() == [1.0] * shape[0]
            assert float(grad.abs().max()) <= ULPS


def test_every_plane_clamped():
    """3, clamp case A: the float64 MS-SSIM is exactly 0 on every plane (most negative v_s -0.0075): L == 1, MS_b == 0, and the
    gradient is exactly zero and finite; with an MSE weight the gradient is the MSE term alone"""
    pred, tgt = _uniform(CLAMP_ALL)
    ref = _reference(CLAMP_ALL, "uniform", (0.0, 1.0))
    assert not ref[5].any() and ref[4].tolist() == [0.0] and ref[0][0] == 1.0
    loss3, grad, frame = _run(pred, tgt, (0.0, 1.0))
    assert float(loss3[0]) == 1.0 and float(loss3[2]) == 0.0 and frame.tolist() == [0.0]
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) == 0.0
    loss3, grad, _ = _run(pred, tgt, (0.3, 0.7))
    r3, rg = _ratios(loss3, grad, _reference(CLAMP_ALL, "uniform", (0.3, 0.7)))
    print(f"msssim_loss clamp A (0.3, 0.7): error / bound  loss3 {r3.max():.3f}  grad {rg:.3f}")
    assert r3.max() <= 1.0 and rg <= 1.0


def test_some_planes_clamped():
    """4, clamp case B: some planes clamped, some not (per-frame MS-SSIM 0.052 and 0.081): values within the bound, the gradient
    finite everywhere, exactly zero on the clamped planes and within the bound on the others"""
    pred, tgt = _uniform(CLAMP_SOME)
    for weights in WEIGHTS:
        ref = _reference(CLAMP_SOME, "uniform", weights)
        live = ref[5]
        assert live.any() and not live.all()
        assert np.allclose(ref[4], [0.052, 0.081], atol=6e-4)
        loss3, grad, frame = _run(pred, tgt, weights)
        r3, rg = _ratios(loss3, grad, ref)
        print(f"msssim_loss clamp B {weights}: error / bound  loss3 {r3.max():.3f}  grad {rg:.3f}")
        assert bool(torch.isfinite(grad).all())
        assert r3.max() <= 1.0 and rg <= 1.0
        assert float(np.abs(frame.double().cpu().numpy() - ref[4]).max()) <= ref[2][2] * CLAMP_SOME[0]
        if weights[0] == 0.0:
            dead = torch.from_numpy(~live).to(DEV)
            assert float(grad[dead].abs().max()) == 0.0 and float(grad[~dead].abs().max()) > 0.0


def test_a_frame_depends_on_its_own_bytes_only():
    """5: frame 0 of a B = 2 call equals the B = 1 call on frame 0 alone: its MS-SSIM bit for bit, its gradient up to the factor
    1 / B of the mean over frames (a power of two: exact); the mean agrees with ops.ms_ssim (another kernel) within the bound"""
    from neuroquant_amd import ops
    for shape in (SHAPES[1], SHAPES[3]):
        for name in ("noisy0.02", "random"):
            pred, tgt = _inputs(shape, name)
            l2_, g2, f2 = _run(pred, tgt, (0.3, 0.7))
            _, g1, f1 = _run(pred[:1], tgt[:1], (0.3, 0.7))
            assert f2[0] != f2[1]
            assert torch.equal(f2[:1], f1)
            assert torch.equal(g2[:1] * 2, g1)
            other = ops.ms_ssim(pred.to(DEV), tgt.to(DEV))
            bound = _reference(shape, name, (0.3, 0.7))[2][2]
            r_mean = abs(float(other.double().mean()) - float(l2_[2])) / bound
            r_frame = float((other.double() - f2.double()).abs().max()) / (shape[0] * bound)
            print(f"msssim_loss {shape} {name}: |mean MS-SSIM - ops.ms_ssim| / bound {r_mean:.3f}, per frame / (B bound) {r_frame:.3f}")
            assert r_mean <= 1.0 and r_frame <= 1.0                  # bound: of the mean; a frame's share of it is B times as large


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_mse_only_is_the_l2_loss_and_forward_only_agrees(shape):
    """6: w_ms = 0 is ops.l2_loss / C in value and gradient, within the bound of test 1; want_grad=False: the same loss3 bits,
    grad untouched (_run asserts it)"""
    from neuroquant_amd import ops
    for name, pred, tgt in _cases(shape)[:2] + _cases(shape)[4:]:
        _, _, bound3, bound_grad = _reference(shape, name, (1.0, 0.0))[:4]
        p, t = pred.to(DEV), tgt.to(DEV)
        loss3, grad = ops.ms_ssim_loss_raw(p, t, 1.0, 0.0)
        q = p.clone().requires_grad_(True)
        l2 = ops.l2_loss(q, t) / shape[1]
        (l2_grad,) = torch.autograd.grad(l2, q)
        assert abs(float(loss3[0]) - float(l2.detach())) <= bound3[0]
        assert float((grad - l2_grad).abs().max()) <= bound_grad
        for weights in WEIGHTS:
            with_grad, _ = ops.ms_ssim_loss_raw(p, t, *weights)
            without, none = ops.ms_ssim_loss_raw(p, t, *weights, want_grad=False)
            assert none is None and torch.equal(with_grad, without)
            raw3, _, _ = _run(pred, tgt, weights, want_grad=False)
            assert torch.equal(raw3, with_grad)


def test_ops_ms_ssim_loss_under_autograd():
    """7: the Function hands grad * g on"""
    from neuroquant_amd import ops
    shape = SHAPES[1]
    pred, tgt = _inputs(shape, "noisy0.2")
    ref3, ref_grad, _, bound_grad = _reference(shape, "noisy0.2", (0.3, 0.7))[:4]
    p = pred.to(DEV).requires_grad_(True)
    loss = ops.ms_ssim_loss(p, tgt.to(DEV), 0.3, 0.7)
    (g,) = torch.autograd.grad(loss * 0.25, p)
    assert loss.shape == () and abs(float(loss.detach()) - ref3[0]) <= 1e-5 * ref3[0]
    assert float(np.abs(g.double().cpu().numpy() - 0.25 * ref_grad).max()) <= 0.25 * bound_grad      # a power of two: exact
    q = pred.to(DEV).requires_grad_(True)
    (g1,) = torch.autograd.grad(ops.ms_ssim_loss(q, tgt.to(DEV)), q)          # the defaults are the `msssim` loss
    with torch.no_grad():                                                     # no gradient wanted: forward only, the same bits
        quiet = ops.ms_ssim_loss(p, tgt.to(DEV), 0.3, 0.7)
    assert not quiet.requires_grad and torch.equal(quiet, loss.detach())
    assert torch.equal(ops.ms_ssim_loss(pred.to(DEV), tgt.to(DEV), 0.3, 0.7), loss.detach())
    assert torch.equal(g1, ops.ms_ssim_loss_raw(pred.to(DEV), tgt.to(DEV), 0.0, 1.0)[1])


def test_refusals_before_any_launch():
    from neuroquant_amd import ops
    x = torch.rand(1, 3, 161, 161, device=DEV)
    low = torch.rand(1, 3, 160, 200, device=DEV)
    with pytest.raises(ValueError):
        ops.ms_ssim_loss_raw(low, low, 0.0, 1.0)
    with pytest.raises(ValueError):
        ops.ms_ssim_loss(low, low)
    with pytest.raises(ValueError):
        ops.ms_ssim_loss_raw(x, torch.rand(1, 3, 161, 162, device=DEV), 0.0, 1.0)
    for w in ((-1.0, 1.0), (float("nan"), 1.0), (0.0, 0.0)):
        with pytest.raises(ValueError):
            ops.ms_ssim_loss_raw(x, x, *w)
        with pytest.raises(ValueError):
            ops.msssim_loss_head_grad(x, tgt=x, w_mse=w[0], w_ms=w[1])
    with pytest.raises(RuntimeError):
        ops.ms_ssim_loss_raw(x, x.cpu(), 0.0, 1.0)
    with pytest.raises(ValueError):
        ops.msssim_loss_head_grad(x)
    with pytest.raises(ValueError):
        ops.msssim_loss_head_grad(x, tgt=x, cache_u8=torch.zeros(2, 3, 161, 161, dtype=torch.uint8, device=DEV),
                                  idx=torch.zeros(1, dtype=torch.int64, device=DEV))


def _tanh_backward(dimg, img):
    from neuroquant_amd import _lib as L
    out = torch.empty_like(dimg)
    rc = L.lib().nq_tanh_out_backward(_ptr(dimg), _ptr(img), _ptr(out), dimg.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return out


def test_head_grad_hands_over():
    """8: image mode is nq_msssim_loss(grad_scale = C) with loss3[0] times C; a cache target equals the float target of the gathered
    frames bit for bit; with a hand-over slot dimg is nq_tanh_out_backward of the image-mode gradient bit for bit and the bias
    gradient its channel sums"""
    from neuroquant_amd import ops
    shape = SHAPES[1]
    B, C, H, W = shape
    pred, tgt = _inputs(shape, "noisy0.02")
    pred = pred.clamp(0.01, 0.99)                                     # an image a tanh head can have produced
    g = torch.Generator().manual_seed(7)
    cache = torch.randint(0, 256, (5,) + shape[1:], generator=g, dtype=torch.uint8)
    idx = torch.tensor([3, 1])
    cache[idx] = (tgt * 255).round().clamp(0, 255).to(torch.uint8)
    p, cache_d, idx_d = pred.to(DEV), cache.to(DEV), idx.to(DEV)
    gathered = ops.gather_frames_u8(cache_d, idx_d)
    before = ops.msssim_loss_head_launches
    want3, want_g, _ = _run(pred, gathered, (0.3, 0.7), scale=float(C))
    loss3, dimg = ops.msssim_loss_head_grad(p, tgt=gathered, w_mse=0.3, w_ms=0.7)           # no hand-over slot: image mode
    assert torch.equal(dimg, want_g) and torch.equal(loss3[1:], want3[1:])
    assert float(loss3[0]) == float(np.float32(C) * want3[0].cpu().numpy())
    loss3c, dimgc = ops.msssim_loss_head_grad(p, cache_u8=cache_d, idx=idx_d, w_mse=0.3, w_ms=0.7)
    assert torch.equal(loss3c, loss3) and torch.equal(dimgc, dimg)

    class Node:
        nq_head = ops._HeadHandoff()
    loss3h, dconv = ops.msssim_loss_head_grad(p, cache_u8=cache_d, idx=idx_d, node=Node, w_mse=0.3, w_ms=0.7)
    assert torch.equal(loss3h, loss3) and dconv is Node.nq_head.dconv and Node.nq_head.version == dconv._version
    assert torch.equal(dconv, _tanh_backward(dimg, p))
    assert torch.equal(Node.nq_head.db, ops.channel_sum(dconv))
    want_db = dconv.double().sum((0, 2, 3))
    assert bool(((Node.nq_head.db.double() - want_db).abs() <= 2.0 ** -18 * dconv.double().abs().sum((0, 2, 3))).all())
    assert ops.msssim_loss_head_launches == before + 3
    # weights (1, 0) are lp_loss(p = 2): value and gradient of ops.l2_loss
    loss3m, dm = ops.msssim_loss_head_grad(p, tgt=gathered, w_mse=1.0, w_ms=0.0)
    q = p.clone().requires_grad_(True)
    l2 = ops.l2_loss(q, gathered)
    (l2_grad,) = torch.autograd.grad(l2, q)
    # (two fp32 sums of 1.7e5 terms in different tree orders: log2(n) roundings of 2^-24 each, ~1e-6 relative apiece)
    assert abs(float(loss3m[0]) - float(l2.detach())) <= 4e-6 * float(l2.detach()) and float((dm - l2_grad).abs().max()) <= 1e-6 * float(l2_grad.abs().max())


def _tiny_model(golden):
    from neuroquant_amd.models import HNeRV
    model = HNeRV(TINY_HNERV)
    model.load_state_dict(state_dict_from_npz(golden("traj_hnerv.npz"), "sd:"))
    return model.to(DEV).train()


def test_trainer_step_gradients(golden):
    """9: one regress step with loss: msssim, weights (0.5, 0.5), on the tiny HNeRV; every parameter gradient equals the one
    obtained by feeding the float64 restatement's dL/dpred into the same backward (the tolerances of
    test_ssim_loss_gpu.py::test_trainer_step_gradients)"""
    from neuroquant_amd.methods import regress
    img = (T(golden("frames_320x640.npz")["frames"]).float() / 255.0)[:2].to(DEV)
    args = regress.parse_args(["--arch", "hnerv", "--synthetic", "8"])
    params = regress.loss_params(args, dict(TINY_HNERV, loss="msssim", loss_weights=[0.5, 0.5]))
    assert params == dict(w_mse=0.5, w_ms=0.5)
    mg, mr = _tiny_model(golden), _tiny_model(golden)
    out_g, elist, _ = mg(img)
    assert len(elist) == 1                                   # fused stack taken
    loss = regress.step_loss(out_g, img, params)
    loss.backward()
    out_r, _, _ = mr(img)
    ref3, ref_grad, _, v = MR.loss_autograd(out_r, img, 0.5, 0.5)
    assert float(v.min()) > 0.01                             # no clamped plane
    assert abs(float(loss.detach()) - float(ref3[0])) <= 1e-5 * float(ref3[0])     # the same images up to the forward's run-to-run bits
    out_r.backward(ref_grad.float().to(DEV))
    n_dec = 0
    for (n, pg), (_, pr) in zip(mg.named_parameters(), mr.named_parameters()):
        assert pg.grad is not None, f"{n} got no gradient"
        np.testing.assert_allclose(pg.grad.double().cpu().numpy(), pr.grad.double().cpu().numpy(), rtol=5e-3,
                                   atol=2e-4 * float(pr.grad.abs().max()) + 1e-9)
        n_dec += not n.startswith("encoder")
    assert n_dec > 4


# ------------------------------------------------------------------------------------------ calibration
MSSSIM = dict(w_mse=0.5, w_ms=0.5)


def _tiny_qnn(golden):
    from neuroquant_amd.models import HNeRV
    from neuroquant_amd.quantization import QuantModel
    z = golden("traj_hnerv.npz")
    model = HNeRV(TINY_HNERV)
    model.load_state_dict(state_dict_from_npz(z, "sd:"))
    model = model.to(DEV).eval()
    emb = T(z["emb"]).to(DEV)
    qnn = QuantModel(model, hadamard=False, weight_quant_params=dict(n_bits=8, channel_wise=True, scale_method="max"))
    qnn.set_bitwidth(BITS)
    qnn.eval()
    qnn.set_quant_state(True)
    with torch.no_grad():
        qnn(emb[:2])
    return z, qnn, emb


def _params(qnn):
    out = []
    for m in qnn.quant_modules():
        out += [m.weight_quantizer.delta.detach().clone(), m.bias_quantizer.delta.detach().clone()]
        if hasattr(m.weight_quantizer, "alpha"):
            out += [m.weight_quantizer.alpha.detach().clone(), m.bias_quantizer.alpha.detach().clone()]
    return out


def test_calibration_captured_equals_eager_and_default_is_what_it_was(golden, monkeypatch):
    """10 (engine): 8 iterations from a CacheLoader with msssim=: every delta and alpha of the captured run bit-identical with
    NQ_GRAPH=0.  A run with default arguments issues no MS-SSIM launch, and its first logged losses are the oracle's (the bar of
    test_hip_parity.py::test_calibration_trajectory_hnerv: 2e-4 before any rounding flip)."""
    from neuroquant_amd import ops
    from neuroquant_amd.quantization import model_reconstruction
    from neuroquant_amd.utils import CacheLoader, FrameCache
    frames_u8 = T(golden("frames_320x640.npz")["frames"]).to(DEV)

    def run(graph, **kw):
        monkeypatch.setenv("NQ_GRAPH", "1" if graph else "0")
        z, qnn, emb = _tiny_qnn(golden)
        order = np.asarray(z["order"])[:, :2]
        before = ops.msssim_loss_head_launches
        model_reconstruction(qnn, cali_data=emb, gt=CacheLoader(FrameCache(frames_u8), list(range(8)), 2, order=order),
                             arch="hnerv", batch_size=2, iters=40, weight=0.01, hadamard=False, b_range=(20, 2), warmup=0.2,
                             lr=0.003, max_steps=8, **kw)
        return _params(qnn), ops.msssim_loss_head_launches - before

    eager, n_e = run(False, msssim=MSSSIM)
    graphed, n_g = run(True, msssim=MSSSIM)
    assert n_e == 8 and 0 < n_g < 8              # replays launch through the graph, not through the wrapper
    assert len(eager) == len(graphed) == 28
    for a, b in zip(eager, graphed):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    rgb, n_rgb = run(True)
    assert n_rgb == 0
    assert any(not torch.equal(a, b) for a, b in zip(rgb, graphed))          # the objective changes the result

    # the default objective against the oracle's log
    z, qnn, emb = _tiny_qnn(golden)
    frames = frames_u8.float() / 255.0
    order = np.asarray(z["order"])
    batches = [dict(img=frames[torch.as_tensor(i, device=DEV)], idx=torch.as_tensor(i, dtype=torch.int64, device=DEV),
                    norm_idx=torch.as_tensor(i, device=DEV).float() / 8) for i in order[0][:3]]
    rec = []
    before = ops.msssim_loss_head_launches
    model_reconstruction(qnn, cali_data=emb, gt=batches, arch="hnerv", batch_size=2, iters=int(z["iters"]), weight=0.01,
                         hadamard=False, b_range=(20, 2), warmup=0.2, lr=0.003, recorder=rec, max_steps=3)
    log, ref = np.array(rec), z["loss_log"]
    assert ops.msssim_loss_head_launches == before and len(log) == 3
    np.testing.assert_array_equal(log[:, 2:], ref[:3, 2:])
    np.testing.assert_allclose(log[:, 0], ref[:3, 0], rtol=2e-4)


def _driver_run(tmp_path, monkeypatch, tag, flags):
    from neuroquant_amd.methods import calibrate_network as cn
    root = logging.getLogger()
    saved = (root.level, list(root.handlers))
    rec, seen = [], {}
    engine = cn.model_reconstruction

    def recording(*a, **kw):                     # the driver's own call, with a recorder to read `rec` from
        seen.update(kw)
        return engine(*a, recorder=rec, **kw)

    monkeypatch.setattr(cn, "model_reconstruction", recording)
    try:
        args = cn.parse_args(["--arch", "hnerv", "--synthetic", "4", "--batch_size", "2", "--channel_wise", "--init", "max",
                              "--iters_w", "8", "--weight", "0.01", "--warmup", "0.2", "--lr", "0.003",
                              "--precision", "6", "5", "4", "5", "5", "6", "6"] + flags)
        args.outf = str(tmp_path / tag)
        cn.seed_all(903)
        cn.calibrate(args, dict(TINY_HNERV))
        for h in list(root.handlers):
            if h not in saved[1]:
                h.close()
                root.removeHandler(h)
        log = "".join(open(os.path.join(args.outf, f)).read() for f in sorted(os.listdir(args.outf)) if f.endswith(".log"))
    finally:
        monkeypatch.setattr(cn, "model_reconstruction", engine)
        root.setLevel(saved[0])
        for h in list(root.handlers):
            if h not in saved[1]:
                root.removeHandler(h)
    return rec, seen, log, args


def test_driver_calibrates_on_msssim_exports_and_plays_back(tmp_path, monkeypatch, capsys):
    """10 (driver): an 8-iteration calibrate_network --rec_loss msssim --export_stream run: finite logged reconstruction losses, the
    objective's log lines, a second run that equals it bit for bit, and decode_stream plays the file back at the PSNR and
    MS-SSIM the driver logged"""
    import re
    from neuroquant_amd import ops
    from neuroquant_amd.methods import decode_stream as ds
    stream = tmp_path / "out" / "model.nqv"
    before = ops.msssim_loss_head_launches
    rec, seen, log, args = _driver_run(tmp_path, monkeypatch, "a", ["--rec_loss", "msssim", "--export_stream", str(stream)])
    assert ops.msssim_loss_head_launches > before
    assert seen["msssim"] == dict(w_mse=0.0, w_ms=1.0) and seen["ssim"] is None and seen["loss_domain"] == "rgb"
    assert len([ln for ln in log.splitlines() if "msssim objective (0.0, 1.0)" in ln]) == 4      # FP, off, on, calibrated
    assert "w_ms * (1 - MS-SSIM)" in log
    assert len(rec) == 8
    for total, rl, b, count in rec:
        assert np.isfinite(total) and np.isfinite(total - rl) and total - rl > 0.0               # rec = loss3[0]
    again, _, _, args2 = _driver_run(tmp_path, monkeypatch, "b", ["--rec_loss", "msssim"])
    assert again == rec
    assert all(float(args.eval_metrics[k]) == float(args2.eval_metrics[k]) for k in args.eval_metrics)
    logged = re.findall(r"Weight quantization w/ opt: best_pred_seen_psnr: ([0-9.]+) \| best_pred_seen_ssim: ([0-9.]+)", log)
    assert logged, log
    capsys.readouterr()
    ds.main(["--stream", str(stream), "--synthetic", "4"])
    played = re.search(r"float: PSNR ([0-9.]+) \| MS-SSIM ([0-9.]+)", capsys.readouterr().out)
    assert played and (played.group(1), played.group(2)) == logged[-1]


def test_twenty_msssim_steps_go_the_right_way(golden):
    """11: a direction check only -- the loss falls and the MS-SSIM of the training frames rises"""
    from neuroquant_amd import ops
    from neuroquant_amd.methods import regress
    from neuroquant_amd.models import HNeRV
    img = (T(golden("frames_320x640.npz")["frames"]).float() / 255.0)[:2].to(DEV)
    args = regress.parse_args(["--arch", "hnerv", "--synthetic", "8"])
    params = regress.loss_params(args, dict(TINY_HNERV, loss="msssim"))
    torch.manual_seed(903)
    model = HNeRV(TINY_HNERV).to(DEV).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=0.)
    losses, ms = [], []
    for step in range(21):
        out, _, _ = model(img)
        loss = regress.step_loss(out, img, params)
        losses.append(float(loss.detach()))
        ms.append(float(ops.ms_ssim(out, img).mean()))
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    print(f"msssim, 20 steps: loss {losses[0]:.5f} -> {losses[-1]:.5f}, MS-SSIM {ms[0]:.4f} -> {ms[-1]:.4f}")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0] and ms[-1] > ms[0]

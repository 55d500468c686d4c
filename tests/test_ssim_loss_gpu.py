"""The SSIM training loss on the GPU: nq_ssim_loss against the float64 restatement (tests/ssim_loss_ref.py),
then the layers above it: ops, autograd and the trainer's step.

Bounds.  e32 is the error of the SAME restatement run in float32 against float64 on the same inputs: what the number format
alone costs.  The kernel is held to 4 * e32 (the project's convention for "same format, other summation order") plus
8 * 2^-24 of the value's scale (a few fp32 ulps, so a lucky restatement cannot make the bound zero):
    |loss3 - ref| <= 4 e32 + 8 * 2^-24 |ref|                     per entry
    max|grad - ref| <= 4 e32_grad + 8 * 2^-24 max|grad_ref|
Worst observed error / bound per shape is printed (run with -s) and recorded in DESIGN.md §20."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import msssim_ref as M
import ssim_loss_ref as SR
from conftest import T, TINY_HNERV, state_dict_from_npz

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULPS = 8 * 2.0 ** -24
WEIGHTS = ((0.0, 1.0), (1.0, 0.0), (0.3, 0.7), (0.7, 0.3))
SENTINEL = -77.25
TH, TW = 8, 118                      # the kernel's tile (ops.SSIM_LOSS_TILE, asserted below)
CROP = (2, 3, 64, 96)
SHAPES = [(1, 1, 11, 11),            # one valid pixel
          (2, 3, 12, 21),
          (1, 3, 11, 140),           # one valid row, two tiles wide
          (1, 3, 140, 11),           # one valid column, 17 tiles high
          (2, 3, TH + 10, TW + 10),  # exactly one tile
          (2, 3, TH + 11, TW + 11),  # one tile plus one row and one column
          (1, 3, 2 * TH + 13, 2 * TW + 7),
          CROP]                      # cut from the real frames


@functools.lru_cache(maxsize=None)
def _frames():
    return M.bunny_frames(2)


def _crop(shape):
    """the real frames' pixels from (301, 517) on, the first C channels"""
    B, C, H, W = shape
    return _frames()[:B, :C, 301:301 + H, 517:517 + W].contiguous()


@functools.lru_cache(maxsize=None)
def _cases(shape):
    """-> [(name, pred, tgt)] float32 CPU tensors; the pred == tgt case has a test of its own"""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(1000 * H + W + B)
    crop = _crop(shape)
    planes = torch.rand(2, B, C, 1, 1, generator=g).expand(2, B, C, H, W).contiguous()
    out = [("uniform", torch.rand(shape, generator=g), torch.rand(shape, generator=g)),
           ("constant", planes[0], planes[1]),
           ("noisy0.02", M.noisy(crop, 0.02), crop)]
    if shape == CROP:
        out += [("noisy0.2", M.noisy(crop, 0.2), crop), ("posterised", M.posterised(crop), crop),
                ("box_blurred", M.box_blurred(crop), crop)]
    return out


@functools.lru_cache(maxsize=None)
def _reference(shape, name, weights):
    """-> (ref3, ref_grad, bound3, bound_grad) as float64 numpy: computed once, shared, never written to"""
    pred, tgt = next((p, t) for n, p, t in _cases(shape) if n == name)
    l64, g64, _ = SR.loss_autograd(pred, tgt, *weights)
    l32, g32, _ = SR.loss_autograd(pred, tgt, *weights, dtype=torch.float32)
    l64, g64 = l64.numpy(), g64.numpy()
    e3 = np.abs(l32.double().numpy() - l64)
    eg = float(np.abs(g32.double().numpy() - g64).max())
    out = (l64, g64, 4 * e3 + ULPS * np.abs(l64), 4 * eg + ULPS * float(np.abs(g64).max()))
    for a in out[:3]:
        a.setflags(write=False)
    return out


def _guarded(n):
    g = 4
    buf = torch.full((n + 2 * g,), SENTINEL, device=DEV, dtype=torch.float32)
    return buf, buf[g:g + n]


def _intact(buf, view):
    g = (buf.numel() - view.numel()) // 2
    return bool((buf[:g] == SENTINEL).all()) and bool((buf[g + view.numel():] == SENTINEL).all())


def _run(pred, tgt, weights, want_grad=True):
    """one nq_ssim_loss call on guarded buffers -> (loss3, grad or None, per-frame SSIM) as tensors on the GPU"""
    from neuroquant_amd import _lib as L
    lib = L.lib()
    B, C, H, W = pred.shape
    pred, tgt = pred.to(DEV).contiguous(), tgt.to(DEV).contiguous()
    nws = lib.nq_ssim_loss_ws_floats(B, C, H, W)
    assert nws > 0
    bufs = {k: _guarded(m) for k, m in (("loss3", 3), ("grad", pred.numel()), ("ws", nws))}
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.nq_ssim_loss(ptr(pred), ptr(tgt), ptr(bufs["loss3"][1]), ptr(bufs["grad"][1]) if want_grad else None,
                          ptr(bufs["ws"][1]), B, C, H, W, weights[0], weights[1], 1.0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert _intact(buf, view), f"{k}: a sentinel next to the buffer was overwritten"
    if not want_grad:
        assert bool((bufs["grad"][1] == SENTINEL).all())
    return bufs["loss3"][1].clone(), bufs["grad"][1].clone().view_as(pred) if want_grad else None, bufs["ws"][1][:B].clone()


def _ratios(got3, got_grad, ref):
    ref3, ref_grad, bound3, bound_grad = ref
    r3 = np.abs(got3.double().cpu().numpy() - ref3) / bound3
    rg = float(np.abs(got_grad.double().cpu().numpy() - ref_grad).max()) / bound_grad
    return r3, rg


def test_tile_constants():
    from neuroquant_amd import ops
    assert ops.SSIM_LOSS_TILE == (TH, TW)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_kernel_against_float64(shape):
    """1: every case and weight pair of one shape, values and gradient; 3: two calls agree bit for bit"""
    worst3, worst_g, where = np.zeros(3), 0.0, None
    for name, pred, tgt in _cases(shape):
        for weights in WEIGHTS:
            loss3, grad, _ = _run(pred, tgt, weights)
            again3, again_grad, _ = _run(pred, tgt, weights)
            assert torch.equal(loss3, again3) and torch.equal(grad, again_grad)
            r3, rg = _ratios(loss3, grad, _reference(shape, name, weights))
            print(f"ssim_loss {shape} {name} {weights}: error / bound  L {r3[0]:.3f}  MSE {r3[1]:.3f}  SSIM {r3[2]:.3f}  "
                  f"grad {rg:.3f}")
            if rg > worst_g:
                worst_g, where = rg, (name, weights)
            worst3 = np.maximum(worst3, r3)
            assert r3.max() <= 1.0 and rg <= 1.0, (name, weights, r3, rg)
    print(f"ssim_loss {shape}: worst error / bound  loss3 {worst3.max():.3f}  grad {worst_g:.3f} at {where}")


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_identical_images(shape):
    """2: pred == tgt gives mean SSIM exactly 1, MSE exactly 0 and (at most) a few ulps of gradient"""
    for img in (_crop(shape), _cases(shape)[0][1], _cases(shape)[1][1]):
        for weights in WEIGHTS:
            loss3, grad, frame = _run(img, img.clone(), weights)
            assert loss3.tolist() == [0.0, 0.0, 1.0]
            assert frame.tolist() == [1.0] * shape[0]
            assert float(grad.abs().max()) <= ULPS


def test_a_frame_depends_on_its_own_bytes_only():
    """3: frame 0's SSIM from a B = 2 call equals the B = 1 call on frame 0 alone, bit for bit"""
    from neuroquant_amd import ops
    for shape in (SHAPES[1], SHAPES[6], CROP):
        _, pred, tgt = _cases((2,) + shape[1:])[2]
        pred, tgt = pred.to(DEV), tgt.to(DEV)
        both, first = ops.ssim(pred, tgt), ops.ssim(pred[:1], tgt[:1])
        assert both.shape == (2,) and first.shape == (1,) and both[0] != both[1]
        assert torch.equal(both[:1], first)
        assert torch.equal(both, ops.ssim(pred, tgt))
        loss3, _ = ops.ssim_loss_raw(pred, tgt, 0.0, 1.0)
        assert abs(float(both.double().mean()) - float(loss3[2])) <= 2.0 ** -23


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_mse_only_is_the_l2_loss_and_forward_only_agrees(shape):
    """4: w_ssim = 0 is ops.l2_loss / C in value and gradient, within the bound of test 1; want_grad=False: the same loss3 bits"""
    from neuroquant_amd import ops
    for name, pred, tgt in _cases(shape):
        ref3, ref_grad, bound3, bound_grad = _reference(shape, name, (1.0, 0.0))
        p, t = pred.to(DEV), tgt.to(DEV)
        loss3, grad = ops.ssim_loss_raw(p, t, 1.0, 0.0)
        q = p.clone().requires_grad_(True)
        l2 = ops.l2_loss(q, t) / shape[1]
        (l2_grad,) = torch.autograd.grad(l2, q)
        assert abs(float(loss3[0]) - float(l2.detach())) <= bound3[0]
        assert float((grad - l2_grad).abs().max()) <= bound_grad
        for weights in WEIGHTS:
            with_grad, _ = ops.ssim_loss_raw(p, t, *weights)
            without, none = ops.ssim_loss_raw(p, t, *weights, want_grad=False)
            assert none is None and torch.equal(with_grad, without)


def _tiny_model(golden):
    from neuroquant_amd.models import HNeRV
    model = HNeRV(TINY_HNERV)
    model.load_state_dict(state_dict_from_npz(golden("traj_hnerv.npz"), "sd:"))
    return model.to(DEV).train()


def test_trainer_step_gradients(golden):
    """5: one regress step with loss: Fusion5 on the tiny HNeRV; every parameter gradient equals the one obtained by feeding the
    float64 restatement's dL/dpred into the same backward (the tolerances of test_fp32_trainer_step_matches_torch)"""
    from neuroquant_amd.methods import regress
    img = (T(golden("frames_320x640.npz")["frames"]).float() / 255.0)[:2].to(DEV)
    args = regress.parse_args(["--arch", "hnerv", "--synthetic", "8"])
    params = regress.loss_params(args, dict(TINY_HNERV, loss="Fusion5"))
    mg, mr = _tiny_model(golden), _tiny_model(golden)
    out_g, elist, _ = mg(img)
    assert len(elist) == 1                                   # fused stack taken
    loss = regress.step_loss(out_g, img, params)
    loss.backward()
    out_r, _, _ = mr(img)
    ref3, ref_grad, _ = SR.loss_autograd(out_r, img, 0.7, 0.3)
    assert abs(float(loss) - float(ref3[0])) <= 1e-5 * float(ref3[0])     # the same images up to the forward's run-to-run bits
    out_r.backward(ref_grad.float().to(DEV))
    n_dec = 0
    for (n, pg), (_, pr) in zip(mg.named_parameters(), mr.named_parameters()):
        assert pg.grad is not None, f"{n} got no gradient"
        np.testing.assert_allclose(pg.grad.double().cpu().numpy(), pr.grad.double().cpu().numpy(), rtol=5e-3,
                                   atol=2e-4 * float(pr.grad.abs().max()) + 1e-9)
        n_dec += not n.startswith("encoder")
    assert n_dec > 4


def test_refusals_before_any_launch():
    """6"""
    from neuroquant_amd import ops
    x = torch.rand(1, 3, 12, 12, device=DEV)
    low = torch.rand(1, 3, 10, 12, device=DEV)
    with pytest.raises(ValueError):
        ops.ssim_loss_raw(low, low, 0.0, 1.0)
    with pytest.raises(ValueError):
        ops.ssim_loss(low, low)
    with pytest.raises(ValueError):
        ops.ssim(low, low)
    with pytest.raises(ValueError):
        ops.ssim_loss_raw(x, torch.rand(1, 3, 12, 13, device=DEV), 0.0, 1.0)
    for w in ((-1.0, 1.0), (float("nan"), 1.0), (0.0, 0.0)):
        with pytest.raises(ValueError):
            ops.ssim_loss_raw(x, x, *w)
        with pytest.raises(ValueError):
            ops.ssim_loss(x, x, *w)
    with pytest.raises(RuntimeError):
        ops.ssim_loss_raw(x.cpu(), x.cpu(), 0.0, 1.0)
    with pytest.raises(RuntimeError):
        ops.ssim_loss_raw(x, x.cpu(), 0.0, 1.0)


def test_ops_ssim_loss_under_autograd():
    """5: the Function hands grad * g on"""
    from neuroquant_amd import ops
    _, pred, tgt = _cases(SHAPES[1])[0]
    ref3, ref_grad, _, bound_grad = _reference(SHAPES[1], "uniform", (0.3, 0.7))
    p = pred.to(DEV).requires_grad_(True)
    loss = ops.ssim_loss(p, tgt.to(DEV), 0.3, 0.7)
    (g,) = torch.autograd.grad(loss * 0.25, p)
    assert loss.shape == () and abs(float(loss) - ref3[0]) <= 1e-5 * ref3[0]
    assert float(np.abs(g.double().cpu().numpy() - 0.25 * ref_grad).max()) <= 0.25 * bound_grad      # a power of two: exact
    q = pred.to(DEV).requires_grad_(True)
    (g1,) = torch.autograd.grad(ops.ssim_loss(q, tgt.to(DEV)), q)             # the defaults are the `ssim` loss
    assert torch.equal(g1, ops.ssim_loss_raw(pred.to(DEV), tgt.to(DEV), 0.0, 1.0)[1])


def test_twenty_fusion5_steps_go_the_right_way(golden):
    """7: a direction check only -- the loss falls and the SSIM of the training frames rises"""
    from neuroquant_amd import ops
    from neuroquant_amd.methods import regress
    from neuroquant_amd.models import HNeRV
    img = (T(golden("frames_320x640.npz")["frames"]).float() / 255.0)[:2].to(DEV)
    args = regress.parse_args(["--arch", "hnerv", "--synthetic", "8"])
    params = regress.loss_params(args, dict(TINY_HNERV, loss="Fusion5"))
    torch.manual_seed(903)
    model = HNeRV(TINY_HNERV).to(DEV).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=0.)
    losses, ssims = [], []
    for step in range(21):
        out, _, _ = model(img)
        loss = regress.step_loss(out, img, params)
        losses.append(float(loss))
        ssims.append(float(ops.ssim(out, img).mean()))
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    print(f"Fusion5, 20 steps: loss {losses[0]:.5f} -> {losses[-1]:.5f}, SSIM {ssims[0]:.4f} -> {ssims[-1]:.4f}")
    assert losses[-1] < losses[0] and ssims[-1] > ssims[0]

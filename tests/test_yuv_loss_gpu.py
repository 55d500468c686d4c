"""The YUV 4:2:0 objective on the GPU: nq_yuv420_loss against the float64 restatement (tests/yuv_loss_ref.py),
then the layers above it: ops, the calibration engine, the trainer's step and the calibration driver.

Bounds.  Every gradient element is the result of fewer than 40 fp32 roundings of terms no larger than the largest gradient
magnitude: max|g - g_ref| <= 1e-5 max|g_ref| (40 * 2^-24 with 4 x margin).  Each entry of loss4 is a sum of non-negative terms
and is held to 1e-5 of itself; db is a signed sum of gradient elements and is held to 1e-5 of max|db_ref|."""
import ctypes
import itertools
import logging
import os

import numpy as np
import pytest
import torch

import yuv_loss_ref as LR
from conftest import BITS, T, TINY_HNERV, state_dict_from_npz

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 1e-5
MATRICES = ("bt601", "bt709")
WEIGHTS = ((6.0, 1.0, 1.0), (0.0, 1.0, 2.0))
SENTINEL = -77.25
IDX_U8 = [2, 0, 2]        # the cache form: B = 3 frames out of a 4-frame cache

# (B, H, W, every float pointer moved off 16-byte alignment)
SHAPES = [(1, 2, 2, False),       # one block
          (1, 2, 4, False),       # smallest vector path: one thread
          (2, 4, 8, False),
          (2, 6, 10, False),      # block path, W % 4 != 0
          (1, 34, 516, False),    # vector path, 2193 threads: 9 workgroups, a ragged last one
          (2, 64, 64, False),
          (2, 4, 8, True)]        # a vector-path shape on the block path


def _lib():
    from neuroquant_amd import _lib as L
    return L.lib()


def _guarded(n, shift):
    """a float buffer of n elements with sentinels either side; shift: start 4 bytes past a 16-byte boundary"""
    g = 5 if shift else 4
    buf = torch.full((n + 2 * g,), SENTINEL, device=DEV, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[g:g + n]


def _intact(buf, view):
    g = (buf.numel() - view.numel()) // 2
    return bool((buf[:g] == SENTINEL).all()) and bool((buf[g + view.numel():] == SENTINEL).all())


def _run(pred, tgt, cache, idx, matrix, full_range, weights, head, shift=False):
    """one nq_yuv420_loss call on guarded buffers -> (loss4, grad, db or None) as tensors on the GPU"""
    lib = _lib()
    B, _, H, W = pred.shape
    n = pred.numel()
    pbuf, pv = _guarded(n, shift)
    pv.copy_(pred.reshape(-1))
    tv = None
    if tgt is not None:
        tbuf, tv = _guarded(n, shift)
        tv.copy_(tgt.reshape(-1))
    nws = lib.nq_yuv420_loss_ws_floats(B, H, W)
    assert nws > 0
    bufs = {k: _guarded(m, shift) for k, m in (("loss", 4), ("grad", n), ("db", 3), ("ws", nws))}
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    if shift:
        assert pv.data_ptr() % 16 == 4 and bufs["grad"][1].data_ptr() % 16 == 4
    rc = lib.nq_yuv420_loss(ptr(pv), ptr(tv), ptr(cache), ptr(idx), ptr(bufs["loss"][1]), ptr(bufs["grad"][1]),
                            ptr(bufs["db"][1]) if head else None, ptr(bufs["ws"][1]), B, H, W, MATRICES.index(matrix),
                            int(full_range), weights[0], weights[1], weights[2], 1.0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert _intact(buf, view), f"{k}: a sentinel next to the buffer was overwritten"
    if not head:
        assert bool((bufs["db"][1] == SENTINEL).all())
    assert _intact(pbuf, pv) and bool((pv == pred.reshape(-1)).all())
    return bufs["loss"][1].clone(), bufs["grad"][1].clone().view_as(pred), bufs["db"][1].clone() if head else None


def _errors(got, ref):
    """(max relative error of loss4 against each entry, gradient error / max|g_ref|, db error / max|db_ref|)"""
    loss4, g, db = (None if t is None else t.double().cpu().numpy() for t in got)
    el = float(np.max(np.abs(loss4 - ref[0]) / np.abs(ref[0])))
    eg = float(np.abs(g - ref[1]).max() / np.abs(ref[1]).max())
    ed = float(np.abs(db - ref[2]).max() / np.abs(ref[2]).max()) if db is not None else 0.0
    return el, eg, ed


@pytest.mark.parametrize("B,H,W,shift", SHAPES, ids=lambda v: str(v))
def test_kernel_against_float64(B, H, W, shift):
    """every matrix, range, weight set, target form and gradient mode of one shape.  The tanh-head gradient equals the
    image-mode gradient passed through nq_tanh_out_backward BIT FOR BIT: the kernel computes the image-mode value with the same
    instructions and then applies that kernel's expression."""
    from neuroquant_amd import ops
    lib = _lib()
    seed = 1000 * H + W + B
    pred_f, tgt_f, _ = LR.images(B, H, W, seed)
    pred_c, _, cache_np = LR.images(4, H, W, seed + 1)          # the cache form: 4 cached frames, B = 3 of them
    pred_c = pred_c[:3]
    tgt_c = cache_np[IDX_U8].astype(np.float32) / np.float32(255)
    cache = torch.from_numpy(cache_np).to(DEV)
    idx = torch.tensor(IDX_U8, device=DEV, dtype=torch.int64)
    worst = [0.0, 0.0, 0.0]
    for matrix, full_range, weights, u8 in itertools.product(MATRICES, (False, True), WEIGHTS, (False, True)):
        pred_np, tgt_np = (pred_c, tgt_c) if u8 else (pred_f, tgt_f)
        pred = torch.from_numpy(pred_np).to(DEV)
        tgt = None if u8 else torch.from_numpy(tgt_np).to(DEV)
        args = (pred, tgt, cache if u8 else None, idx if u8 else None, matrix, full_range, weights)
        out = {}
        for head in (False, True):
            got = _run(*args, head, shift)
            again = _run(*args, head, shift)
            for a, b in zip(got, again):                                   # two calls: bit-identical
                assert (a is None and b is None) or torch.equal(a, b)
            ref = LR.loss_f64(pred_np, tgt_np, matrix, full_range, weights, head=head)
            e = _errors(got, ref)
            worst = [max(a, b) for a, b in zip(worst, e)]
            assert max(e) <= BOUND, (matrix, full_range, weights, u8, head, e)
            out[head] = got
        (l_img, g_img, _), (l_head, g_head, db) = out[False], out[True]
        assert torch.equal(l_img, l_head)
        # L from the plane MSEs in the arithmetic of the finishing launch: a zero weight contributes exactly nothing
        lw = [np.float32(3.0 * w / sum(weights)) for w in weights]
        m = l_img.cpu().numpy()
        assert m[0] == np.float32(np.float32(lw[0] * m[1] + lw[1] * m[2]) + lw[2] * m[3])
        if weights[0] == 0.0:
            assert m[0] == np.float32(lw[1] * m[2]) + np.float32(lw[2] * m[3])
        # head mode = image mode through the tanh backward kernel, bit for bit
        through = torch.empty_like(g_img)
        rc = lib.nq_tanh_out_backward(ctypes.c_void_p(g_img.data_ptr()), ctypes.c_void_p(pred.data_ptr()),
                                      ctypes.c_void_p(through.data_ptr()), g_img.numel(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        assert torch.equal(through, g_head)
        cs = ops.channel_sum(g_head).double().cpu().numpy()
        ref_db = LR.loss_f64(pred_np, tgt_np, matrix, full_range, weights, head=True)[2]
        assert np.abs(cs - db.double().cpu().numpy()).max() <= BOUND * np.abs(ref_db).max()
    print(f"yuv420_loss ({B}, {H}, {W}){' shifted' if shift else ''}: worst loss4 {worst[0]:.2e}, grad {worst[1]:.2e}, "
          f"db {worst[2]:.2e} (bound {BOUND:.0e})")


def test_ops_wrappers_and_autograd():
    from neuroquant_amd import ops
    pred_np, tgt_np, tgt_u8 = LR.images(2, 6, 10, seed=11)
    pred, tgt = torch.from_numpy(pred_np).to(DEV), torch.from_numpy(tgt_np).to(DEV)
    for matrix, full_range, weights in (("bt709", False, (6, 1, 1)), ("bt601", True, (0, 1, 2))):
        ref4, ref_g, _ = LR.loss_f64(pred_np, tgt_np, matrix, full_range, weights)
        p = pred.clone().requires_grad_(True)
        before = ops.yuv420_loss_launches
        loss = ops.yuv420_loss(p, tgt, matrix, full_range, weights)
        assert ops.yuv420_loss_launches == before + 1
        (g,) = torch.autograd.grad(loss / 3, p)                              # parameter-free: the upstream factor 1/3
        assert abs(float(loss.detach()) - ref4[0]) <= BOUND * ref4[0]
        assert np.abs(g.double().cpu().numpy() - ref_g / 3).max() <= BOUND * np.abs(ref_g / 3).max()
        # the raw op: both target forms agree bit for bit (the cache holds tgt exactly), head mode hands db over
        cache = torch.from_numpy(tgt_u8).to(DEV)
        a = ops.yuv420_loss_raw(pred, tgt=tgt, matrix=matrix, full_range=full_range, weights=weights, head=True)
        b = ops.yuv420_loss_raw(pred, cache_u8=cache, idx=torch.arange(2, device=DEV), matrix=matrix, full_range=full_range,
                                weights=weights, head=True)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        assert a[2].shape == (3,) and a[0].shape == (4,)
    # an image without a decoder node behind it: dL/dpred
    loss4, g = ops.yuv420_loss_head_grad(pred, tgt=tgt)
    ref4, ref_g, _ = LR.loss_f64(pred_np, tgt_np)
    assert np.abs(g.double().cpu().numpy() - ref_g).max() <= BOUND * np.abs(ref_g).max()
    with pytest.raises(ValueError):
        ops.yuv420_loss_raw(pred, tgt=tgt, cache_u8=torch.zeros(2, 3, 6, 10, dtype=torch.uint8, device=DEV), idx=torch.arange(2))


# ------------------------------------------------------------------------------------------ calibration engine
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


YUV = dict(matrix="bt601", full_range=False, weights=(4.0, 1.0, 2.0))


def _params(qnn):
    out = []
    for m in qnn.quant_modules():
        out += [m.weight_quantizer.delta.detach().clone(), m.bias_quantizer.delta.detach().clone()]
        if hasattr(m.weight_quantizer, "alpha"):
            out += [m.weight_quantizer.alpha.detach().clone(), m.bias_quantizer.alpha.detach().clone()]
    return out


def test_calibration_first_loss_is_the_ops_loss(golden):
    """6 iterations with a recorder (2 of phase 1, 4 of phase 2): the first recorded total - round is the loss of the model as
    it stood before the call.  Another forward computes it, so it is held to 1e-6 relative."""
    from neuroquant_amd import ops
    from neuroquant_amd.quantization import model_reconstruction
    from neuroquant_amd.utils import CacheLoader, FrameCache
    z, qnn, emb = _tiny_qnn(golden)
    frames_u8 = T(golden("frames_320x640.npz")["frames"]).to(DEV)
    order = np.asarray(z["order"])[:, :2]
    first = torch.as_tensor(order[0, 0], device=DEV, dtype=torch.int64)
    qnn.train()
    with torch.no_grad():
        img0 = qnn(emb[first])[0]
    want = ops.yuv420_loss_raw(img0, cache_u8=frames_u8, idx=first, **YUV)[0]
    rgb = float(ops.l2_loss(img0, ops.gather_frames_u8(frames_u8, first)))
    rec = []
    before = ops.yuv420_loss_launches
    model_reconstruction(qnn, cali_data=emb, gt=CacheLoader(FrameCache(frames_u8), list(range(8)), 2, order=order), arch="hnerv",
                         batch_size=2, iters=40, weight=0.01, hadamard=False, b_range=(20, 2), warmup=0.2, lr=0.003,
                         recorder=rec, max_steps=6, loss_domain="yuv420", yuv=YUV)
    assert len(rec) == 6 and ops.yuv420_loss_launches == before + 6
    got = rec[0][0] - rec[0][1]
    print(f"first yuv420 loss {got!r}, ops {float(want[0])!r}, rgb lp_loss {rgb!r}")
    assert abs(got - float(want[0])) <= 1e-6 * float(want[0])
    assert abs(got - rgb) > 1e-3 * rgb                                        # and it is not the RGB loss
    with pytest.raises(ValueError):
        model_reconstruction(qnn, cali_data=emb, gt=[], loss_domain="yuv")
    with pytest.raises(ValueError):
        model_reconstruction(qnn, cali_data=emb, gt=[], loss_domain="yuv420", yuv=dict(weights=(0, 0, 0)))


def test_calibration_captured_equals_eager_and_default_launches_none(golden, monkeypatch):
    """8 iterations from a CacheLoader (2 of phase 1; of the 6 of phase 2 three run eagerly, one is captured, two replay): every
    delta and alpha bit-identical with NQ_GRAPH=0.  A run with the default loss_domain issues no nq_yuv420_loss."""
    from neuroquant_amd import ops
    from neuroquant_amd.quantization import model_reconstruction
    from neuroquant_amd.utils import CacheLoader, FrameCache
    frames_u8 = T(golden("frames_320x640.npz")["frames"]).to(DEV)

    def run(graph, **kw):
        monkeypatch.setenv("NQ_GRAPH", "1" if graph else "0")
        z, qnn, emb = _tiny_qnn(golden)
        order = np.asarray(z["order"])[:, :2]
        seen = []
        before = ops.yuv420_loss_launches
        model_reconstruction(qnn, cali_data=emb, gt=CacheLoader(FrameCache(frames_u8), list(range(8)), 2, order=order),
                             arch="hnerv", batch_size=2, iters=40, weight=0.01, hadamard=False, b_range=(20, 2), warmup=0.2,
                             lr=0.003, max_steps=8, step_hook=seen.append, **kw)
        return _params(qnn), seen, ops.yuv420_loss_launches - before

    eager, seen_e, n_e = run(False, loss_domain="yuv420", yuv=YUV)
    graphed, seen_g, n_g = run(True, loss_domain="yuv420", yuv=YUV)
    assert seen_e[:8] == seen_g[:8] == list(range(8))
    assert n_e == 8 and n_g == 6                 # phase 2: three eager iterations + one capture, then replays
    assert len(eager) == len(graphed) == 28
    for a, b in zip(eager, graphed):
        assert torch.equal(a, b)
    rgb, _, n_rgb = run(True)
    assert n_rgb == 0
    assert any(not torch.equal(a, b) for a, b in zip(rgb, graphed))          # the objective changes the result


# ------------------------------------------------------------------------------------------ trainer
def test_trainer_step_matches_torch(golden):
    """one step of methods/regress.py with loss: yuv420 (flags through its own parser) against torch CPU autograd of the torch
    restatement through the same model: the comparison and tolerances of test_fp32_trainer_step_matches_torch."""
    from neuroquant_amd.methods import regress
    from neuroquant_amd.models import HNeRV
    z = golden("traj_hnerv.npz")
    sd = state_dict_from_npz(z, "sd:")
    frames = T(golden("frames_320x640.npz")["frames"]).float() / 255.0
    args = regress.parse_args(["--arch", "hnerv", "--synthetic", "8", "--yuv_weights", "4", "1", "2", "--yuv_matrix", "bt601",
                               "--yuv_range", "full"])
    assert regress.loss_params(args, dict(TINY_HNERV, loss="l2")) is None
    with pytest.raises(NotImplementedError):
        regress.loss_params(args, dict(TINY_HNERV, loss="l1"))
    yuv = regress.loss_params(args, dict(TINY_HNERV, loss="yuv420"))
    assert yuv == dict(matrix="bt601", full_range=True, weights=(4.0, 1.0, 2.0))
    mg = HNeRV(TINY_HNERV); mg.load_state_dict(sd); mg.to(DEV).train()
    mc = HNeRV(TINY_HNERV); mc.load_state_dict(sd); mc.train()
    img_c = frames[:2]; img_g = img_c.to(DEV)
    out_g, elist, _ = mg(img_g)
    assert len(elist) == 1                                   # fused stack taken
    regress.step_loss(out_g, img_g, yuv).backward()
    out_c, _, _ = mc(img_c)
    (LR.loss_torch(out_c, img_c, **yuv)[0] / 3).backward()

    def close(a, b, rtol, atol):
        np.testing.assert_allclose(a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy(), rtol=rtol, atol=atol)

    close(out_g, out_c, rtol=1e-4, atol=3e-5)
    n_enc = 0
    for (n, pg), (_, pc) in zip(mg.named_parameters(), mc.named_parameters()):
        assert pg.grad is not None, f"{n} got no gradient"
        close(pg.grad, pc.grad, rtol=5e-3, atol=2e-4 * float(pc.grad.abs().max()) + 1e-9)
        n_enc += n.startswith("encoder")
    assert n_enc > 10


# ------------------------------------------------------------------------------------------ driver
def test_driver_calibrates_and_reports_yuv(tmp_path):
    from neuroquant_amd.methods import calibrate_network as cn
    root = logging.getLogger()
    saved = (root.level, list(root.handlers))
    try:
        args = cn.parse_args(["--arch", "hnerv", "--synthetic", "4", "--batch_size", "2", "--channel_wise", "--init", "max",
                              "--iters_w", "8", "--weight", "0.01", "--warmup", "0.2", "--lr", "0.003",
                              "--precision", "6", "5", "4", "5", "5", "6", "6", "--loss_domain", "yuv420",
                              "--yuv_weights", "6", "1", "1"])
        dflt = cn.parse_args(["--arch", "hnerv"])
        assert dflt.loss_domain == "rgb" and dflt.yuv_weights == [6.0, 1.0, 1.0]
        assert cn.yuv_loss_params(args) == dict(matrix="bt709", full_range=False, weights=(6.0, 1.0, 1.0))
        args.outf = str(tmp_path / "run")
        cn.seed_all(903)
        cn.calibrate(args, dict(TINY_HNERV))
        for h in list(root.handlers):
            if h not in saved[1]:
                h.close()
                root.removeHandler(h)
        log = "".join(open(os.path.join(args.outf, f)).read() for f in sorted(os.listdir(args.outf)) if f.endswith(".log"))
    finally:
        root.setLevel(saved[0])
        for h in list(root.handlers):
            if h not in saved[1]:
                root.removeHandler(h)
    lines = [ln for ln in log.splitlines() if "yuv420: PSNR-Y " in ln]
    assert len(lines) == 4 and all(" U " in ln and " V " in ln and "| 6:1:1 " in ln for ln in lines)   # FP, off, on, calibrated
    m = args.eval_metrics
    assert set(cn.METRIC_NAMES) | set(cn.YUV_METRIC_NAMES) == set(m)
    y, u, v, mean = (float(m[k]) for k in cn.YUV_METRIC_NAMES)
    assert all(np.isfinite(t) and t > 0 for t in (y, u, v, mean))
    assert abs(mean - (6 * y + u + v) / 8) < 1e-9
    assert "best_psnr_y" not in log and "best_pred_seen_psnr" in log          # the existing report line keeps its four entries

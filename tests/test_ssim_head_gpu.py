"""The MSE + SSIM loss behind the tanh head on the GPU: nq_ssim_loss_head against the float64 restatement
(tests/ssim_head_ref.py) in image and in head mode, with float and uint8-cache targets, then the layers above it: ops, the
calibration engine and the driver.

Bounds.  e32 is the error of the SAME restatement run in float32 against float64 on the same inputs: what the number format
alone costs.  The kernel is held to 4 * e32 plus 8 * 2^-24 of the value's scale (the project's convention, test_ssim_loss_gpu.py):
    |loss3 - ref| <= 4 e32 + 8 * 2^-24 |ref|                     per entry
    max|grad - ref| <= 4 e32_grad + 8 * 2^-24 max|grad_ref|      image mode and head mode, each against its own reference
The bias gradient is held to the float64 sum of the gradient the same call wrote: every backward workgroup adds its tile in
double and stores one float, the finishing launch adds those in double and stores one float, so the error is one fp32
rounding per stored partial plus one for the result, 2^-24 sum|dconv| each; with a margin of two
    |db[c] - sum64(dconv[:, c])| <= 2^-22 sum|dconv[:, c]|
Worst observed error / bound per shape is printed (run with -s) and recorded in DESIGN.md §21."""
import ctypes
import functools
import logging
import os

import numpy as np
import pytest
import torch

import msssim_ref as M
import ssim_head_ref as HR
from conftest import BITS, T, TINY_HNERV, state_dict_from_npz

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULPS = 8 * 2.0 ** -24
WEIGHTS = ((0.0, 1.0), (1.0, 0.0), (0.3, 0.7), (0.7, 0.3))
SENTINEL = -77.25
TH, TW = 8, 118                      # the kernel's tile (ops.SSIM_LOSS_TILE)
CROP = (2, 3, 64, 96)
SHAPES = [(1, 1, 11, 11),            # one valid pixel
          (2, 3, 12, 21),
          (1, 3, 11, 140),           # one valid row, two tiles wide
          (1, 3, 140, 11),           # one valid column, 18 backward tiles high
          (2, 3, TH + 10, TW + 10),  # exactly one forward tile
          (2, 3, TH + 11, TW + 11),  # one tile plus one row and one column
          (1, 3, 2 * TH + 13, 2 * TW + 7),
          CROP]                      # cut from the real frames
N_CACHE = 5
TARGETS = ("float", "cache", "cache_repeated")     # cache: idx [3, 1]; cache_repeated: idx [2, 2]


@functools.lru_cache(maxsize=None)
def _frames():
    return M.bunny_frames(2)


def _crop(shape):
    """the real frames' pixels from (301, 517) on, the first C channels"""
    B, C, H, W = shape
    return _frames()[:B, :C, 301:301 + H, 517:517 + W].contiguous()


@functools.lru_cache(maxsize=None)
def _cases(shape):
    """-> [(name, pred, tgt)] float32 CPU tensors: the inputs of test_ssim_loss_gpu.py"""
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
def _target(shape, name, kind):
    """-> (pred, tgt float32, cache uint8 or None, idx or None) on the CPU.  The cache holds N_CACHE frames: the case's target
    rounded to bytes at the indexed places, noise elsewhere; tgt is then what the bytes say, cache[idx] / 255."""
    pred, tgt = next((p, t) for n, p, t in _cases(shape) if n == name)
    if kind == "float":
        return pred, tgt, None, None
    B = shape[0]
    idx = torch.tensor(([3, 1] if kind == "cache" else [2, 2])[:B], dtype=torch.int64)
    g = torch.Generator().manual_seed(7)
    cache = torch.randint(0, 256, (N_CACHE,) + shape[1:], generator=g, dtype=torch.uint8)
    q = (tgt * 255).round().clamp(0, 255).to(torch.uint8)
    for b in range(B):
        cache[idx[b]] = q[b] if kind == "cache" else q[0]
    return pred, cache[idx].float() / 255.0, cache, idx


@functools.lru_cache(maxsize=None)
def _reference(shape, name, kind, weights):
    """-> dict of float64 numpy arrays: loss3, g_img, g_head and their bounds; computed once, shared, never written to"""
    pred, tgt, _, _ = _target(shape, name, kind)
    C = float(shape[1])
    r64 = HR.head_closed(pred, tgt, *weights, C)
    r32 = HR.head_closed(pred, tgt, *weights, C, dtype=torch.float32)
    out = {}
    for key, a, b in (("loss3", r64[0], r32[0]), ("g_img", r64[1], r32[1]), ("g_head", r64[2], r32[2])):
        a, b = a.numpy(), b.double().numpy()
        out[key] = a
        if key == "loss3":
            out["bound_" + key] = 4 * np.abs(b - a) + ULPS * np.abs(a)
        else:
            out["bound_" + key] = 4 * float(np.abs(b - a).max()) + ULPS * float(np.abs(a).max())
    for a in out.values():
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


def _run(pred, tgt=None, cache=None, idx=None, weights=(0.7, 0.3), head=True, scale=None):
    """one nq_ssim_loss_head call on guarded buffers -> (loss3, grad, db or None, per-frame SSIM) as tensors on the GPU"""
    from neuroquant_amd import _lib as L
    lib = L.lib()
    B, C, H, W = pred.shape
    pred = pred.to(DEV).contiguous()
    tgt = tgt.to(DEV).contiguous() if cache is None else None
    cache = cache.to(DEV).contiguous() if cache is not None else None
    idx = idx.to(DEV).contiguous() if cache is not None else None
    nws = lib.nq_ssim_loss_head_ws_floats(B, C, H, W)
    assert nws > 0
    bufs = {k: _guarded(m) for k, m in (("loss3", 3), ("grad", pred.numel()), ("db", C), ("ws", nws))}
    rc = lib.nq_ssim_loss_head(_ptr(pred), _ptr(tgt), _ptr(cache), _ptr(idx), _ptr(bufs["loss3"][1]), _ptr(bufs["grad"][1]),
                               _ptr(bufs["db"][1]) if head else None, _ptr(bufs["ws"][1]), B, C, H, W, weights[0], weights[1],
                               float(C) if scale is None else scale, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert _intact(buf, view), f"{k}: a sentinel next to the buffer was overwritten"
    if not head:
        assert bool((bufs["db"][1] == SENTINEL).all())
    return (bufs["loss3"][1].clone(), bufs["grad"][1].clone().view_as(pred), bufs["db"][1].clone() if head else None,
            bufs["ws"][1][:B].clone())


def _tanh_backward(dimg, img):
    from neuroquant_amd import _lib as L
    out = torch.empty_like(dimg)
    rc = L.lib().nq_tanh_out_backward(_ptr(dimg), _ptr(img), _ptr(out), dimg.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return out


def _db_ok(db, dconv):
    want = dconv.double().sum((0, 2, 3))
    room = 2.0 ** -22 * dconv.double().abs().sum((0, 2, 3))
    return bool(((db.double() - want).abs() <= room).all()), float(((db.double() - want).abs() / room.clamp_min(1e-300)).max())


def test_tile_constants():
    from neuroquant_amd import ops
    assert ops.SSIM_LOSS_TILE == (TH, TW)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_kernel_against_float64(shape):
    """every case, weight pair and kind of target of one shape, image and head mode: values, gradient, bias gradient; head mode
    is the tanh backward of image mode bit for bit; a cache target equals the float target gather_frames_u8 makes of it, in
    every output; two calls agree bit for bit"""
    from neuroquant_amd import ops
    worst = dict(loss3=0.0, g_img=0.0, g_head=0.0, db=0.0)
    where = {}
    for name, _, _ in _cases(shape):
        for kind in TARGETS:
            pred, tgt, cache, idx = _target(shape, name, kind)
            for weights in WEIGHTS:
                ref = _reference(shape, name, kind, weights)
                i3, ig, none, iframe = _run(pred, tgt, cache, idx, weights, head=False)
                h3, hg, hdb, hframe = _run(pred, tgt, cache, idx, weights, head=True)
                a3, ag, adb, aframe = _run(pred, tgt, cache, idx, weights, head=True)
                assert none is None
                j3, jg, _, jframe = _run(pred, tgt, cache, idx, weights, head=False)         # two calls agree, in both modes
                assert torch.equal(i3, j3) and torch.equal(ig, jg) and torch.equal(iframe, jframe)
                assert torch.equal(h3, a3) and torch.equal(hg, ag) and torch.equal(hdb, adb) and torch.equal(hframe, aframe)
                assert torch.equal(i3, h3) and torch.equal(iframe, hframe)
                assert torch.equal(hg, _tanh_backward(ig, pred.to(DEV)))
                if cache is not None:
                    gathered = ops.gather_frames_u8(cache.to(DEV), idx.to(DEV))
                    assert torch.equal(gathered.cpu(), tgt)
                    f3, fg, fdb, fframe = _run(pred, gathered, None, None, weights, head=True)
                    assert torch.equal(f3, h3) and torch.equal(fg, hg) and torch.equal(fdb, hdb) and torch.equal(fframe, hframe)
                    assert torch.equal(_run(pred, gathered, None, None, weights, head=False)[1], ig)
                r3 = float((np.abs(h3.double().cpu().numpy() - ref["loss3"]) / ref["bound_loss3"]).max())
                ri = float(np.abs(ig.double().cpu().numpy() - ref["g_img"]).max()) / ref["bound_g_img"]
                rh = float(np.abs(hg.double().cpu().numpy() - ref["g_head"]).max()) / ref["bound_g_head"]
                ok_db, rdb = _db_ok(hdb, hg)
                print(f"ssim_loss_head {shape} {name} {kind} {weights}: error / bound  loss3 {r3:.3f}  image grad {ri:.3f}  "
                      f"head grad {rh:.3f}  db {rdb:.3f}")
                for k, v in (("loss3", r3), ("g_img", ri), ("g_head", rh), ("db", rdb)):
                    if v > worst[k]:
                        worst[k], where[k] = v, (name, kind, weights)
                assert r3 <= 1.0 and ri <= 1.0 and rh <= 1.0 and ok_db, (name, kind, weights, r3, ri, rh, rdb)
    print(f"ssim_loss_head {shape}: worst error / bound  " + "  ".join(f"{k} {v:.3f} at {where.get(k)}" for k, v in worst.items()))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_image_mode_is_nq_ssim_loss(shape):
    """float target, db == NULL: the gradient, MSE, SSIM and per-frame SSIM of nq_ssim_loss(grad_scale = C) bit for bit, and
    loss3[0] within one fp32 ulp of C * L"""
    from neuroquant_amd import _lib as L
    lib = L.lib()
    B, C, H, W = shape
    for name, pred, tgt in _cases(shape):
        p, t = pred.to(DEV), tgt.to(DEV)
        for weights in WEIGHTS:
            loss3, grad, _, frame = _run(pred, tgt, None, None, weights, head=False)
            old3, old_grad = torch.empty(3, device=DEV), torch.empty_like(p)
            ws = torch.empty(lib.nq_ssim_loss_ws_floats(B, C, H, W), device=DEV)
            rc = lib.nq_ssim_loss(_ptr(p), _ptr(t), _ptr(old3), _ptr(old_grad), _ptr(ws), B, C, H, W, weights[0], weights[1],
                                  float(C), torch.cuda.current_stream().cuda_stream)
            assert rc == 0
            torch.cuda.synchronize()
            assert torch.equal(grad, old_grad) and torch.equal(loss3[1:], old3[1:]) and torch.equal(frame, ws[:B])
            want = float(C) * float(old3[0].double())
            assert abs(float(loss3[0].double()) - want) <= float(np.spacing(np.float32(want))), (name, weights)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_identical_images(shape):
    """pred == tgt: loss3 == [0, 0, 1] and (at most) a few ulps of gradient, in both modes and from the cache"""
    cache = (_crop(shape) * 255).round().to(torch.uint8)
    exact = cache.float() / 255.0
    for img in (exact, _cases(shape)[0][1], _cases(shape)[1][1]):
        for weights in WEIGHTS:
            for head in (False, True):
                loss3, grad, db, frame = _run(img, img.clone(), None, None, weights, head=head)
                assert loss3.tolist() == [0.0, 0.0, 1.0]
                assert frame.tolist() == [1.0] * shape[0]
                assert float(grad.abs().max()) <= ULPS
                if head:       # the sum of B H W values of at most 8 * 2^-24 each, and the sum of what was written
                    assert float(db.abs().max()) <= shape[0] * shape[2] * shape[3] * ULPS
                    assert _db_ok(db, grad)[0]
    B, _, H, W = shape
    loss3, grad, db, _ = _run(exact, None, cache, torch.arange(B), (0.7, 0.3), head=True)
    assert loss3.tolist() == [0.0, 0.0, 1.0] and float(grad.abs().max()) <= ULPS
    assert float(db.abs().max()) <= B * H * W * ULPS and _db_ok(db, grad)[0]


def test_a_frame_depends_on_its_own_bytes_only():
    """frame 0 of a B = 2 call equals the B = 1 call on frame 0 alone: its SSIM bit for bit, its gradient up to the factor
    1 / B of the mean over frames (a power of two: exact)"""
    for shape in (SHAPES[1], SHAPES[5], CROP):
        for kind in ("float", "cache"):
            pred, tgt, cache, idx = _target(shape, "noisy0.02", kind)
            for head in (False, True):
                _, g2, _, f2 = _run(pred, tgt, cache, idx, (0.7, 0.3), head=head)
                _, g1, _, f1 = _run(pred[:1], tgt[:1], cache, idx[:1] if idx is not None else None, (0.7, 0.3), head=head)
                assert f2[0] != f2[1]
                assert torch.equal(f2[:1], f1)
                assert torch.equal(g2[:1] * 2, g1)


@pytest.mark.parametrize("shape", [(2, 3, 64, 64), (1, 3, 32, 128)], ids=str)
def test_mse_only_is_the_l2_tanh_head(shape):
    """weights (1, 0) with scale = C against nq_l2_loss_tanh_head where that kernel applies (H W % 4096 == 0): loss and dconv
    within the bounds of test_kernel_against_float64 (both kernels round the same float64 values).  db: the two kernels sum
    their own gradients, so db is compared through the exact (float64) sums of the two written tensors: ours is within
    2^-22 sum|grad| of its sum (the bound of test_kernel_against_float64), the other kernel adds in fp32 over 4096-element chunks
    (a tree of depth 12 plus the chunk and frame sums: 16 roundings, 2^-20 sum|dconv|), and the two exact sums differ by what the
    written tensors say, nothing assumed.  Against the float64 reference's db only the worst case holds: every element off by
    bound_grad in the same direction."""
    from neuroquant_amd import ops
    B, C, H, W = shape
    g = torch.Generator().manual_seed(H + W)
    tgt = torch.rand(shape, generator=g)
    pred = (tgt + 0.05 * torch.randn(shape, generator=g)).clamp(0.01, 0.99)
    cache = (tgt * 255).round().to(torch.uint8)
    for kind in ("float", "cache"):
        t = tgt if kind == "float" else cache.float() / 255.0
        r64 = HR.head_closed(pred, t, 1.0, 0.0, float(C))
        r32 = HR.head_closed(pred, t, 1.0, 0.0, float(C), dtype=torch.float32)
        bound_l = 4 * abs(float(r32[0][0]) - float(r64[0][0])) + ULPS * float(r64[0][0])
        bound_g = 4 * float((r32[2].double() - r64[2]).abs().max()) + ULPS * float(r64[2].abs().max())
        kw = dict(tgt=t.to(DEV)) if kind == "float" else dict(cache_u8=cache.to(DEV), idx=torch.arange(B, device=DEV))
        loss, dconv, db = ops.l2_loss_tanh_head_raw(pred.to(DEV), **kw)
        if kind == "float":
            loss3, grad, mine, _ = _run(pred, t, None, None, (1.0, 0.0), head=True)
        else:
            loss3, grad, mine, _ = _run(pred, None, cache, torch.arange(B), (1.0, 0.0), head=True)
        assert abs(float(loss3[0]) - float(r64[0][0])) <= bound_l and abs(float(loss) - float(r64[0][0])) <= bound_l
        assert abs(float(loss3[0]) - float(loss)) <= bound_l
        assert float((grad.double().cpu() - r64[2]).abs().max()) <= bound_g
        assert float((grad - dconv).abs().max()) <= bound_g
        sum_mine, sum_other = grad.double().sum((0, 2, 3)), dconv.double().sum((0, 2, 3))
        mass_mine, mass_other = grad.double().abs().sum((0, 2, 3)), dconv.double().abs().sum((0, 2, 3))
        assert bool(((mine.double() - sum_mine).abs() <= 2.0 ** -22 * mass_mine).all())
        room = (sum_mine - sum_other).abs() + 2.0 ** -22 * mass_mine + 2.0 ** -20 * mass_other
        print(f"ssim_loss_head {shape} {kind}: |db - db of l2_loss_tanh_head| / room {float(((mine.double() - db.double()).abs() / room).max()):.3f}")
        assert bool(((mine.double() - db.double()).abs() <= room).all())
        assert bool(((mine.double().cpu() - r64[3]).abs() <= B * H * W * bound_g + 2.0 ** -22 * mass_mine.cpu()).all())


def test_ops_wrapper_counts_and_hands_over():
    from neuroquant_amd import ops
    shape = SHAPES[1]
    pred, tgt, cache, idx = _target(shape, "uniform", "cache")
    p, t = pred.to(DEV), tgt.to(DEV)
    before = ops.ssim_loss_head_launches
    loss3, g = ops.ssim_loss_head_grad(p, tgt=t, w_mse=0.3, w_ssim=0.7)                      # no hand-over slot: image mode
    want3, want_g, _, _ = _run(pred, tgt, None, None, (0.3, 0.7), head=False)
    assert torch.equal(loss3, want3) and torch.equal(g, want_g)
    loss3c, gc = ops.ssim_loss_head_grad(p, cache_u8=cache.to(DEV), idx=idx.to(DEV), w_mse=0.3, w_ssim=0.7)
    assert torch.equal(loss3c, want3) and torch.equal(gc, want_g)

    class Node:
        nq_head = ops._HeadHandoff()
    loss3h, gh = ops.ssim_loss_head_grad(p, tgt=t, w_mse=0.3, w_ssim=0.7, node=Node)
    h3, hg, hdb, _ = _run(pred, tgt, None, None, (0.3, 0.7), head=True)
    assert torch.equal(loss3h, h3) and torch.equal(gh, hg) and gh is Node.nq_head.dconv and torch.equal(Node.nq_head.db, hdb)
    assert Node.nq_head.version == gh._version
    assert ops.ssim_loss_head_launches == before + 3
    with pytest.raises(ValueError):
        ops.ssim_loss_head_grad(p, tgt=t, cache_u8=cache.to(DEV), idx=idx.to(DEV))
    with pytest.raises(ValueError):
        ops.ssim_loss_head_grad(p, tgt=t, w_mse=0.0, w_ssim=0.0)
    assert ops.ssim_loss_head_launches == before + 3


# ------------------------------------------------------------------------------------------ calibration engine
SSIM = dict(w_mse=0.7, w_ssim=0.3)


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


def test_calibration_first_ada_iteration_gradients(golden):
    """six iterations (two of phase 1, four of phase 2) with ssim=dict(0.7, 0.3): every parameter gradient of the first `ada`
    iteration, and the dL/dW^, dL/db^ behind it, equal what the SAME backward gives when it is fed C times the float64
    restatement's dL/dpred (the tolerances of test_ssim_loss_gpu.py::test_trainer_step_gradients)"""
    from neuroquant_amd import ops
    from neuroquant_amd.quantization import model_reconstruction
    z, qnn, emb = _tiny_qnn(golden)
    frames = (T(golden("frames_320x640.npz")["frames"]).float() / 255.0).to(DEV)
    batches = [dict(img=frames[i:i + 2], idx=torch.arange(i, i + 2), norm_idx=torch.arange(i, i + 2).float() / 8) for i in (0, 2)]
    got = {}

    def probe(phase, layers, grads):
        if phase != "ada" or got:
            return
        got["arena"] = [(L.W.grad.clone(), L.b.grad.clone()) for L in layers]
        got["params"] = [g.clone() for g in grads]
        # the same weights (the engine's overrides are still in place), the same batch, the same backward
        img, inputs = batches[0]["img"], emb[batches[0]["idx"].to(DEV)]
        for L in layers:
            L.W.grad = L.b.grad = None
        out = qnn(inputs)[0]
        ref3, ref_grad = HR.head_closed(out, img, SSIM["w_mse"], SSIM["w_ssim"], 3.0)[:2]       # C * dL/dpred: image mode
        got["rec"] = float(ref3[0])
        out.backward(ref_grad.float().to(DEV))
        got["ref_arena"] = [(L.W.grad.clone(), L.b.grad.clone()) for L in layers]
        items = []
        for L in layers:
            wq, bq = L.m.weight_quantizer, L.m.bias_quantizer
            items.append((L.src, L.W.grad, wq.alpha.data, wq.delta.data, wq.zero_point, wq.n_levels, 0.0))
            items.append((L.bias, L.b.grad, bq.alpha.data, bq.delta.data, bq.zero_point, bq.n_levels, 0.0))
        got["ref_params"] = [g.clone() for g in ops.adaround_backward_multi(items, 0)]   # (count 1 < warmup: regulariser off)

    rec = []
    before = ops.ssim_loss_head_launches
    model_reconstruction(qnn, cali_data=emb, gt=batches, arch="hnerv", batch_size=2, iters=40, weight=0.01, hadamard=False,
                         b_range=(20, 2), warmup=0.2, lr=0.003, recorder=rec, max_steps=6, probe=probe, ssim=SSIM)
    assert len(rec) == 6 and ops.ssim_loss_head_launches == before + 6
    assert rec[2][1] == 0.0 and abs(rec[2][0] - got["rec"]) <= 1e-5 * got["rec"]            # the logged rec is loss3[0]
    assert len(got["params"]) == len(got["ref_params"]) == 2 * len(got["arena"]) and len(got["arena"]) > 4

    def close(a, b):
        np.testing.assert_allclose(a.double().cpu().numpy(), b.double().cpu().numpy(), rtol=5e-3,
                                   atol=2e-4 * float(b.abs().max()) + 1e-9)

    for (gw, gb), (rw, rb) in zip(got["arena"], got["ref_arena"]):
        close(gw, rw)
        close(gb, rb)
    for g, r in zip(got["params"], got["ref_params"]):
        close(g, r)


def test_calibration_captured_equals_eager_and_default_launches_none(golden, monkeypatch):
    """8 iterations from a CacheLoader (targets read from the uint8 cache; in phase 2 three run eagerly, one is captured, the
    rest replay): every delta and alpha bit-identical with NQ_GRAPH=0.  A run with default arguments issues no
    nq_ssim_loss_head."""
    from neuroquant_amd import ops
    from neuroquant_amd.quantization import model_reconstruction
    from neuroquant_amd.utils import CacheLoader, FrameCache
    frames_u8 = T(golden("frames_320x640.npz")["frames"]).to(DEV)

    def run(graph, **kw):
        monkeypatch.setenv("NQ_GRAPH", "1" if graph else "0")
        z, qnn, emb = _tiny_qnn(golden)
        order = np.asarray(z["order"])[:, :2]
        before = ops.ssim_loss_head_launches
        model_reconstruction(qnn, cali_data=emb, gt=CacheLoader(FrameCache(frames_u8), list(range(8)), 2, order=order),
                             arch="hnerv", batch_size=2, iters=40, weight=0.01, hadamard=False, b_range=(20, 2), warmup=0.2,
                             lr=0.003, max_steps=8, **kw)
        return _params(qnn), ops.ssim_loss_head_launches - before

    eager, n_e = run(False, ssim=SSIM)
    graphed, n_g = run(True, ssim=SSIM)
    assert n_e == 8 and 0 < n_g < 8              # replays launch through the graph, not through the wrapper
    assert len(eager) == len(graphed) == 28
    for a, b in zip(eager, graphed):
        assert torch.equal(a, b)
    rgb, n_rgb = run(True)
    assert n_rgb == 0
    assert any(not torch.equal(a, b) for a, b in zip(rgb, graphed))          # the objective changes the result


def test_staged_form_hands_over_like_the_autograd_node(golden):
    """the hand-driven decoder of the data-parallel captured form (node=): ops.decoder_forward_manual + ssim_loss_head_grad(node=)
    + decoder_backward_steps leave the loss, the head gradient and every weight and bias gradient that the autograd node leaves
    from the same weights (the same kernels stage by stage; 1e-5 of the largest entry covers a different arena layout)"""
    from neuroquant_amd import ops
    from neuroquant_amd.models._decode import _fused_stack
    z, qnn, emb = _tiny_qnn(golden)
    frames_u8 = T(golden("frames_320x640.npz")["frames"]).to(DEV)
    idx = torch.tensor([5, 2], device=DEV)
    spec, provs = _fused_stack(qnn.model)
    with torch.no_grad():
        weights = [tuple(t.detach().clone() for t in p()) for p in provs]
    inputs = emb[idx]
    leaves = [(W.clone().requires_grad_(True), b.clone().requires_grad_(True)) for W, b in weights]
    out = ops.decoder_stack(inputs, spec, leaves)
    loss3, g = ops.ssim_loss_head_grad(out, cache_u8=frames_u8, idx=idx, **SSIM)
    assert isinstance(out.grad_fn.nq_head, ops._HeadHandoff) and g is out.grad_fn.nq_head.dconv      # head mode taken
    out.backward(g)
    img_out, node = ops.decoder_forward_manual(inputs, spec, weights, two_phase=True)
    assert torch.equal(img_out, out.detach())
    loss3m, gm = ops.ssim_loss_head_grad(img_out, cache_u8=frames_u8, idx=idx, node=node, **SSIM)
    assert gm is node.nq_head.dconv and torch.equal(loss3m, loss3) and torch.equal(gm, g)
    steps = ops.decoder_backward_steps(node, gm)
    while True:
        try:
            next(steps)
        except StopIteration as fin:
            res = fin.value
            break
    assert len(leaves) > 4
    for i, (W, b) in enumerate(leaves):
        for want, got in ((W.grad, res[2 + 2 * i]), (b.grad, res[3 + 2 * i])):
            assert want is not None and got is not None
            np.testing.assert_allclose(got.double().cpu().numpy(), want.double().cpu().numpy(), rtol=0,
                                       atol=1e-5 * float(want.abs().max()) + 1e-30)


# ------------------------------------------------------------------------------------------ driver
def test_driver_calibrates_on_fusion5_and_reports_ssim(tmp_path, monkeypatch):
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
                              "--precision", "6", "5", "4", "5", "5", "6", "6", "--rec_loss", "Fusion5"])
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
    assert seen["ssim"] == dict(w_mse=0.7, w_ssim=0.3) and seen["loss_domain"] == "rgb"
    lines = [ln for ln in log.splitlines() if "ssim objective" in ln and ": SSIM " in ln]
    assert len(lines) == 4                                                   # FP, off, on, calibrated
    m = args.eval_metrics
    assert set(cn.METRIC_NAMES) | {cn.SSIM_METRIC_NAME} == set(m)
    assert 0.0 < float(m[cn.SSIM_METRIC_NAME]) <= 1.0
    assert "best_pred_seen_psnr" in log and "best_" + cn.SSIM_METRIC_NAME not in log   # the report line keeps its four entries
    assert len(rec) > 0
    for total, rl, b, count in rec:
        assert np.isfinite(total - rl) and total - rl > 0.0                  # rec = loss3[0]

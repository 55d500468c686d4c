"""MS-SSIM on the GPU (ops.ms_ssim -> nq_ms_ssim, neuroquant_amd/csrc/msssim.hip) against the float64 restatement of the
definition (tests/msssim_ref.py), and through the evaluation of the drivers.

Tolerance of every parity figure: |gpu - f64| <= max(4 * e32, 1e-6), never more than 5e-5, where e32 is the largest
|ms_ssim(fp32 on the CPU) - ms_ssim(float64)| of the same case, both from the helper (neither is the code under test).
4 x: another summation order; 1e-6: ~16 fp32 ulps at 1.0, for the cases where the CPU's fp32 run happens to land within
an ulp; 5e-5: half a unit of the fourth decimal the drivers print.  pytorch_msssim is not installed anywhere this
project runs: parity with the package's last bits is not pinned."""
import logging
import re
import types

import pytest
import torch
import torch.nn.functional as F

import msssim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
CROPS = [(161, 161), (176, 208), (323, 645), (480, 960)]


def _tolerance(X, Y, want):
    e32 = (R.ms_ssim_f64(X, Y, dtype=torch.float32).double() - want).abs().max().item()
    return min(max(4 * e32, 1e-6), 5e-5), e32


def _check(tag, X, Y):
    from neuroquant_amd import ops
    want = R.ms_ssim_f64(X, Y)
    tol, e32 = _tolerance(X, Y, want)
    got = ops.ms_ssim(X.to(DEV).contiguous(), Y.to(DEV).contiguous())
    assert got.shape == (X.shape[0],) and got.dtype == torch.float32 and got.is_cuda
    err = (got.cpu().double() - want).abs().max().item()
    print(f"{tag}: f64 {[round(v, 6) for v in want.tolist()]} gpu {[round(v, 6) for v in got.tolist()]} "
          f"err {err:.2e} e32 {e32:.2e} tol {tol:.2e}")
    return err, tol


@pytest.fixture(scope="module")
def pairs():
    """two calls of two frames, a different degradation for every frame of a call: (tag, X, Y)."""
    Y = R.bunny_frames(2)
    a = torch.cat([R.noisy(Y[:1], 0.014, seed=1), R.noisy(Y[1:], 0.05, seed=2)])
    b = torch.cat([R.posterised(Y[:1]), R.box_blurred(Y[1:])])
    return [("noise 0.014 | noise 0.05", a, Y), ("posterised | box blur", b, Y)]


def test_parity_full_size(pairs):
    bad = []
    for tag, X, Y in pairs:
        err, tol = _check(f"640x1280 {tag}", X, Y)
        if err > tol:
            bad.append((tag, err, tol))
    assert not bad, bad


@pytest.mark.parametrize("h,w", CROPS)
def test_parity_crops(pairs, h, w):
    """the minimum size, sizes that are no multiple of the tile, odd sizes (pooling with padding)."""
    bad = []
    for tag, X, Y in pairs:
        top, left = 120, 300
        err, tol = _check(f"{h}x{w} {tag}", X[:, :, top:top + h, left:left + w].contiguous(),
                          Y[:, :, top:top + h, left:left + w].contiguous())
        if err > tol:
            bad.append((tag, err, tol))
    assert not bad, bad


def test_known_answers_and_reproducibility():
    from neuroquant_amd import ops
    Y = R.bunny_frames(8).to(DEV)
    one = torch.ones(2, device=DEV)
    assert torch.equal(ops.ms_ssim(Y[:2], Y[:2]), one)                       # identical -> exactly 1
    assert torch.equal(ops.ms_ssim(1 - Y[:2], Y[:2]), 0 * one)               # inverted -> relu, 0^w = 0
    g = torch.Generator(device=DEV).manual_seed(5)
    X = (Y + 0.02 * torch.randn(Y.shape, device=DEV, generator=g)).clamp(0, 1)
    all8 = ops.ms_ssim(X, Y)
    print("8 frames", all8.tolist())
    assert all8.shape == (8,) and bool(((all8 > 0.9) & (all8 < 1)).all())
    assert torch.equal(ops.ms_ssim(X[:1], Y[:1]), all8[:1])                  # F = 1 and F = 8: the same bits for frame 0
    assert torch.equal(ops.ms_ssim(X[5:6], Y[5:6]), all8[5:6])
    assert torch.equal(ops.ms_ssim(X, Y), all8)                              # call to call
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = ops.ms_ssim(X, Y)
    side.synchronize()
    assert torch.equal(on_side, all8)
    # inputs are detached: no gradient is recorded
    Xr = X[:1].clone().requires_grad_(True)
    assert not ops.ms_ssim(Xr, Y[:1]).requires_grad
    from neuroquant_amd import utils
    single = utils.msssim_fn_single(X[:2], Y[:2])
    batch = utils.msssim_fn_batch([X[:2], Y[:2]], Y[:2])
    assert not single.is_cuda and torch.equal(single, all8[:2].cpu())
    assert batch.shape == (2, 2) and torch.equal(batch[0], single) and torch.equal(batch[1], torch.ones(2))


def test_small_frames_raise():
    from neuroquant_amd import ops
    z = torch.zeros(1, 3, 160, 640, device=DEV)
    with pytest.raises(ValueError):
        ops.ms_ssim(z, z)
    with pytest.raises(RuntimeError):
        ops.ms_ssim(z, z[:, :, :, :600])


def _args(n):
    from neuroquant_amd.utils import data_split
    args = types.SimpleNamespace(arch="hnerv", print_freq=50, data_split="1_1_1")
    _, args.val_ind_list = data_split(list(range(n)), [int(x) for x in args.data_split.split("_")], False, 0)
    return args


def test_evaluate_reports_msssim_of_the_trained_model(caplog):
    """HNeRV-3M of the committed checkpoint fixture on the first four of its eight real frames, through the drivers'
    evaluate().  The fixture holds the decoder and the embeddings only (its encoder is untrained), so encode() hands out
    the stored embedding of the frame evaluate() is at."""
    import tools_path  # noqa: F401
    import precision_gate as pg
    from neuroquant_amd.methods.calibrate_network import evaluate
    from neuroquant_amd.utils import FrameCache
    model, emb, _ = pg.load_fixture_checkpoint("hnerv3m_bunny8real_f16.npz", DEV)
    frames_u8 = pg.bunny_real_640(DEV, 8)[:4].contiguous()
    calls = []

    def encode(img):
        calls.append(1)
        return emb[len(calls) - 1:len(calls)]

    model.encode = encode
    args = _args(4)
    assert args.val_ind_list == []
    with caplog.at_level(logging.INFO):
        res, embeds = evaluate(model, FrameCache(frames_u8), args, pg.HNERV_3M)
    assert len(res) == 2 and len(embeds) == 4 and len(calls) == 4
    m = args.eval_metrics
    assert list(m) == ["pred_seen_psnr", "pred_seen_ssim", "pred_unseen_psnr", "pred_unseen_ssim"]
    assert torch.equal(m["pred_seen_psnr"], res[0]) and torch.equal(m["pred_unseen_psnr"], res[1])
    assert float(res[1]) == 0.0 and float(m["pred_unseen_ssim"]) == 0.0

    frames = frames_u8.float().cpu() / 255.0
    with torch.no_grad():
        decoded = torch.cat([model.decode(emb[i:i + 1])[0] for i in range(4)]).cpu()
    want = R.ms_ssim_f64(decoded, frames)
    tol, e32 = _tolerance(decoded, frames, want)
    got = float(m["pred_seen_ssim"])
    print(f"evaluate: PSNR {float(res[0]):.3f} MS-SSIM {got:.7f} f64 per frame {want.tolist()} mean {want.mean().item():.7f} "
          f"e32 {e32:.2e} tol {tol:.2e}")
    assert abs(got - want.mean().item()) <= tol
    lines = [r.getMessage() for r in caplog.records if "Eval at Step" in r.getMessage()]
    print(lines)
    assert lines and all(re.search(r"PSNR \d+\.\d+, MS-SSIM 0\.9\d{1,3}$", ln) for ln in lines)
    assert abs(float(lines[-1].rsplit(" ", 1)[1]) - got) <= 5.1e-5            # the mean of the four, to four decimals


class _BlurModel:
    """stand-in for a model at a size no shipped stride set can build: decode() returns a blurred copy of the frame."""

    def eval(self):
        return self

    def train(self):
        return self

    def encode(self, img):
        return img

    def decode(self, emb):
        c = emb.shape[1]
        k = torch.full((c, 1, 3, 3), 1.0 / 9.0, device=emb.device)
        return F.conv2d(F.pad(emb, (1, 1, 1, 1), mode="replicate"), k, groups=c), [emb], 1e-3


def test_evaluate_on_small_frames_keeps_psnr_and_stores_nan(caplog):
    from neuroquant_amd.methods.calibrate_network import evaluate
    from neuroquant_amd.utils import FrameCache
    frames_u8 = (R.bunny_frames(3)[:, :, 200:296, 400:528] * 255).round().to(torch.uint8).to(DEV).contiguous()
    args = _args(3)
    with caplog.at_level(logging.INFO):
        res, embeds = evaluate(_BlurModel(), FrameCache(frames_u8), args, {"batch_size": 1})
    assert len(embeds) == 3 and 10.0 < float(res[0]) < 60.0 and float(res[1]) == 0.0
    assert torch.isnan(args.eval_metrics["pred_seen_ssim"]) and torch.equal(args.eval_metrics["pred_seen_psnr"], res[0])
    assert any(r.getMessage().endswith("MS-SSIM n/a") for r in caplog.records)

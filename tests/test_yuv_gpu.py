"""8-bit YUV 4:2:0 on the GPU: the two conversion kernels held bit-exact to the numpy float32 restatement (tests/yuv_ref.py) on
both of their paths, the exact plane error sums, the player's out='yuv420', and the decode_stream / load_frames drivers on a
.y4m file they wrote themselves.  Every shape is tiny."""
import numpy as np
import pytest
import torch

import yuv_ref as R
from conftest import TINY_HNERV
from test_bitstream_gpu import _quant_model        # the way that module builds its tiny quantised HNeRV

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 64
PAIRS = [(m, fr) for m in ("bt709", "bt601") for fr in (False, True)]
# (n, H, W): one block; the block kernel with chroma rows of odd length; (1, 6, 10); the smallest vector shape; vector shapes
SHAPES = [(1, 2, 2), (2, 4, 6), (1, 6, 10), (3, 2, 8), (2, 16, 32), (1, 10, 24)]
CODE = {"bt601": 0, "bt709": 1}


@pytest.fixture(scope="module")
def ops():
    from neuroquant_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _raw(fn_name, src, n, H, W, matrix, full_range, out_bytes):
    """the C entry into a buffer with SENT sentinel bytes after its end -> (output bytes, sentinels) on the host"""
    from neuroquant_amd import _lib
    buf = torch.full((out_bytes + SENT,), 0xA5, dtype=torch.uint8, device=DEV)
    _lib.check(getattr(_lib.lib(), fn_name)(src.data_ptr(), buf.data_ptr(), n, H, W, CODE[matrix], int(full_range), _stream()),
               fn_name)
    buf = buf.cpu().numpy()
    return buf[:out_bytes], buf[out_bytes:]


@pytest.mark.parametrize("matrix, full_range", PAIRS)
@pytest.mark.parametrize("shape", SHAPES)
def test_frames_to_yuv420_bit_exact(ops, shape, matrix, full_range):
    n, H, W = shape
    x = R.edge_frames(n, H, W, seed=n * 1000 + H * 10 + W)
    want = R.rgb_to_yuv420(x, matrix, full_range)
    fb = R.frame_bytes(H, W)
    assert want.shape == (n, fb)
    x_d = torch.from_numpy(x).to(DEV)
    assert x_d.data_ptr() % 16 == 0
    got = ops.frames_to_yuv420(x_d, matrix, full_range)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, fb)
    assert np.array_equal(got.cpu().numpy(), want)
    runs = [_raw("nq_frames_to_yuv420", x_d, n, H, W, matrix, full_range, n * fb) for _ in range(2)]
    for out, sent in runs:
        assert np.array_equal(out.reshape(n, fb), want) and (sent == 0xA5).all()
    assert np.array_equal(runs[0][0], runs[1][0])
    if W % 8 == 0:      # the same floats one element into a buffer: not 16-byte aligned, the block kernel takes them
        off = torch.cat([torch.zeros(1, device=DEV), x_d.reshape(-1)])[1:]
        assert off.data_ptr() % 16 != 0
        out, sent = _raw("nq_frames_to_yuv420", off, n, H, W, matrix, full_range, n * fb)
        assert np.array_equal(out.reshape(n, fb), want) and (sent == 0xA5).all()


@pytest.mark.parametrize("matrix, full_range", PAIRS)
@pytest.mark.parametrize("shape", SHAPES)
def test_yuv420_to_rgb_u8_bit_exact(ops, shape, matrix, full_range):
    n, H, W = shape
    fb = R.frame_bytes(H, W)
    buf = np.random.default_rng(n * 1000 + H * 10 + W).integers(0, 256, size=(n, fb), dtype=np.uint8)
    buf.reshape(-1)[:4] = (0, 255, 16, 235)[:min(4, buf.size)]
    want = R.yuv420_to_rgb(buf, H, W, matrix, full_range)
    b_d = torch.from_numpy(buf).to(DEV)
    got = ops.yuv420_to_rgb_u8(b_d, H, W, matrix, full_range)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, 3, H, W)
    assert np.array_equal(got.cpu().numpy(), want)
    runs = [_raw("nq_yuv420_to_rgb_u8", b_d, n, H, W, matrix, full_range, n * 3 * H * W) for _ in range(2)]
    for out, sent in runs:
        assert np.array_equal(out.reshape(n, 3, H, W), want) and (sent == 0xA5).all()
    if W % 8 == 0:      # one byte into a buffer: the block kernel
        off = torch.cat([torch.zeros(1, dtype=torch.uint8, device=DEV), b_d.reshape(-1)])[1:]
        assert off.data_ptr() % 8 != 0
        out, sent = _raw("nq_yuv420_to_rgb_u8", off, n, H, W, matrix, full_range, n * 3 * H * W)
        assert np.array_equal(out.reshape(n, 3, H, W), want) and (sent == 0xA5).all()
    if n == 1:          # one flat frame
        assert np.array_equal(ops.yuv420_to_rgb_u8(b_d[0], H, W, matrix, full_range).cpu().numpy(), want)


# (2, 4, 6), (3, 16, 32): byte loads / 16-byte loads, one workgroup per frame; (1, 50, 62): two workgroups, the second partly
# past the frame, byte loads; (2, 64, 96): three workgroups per frame, both plane boundaries inside the second
@pytest.mark.parametrize("shape", [(2, 4, 6), (3, 16, 32), (1, 50, 62), (2, 64, 96)])
def test_yuv420_sse_exact(ops, shape):
    n, H, W = shape
    fb = R.frame_bytes(H, W)
    rng = np.random.default_rng(H * W)
    a = rng.integers(0, 256, size=(n, fb), dtype=np.uint8)
    b = rng.integers(0, 256, size=(n, fb), dtype=np.uint8)
    a[0, :3], b[0, :3] = 255, 0                     # the largest difference
    want = R.plane_sse(a, b, H, W)
    a_d, b_d = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    got = [ops.yuv420_sse(a_d, b_d, H, W) for _ in range(2)]
    assert got[0].dtype == torch.int64 and tuple(got[0].shape) == (n, 3)
    assert np.array_equal(got[0].cpu().numpy(), want) and torch.equal(got[0], got[1])
    px = np.array([H * W, H * W // 4, H * W // 4], dtype=np.float64)
    psnr = ops.yuv420_psnr(a_d, b_d, H, W)
    assert psnr.dtype == torch.float64
    np.testing.assert_allclose(psnr.cpu().numpy(), 10 * np.log10(255.0 ** 2 * px / want), rtol=1e-12)
    assert not ops.yuv420_sse(a_d, a_d.clone(), H, W).any()
    assert bool(torch.isinf(ops.yuv420_psnr(a_d, a_d.clone(), H, W)).all())
    # only one plane differs
    c = a.copy()
    c[:, H * W] ^= 1                                # the first U sample of every frame
    only_u = ops.yuv420_sse(a_d, torch.from_numpy(c).to(DEV), H, W).cpu().numpy()
    assert np.array_equal(only_u, np.array([[0, 1, 0]] * n))


# ------------------------------------------------------------------------------------------ player and drivers
@pytest.fixture(scope="module")
def stream_path(golden, tmp_path_factory):
    """a stream of the tiny HNeRV (8 frames of 320 x 640), quantisers straight after their initialisation; read-only"""
    from neuroquant_amd.bitstream import write_stream
    z, qnn, emb = _quant_model(golden, "traj_hnerv.npz", "hnerv", False)
    path = tmp_path_factory.mktemp("yuv") / "m.nqv"
    write_stream(qnn, str(path), "hnerv", dict(TINY_HNERV), embeddings=emb)
    return str(path)


def test_player_yuv420(ops, stream_path):
    from neuroquant_amd.bitstream import StreamDecoder
    dec = StreamDecoder(stream_path)
    f0, u0 = dec.decode([0, 1]), dec.decode([0, 1], out="u8")
    for matrix, full_range in PAIRS:
        got = dec.decode([0, 1], out="yuv420", matrix=matrix, full_range=full_range)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 320 * 640 * 3 // 2)
        assert torch.equal(got, ops.frames_to_yuv420(dec.decode([0, 1]), matrix, full_range))
    assert torch.equal(dec.decode([0, 1], out="yuv420"), ops.frames_to_yuv420(f0))       # bt709, limited
    assert np.array_equal(dec.decode([0, 1], out="yuv420").cpu().numpy(), R.rgb_to_yuv420(f0.cpu().numpy()))
    assert torch.equal(dec.decode([0, 1]), f0) and torch.equal(dec.decode([0, 1], out="float"), f0)
    assert torch.equal(dec.decode([0, 1], out="u8"), u0) and torch.equal(u0, ops.frames_to_u8(f0))
    assert torch.equal(dec.decode([0, 1], out="u8", layout="hwc"), u0.permute(0, 2, 3, 1))
    with pytest.raises(ValueError):
        dec.decode([0], out="yuv420", layout="hwc")
    with pytest.raises(ValueError):
        dec.decode([0], out="yuv420", matrix="bt2020")
    with pytest.raises(ValueError):
        dec.decode([0], out="yuv")


def test_drivers_write_and_read_y4m(ops, stream_path, tmp_path):
    from neuroquant_amd.bitstream import StreamDecoder
    from neuroquant_amd.methods import decode_stream as DS
    from neuroquant_amd.methods.calibrate_network import load_frames, parse_args as cn_args
    from neuroquant_amd.videoio import open_yuv, write_y4m
    out = str(tmp_path / "tmp.y4m")
    res = DS.run(DS.parse_args(["--stream", stream_path, "--out", out, "--fps", "25", "--batch_size", "2"]))
    dec = StreamDecoder(stream_path)
    clip = open_yuv(out)
    assert (clip.H, clip.W, clip.frames, clip.fps, clip.full_range) == (320, 640, dec.frames, (25, 1), False)
    assert res["frames"] == dec.frames == 8 and "psnr_y" not in res and "psnr" not in res
    own = clip.read(0, clip.frames)
    played = torch.cat([dec.decode([j, j + 1], out="yuv420") for j in range(0, dec.frames, 2)])
    assert np.array_equal(own, played.cpu().numpy())
    # the same file as ground truth: its own bytes against the decoded 4:2:0 frames
    res = DS.main(["--stream", stream_path, "--frames", out, "--batch_size", "2"])
    for k in ("psnr_y", "psnr_u", "psnr_v", "psnr_yuv_611"):
        assert np.isinf(float(res[k])) and float(res[k]) > 0, k
    for k in ("psnr", "psnr_u8", "ssim", "ssim_u8"):
        assert np.isfinite(float(res[k])), k
    # a raw .yuv next to it holds the same bytes, in full range on request
    raw = str(tmp_path / "tmp_640x320.yuv")
    DS.run(DS.parse_args(["--stream", stream_path, "--out", raw, "--range", "full", "--matrix", "bt601"]))
    full = torch.cat([dec.decode([j], out="yuv420", matrix="bt601", full_range=True) for j in range(dec.frames)])
    assert np.array_equal(open_yuv(raw).read(0, 8), full.cpu().numpy())
    # load_frames: the calibration drivers' view of the clip
    args = cn_args(["--arch", "hnerv", "--data_path", out])
    gt = load_frames(args, dict(TINY_HNERV), DEV)
    want = ops.yuv420_to_rgb_u8(torch.from_numpy(own).to(DEV), 320, 640)
    assert gt.dtype == torch.uint8 and tuple(gt.shape) == (8, 3, 320, 640) and torch.equal(gt, want)
    one = load_frames(cn_args(["--arch", "hnerv", "--data_path", out, "--yuv_frames", "1"]), dict(TINY_HNERV), DEV)
    assert tuple(one.shape) == (1, 3, 320, 640) and torch.equal(one, want[:1])
    from types import SimpleNamespace
    bare = load_frames(SimpleNamespace(synthetic=0, seed=0, data_path=out), dict(TINY_HNERV), DEV)   # no yuv_* attributes
    assert torch.equal(bare, want)
    # a larger clip is centre-cropped: RGB rows / columns of the converted frame
    big = np.random.default_rng(5).integers(0, 256, size=(2, 324 * 644 * 3 // 2), dtype=np.uint8)
    with write_y4m(str(tmp_path / "big.y4m"), 324, 644) as f:
        f.write(big)
    got = load_frames(cn_args(["--arch", "hnerv", "--data_path", str(tmp_path / "big.y4m")]), dict(TINY_HNERV), DEV)
    assert torch.equal(got, ops.yuv420_to_rgb_u8(torch.from_numpy(big).to(DEV), 324, 644)[:, :, 2:322, 2:642])
    with write_y4m(str(tmp_path / "small.y4m"), 318, 640) as f:
        f.write(np.zeros((1, 318 * 640 * 3 // 2), np.uint8))
    with pytest.raises(ValueError, match="smaller"):
        load_frames(cn_args(["--arch", "hnerv", "--data_path", str(tmp_path / "small.y4m")]), dict(TINY_HNERV), DEV)
    # a centre crop that starts on an odd row cannot crop the chroma planes
    with write_y4m(str(tmp_path / "odd.y4m"), 322, 640) as f:
        f.write(np.zeros((1, 322 * 640 * 3 // 2), np.uint8))
    with pytest.raises(ValueError, match="must be even"):
        DS.run(DS.parse_args(["--stream", stream_path, "--frames", str(tmp_path / "odd.y4m")]))

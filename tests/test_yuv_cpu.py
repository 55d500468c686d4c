"""8-bit YUV 4:2:0 video in and out, host side (no GPU): known answers and properties of the numpy restatement of the
conversions (tests/yuv_ref.py), the .y4m / .yuv container code (neuroquant_amd/videoio.py), and the argument checks of the
C entries and their ops wrappers before any device call."""
import ctypes

import numpy as np
import pytest

import yuv_ref as R
from neuroquant_amd.videoio import (centre_crop_offsets, crop_yuv420, open_yuv, parse_fps, parse_size, write_y4m)

PAIRS = [(m, fr) for m in ("bt709", "bt601") for fr in (False, True)]


def _flat(rgb):
    """colours (k, 3) in [0, 1] -> k flat 2 x 2 frames (k, 3, 2, 2) float32"""
    c = np.asarray(rgb, dtype=np.float32).reshape(-1, 3)
    return np.broadcast_to(c[:, :, None, None], (c.shape[0], 3, 2, 2)).copy()


# ------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("matrix, full_range, colour, want", [
    ("bt709", False, (1, 1, 1), (235, 128, 128)),
    ("bt709", False, (0, 0, 0), (16, 128, 128)),
    ("bt709", False, (1, 0, 0), (63, 102, 240)),
    ("bt709", False, (0, 1, 0), (173, 42, 26)),
    ("bt709", False, (0, 0, 1), (32, 240, 118)),
    ("bt709", True, (1, 0, 0), (54, 99, 255)),
    ("bt601", False, (1, 0, 0), (81, 90, 240)),
    ("bt601", True, (0, 0, 1), (29, 255, 107)),
])
def test_known_answers(matrix, full_range, colour, want):
    got = R.rgb_to_yuv420(_flat([colour]), matrix, full_range)
    assert got.shape == (1, 6) and got.dtype == np.uint8
    assert got[0].tolist() == [want[0]] * 4 + [want[1], want[2]]


def test_constants_are_the_documented_floats():
    """the floats listed in csrc/yuv.hip and DESIGN.md §16"""
    want = dict(bt601=dict(kr="0x1.322d0ep-2", kg="0x1.2c8b44p-1", kb="0x1.d2f1aap-4", icb="0x1.20f066p-1", icr="0x1.6d314ep-1",
                           c_r="0x1.66e978p+0", c_b="0x1.c5a1cap+0", c_gb="0x1.606544p-2", c_gr="0x1.6da346p-1"),
                bt709=dict(kr="0x1.b367a0p-3", kg="0x1.6e2eb2p-1", kb="0x1.27bb30p-4", icb="0x1.13ebeap-1", icr="0x1.451ee2p-1",
                           c_r="0x1.932618p+0", c_b="0x1.db089ap+0", c_gb="0x1.7fa3dep-3", c_gr="0x1.df5bf8p-2"))
    for m, table in want.items():
        k = R.constants(m)
        for name, text in table.items():
            assert float(k[name]) == float.fromhex(text), (m, name)
        for name, text in (("i219", "0x1.2b404ap-8"), ("i224", "0x1.24924ap-8"), ("i255", "0x1.010102p-8")):
            assert float(k[name]) == float.fromhex(text)


@pytest.mark.parametrize("matrix, full_range", PAIRS)
def test_float32_restatement_against_float64(matrix, full_range):
    """Every float32 code lies within 0.5 + 1e-3 of the unrounded float64 value and at most 1 from the float64 code.  The
    margin is derived, not measured: the values are at most 256 in magnitude and pass through about ten float32 roundings
    (2^-24 relative each) and constants rounded to float32, an error of about 1e-4."""
    x = R.edge_frames(3, 16, 24, seed=7)
    x[1, :, 4:8, 6:12] = np.nan                   # a NaN patch
    got = R.rgb_to_yuv420(x, matrix, full_range).astype(np.float64)
    exact = R.rgb_to_yuv420_f64(x, matrix, full_range)
    assert got.shape == exact.shape == (3, R.frame_bytes(16, 24))
    err = np.abs(got - exact).max()
    code64 = np.clip(np.rint(exact), 0, 255)
    print("%s full=%s: max |code - float64 value| %.6f, max code difference %d" % (matrix, full_range, err,
                                                                                    int(np.abs(got - code64).max())))
    assert err <= 0.5 + 1e-3
    assert np.abs(got - code64).max() <= 1
    # the NaN patch is black
    black = R.rgb_to_yuv420(np.zeros((1, 3, 2, 2), np.float32), matrix, full_range)[0]
    assert got[1, 4 * 24 + 6] == black[0] and got[1, 16 * 24 + 2 * 12 + 3] == black[4]


@pytest.mark.parametrize("matrix", ("bt709", "bt601"))
@pytest.mark.parametrize("full_range, bound_colours, bound_greys", [(False, 2, 1), (True, 1, 0)])
def test_round_trip_rgb8(matrix, full_range, bound_colours, bound_greys):
    """RGB8 -> YUV -> RGB8 on flat 2 x 2 blocks: properties of the arithmetic, not tolerances."""
    colours = np.random.default_rng(0).integers(0, 256, size=(2000, 3))
    greys = np.repeat(np.arange(256)[:, None], 3, axis=1)
    for c, bound in ((colours, bound_colours), (greys, bound_greys)):
        x = _flat(c.astype(np.float32) / np.float32(255))
        yuv = R.rgb_to_yuv420(x, matrix, full_range)
        back = R.yuv420_to_rgb(yuv, 2, 2, matrix, full_range)
        err = np.abs(back.astype(np.int64) - c[:, :, None, None]).max()
        print("%s full=%s: round-trip max error %d (bound %d)" % (matrix, full_range, err, bound))
        assert err <= bound
        if c is greys:
            assert (yuv[:, 4:] == 128).all()


def test_plane_layout_and_block_mean():
    """Y row-major, then U, then V; chroma is the mean of its 2 x 2 block, not a sample of it"""
    x = np.zeros((1, 3, 2, 4), np.float32)
    x[0, :, :, 2:] = 1.0                          # right block white
    x[0, 0, 0, 0] = 1.0                           # one red pixel in the left block
    got = R.rgb_to_yuv420(x, "bt709", False)[0]
    assert got[:8].tolist() == [63, 16, 235, 235, 16, 16, 235, 235]
    assert got[8:].tolist() == [122, 128, 156, 128]     # (102 - 128) / 4 and (240 - 128) / 4 off 128, rounded
    rgb = R.yuv420_to_rgb(got[None], 2, 4)
    assert rgb.shape == (1, 3, 2, 4) and (rgb[0, :, :, 2:] == 255).all()


# ------------------------------------------------------------------------------------------ videoio
def _frames(k, H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(k, H * W * 3 // 2), dtype=np.uint8)


@pytest.mark.parametrize("H, W", [(2, 2), (6, 10)])
def test_y4m_round_trip(tmp_path, H, W):
    fr = _frames(3, H, W)
    path = str(tmp_path / "a.y4m")
    with write_y4m(path, H, W, fps=(30000, 1001), full_range=True) as f:
        f.write(fr[:2])
        f.write(fr[2])                             # one flat frame
    data = open(path, "rb").read()
    head = b"YUV4MPEG2 W%d H%d F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n" % (W, H)
    assert data.startswith(head + b"FRAME\n") and len(data) == len(head) + 3 * (6 + fr.shape[1])
    clip = open_yuv(path)
    assert (clip.H, clip.W, clip.frames, clip.fps, clip.full_range) == (H, W, 3, (30000, 1001), True)
    assert np.array_equal(clip.read(0, 3), fr) and np.array_equal(clip.read(1, 2), fr[1:]) and clip.read(3, 0).shape == (0, fr.shape[1])
    assert clip.read(0, 3).dtype == np.uint8
    with pytest.raises(ValueError):
        clip.read(2, 2)
    with pytest.raises(ValueError):
        open_yuv(path, size=(W + 2, H))
    with write_y4m(str(tmp_path / "b.y4m"), H, W) as f:
        with pytest.raises(ValueError):
            f.write(fr[:, :-1])
    assert open(tmp_path / "b.y4m", "rb").read() == b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n" % (W, H)
    assert open_yuv(str(tmp_path / "b.y4m")).frames == 0 and open_yuv(str(tmp_path / "b.y4m")).full_range is False
    with pytest.raises(ValueError):
        write_y4m(str(tmp_path / "c.y4m"), 3, 4)


def _y4m(tmp_path, name, tags, body):
    p = tmp_path / name
    p.write_bytes(b"YUV4MPEG2 " + tags + b"\n" + body)
    return str(p)


def test_y4m_headers_accepted_and_refused(tmp_path):
    fr = _frames(2, 2, 4).tobytes()
    body = b"FRAME\n" + fr[:12] + b"FRAME Ixyz\n" + fr[12:]          # FRAME lines may carry parameters
    for i, chroma in enumerate((b"", b" C420", b" C420jpeg", b" C420mpeg2", b" C420paldv")):
        clip = open_yuv(_y4m(tmp_path, "ok%d.y4m" % i, b"W4 H2 F25:1 Ip A1:1" + chroma, body))
        assert (clip.H, clip.W, clip.frames, clip.full_range) == (2, 4, 2, None)
        assert clip.read(0, 2).tobytes() == fr
    for name, tags, word in (("il.y4m", b"W4 H2 F25:1 It A1:1 C420jpeg", "It"), ("c422.y4m", b"W4 H2 F25:1 Ip C422", "C422"),
                             ("p10.y4m", b"W4 H2 F25:1 Ip C420p10", "C420p10"), ("mono.y4m", b"W4 H2 Ip Cmono", "Cmono")):
        with pytest.raises(ValueError, match=word):
            open_yuv(_y4m(tmp_path, name, tags, body))
    with pytest.raises(ValueError, match="cut short"):               # the last frame lacks one byte
        open_yuv(_y4m(tmp_path, "short.y4m", b"W4 H2 F25:1 Ip C420jpeg", body[:-1]))
    with pytest.raises(ValueError):
        open_yuv(_y4m(tmp_path, "noframe.y4m", b"W4 H2 F25:1 Ip C420jpeg", b"FRAMF\n" + fr[:12]))
    with pytest.raises(ValueError):
        open_yuv(_y4m(tmp_path, "nosize.y4m", b"W4 F25:1 Ip", body))
    with pytest.raises(ValueError):
        open_yuv(_y4m(tmp_path, "odd.y4m", b"W3 H2 F25:1 Ip", body))
    (tmp_path / "other.y4m").write_bytes(b"RIFF....")
    with pytest.raises(ValueError):
        open_yuv(str(tmp_path / "other.y4m"))


def test_raw_yuv_size_from_name_or_argument(tmp_path):
    fr = _frames(3, 6, 10)
    named = tmp_path / "clip_10x6_420.yuv"
    named.write_bytes(fr.tobytes())
    clip = open_yuv(str(named))
    assert (clip.W, clip.H, clip.frames, clip.fps, clip.full_range) == (10, 6, 3, None, None)
    assert np.array_equal(clip.read(0, 3), fr) and np.array_equal(clip.read(2, 1), fr[2:])
    dotted = tmp_path / "clip_10x6.yuv"
    dotted.write_bytes(fr.tobytes())
    assert open_yuv(str(dotted)).frames == 3
    plain = tmp_path / "clip.yuv"
    plain.write_bytes(fr.tobytes())
    with pytest.raises(ValueError, match="size"):
        open_yuv(str(plain))
    assert open_yuv(str(plain), size=(10, 6)).frames == 3
    assert open_yuv(str(named), size=(6, 10)).H == 10                # the argument wins over the name
    ragged = tmp_path / "ragged_10x6.yuv"
    ragged.write_bytes(fr.tobytes()[:-1])
    with pytest.raises(ValueError, match="whole number"):
        open_yuv(str(ragged))


def test_crop_yuv420(tmp_path):
    H, W, h, w = 8, 12, 4, 8
    fr = _frames(2, H, W)
    assert centre_crop_offsets(H, W, h, w) == (2, 2)
    got = crop_yuv420(fr, H, W, 2, 2, h, w)
    Y = fr[:, :H * W].reshape(2, H, W)[:, 2:6, 2:10]
    U = fr[:, H * W:H * W * 5 // 4].reshape(2, H // 2, W // 2)[:, 1:3, 1:5]
    V = fr[:, H * W * 5 // 4:].reshape(2, H // 2, W // 2)[:, 1:3, 1:5]
    assert np.array_equal(got, np.concatenate([Y.reshape(2, -1), U.reshape(2, -1), V.reshape(2, -1)], axis=1))
    assert np.array_equal(crop_yuv420(fr, H, W, 0, 0, H, W), fr)
    with pytest.raises(ValueError, match="even"):
        crop_yuv420(fr, H, W, 1, 2, h, w)
    with pytest.raises(ValueError, match="even"):
        crop_yuv420(fr, H, W, 2, 3, h, w)
    with pytest.raises(ValueError):
        crop_yuv420(fr, H, W, 6, 2, h, w)
    with pytest.raises(ValueError, match="smaller"):
        centre_crop_offsets(2, 12, h, w)
    assert parse_fps("25") == (25, 1) and parse_fps("30000:1001") == (30000, 1001) and parse_size("1920x1080") == (1920, 1080)
    for bad in ("0", "a", "30:0", "-1"):
        with pytest.raises(ValueError):
            parse_fps(bad)


# ------------------------------------------------------------------------------------------ C ABI and ops without a GPU
@pytest.fixture(scope="module")
def lib():
    from neuroquant_amd import _lib
    return _lib.lib()


def test_frame_bytes(lib):
    from neuroquant_amd import ops
    assert lib.nq_yuv420_frame_bytes(6, 10) == 90 == ops.yuv420_frame_bytes(6, 10) == R.frame_bytes(6, 10)
    assert lib.nq_yuv420_frame_bytes(1080, 1920) == 1080 * 1920 * 3 // 2
    for H, W in ((5, 10), (6, 9), (0, 10), (6, 0), (-6, 10), (6, -10), (-6, -10)):
        assert lib.nq_yuv420_frame_bytes(H, W) == 0
    assert lib.nq_yuv420_frame_bytes(2 ** 32, 2 ** 31) == 0          # the product of 3 planes is past int64


def test_launch_entries_reject_bad_arguments_without_a_device(lib):
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    INVALID = -1
    for fn in (lib.nq_frames_to_yuv420, lib.nq_yuv420_to_rgb_u8):
        # (src, dst, n, H, W, matrix, full_range, stream)
        assert fn(None, p, 1, 2, 2, 1, 0, None) == INVALID
        assert fn(p, None, 1, 2, 2, 1, 0, None) == INVALID
        for n, H, W in ((0, 2, 2), (-1, 2, 2), (1, 3, 2), (1, 2, 3), (1, 0, 2), (1, 2, -2), (2 ** 40, 2 ** 30, 2 ** 30)):
            assert fn(p, p, n, H, W, 1, 0, None) == INVALID, (n, H, W)
        for matrix, fr in ((2, 0), (-1, 0), (0, 2), (1, -1)):
            assert fn(p, p, 1, 2, 2, matrix, fr, None) == INVALID
    # nq_yuv420_sse(a, b, sse, n, H, W, stream)
    for hole in range(3):
        args = [p, p, p]
        args[hole] = None
        assert lib.nq_yuv420_sse(*args, 1, 2, 2, None) == INVALID
    for n, H, W in ((0, 2, 2), (-1, 2, 2), (1, 3, 2), (1, 2, 3), (1, 0, 2), (2 ** 40, 2 ** 30, 2 ** 30)):
        assert lib.nq_yuv420_sse(p, p, p, n, H, W, None) == INVALID


def test_ops_wrappers_raise_value_error():
    import torch
    from neuroquant_amd import ops
    with pytest.raises(ValueError, match="frames_to_yuv420"):
        ops.frames_to_yuv420(torch.zeros(1, 3, 3, 4))                # odd H
    with pytest.raises(ValueError, match="frames_to_yuv420"):
        ops.frames_to_yuv420(torch.zeros(1, 3, 4, 5))                # odd W
    with pytest.raises(ValueError, match="frames_to_yuv420"):
        ops.frames_to_yuv420(torch.zeros(1, 4, 2, 2))                # not three planes
    with pytest.raises(ValueError, match="frames_to_yuv420"):
        ops.frames_to_yuv420(torch.zeros(3, 2, 2))
    with pytest.raises(ValueError, match="frames_to_yuv420"):
        ops.frames_to_yuv420(torch.zeros(1, 3, 2, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="frames_to_yuv420"):
        ops.frames_to_yuv420(torch.zeros(1, 3, 2, 2), matrix="bt2020")
    with pytest.raises(ValueError, match="yuv420_to_rgb_u8"):
        ops.yuv420_to_rgb_u8(torch.zeros(1, 6, dtype=torch.uint8), 2, 3)
    with pytest.raises(ValueError, match="yuv420_to_rgb_u8"):
        ops.yuv420_to_rgb_u8(torch.zeros(1, 7, dtype=torch.uint8), 2, 2)
    with pytest.raises(ValueError, match="yuv420_to_rgb_u8"):
        ops.yuv420_to_rgb_u8(torch.zeros(1, 6), 2, 2)                # float bytes
    with pytest.raises(ValueError, match="yuv420_to_rgb_u8"):
        ops.yuv420_to_rgb_u8(torch.zeros(1, 6, dtype=torch.uint8), 2, 2, matrix="rec709")
    with pytest.raises(ValueError, match="yuv420_sse"):
        ops.yuv420_sse(torch.zeros(1, 6, dtype=torch.uint8), torch.zeros(1, 7, dtype=torch.uint8), 2, 2)
    with pytest.raises(ValueError, match="yuv420_sse"):
        ops.yuv420_psnr(torch.zeros(1, 6, dtype=torch.uint8), torch.zeros(1, 6, dtype=torch.uint8), 3, 2)
    # well-formed arguments on the host: refused like every other op (no CPU path)
    with pytest.raises(RuntimeError):
        ops.frames_to_yuv420(torch.zeros(1, 3, 2, 2))
    with pytest.raises(RuntimeError):
        ops.yuv420_to_rgb_u8(torch.zeros(1, 6, dtype=torch.uint8), 2, 2)

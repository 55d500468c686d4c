"""Packed bit stream, host side (no GPU): known answers of the numpy restatement of the format (tests/bitstream_ref.py),
nq_packed_words against its formula, argument checks of the three launch entries before any device call, and the package's
container reader on files written by the restatement's writer."""
import ctypes
import json
import struct

import numpy as np
import pytest

import bitstream_ref as R


@pytest.fixture(scope="module")
def lib():
    from neuroquant_amd import _lib
    return _lib.lib()


def test_reference_packer_known_answers():
    w = R.pack([1, 2, 3], 2)                       # 01 | 10 << 2 | 11 << 4
    assert w.dtype == np.dtype("<u4") and w.tolist() == [0x39]
    # 11 three-bit levels: level 10 occupies bits 30..32 and straddles words 0 and 1
    lv = np.array([7, 0, 5, 2, 1, 6, 3, 4, 7, 0, 0b101], dtype=np.uint8)
    w = R.pack(lv, 3)
    want = sum(int(v) << (3 * i) for i, v in enumerate(lv))
    assert w.tolist() == [want & 0xFFFFFFFF, want >> 32] and len(w) == 2
    assert (w[0] >> 30) == 0b01 and w[1] == 0b1     # low two bits of level 10 end word 0, its top bit starts word 1
    assert np.array_equal(R.unpack(w, 11, 3), lv)
    for b in range(1, 9):                          # round trip at every width, tail bits zero
        rng = np.random.default_rng(b)
        lv = rng.integers(0, 2 ** b, size=77, dtype=np.uint8)
        w = R.pack(lv, b)
        assert len(w) == R.packed_words(77, b) and np.array_equal(R.unpack(w, 77, b), lv)
        assert int(w[-1]) >> ((77 * b - 1) % 32 + 1) == 0


def test_packed_words_matches_the_formula(lib):
    for b in range(1, 9):
        for n in (1, 31, 32, 33, 4097):
            assert lib.nq_packed_words(n, b) == -(-(n * b) // 32) == R.packed_words(n, b)
    for b in (0, 9, -1):
        assert lib.nq_packed_words(32, b) == 0
    for b in range(1, 9):
        assert lib.nq_packed_words(0, b) == 0 and lib.nq_packed_words(-5, b) == 0
    assert lib.nq_packed_words(2 ** 62, 8) == 0    # n * n_bits past int64: refused, not wrapped


def test_launch_entries_reject_bad_arguments_without_a_device(lib):
    buf = (ctypes.c_uint32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    INVALID = -1
    # nq_pack_levels(levels, words, n, n_bits, stream)
    assert lib.nq_pack_levels(None, p, 32, 4, None) == INVALID
    assert lib.nq_pack_levels(p, None, 32, 4, None) == INVALID
    assert lib.nq_pack_levels(p, p, 0, 4, None) == INVALID
    assert lib.nq_pack_levels(p, p, -1, 4, None) == INVALID
    for b in (0, 9, -3):
        assert lib.nq_pack_levels(p, p, 32, b, None) == INVALID
    # nq_unpack_dequant(words, delta, zp, w, rows, row_len, n_bits, stream)
    for hole in range(4):
        args = [p, p, p, p]
        args[hole] = None
        assert lib.nq_unpack_dequant(*args, 2, 8, 4, None) == INVALID
    assert lib.nq_unpack_dequant(p, p, p, p, 0, 8, 4, None) == INVALID
    assert lib.nq_unpack_dequant(p, p, p, p, 2, 0, 4, None) == INVALID
    assert lib.nq_unpack_dequant(p, p, p, p, -2, 8, 4, None) == INVALID
    for b in (0, 9):
        assert lib.nq_unpack_dequant(p, p, p, p, 2, 8, b, None) == INVALID
    # nq_frames_to_u8(src, dst, n, C, HW, layout, stream)
    assert lib.nq_frames_to_u8(None, p, 1, 3, 4, 0, None) == INVALID
    assert lib.nq_frames_to_u8(p, None, 1, 3, 4, 0, None) == INVALID
    for n, C, HW in ((0, 3, 4), (1, 0, 4), (1, 3, 0), (-1, 3, 4)):
        assert lib.nq_frames_to_u8(p, p, n, C, HW, 0, None) == INVALID
    for layout in (-1, 2):
        assert lib.nq_frames_to_u8(p, p, 1, 3, 4, layout, None) == INVALID


def test_ops_refuse_cpu_tensors():
    import torch
    from neuroquant_amd import ops
    with pytest.raises(RuntimeError):
        ops.pack_levels(torch.zeros(32, dtype=torch.uint8), 4)
    with pytest.raises(RuntimeError):
        ops.unpack_dequant(torch.zeros(4, dtype=torch.int32), torch.ones(1), torch.zeros(1), (32,), 4)
    with pytest.raises(RuntimeError):
        ops.frames_to_u8(torch.zeros(1, 3, 2, 2))


def _sample(path, version=1):
    rng = np.random.default_rng(0)
    lv = rng.integers(0, 8, size=5 * 7, dtype=np.uint8)
    sections = [("w0.levels", "u32", R.pack(lv, 3)),
                ("w0.delta", "f16", np.array([0.5, 0.25, 1.0, 2.0, 0.125], dtype=np.float16)),   # 10 bytes: padded to 12
                ("w0.zero_point", "f32", np.arange(5, dtype=np.float32)),
                ("b0.soft", "f32", rng.standard_normal(5).astype(np.float32))]
    header = dict(arch="hnerv", cfg=dict(crop_h=2, crop_w=2), frames=1, hadamard=False, bias="soft", embedding_shape=None,
                  layers=[dict(shape=[5, 7, 1, 1], c_in_stored=7, n_bits=3, scale_rows=5, delta_dtype="f16",
                               zero_point_dtype="f32")])
    return R.write(str(path), header, sections, version=version), sections, lv


def test_read_container_parses_a_reference_file(tmp_path):
    from neuroquant_amd.bitstream import read_container
    path = tmp_path / "a.nqv"
    written, sections, lv = _sample(path)
    header, sec = read_container(str(path))
    assert header == written and header["version"] == 1
    assert list(sec) == [s[0] for s in sections]
    for name, tag, arr in sections:
        assert sec[name].dtype == np.dtype(R.DTYPES[tag]) and np.array_equal(sec[name], arr)
    assert np.array_equal(R.unpack(sec["w0.levels"], 35, 3), lv)
    offs = [s["offset"] for s in header["sections"]]
    assert all(o % 4 == 0 for o in offs) and offs[2] == offs[1] + 12


def test_read_container_rejects_damaged_files(tmp_path):
    from neuroquant_amd.bitstream import read_container
    path = tmp_path / "a.nqv"
    header, _, _ = _sample(path)
    good = path.read_bytes()

    def refused(data, name):
        f = tmp_path / name
        f.write_bytes(data)
        with pytest.raises(ValueError):
            read_container(str(f))

    refused(b"NQV2" + good[4:], "magic.nqv")
    refused(good[:-1], "short.nqv")                 # one byte gone from the last section
    refused(good[:10], "header_cut.nqv")
    v2 = tmp_path / "v2.nqv"
    _sample(v2, version=2)
    with pytest.raises(ValueError):
        read_container(str(v2))

    def rewrite(mutate, name):
        (hlen,) = struct.unpack("<I", good[4:8])
        h = json.loads(good[8:8 + hlen])
        mutate(h)
        hj = json.dumps(h).encode()
        refused(b"NQV1" + struct.pack("<I", len(hj)) + hj.ljust(R.align4(8 + len(hj)) - 8, b"\0") + good[R.align4(8 + hlen):], name)

    def past_end(h):
        h["sections"][-1]["count"] += 4
        h["sections"][-1]["bytes"] += 16
    rewrite(past_end, "past_end.nqv")

    def overlap(h):
        h["sections"][1]["offset"] -= 4
    rewrite(overlap, "overlap.nqv")


def test_stored_tensors_checks_packed_tensors_on_the_host(tmp_path):
    """A packed tensor is validated before any upload: its section present, u32 and exactly packed_words(n, n_bits) long."""
    from neuroquant_amd.bitstream import coded_tensors, read_container, stored_tensors
    path = tmp_path / "a.nqv"
    _, sections, _ = _sample(path)
    header, sec = read_container(str(path))
    stored = stored_tensors(header, sec)
    assert list(stored) == ["w0"]
    w0 = stored["w0"]
    assert (w0.name, w0.coding, w0.n, w0.n_bits, w0.chunk) == ("w0", "packed", 35, 3, None)
    assert np.array_equal(w0.words, sections[0][2]) and len(w0.words) == R.packed_words(35, 3) == 4 and w0.nbytes == 16
    assert coded_tensors(header, sec) == {}
    words = sec["w0.levels"]
    damaged = {"missing": {k: v for k, v in sec.items() if k != "w0.levels"},
               "one word short": dict(sec, **{"w0.levels": words[:-1]}),
               "one word long": dict(sec, **{"w0.levels": np.concatenate([words, words[:1]])}),
               "f32": dict(sec, **{"w0.levels": words.view("<f4")})}
    for what, bad in damaged.items():
        with pytest.raises(ValueError, match="w0"):
            stored_tensors(header, bad, what)
        with pytest.raises(ValueError, match="w0"):     # the filter over it refuses the same files
            coded_tensors(header, bad, what)


def test_stored_tensors_on_a_coded_file(tmp_path):
    from neuroquant_amd.bitstream import coded_tensors, read_container, stored_tensors
    from test_rans_cpu import CHUNK, N_B, N_W, _coded_file
    path = tmp_path / "c.nqv"
    _coded_file(path)
    header, sec = read_container(str(path))
    stored = stored_tensors(header, sec)
    assert sorted(stored) == ["b0", "w0"]
    assert [(s.coding, s.n, s.n_bits, s.chunk) for s in (stored["w0"], stored["b0"])] == [("rans", N_W, 3, CHUNK), ("rans", N_B, 4, 64)]
    coded = coded_tensors(header, sec)
    assert sorted(coded) == ["b0", "w0"]
    for name, chunk in (("w0", CHUNK), ("b0", 64)):
        *parts, got_chunk = coded[name]
        assert got_chunk == chunk and len(parts) == 4
        for a, k in zip(parts, ("freq", "states", "offsets", "words")):
            assert a is sec[f"{name}.rans_{k}"]
        assert stored[name].nbytes == sum(a.nbytes for a in parts) and stored[name].words is parts[3]

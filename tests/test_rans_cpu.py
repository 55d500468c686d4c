"""Entropy-coded levels, host side (no GPU): known answers and round trips of the plain-Python restatement (tests/rans_ref.py),
the package's numpy encoder against it byte for byte, the size conditions `auto` rests on, nq_rans_chunks against its formula,
nq_rans_decode's argument checks before any device call, `u16` sections in the container reader, and the player's host
validation of damaged coded files, one file per rule."""
import ctypes
import struct

import numpy as np
import pytest

import bitstream_ref
import rans_ref as R

L = 1 << 16


@pytest.fixture(scope="module")
def lib():
    from neuroquant_amd import _lib
    return _lib.lib()


def _peaked(rng, n, b, sigma=1.5):
    return np.clip(np.rint(rng.normal((1 << b) / 2, sigma, n)), 0, (1 << b) - 1).astype(np.uint8)


def _rare(n, b):
    lv = np.full(n, min(3, (1 << b) - 1), dtype=np.uint8)
    lv[n // 3] = 0                                   # one occurrence among n
    return lv


# ------------------------------------------------------------------------------------------ restatement: known answers
def test_hand_computed_two_symbols_three_levels():
    """Two symbols over three levels, table f = [2048, 1024, 1024] (cum = [0, 2048, 3072]).  Symbol 0 is lane 0's, symbol 1 lane
    1's; both states start at 2^16 and neither reaches f << 20, so no word is emitted:
        lane 1, level 0: x = (65536 // 2048 << 12) + 65536 % 2048 + 0    = 131072
        lane 0, level 2: x = (65536 // 1024 << 12) + 65536 % 1024 + 3072 = 265216"""
    f, cum = [2048, 1024, 1024, 0], [0, 2048, 3072, 4096]
    states, words = R.encode_chunk([2, 0], f, cum)
    assert words == [] and states == [265216, 131072] + [L] * 62
    _, lut = R.tables(f)
    assert lut[3072] == 2 and lut[0] == 0 and lut[2047] == 0 and lut[2048] == 1
    # decode by hand: lane 0: slot = 265216 & 4095 = 3072 -> level 2, x = 1024 * 64 + 3072 - 3072 = 65536
    assert R.decode_chunk(states, words, 2, f, cum, lut) == [2, 0]


def test_hand_computed_renormalisation_word():
    """129 symbols, so lane 0 owns three (0, 64, 128) and every other lane two; table f = [2048, 1024, 1023, 1].  Lane 0 codes
    1, 1, 3 (encoded in the order 3, 1, 1):
        level 3 (f 1, cum 4095):     x = (65536 << 12) + 4095                          = 268439551
        level 1 (f 1024, cum 2048):  x = (268439551 // 1024 << 12) + 1023 + 2048       = 1073757183   (< 2^30: no word)
        level 1 again: 1073757183 >= 1024 << 20 -> emit 1073757183 & 0xffff = 15359, x = 16384
                                     x = (16384 // 1024 << 12) + 0 + 2048              = 67584
    Every other lane codes level 0 twice: 65536 -> 131072 -> 262144, no word."""
    f, cum = [2048, 1024, 1023, 1], [0, 2048, 3072, 4095]
    sym = [0] * 129
    sym[0], sym[64], sym[128] = 1, 1, 3
    states, words = R.encode_chunk(sym, f, cum)
    assert words == [15359] and states == [67584] + [262144] * 63
    assert R.decode_chunk(states, words, 129, f, cum, R.tables(f)[1]) == sym


def test_constant_tensor_costs_no_word():
    for n, chunk in ((1000, 64), (1000, 4096), (64, 64)):
        f, states, offsets, words = R.encode([5] * n, 6, chunk)
        assert f[5] == 4096 and sum(f) == 4096 and words == [] and offsets == [0] * (-(-n // chunk) + 1)
        assert all(s == L for s in states) and len(states) == 64 * -(-n // chunk)   # x = (x // 4096 << 12) + x % 4096 = x
        assert R.decode(f, states, offsets, words, n, chunk) == [5] * n


def test_single_symbol():
    f, states, offsets, words = R.encode([2], 3, 64)
    assert f == [0, 0, 4096, 0, 0, 0, 0, 0] and states == [L] * 64 and offsets == [0, 0] and words == []
    assert R.decode(f, states, offsets, words, 1, 64) == [2]


def test_normalisation_rule():
    assert R.normalise([1, 1, 1, 1]) == [1024] * 4
    assert R.normalise([3, 0, 1, 0]) == [3072, 0, 1024, 0]
    f = R.normalise([1, 49999, 0, 0])                 # floor(4096 / 50000) = 0 -> 1; the deficit goes to the largest count
    assert f == [1, 4095, 0, 0]
    f = R.normalise([100000] * 3 + [1] * 253)         # 253 floors of 0 lifted to 1 push the sum past 4096
    assert sum(f) == 4096 and min(f) == 1 and f[3:] == [1] * 253
    assert f[:3] == [1281] * 3                        # 3 * 1364 + 253 = 4345: the excess of 249 came off the largest, in turn
    assert R.normalise([100000] * 3 + [1] * 252 + [0])[:3] == [1281, 1281, 1282]   # 248 to shed: lowest symbol first
    assert R.normalise([0, 7, 0, 0]) == [0, 4096, 0, 0]


@pytest.mark.parametrize("b", range(1, 9))
def test_restatement_round_trip(b):
    rng = np.random.default_rng(b)
    for n in (1, 63, 64, 65, 129, 4097):
        for chunk in (64, 128):
            for kind in ("uniform", "peaked"):
                lv = (rng.integers(0, 1 << b, n) if kind == "uniform" else _peaked(rng, n, b)).tolist()
                f, states, offsets, words = R.encode(lv, b, chunk)
                chunks = -(-n // chunk)
                assert sum(f) == 4096 and len(f) == 1 << b and len(states) == 64 * chunks and len(offsets) == chunks + 1
                assert all(L <= s < 1 << 32 for s in states) and all(0 <= w < 1 << 16 for w in words)
                last = n - (chunks - 1) * chunk      # lanes without a symbol in the short last chunk keep 2^16
                assert all(s == L for s in states[64 * (chunks - 1) + last:64 * chunks])
                assert R.decode(f, states, offsets, words, n, chunk) == lv, (n, chunk, kind)   # asserts states and cursor too


# ------------------------------------------------------------------------------------------ package against restatement
CASES = [("uniform", 5, 4097, 64), ("uniform", 2, 4097, 128), ("uniform", 8, 1000, 4096), ("peaked", 6, 5000, 128),
         ("peaked", 4, 129, 64), ("peaked", 8, 4097, 64), ("rare", 2, 50000, 4096), ("rare", 6, 50000, 32768),
         ("constant", 3, 300, 64), ("uniform", 1, 65, 64), ("uniform", 7, 1, 64)]


@pytest.mark.parametrize("kind,b,n,chunk", CASES)
def test_package_encoder_equals_restatement_byte_for_byte(kind, b, n, chunk):
    from neuroquant_amd.bitstream import rans_encode, rans_normalise, rans_validate
    rng = np.random.default_rng(n + b)
    lv = {"uniform": lambda: rng.integers(0, 1 << b, n).astype(np.uint8), "peaked": lambda: _peaked(rng, n, b),
          "rare": lambda: _rare(n, b), "constant": lambda: np.full(n, 5, dtype=np.uint8)}[kind]()
    want = R.encode(lv.tolist(), b, chunk)
    got = rans_encode(lv.reshape(1, -1), b, chunk)
    assert [a.dtype for a in got] == [np.dtype("uint16"), np.dtype("uint32"), np.dtype("uint32"), np.dtype("uint16")]
    for g, w, fmt in zip(got, want, "HIIH"):
        assert g.astype("<u%d" % g.dtype.itemsize).tobytes() == struct.pack("<%d%s" % (len(w), fmt), *w)
    counts = np.bincount(lv, minlength=1 << b)
    assert rans_normalise(counts).tolist() == R.normalise(counts.tolist()) == want[0] and int(got[0].sum()) == 4096
    if kind == "rare":
        assert want[0][0] == 1
    rans_validate(*got, n, b, chunk)
    assert R.decode(*[a.tolist() for a in got], n, chunk) == lv.tolist()


def test_package_encoder_refuses_bad_arguments():
    from neuroquant_amd.bitstream import rans_encode
    lv = np.zeros(10, dtype=np.uint8)
    for b, chunk in ((0, 64), (9, 64), (4, 0), (4, 96), (4, -64)):
        with pytest.raises(ValueError):
            rans_encode(lv, b, chunk)
    with pytest.raises(ValueError):
        rans_encode(np.zeros(0, dtype=np.uint8), 4, 64)
    with pytest.raises(ValueError):
        rans_encode(np.array([4], dtype=np.uint8), 2, 64)


def test_coded_sizes_decide_auto():
    """Conditions, not measurements: 200 000 peaked 6-bit levels in one chunk cost less coded than packed (the restatement
    gives 66.7 KB against 150 KB); 4097 uniform 2-bit levels cost more (2 bits of entropy each plus 256 bytes of states per
    chunk and the table), so `auto` keeps them packed."""
    from neuroquant_amd.bitstream import rans_encode
    rng = np.random.default_rng(0)
    lv = _peaked(rng, 200_000, 6)
    got = rans_encode(lv, 6, 200_000 // 64 * 64 + 64)
    coded = sum((a.nbytes + 3) // 4 * 4 for a in got)
    packed = 4 * -(-200_000 * 6 // 32)
    assert len(got[2]) == 2 and coded == R.section_bytes(6, 1, len(got[3])) and coded < packed
    p = np.bincount(lv, minlength=64) / lv.size
    entropy = -(p[p > 0] * np.log2(p[p > 0])).sum() * lv.size / 8
    print("200000 peaked 6-bit levels: coded %d bytes, packed %d, entropy %.0f" % (coded, packed, entropy))
    assert entropy < coded < 1.02 * entropy           # 12-bit probabilities and 256 + 128 + 8 bytes of side information
    lv = rng.integers(0, 4, 4097).astype(np.uint8)
    got = rans_encode(lv, 2, 4160)
    assert sum((a.nbytes + 3) // 4 * 4 for a in got) > 4 * -(-4097 * 2 // 32)


# ------------------------------------------------------------------------------------------ C ABI, ops
def test_rans_chunks_matches_the_formula(lib):
    for n in (1, 63, 64, 65, 4097, 2 ** 40):
        for chunk in (64, 128, 4096, 32768):
            assert lib.nq_rans_chunks(n, chunk) == -(-n // chunk)
    for n, chunk in ((0, 64), (-1, 64), (10, 0), (10, -64), (10, 63), (10, 96), (10, 1)):
        assert lib.nq_rans_chunks(n, chunk) == 0


def test_rans_decode_rejects_bad_arguments_without_a_device(lib):
    buf = (ctypes.c_uint32 * 512)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    INVALID = -1
    # nq_rans_decode(words, states, offsets, freq, n, n_bits, chunk, delta, zp, row_len, levels, w, stream)
    for hole in range(4):
        args = [p, p, p, p]
        args[hole] = None
        assert lib.nq_rans_decode(*args, 64, 4, 64, p, p, 8, p, p, None) == INVALID
    for n in (0, -5):
        assert lib.nq_rans_decode(p, p, p, p, n, 4, 64, p, p, 8, p, p, None) == INVALID
    for b in (0, 9, -1):
        assert lib.nq_rans_decode(p, p, p, p, 64, b, 64, p, p, 8, p, p, None) == INVALID
    for chunk in (0, -64, 63, 96, 1):
        assert lib.nq_rans_decode(p, p, p, p, 64, 4, chunk, p, p, 8, p, p, None) == INVALID
    for row_len in (0, -8):
        assert lib.nq_rans_decode(p, p, p, p, 64, 4, 64, p, p, row_len, p, p, None) == INVALID
    assert lib.nq_rans_decode(p, p, p, p, 64, 4, 64, p, p, 8, None, None, None) == INVALID        # both outputs null
    assert lib.nq_rans_decode(p, p, p, p, 64, 4, 64, None, p, 8, p, p, None) == INVALID           # w wanted, no delta
    assert lib.nq_rans_decode(p, p, p, p, 64, 4, 64, p, None, 8, None, p, None) == INVALID        # w wanted, no zero-point
    assert lib.nq_rans_decode(p, p, p, p, 2 ** 32 + 5, 4, 64, p, p, 8, p, p, None) == -2          # 32-bit offsets: unsupported


def test_ops_refuse_cpu_tensors():
    import torch
    from neuroquant_amd import ops
    words, freq = torch.zeros(4, dtype=torch.int16), torch.zeros(16, dtype=torch.int16)
    states, offsets = torch.zeros(64, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ops.rans_decode(words, states, offsets, freq, 64, 4, 64)
    with pytest.raises(RuntimeError):
        ops.rans_decode_dequant(words, states, offsets, freq, torch.ones(1), torch.zeros(1), (64,), 4, 64)


# ------------------------------------------------------------------------------------------ container
N_W, N_B, CHUNK = 16 * 16 * 3 * 3, 16, 1024          # three chunks, the last short; 16 symbols a lane: words exist


def _coded_file(path, mutate=None, mutate_header=None):
    """one 3-bit (16, 16, 3, 3) layer with a coded weight and a coded 4-bit hard bias, both from the restatement's encoder;
    `mutate(parts)` damages the weight's {freq, states, offsets, words} lists, `mutate_header(layer)` its header entry."""
    rng = np.random.default_rng(5)
    wl, bl = _peaked(rng, N_W, 3), rng.integers(0, 16, N_B).astype(np.uint8)
    parts = dict(zip(("freq", "states", "offsets", "words"), (list(v) for v in R.encode(wl.tolist(), 3, CHUNK))))
    assert len(parts["words"]) > 3 and len(parts["offsets"]) == 4
    if mutate:
        mutate(parts)
    bparts = R.encode(bl.tolist(), 4, 64)
    tags = dict(freq="u16", states="u32", offsets="u32", words="u16")
    sections = [(f"w0.rans_{k}", tags[k], np.array(v, dtype=np.int64)) for k, v in parts.items()]
    sections += [("w0.delta", "f16", np.full(16, 0.5, dtype=np.float16)), ("w0.zero_point", "f32", np.arange(16, dtype=np.float32))]
    sections += [(f"b0.rans_{k}", tags[k], np.array(v, dtype=np.int64)) for k, v in zip(tags, bparts)]
    sections += [("b0.delta", "f32", np.ones(1, dtype=np.float32)), ("b0.zero_point", "f32", np.zeros(1, dtype=np.float32))]
    lay = dict(shape=[16, 16, 3, 3], c_in_stored=16, n_bits=3, scale_rows=16, delta_dtype="f16", zero_point_dtype="f32",
               levels_coding="rans", rans_chunk=CHUNK, bias_n_bits=4, bias_scale_rows=1, bias_delta_dtype="f32",
               bias_zero_point_dtype="f32", bias_levels_coding="rans", bias_rans_chunk=64)
    if mutate_header:
        mutate_header(lay)
    header = dict(arch="hnerv", cfg=dict(crop_h=2, crop_w=2), frames=1, hadamard=False, bias="hard", embedding_shape=None,
                  layers=[lay])
    return bitstream_ref.write(str(path), header, sections), sections, wl, bl


def test_read_container_parses_u16_sections(tmp_path):
    from neuroquant_amd.bitstream import coded_tensors, read_container
    path = tmp_path / "c.nqv"
    written, sections, wl, bl = _coded_file(path)
    header, sec = read_container(str(path))
    assert header == written and header["version"] == 1 and list(sec) == [s[0] for s in sections]
    for name, tag, arr in sections:
        assert sec[name].dtype == np.dtype({"u16": "<u2", "u32": "<u4", "f16": "<f2", "f32": "<f4"}[tag])
        assert np.array_equal(sec[name], arr)
    assert all(s["offset"] % 4 == 0 for s in header["sections"])
    coded = coded_tensors(header, sec)
    assert sorted(coded) == ["b0", "w0"] and coded["w0"][4] == CHUNK and coded["b0"][4] == 64
    assert R.read_coded_levels(str(path), "w0") == wl.tolist() and R.read_coded_levels(str(path), "b0") == bl.tolist()
    # a section of no entries (a constant tensor's words) is a legal section, also as the last one of a file
    empty = tmp_path / "e.nqv"
    bitstream_ref.write(str(empty), dict(layers=[]), [("a", "u16", np.arange(3)), ("w0.rans_words", "u16", np.zeros(0)), ("z", "u16", np.zeros(0))])
    _, sec = read_container(str(empty))
    assert sec["a"].tolist() == [0, 1, 2] and sec["w0.rans_words"].size == 0 and sec["z"].size == 0


def _set(key, fn):
    def mutate(parts):
        parts[key] = fn(parts[key])
    return mutate


DAMAGE = {
    "table_sum": dict(mutate=_set("freq", lambda f: [f[0] + 1] + f[1:])),
    "table_size": dict(mutate=_set("freq", lambda f: f + [0] * 8)),
    "chunk_zero": dict(mutate_header=lambda lay: lay.update(rans_chunk=0)),
    "chunk_negative": dict(mutate_header=lambda lay: lay.update(rans_chunk=-128)),
    "chunk_not_multiple_of_64": dict(mutate_header=lambda lay: lay.update(rans_chunk=96)),
    "chunk_missing": dict(mutate_header=lambda lay: lay.pop("rans_chunk")),
    "chunk_count": dict(mutate_header=lambda lay: lay.update(rans_chunk=64)),          # ceil(n / 64) chunks, offsets for fewer
    "offsets_start": dict(mutate=_set("offsets", lambda o: [1] + o[1:])),
    "offsets_decrease": dict(mutate=_set("offsets", lambda o: o[:1] + [o[2] + 1] + o[2:])),
    "offsets_end_short": dict(mutate=_set("words", lambda w: w + [0])),
    "offsets_end_long": dict(mutate=_set("words", lambda w: w[:-1])),
    "states_count": dict(mutate=_set("states", lambda s: s[:-1])),
    "state_below_bound": dict(mutate=_set("states", lambda s: [L - 1] + s[1:])),
    "unknown_coding": dict(mutate_header=lambda lay: lay.update(levels_coding="huffman")),
    "bias_table_size": dict(mutate_header=lambda lay: lay.update(bias_n_bits=3)),       # 16 entries stored, 2^3 expected
}


@pytest.mark.parametrize("rule", sorted(DAMAGE))
def test_player_validation_refuses_damaged_coded_files(tmp_path, rule):
    from neuroquant_amd.bitstream import coded_tensors, read_container
    good = tmp_path / "good.nqv"
    _coded_file(good)
    assert len(coded_tensors(*read_container(str(good)))) == 2
    bad = tmp_path / (rule + ".nqv")
    _coded_file(bad, **DAMAGE[rule])
    header, sec = read_container(str(bad))             # the container itself is sound
    with pytest.raises(ValueError):
        coded_tensors(header, sec, what=str(bad))


def test_player_validation_refuses_a_missing_section(tmp_path):
    from neuroquant_amd.bitstream import coded_tensors, read_container
    path = tmp_path / "m.nqv"
    _coded_file(path)
    header, sec = read_container(str(path))
    del sec["w0.rans_states"]
    with pytest.raises(ValueError):
        coded_tensors(header, sec)

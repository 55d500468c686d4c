"""Plain-Python restatement of the entropy-coded levels of a `.nqv` file, written from that section: scalar
loops over Python ints, nothing imported from the package and no numpy vector code shared with it.

The code: static model per tensor (frequencies f[s] over the 2^n_bits levels, sum 4096), 32-bit states with lower bound 2^16,
16-bit words.  A tensor is cut into chunks of `chunk` symbols; inside a chunk lane l (0..63) owns symbols l, l + 64, ...
Decoding step t, for every lane whose symbol 64 t + l exists, lanes ascending:
    slot = x & 4095;  s = symbol(slot);  x = f[s] * (x >> 12) + slot - cum[s];  if x < 2^16: x = (x << 16) | next word
Encoding is the mirror: steps last to first, lanes 63 .. 0, `if x >= f[s] << 20: emit x & 0xffff, x >>= 16`, then
`x = ((x // f) << 12) + x % f + cum[s]`; every state starts at 2^16, the words are reversed at the end, the 64 final states
are stored."""
import json
import struct

PROB_BITS = 12
M = 1 << PROB_BITS
L = 1 << 16
LANES = 64


def normalise(counts):
    """f[s] = max(1, floor(c[s] * 4096 / n)) where c[s] > 0, else 0; while the sum exceeds 4096 the largest f > 1 loses one
    (lowest symbol on ties); a deficit goes whole to the symbol with the largest count (lowest symbol on ties)."""
    n = sum(counts)
    f = [max(1, c * M // n) if c > 0 else 0 for c in counts]
    while sum(f) > M:
        best = -1
        for s in range(len(f)):
            if f[s] > 1 and (best < 0 or f[s] > f[best]):
                best = s
        f[best] -= 1
    if sum(f) < M:
        best = 0
        for s in range(len(counts)):
            if counts[s] > counts[best]:
                best = s
        f[best] += M - sum(f)
    return f


def tables(f):
    cum, lut, acc = [], [], 0
    for s, fs in enumerate(f):
        cum.append(acc)
        lut += [s] * fs
        acc += fs
    assert acc == M
    return cum, lut


def encode_chunk(sym, f, cum):
    """-> (64 final states, words in the order the decoder reads them)"""
    x, out = [L] * LANES, []
    steps = -(-len(sym) // LANES)
    for t in range(steps - 1, -1, -1):
        for lane in range(LANES - 1, -1, -1):
            i = t * LANES + lane
            if i >= len(sym):
                continue
            s = sym[i]
            fs, xs = f[s], x[lane]
            assert fs > 0
            if xs >= fs << 20:
                out.append(xs & 0xFFFF)
                xs >>= 16
            x[lane] = ((xs // fs) << PROB_BITS) + xs % fs + cum[s]
            assert L <= x[lane] < 1 << 32
    out.reverse()
    return x, out


def decode_chunk(states, words, n, f, cum, lut):
    x, pos, sym = list(states), 0, [0] * n
    assert len(x) == LANES
    for t in range(-(-n // LANES)):
        for lane in range(LANES):
            i = t * LANES + lane
            if i >= n:
                break
            slot = x[lane] & (M - 1)
            s = lut[slot]
            sym[i] = s
            xs = f[s] * (x[lane] >> PROB_BITS) + slot - cum[s]
            if xs < L:
                xs = (xs << 16) | words[pos]
                pos += 1
            x[lane] = xs
    assert pos == len(words), (pos, len(words))            # every word consumed
    assert all(v == L for v in x), "every state returns to 2^16"
    return sym


def encode(levels, n_bits, chunk):
    """flat list of ints -> (freq, states, offsets, words), plain lists"""
    levels = [int(v) for v in levels]
    assert levels and chunk > 0 and chunk % LANES == 0 and max(levels) < 1 << n_bits
    counts = [0] * (1 << n_bits)
    for v in levels:
        counts[v] += 1
    f = normalise(counts)
    cum, _ = tables(f)
    states, offsets, words = [], [0], []
    for base in range(0, len(levels), chunk):
        st, w = encode_chunk(levels[base:base + chunk], f, cum)
        states += st
        words += w
        offsets.append(len(words))
    return f, states, offsets, words


def decode(f, states, offsets, words, n, chunk):
    f = [int(v) for v in f]
    cum, lut = tables(f)
    out = []
    assert len(offsets) == -(-n // chunk) + 1 and offsets[0] == 0 and offsets[-1] == len(words)
    for c, base in enumerate(range(0, n, chunk)):
        out += decode_chunk([int(v) for v in states[c * LANES:(c + 1) * LANES]],
                            [int(v) for v in words[offsets[c]:offsets[c + 1]]], min(chunk, n - base), f, cum, lut)
    return out


def section_bytes(n_bits, chunks, n_words):
    """bytes of a coded tensor's four sections in a file (each padded to 4 bytes)"""
    a4 = lambda v: (v + 3) // 4 * 4
    return a4(2 << n_bits) + 4 * LANES * chunks + 4 * (chunks + 1) + a4(2 * n_words)


_FMT = {"u16": "H", "u32": "I"}


def read_coded_levels(path, name):
    """levels (list of ints) of the coded tensor `name` ('w3', 'b0', ...) of a `.nqv` file, read with this module alone."""
    data = open(path, "rb").read()
    assert data[:4] == b"NQV1"
    (hlen,) = struct.unpack("<I", data[4:8])
    header = json.loads(data[8:8 + hlen].decode("utf-8"))
    start = (8 + hlen + 3) // 4 * 4
    sec = {}
    for s in header["sections"]:
        if s["name"].startswith(name + ".rans_"):
            sec[s["name"].split(".")[1]] = list(struct.unpack_from("<%d%s" % (s["count"], _FMT[s["dtype"]]), data, start + s["offset"]))
    lay = header["layers"][int(name[1:])]
    if name[0] == "w":
        assert lay["levels_coding"] == "rans"
        n, chunk = lay["shape"][0] * lay["c_in_stored"] * lay["shape"][2] * lay["shape"][3], lay["rans_chunk"]
    else:
        assert lay["bias_levels_coding"] == "rans"
        n, chunk = lay["shape"][0], lay["bias_rans_chunk"]
    return decode(sec["rans_freq"], sec["rans_states"], sec["rans_offsets"], sec["rans_words"], n, chunk)

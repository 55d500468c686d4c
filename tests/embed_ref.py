"""Numpy restatement of the quantised frame embeddings of a `.nqv` file, written from that section: the
arithmetic, the symbols and the three section layouts.  Nothing is imported from the package; packing comes from
bitstream_ref, the entropy code from rans_ref (or from an encoder the caller hands in).

x is (N, C, h, w) fp32, E = C*h*w.  One (delta, zero_point) per channel c from the 'max' rule over all frames of that channel:
    lo = min(min x, 0); hi = max(max x, 0); delta = max(fp32((double(hi) - double(lo)) / (2^b - 1)), 1e-8); zp = rint(-lo / delta)
    level = clamp(rint(x / delta[c]) + zp[c], 0, 2^b - 1)                      (fp32, every step rounded)
Symbols, frame-major (N, E):  sym[t] = level[t], or (temporal) sym[0] = level[0], sym[t] = (level[t] - level[t-1]) mod 2^b.
Restore: level[t] = (level[t-1] + sym[t]) & (2^b - 1);  value = (fp32(level) - zp[c]) * delta[c].
"""
import numpy as np

import bitstream_ref as R
import rans_ref

MODES = ("packed", "rans", "temporal")        # ties between equal sizes go in this order
LAYOUT = {"packed": (False, "packed"), "rans": (False, "rans"), "temporal": (True, "rans")}   # mode -> (temporal, coding)
RANS_KINDS = ("rans_freq", "rans_states", "rans_offsets", "rans_words")
RANS_TAGS = ("u16", "u32", "u32", "u16")
F32 = np.float32


def scales(x, b):
    """-> (delta, zp), fp32 (C,)"""
    x = np.asarray(x, dtype=F32)
    C = x.shape[1]
    rows = x.transpose(1, 0, 2, 3).reshape(C, -1)
    lo = np.minimum(rows.min(axis=1), F32(0))
    hi = np.maximum(rows.max(axis=1), F32(0))
    delta = ((hi.astype(np.float64) - lo.astype(np.float64)) / float(2 ** b - 1)).astype(F32)
    delta = np.maximum(delta, F32(1e-8))
    zp = np.rint((-lo) / delta).astype(F32)
    return delta, zp


def levels(x, delta, zp, b):
    """-> uint8 (N, E)"""
    x = np.asarray(x, dtype=F32)
    d, z = delta.reshape(1, -1, 1, 1).astype(F32), zp.reshape(1, -1, 1, 1).astype(F32)
    xi = (np.rint((x / d).astype(F32)) + z).astype(F32)
    return np.clip(xi, F32(0), F32(2 ** b - 1)).astype(np.uint8).reshape(x.shape[0], -1)


def symbols(lv, b, temporal):
    lv = np.asarray(lv, dtype=np.int64)
    if not temporal:
        return lv.astype(np.uint8)
    out = lv.copy()
    out[1:] = (lv[1:] - lv[:-1]) % (1 << b)
    return out.astype(np.uint8)


def levels_from_symbols(sym, b, temporal):
    sym = np.asarray(sym, dtype=np.int64)
    if not temporal:
        return (sym & ((1 << b) - 1)).astype(np.uint8)
    out = np.zeros_like(sym)
    prev = np.zeros(sym.shape[1], dtype=np.int64)
    for t in range(sym.shape[0]):
        prev = (prev + sym[t]) & ((1 << b) - 1)
        out[t] = prev
    return out.astype(np.uint8)


def dequant(lv, delta, zp, shape):
    d, z = delta.reshape(1, -1, 1, 1).astype(F32), zp.reshape(1, -1, 1, 1).astype(F32)
    return ((np.asarray(lv).reshape(shape).astype(F32) - z) * d).astype(F32)


def restore(sym, delta, zp, shape, b, temporal):
    return dequant(levels_from_symbols(np.asarray(sym).reshape(shape[0], -1), b, temporal), delta, zp, shape)


def scale_section(a):
    """fp16 when every entry survives the round trip, else fp32"""
    a = np.asarray(a, dtype=F32).reshape(-1)
    ok = np.array_equal(a.astype(np.float16).astype(F32), a)
    return ("f16", a.astype(np.float16)) if ok else ("f32", a)


def _ref_encode(sym, b, chunk):
    f, st, off, w = rans_ref.encode(np.asarray(sym).reshape(-1).tolist(), b, chunk)
    return np.array(f, np.uint16), np.array(st, np.uint32), np.array(off, np.uint32), np.array(w, np.uint16)


def sections(lv, delta, zp, b, mode, chunk=32768, encode=_ref_encode):
    """levels (N, E) -> (the header's `embedding` entry, [(name, tag, array)]) for one of MODES.  encode(symbols, b, chunk) ->
    (freq, states, offsets, words).  A single frame is always packed."""
    lv = np.asarray(lv)
    N = lv.shape[0]
    temporal, coding = LAYOUT["packed" if N == 1 else mode]
    sym = symbols(lv, b, temporal)
    entry = {"bits": int(b), "scale_rows": int(len(delta)), "temporal": temporal, "coding": coding}
    out = [("embeddings.delta",) + scale_section(delta), ("embeddings.zero_point",) + scale_section(zp)]
    out.append(("embeddings.levels", "u32", R.pack(sym if coding == "packed" else sym[0], b)))
    if coding == "rans":
        entry["rans_chunk"] = int(chunk)
        out += [(f"embeddings.{k}", t, np.asarray(a)) for k, t, a in zip(RANS_KINDS, RANS_TAGS, encode(sym[1:], b, chunk))]
    return entry, out


def section_bytes(secs):
    return sum(R.align4(np.asarray(a).size * np.dtype(R.DTYPES[t]).itemsize) for _, t, a in secs)


def smallest(bytes_by_mode):
    return min(MODES, key=lambda m: bytes_by_mode[m])


def symbols_of(entry, sec, shape):
    """the (N, E) symbols a file's sections hold, decoded with bitstream_ref / rans_ref alone"""
    N, E, b = shape[0], int(np.prod(shape[1:])), entry["bits"]
    if entry["coding"] == "packed":
        return R.unpack(sec["embeddings.levels"], N * E, b).reshape(N, E)
    first = R.unpack(sec["embeddings.levels"], E, b)
    rest = rans_ref.decode(*(sec[f"embeddings.{k}"] for k in RANS_KINDS), (N - 1) * E, entry["rans_chunk"])
    return np.concatenate([first, np.array(rest, dtype=np.uint8)]).reshape(N, E)


def restore_file(header, sec):
    """fp32 embeddings of a parsed file that stores them as levels"""
    entry, shape = header["embedding"], tuple(header["embedding_shape"])
    return restore(symbols_of(entry, sec, shape), sec["embeddings.delta"].astype(F32), sec["embeddings.zero_point"].astype(F32),
                   shape, entry["bits"], entry["temporal"])

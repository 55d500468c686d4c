"""Bit-stream container (`.nqv`) of a calibrated model and the GPU player that decodes it.

`write_stream` turns a calibrated `QuantModel` into ONE self-describing file whose size is the nominal bit-rate: the integer
levels of `export._levels`, packed at their bit-width by a HIP kernel, the quantiser scales, the biases and (HNeRV) the frame
embeddings.  `read_container` parses such a file with numpy alone.  `StreamDecoder` opens a file -- no QuantModel, no
checkpoint -- rebuilds every weight bit for bit (unpack + dequantise on the GPU, inverse Hadamard where the file says so),
builds each layer's convolution operand once and then decodes frames with the very launches the no-grad branch of
`models/_decode.run_decoder` issues, so for the same batch size and convolution precision its output equals the live
model's evaluation bit for bit.

By default (`coding="packed"`) the file realises the NOMINAL size (bits x parameters).  `coding="rans"` / `"auto"` store the
levels entropy coded instead (§12): a 64-lane interleaved rANS code with one frequency table per tensor, encoded here on the
host (`rans_encode`) and decoded at open by a HIP kernel, one wavefront per chunk.  The weights a player rebuilds are the same
floats either way.  Scales and soft biases are not coded.

HNeRV's frame embeddings are fp32 by default.  `embedding_bits=` stores them as levels of 2..8 bits with one
scale per embedding channel: packed, rANS coded, or rANS coded as frame-to-frame differences, whichever is smallest.  The
player rebuilds them once at open (`ops.embed_restore`) and decodes as before.  `quantise_embeddings` gives the tensor such a
file restores, so that a model can be calibrated and evaluated on what its file will hold.
"""
import collections
import json
import math
import os
import struct

import numpy as np
import torch

from . import ops

MAGIC = b"NQV1"
VERSION = 1
_DTYPES = {"u16": "<u2", "u32": "<u4", "f16": "<f2", "f32": "<f4"}
CODINGS = ("packed", "rans", "auto")
# rANS constants (csrc/rans.hip holds the same three)
RANS_PROB_BITS = 12
RANS_M = 1 << RANS_PROB_BITS
RANS_L = 1 << 16
RANS_LANES = 64
DEFAULT_CHUNK = 32768
# the sections of a level tensor per coding, in file order: (name after the tensor's stem, dtype tag)
_RANS_PARTS = (("rans_freq", "u16"), ("rans_states", "u32"), ("rans_offsets", "u32"), ("rans_words", "u16"))
_LEVEL_PARTS = {"packed": (("levels", "u32"),), "rans": _RANS_PARTS}


def _align4(n):
    return (n + 3) & ~3


def _check_chunk(chunk, what):
    if not isinstance(chunk, int) or chunk <= 0 or chunk % RANS_LANES:
        raise ValueError(f"{what}: chunk must be a positive multiple of {RANS_LANES}, got {chunk!r}")


def _check_bits(bits, lo, hi, what):
    if not isinstance(bits, int) or isinstance(bits, bool) or not lo <= bits <= hi:
        raise ValueError(f"{what} must be an integer in {lo}..{hi}, got {bits!r}")


# ------------------------------------------------------------------------------------------ container (host only)
def _write_container(path, header, sections):
    """sections: [(name, dtype tag, numpy array)] -> (the header as written, file size).  Section offsets count from the start
    of the payload (the first 4-byte boundary after the header), so they do not depend on the header's own length."""
    table, pos, blobs = [], 0, []
    for name, tag, arr in sections:
        raw = np.ascontiguousarray(arr.reshape(-1)).astype(_DTYPES[tag], copy=False).tobytes()
        table.append(dict(name=name, dtype=tag, count=int(arr.size), offset=pos, bytes=len(raw)))
        blobs.append(raw + b"\0" * (_align4(len(raw)) - len(raw)))
        pos += len(blobs[-1])
    header = dict(header, version=VERSION, sections=table)
    hj = json.dumps(header, separators=(",", ":"), sort_keys=True).encode("utf-8")
    start = _align4(8 + len(hj))
    os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
    with open(path, "wb") as f:
        f.write(MAGIC + struct.pack("<I", len(hj)) + hj + b"\0" * (start - 8 - len(hj)))
        for b in blobs:
            f.write(b)
    return header, start + pos


def read_container(path):
    """-> (header dict, {section name: 1-D numpy array}).  Pure Python / numpy, no GPU.  ValueError for a bad magic, an unknown
    version, a truncated file and sections that overlap, are misaligned or run past the end."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 8 or data[:4] != MAGIC:
        raise ValueError(f"{path}: not an NQV1 stream (bad magic)")
    (hlen,) = struct.unpack("<I", data[4:8])
    if 8 + hlen > len(data):
        raise ValueError(f"{path}: truncated inside the header")
    try:
        header = json.loads(data[8:8 + hlen].decode("utf-8"))
    except (UnicodeDecodeError, json.JSONDecodeError) as e:
        raise ValueError(f"{path}: unreadable header ({e})") from None
    if not isinstance(header, dict) or header.get("version") != VERSION:
        raise ValueError(f"{path}: unknown container version {header.get('version') if isinstance(header, dict) else None!r}")
    start = _align4(8 + hlen)
    out, end = {}, 0
    for s in sorted(header.get("sections", []), key=lambda s: s["offset"]):
        tag, off, nbytes, count = s.get("dtype"), s["offset"], s["bytes"], s["count"]
        if tag not in _DTYPES or off % 4 or off < end or nbytes != count * np.dtype(_DTYPES[tag]).itemsize or s["name"] in out:
            raise ValueError(f"{path}: section {s.get('name')!r} is misaligned, overlaps its neighbour or is inconsistent")
        if start + off + nbytes > len(data):
            raise ValueError(f"{path}: section {s['name']!r} runs past the end of the file")
        out[s["name"]] = np.frombuffer(data, dtype=_DTYPES[tag], count=count, offset=start + off)
        end = off + _align4(nbytes)
    if start + end != len(data):
        raise ValueError(f"{path}: file is {len(data)} bytes, header and sections make {start + end} (truncated?)")
    return header, out


# ------------------------------------------------------------------------------------------ rANS (host only)
def rans_normalise(counts):
    """histogram -> frequencies that sum to 4096, a symbol that occurs keeps f >= 1 (the rule of DESIGN.md §12):
    f = max(1, floor(c * 4096 / n)); while the sum exceeds 4096 the largest f > 1 loses one (lowest symbol on ties); a
    deficit goes whole to the symbol with the largest count (lowest symbol on ties)."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    n = int(c.sum())
    if n <= 0 or (c < 0).any():
        raise ValueError("rans_normalise: need a non-empty histogram of non-negative counts")
    f = np.where(c > 0, np.maximum(1, c * RANS_M // n), 0)
    while int(f.sum()) > RANS_M:
        f[int(np.argmax(np.where(f > 1, f, 0)))] -= 1   # argmax returns the first (lowest) of equal maxima
    f[int(np.argmax(c))] += RANS_M - int(f.sum())
    return f.astype(np.uint16)


def rans_encode(levels, n_bits, chunk=DEFAULT_CHUNK):
    """levels (uint8, any shape, taken flat in C order) -> (freq u16 [2^n_bits], states u32 [64 * chunks], offsets u32
    [chunks + 1], words u16), the four sections of a coded tensor.  Host numpy, vectorised over chunks and lanes: the Python
    loop runs over the chunk's steps, last to first, and mirrors the decoder exactly (lanes 63 .. 0 inside a step, the words
    reversed at the end)."""
    lv = np.ascontiguousarray(np.asarray(levels).reshape(-1)).astype(np.int64)
    n, n_bits, chunk = lv.size, int(n_bits), int(chunk)
    if n == 0:
        raise ValueError("rans_encode: no levels to code")
    _check_bits(n_bits, 1, 8, "rans_encode: n_bits")
    _check_chunk(chunk, "rans_encode")
    if int(lv.max()) >= 1 << n_bits or int(lv.min()) < 0:
        raise ValueError(f"rans_encode: level {int(lv.max())} does not fit {n_bits} bits")
    freq = rans_normalise(np.bincount(lv, minlength=1 << n_bits))
    f_of = freq.astype(np.uint64)
    cum_of = np.concatenate([[0], np.cumsum(f_of)[:-1]]).astype(np.uint64)
    chunks = -(-n // chunk)
    steps = -(-min(chunk, n) // RANS_LANES)
    sym = np.zeros(chunks * steps * RANS_LANES, dtype=np.int64)
    live = np.zeros(sym.size, dtype=bool)
    sym[:n], live[:n] = lv, True                  # one chunk: steps * 64 >= n; several: steps * 64 == chunk
    sym, live = sym.reshape(chunks, steps, RANS_LANES), live.reshape(chunks, steps, RANS_LANES)
    x = np.full((chunks, RANS_LANES), RANS_L, dtype=np.uint64)
    emitted = np.zeros((chunks, steps, RANS_LANES), dtype=bool)
    word = np.zeros((chunks, steps, RANS_LANES), dtype=np.uint16)
    for t in range(steps - 1, -1, -1):
        a = live[:, t]
        f = np.where(a, f_of[sym[:, t]], 1).astype(np.uint64)
        e = a & (x >= (f << np.uint64(20)))
        emitted[:, t], word[:, t] = e, (x & np.uint64(0xFFFF)).astype(np.uint16)
        x = np.where(e, x >> np.uint64(16), x)
        x = np.where(a, ((x // f) << np.uint64(RANS_PROB_BITS)) + x % f + cum_of[sym[:, t]], x)
    # decode order inside a chunk: steps ascending, lanes ascending -- C order of (chunk, step, lane)
    words = word[emitted]
    offsets = np.concatenate([[0], np.cumsum(emitted.sum(axis=(1, 2)))]).astype(np.uint32)
    return freq, x.astype(np.uint32).reshape(-1), offsets, words


def rans_validate(freq, states, offsets, words, n, n_bits, chunk, what="coded tensor"):
    """Host check of a coded tensor's four sections before they reach the GPU; ValueError names the rule that failed."""
    if not isinstance(n_bits, int) or not 1 <= n_bits <= 8 or len(freq) != 1 << n_bits or int(np.sum(freq, dtype=np.int64)) != RANS_M:
        raise ValueError(f"{what}: the frequency table must hold 2^n_bits entries that sum to {RANS_M}")
    _check_chunk(chunk, what)
    chunks = -(-int(n) // chunk)
    if len(offsets) != chunks + 1:
        raise ValueError(f"{what}: {len(offsets)} offsets stored, {n} levels in chunks of {chunk} need {chunks + 1}")
    o = np.asarray(offsets, dtype=np.int64)
    if o[0] != 0 or (np.diff(o) < 0).any() or o[-1] != len(words):
        raise ValueError(f"{what}: offsets must start at 0, never decrease and end at the number of words ({len(words)})")
    if len(states) != RANS_LANES * chunks or (np.asarray(states, dtype=np.int64) < RANS_L).any():
        raise ValueError(f"{what}: need {RANS_LANES} states per chunk, each at least {RANS_L}")


# ------------------------------------------------------------------------------------------ stored level tensors (host only)
class StoredLevels(collections.namedtuple("StoredLevels", "name n n_bits coding arrays chunk")):
    """One run of `n` levels of `n_bits` bits as a file holds it under the section stem `name`: coding 'packed' with
    arrays = (u32 words,) and no chunk, or coding 'rans' with arrays = (freq, states, offsets, words).  Only `_stored_levels`
    makes one, so holding one means the host checks have passed."""
    words = property(lambda self: self.arrays[-1])
    nbytes = property(lambda self: sum(a.nbytes for a in self.arrays))   # of its sections, unpadded


def _stored_levels(sec, name, n, n_bits, coding, chunk, what):
    """The level tensor `name` of `read_container`'s sections -> StoredLevels, checked on the host before anything of it
    reaches the GPU; the only place that looks level sections up.  ValueError names the missing section or the failed rule."""
    if coding not in tuple(_LEVEL_PARTS):
        raise ValueError(f"{what}: {name} is stored in an unknown coding {coding!r}")
    _check_bits(n_bits, 1, 8, f"{what}: {name}: n_bits")
    arrays = [sec.get(f"{name}.{k}") for k, _ in _LEVEL_PARTS[coding]]
    for (k, tag), a in zip(_LEVEL_PARTS[coding], arrays):
        if a is None:
            raise ValueError(f"{what}: {name} is stored {coding} but section {name}.{k} is missing")
        if a.dtype != np.dtype(_DTYPES[tag]):
            raise ValueError(f"{what}: {name}.{k} must be a {tag} section, got {a.dtype}")
    if coding == "rans":
        rans_validate(*arrays, n, n_bits, chunk, what=f"{what}: {name}")
    elif len(arrays[0]) != (n * n_bits + 31) // 32:
        raise ValueError(f"{what}: {name}.levels must hold {(n * n_bits + 31) // 32} u32 words ({n} symbols of {n_bits} bits), "
                         f"got {len(arrays[0])}")
    return StoredLevels(name, n, n_bits, coding, tuple(arrays), chunk if coding == "rans" else None)


def stored_tensors(header, sec, what="stream"):
    """{tensor name ('w0', 'b3', ...): StoredLevels} for every weight and hard-bias tensor of a parsed file (`read_container`'s
    header and sections), packed ones included.  Host only: this is the check the player runs before anything of a level
    tensor reaches the GPU.  ValueError for an unknown coding, a missing or mistyped section or a failed rule."""
    out = {}
    for i, lay in enumerate(header["layers"]):
        co, _, k, k2 = lay["shape"]
        for name, prefix, n in ((f"w{i}", "", co * lay["c_in_stored"] * k * k2), (f"b{i}", "bias_", co)):
            coding = lay.get(prefix + "levels_coding", "packed")
            if prefix and header.get("bias") != "hard":
                if coding != "packed":
                    raise ValueError(f"{what}: {name} is marked as coded but the stream stores soft biases")
                continue
            out[name] = _stored_levels(sec, name, n, lay.get(prefix + "n_bits"), coding, lay.get(prefix + "rans_chunk"), what)
    return out


def coded_tensors(header, sec, what="stream"):
    """{tensor name: (freq, states, offsets, words, chunk)} for the rANS-coded tensors among `stored_tensors`."""
    return {name: (*st.arrays, st.chunk) for name, st in stored_tensors(header, sec, what).items() if st.coding == "rans"}


# ------------------------------------------------------------------------------------------ embeddings (host only)
EMBED_MODES = ("packed", "rans", "temporal")   # the order in which ties between equal sizes are resolved
# mode -> (temporal, coding) of the header's `embedding` entry
_EMBED_LAYOUT = {"packed": (False, "packed"), "rans": (False, "rans"), "temporal": (True, "rans")}


def smallest_embedding_mode(bytes_by_mode):
    """{mode: section bytes} -> the mode `write_stream` keeps: the fewest bytes, ties in the order packed, rans, temporal."""
    return min((m for m in EMBED_MODES if m in bytes_by_mode), key=lambda m: bytes_by_mode[m])


def embedding_sections(header, sec, what="stream"):
    """The quantised embeddings of a parsed file (`read_container`'s header and sections), checked on the host before anything
    of them reaches the GPU: the counterpart of `stored_tensors`.  -> None for a file that stores fp32 embeddings (no
    `embedding` entry), else dict(bits, temporal, coding, chunk, shape, delta, zero_point, levels, rans) with `rans` the four
    coded arrays (None for coding 'packed'), and `stored`, the same two runs of levels as (StoredLevels, StoredLevels or None)
    for `restore_embeddings`.  ValueError names the rule that failed."""
    entry = header.get("embedding")
    if entry is None:
        return None
    shape = header.get("embedding_shape")
    if header.get("arch") != "hnerv" or not isinstance(entry, dict):
        raise ValueError(f"{what}: only an HNeRV stream stores embeddings, described by a table")
    if (not isinstance(shape, list) or len(shape) != 4 or not all(isinstance(v, int) and not isinstance(v, bool) and v > 0 for v in shape)
            or shape[0] != header.get("frames")):
        raise ValueError(f"{what}: embedding_shape must be (frames, C, h, w) with positive sizes, got {shape!r} for "
                         f"{header.get('frames')!r} frames")
    N, C, E = shape[0], shape[1], shape[1] * shape[2] * shape[3]
    bits, temporal, coding = entry.get("bits"), entry.get("temporal"), entry.get("coding")
    _check_bits(bits, 2, 8, f"{what}: embedding bits")
    if not isinstance(temporal, bool):
        raise ValueError(f"{what}: embedding temporal must be true or false, got {temporal!r}")
    if coding not in ("packed", "rans"):
        raise ValueError(f"{what}: embeddings are stored in an unknown coding {coding!r}")
    if entry.get("scale_rows") != C:
        raise ValueError(f"{what}: embedding scale_rows is {entry.get('scale_rows')!r}, the embeddings have {C} channels")
    if coding == "rans" and N < 2:
        raise ValueError(f"{what}: coding 'rans' codes the frames after the first, the stream holds {N}")
    if "embeddings" in sec:
        raise ValueError(f"{what}: quantised embeddings and an fp32 'embeddings' section in one file")
    delta, zp = sec.get("embeddings.delta"), sec.get("embeddings.zero_point")
    for name, a in (("delta", delta), ("zero_point", zp)):
        if a is None:
            raise ValueError(f"{what}: embeddings are stored as levels but section embeddings.{name} is missing")
        if a.dtype.kind != "f" or len(a) != C:
            raise ValueError(f"{what}: embeddings.{name} must hold {C} floats (one per channel), got {len(a)} of {a.dtype}")
    # frame 0 (coding 'packed': every frame) at its bit-width, the frames after it rANS coded
    packed = _stored_levels(sec, "embeddings", N * E if coding == "packed" else E, bits, "packed", None, what)
    coded = _stored_levels(sec, "embeddings", (N - 1) * E, bits, "rans", entry.get("rans_chunk"), what) if coding == "rans" else None
    return dict(bits=bits, temporal=temporal, coding=coding, chunk=coded and coded.chunk, shape=tuple(shape), delta=delta,
                zero_point=zp, levels=packed.words, rans=coded and list(coded.arrays), stored=(packed, coded))


# ------------------------------------------------------------------------------------------ stored level tensors (GPU)
def _upload(a, device):
    """host array -> tensor on `device`, from a writable copy; unsigned travels as the signed dtype of the same width"""
    a = np.array(a)
    return torch.from_numpy(a.view(f"i{a.dtype.itemsize}") if a.dtype.kind == "u" else a).to(device)


class _DeviceLevels:
    """A StoredLevels uploaded once; `dequant(delta, zp, shape)` -> fp32 (level - zp) * delta, as often as wanted.  Legal
    only on what `_stored_levels` returned: the coded arrays go to the kernel as trusted."""

    def __init__(self, st, device):
        self.st = st
        if st.coding == "packed":
            self.dev = (_upload(st.words, device),)
        else:   # one host buffer, one upload: the four arrays side by side at 4-byte boundaries, viewed by type on the device
            starts = np.cumsum([0] + [_align4(a.nbytes) for a in st.arrays])
            host = np.zeros(int(starts[-1]), dtype=np.uint8)
            for a, o in zip(st.arrays, starts):
                host[o:o + a.nbytes] = a.view(np.uint8)
            dev = torch.from_numpy(host).to(device)
            self.dev = tuple(dev[o:o + a.nbytes].view(torch.int16 if a.dtype.itemsize == 2 else torch.int32)
                             for a, o in zip(st.arrays, starts))

    def dequant(self, delta, zp, shape):
        st = self.st
        if st.coding == "packed":
            return ops.unpack_dequant(self.dev[0], delta, zp, shape, st.n_bits)
        freq, states, offsets, words = self.dev
        return ops.rans_decode_dequant(words, states, offsets, freq, delta, zp, shape, st.n_bits, st.chunk, trusted=True)


# uint8 levels on the GPU -> the sections [(section name, tag, array)] that store them, one function per coding
def _packed_section(name, levels_u8, n_bits):
    return [(f"{name}.levels", "u32", ops.pack_levels(levels_u8, n_bits).cpu().numpy().view(np.uint32))]


def _rans_sections(name, levels_u8, n_bits, chunk):
    return [(f"{name}.{k}", tag, a) for (k, tag), a in zip(_RANS_PARTS, rans_encode(levels_u8.cpu().numpy(), n_bits, chunk))]


def _section_bytes(sections):
    return sum(_align4(np.asarray(a).size * np.dtype(_DTYPES[t]).itemsize) for _, t, a in sections)


def _as_stored(sections):
    """sections -> what `read_container` gives for the file they make: a writer puts this through the reader's own functions"""
    return {name: np.asarray(a).reshape(-1).astype(_DTYPES[tag]) for name, tag, a in sections}


def _scale_section(t):
    """fp16 when every entry survives the round trip (true after AdaRound's init, quantizer.py:264-265), else fp32."""
    t = t.detach().float().reshape(-1).cpu()
    tag = "f16" if torch.equal(t.half().float(), t) else "f32"
    return tag, t.numpy().astype(_DTYPES[tag])


# ------------------------------------------------------------------------------------------ embeddings (GPU)
class QuantisedEmbeddings:
    """HNeRV's frame embeddings quantised to `bits` bits: `source` (N, C, h, w) fp32 as given, `delta` /
    `zero_point` one per channel ('max' rule, not rounded to fp16), `levels` uint8 (N, C*h*w) and `restored`, the fp32 tensor
    a player rebuilds from a file that stores these levels: what a model whose file is to store them must be evaluated on."""

    def __init__(self, source, bits, delta, zero_point, levels, restored):
        self.source, self.bits, self.delta, self.zero_point = source, bits, delta, zero_point
        self.levels, self.restored, self.shape = levels, restored, tuple(source.shape)


def _embedding_tensor(x):
    x = (torch.cat(list(x), 0) if isinstance(x, (list, tuple)) else x).detach().float()
    if x.dim() != 4 or x.numel() == 0:
        raise ValueError(f"embeddings must be a non-empty (N, C, h, w) tensor, got shape {tuple(x.shape)}")
    return x.contiguous()


@torch.no_grad()
def quantise_embeddings(x, bits):
    """(N, C, h, w) fp32 embeddings (tensor or the list `evaluate()` returned) on the GPU -> QuantisedEmbeddings.  One
    (delta, zero_point) per channel from `ops.scale_init_max` on the channel-major view (C, N, h, w): 0 lies in the range, the
    step is at least 1e-8, an all-zero channel restores to exact zeros.  ValueError for bits outside 2..8 and for embeddings
    that are not finite."""
    x = _embedding_tensor(x)
    _check_bits(bits, 2, 8, "embedding bits")
    if not bool(torch.isfinite(x).all()):
        raise ValueError("embeddings are not finite: they cannot be quantised")
    delta, zp = ops.scale_init_max(x.transpose(0, 1).contiguous(), 2 ** bits, True)
    delta, zp = delta.reshape(-1).contiguous(), zp.reshape(-1).contiguous()
    levels, _ = ops.embed_symbols(x, delta, zp, bits, False)
    restored = ops.embed_restore(levels.float(), delta, zp, x.shape, bits, False)
    return QuantisedEmbeddings(x, bits, delta, zp, levels, restored)


# the kinds `write_stream`'s size summary files encode_embeddings' sections under, in the order it returns them
_EMBED_KINDS = ("embedding_scales",) * 2 + ("embedding_levels",) + ("embedding_rans",) * len(_RANS_PARTS)


@torch.no_grad()
def encode_embeddings(x, bits, mode, chunk=DEFAULT_CHUNK):
    """The embeddings x (fp32 tensor / list, or a QuantisedEmbeddings of the same `bits`) as one of EMBED_MODES would store
    them -> (the header's `embedding` entry, sections [(name, tag, array)]).  'packed': all N * E levels at their bit-width;
    'rans': frame 0's levels packed, the other frames' levels rANS coded; 'temporal': frame 0's levels packed, the
    frame-to-frame differences modulo 2^bits rANS coded.  A single frame is always stored packed."""
    if mode not in EMBED_MODES:
        raise ValueError(f"mode must be one of {EMBED_MODES}, got {mode!r}")
    q = x if isinstance(x, QuantisedEmbeddings) else quantise_embeddings(x, bits)
    if q.bits != bits:
        raise ValueError(f"embeddings were quantised to {q.bits} bits, asked to store {bits}")
    _check_chunk(chunk, "encode_embeddings")
    N, C = q.shape[:2]
    temporal, coding = _EMBED_LAYOUT["packed" if N == 1 else mode]
    _, symbols = ops.embed_symbols(q.source, q.delta, q.zero_point, bits, temporal)
    entry = dict(bits=bits, scale_rows=C, temporal=temporal, coding=coding)
    sections = [(f"embeddings.{key}", *_scale_section(t)) for key, t in (("delta", q.delta), ("zero_point", q.zero_point))]
    sections += _packed_section("embeddings", symbols if coding == "packed" else symbols[0], bits)
    if coding == "rans":
        entry["rans_chunk"] = chunk
        sections += _rans_sections("embeddings", symbols[1:], bits, chunk)
    return entry, sections


@torch.no_grad()
def restore_embeddings(emb, device):
    """`embedding_sections`' result -> the fp32 embeddings (N, C, h, w) on `device`: the symbols through the decode of every
    other level tensor (a step of one and a zero point of zero leave the integers), then one `ops.embed_restore`."""
    one, zero = torch.ones(1, device=device), torch.zeros(1, device=device)
    runs = [_DeviceLevels(st, device).dequant(one, zero, (st.n,)) for st in emb["stored"] if st is not None]
    sym = runs[0] if len(runs) == 1 else torch.cat(runs)
    delta, zp = _upload(emb["delta"], device).float(), _upload(emb["zero_point"], device).float()
    return ops.embed_restore(sym, delta, zp, emb["shape"], emb["bits"], emb["temporal"])


def _embedding_stream_sections(q, chunk, frames, device):
    """write_stream's part for quantised embeddings -> (entry, sections, {mode: bytes}): all three modes, the smallest kept and
    read back from the very arrays the file will hold by the player's own functions: q.restored must come out bit for bit."""
    built = {m: encode_embeddings(q, q.bits, m, chunk) for m in EMBED_MODES}
    sizes = {m: _section_bytes(s) for m, (_, s) in built.items()}
    entry, sections = built[smallest_embedding_mode(sizes)]
    header = dict(arch="hnerv", frames=frames, embedding_shape=list(q.shape), embedding=entry)
    if not torch.equal(restore_embeddings(embedding_sections(header, _as_stored(sections), "write_stream"), device), q.restored):
        raise RuntimeError("write_stream: the stored embedding levels do not reproduce the embeddings the model was evaluated on")
    return entry, sections, sizes


# ------------------------------------------------------------------------------------------ writer
def _layer_side(q, x, name, prefix, kind, coding, chunk):
    """One side of a layer, its weight (prefix '', kind 'weight') or its hard bias ('bias_', 'bias'): tensor x under quantiser q
    as level sections in the coding chosen, then two scale sections -> ([(kind in the size summary, section)], the layer
    entry's keys, entropy of the levels in bits).  The player's own host check and device decode read the level sections back
    and q's hard-rounded forward must come out bit for bit, so a file that cannot reproduce the model is never written."""
    from .export import _entropy_bits, _levels
    from .quantization.quantizer import AdaRoundQuantizer
    if isinstance(q, AdaRoundQuantizer):
        hard = ops.adaround_forward(x, q.alpha.data, q.delta.data, q.zero_point, q.n_levels, False)
    else:
        hard = ops.uaq_forward(x, q.delta.data, q.zero_point, q.n_levels)
    levels = _levels(q, x)
    chosen, secs = "packed", _packed_section(name, levels, q.n_bits)
    if coding != "packed":
        coded = _rans_sections(name, levels, q.n_bits, chunk)
        if coding == "rans" or _section_bytes(coded) < _section_bytes(secs):
            chosen, secs = "rans", coded
    stored = _stored_levels(_as_stored(secs), name, x.numel(), int(q.n_bits), chosen, chunk, "write_stream")
    delta, zp = q.delta.detach().float().reshape(-1), q.zero_point.detach().float().reshape(-1)
    if not torch.equal(_DeviceLevels(stored, x.device).dequant(delta, zp, x.shape), hard):
        raise RuntimeError(f"write_stream: {'coded' if chosen == 'rans' else 'packed'} levels do not reproduce the quantiser's output")
    kinds = [k for k, _ in _LEVEL_PARTS[chosen]] + ["delta", "zero_point"]
    entry = {prefix + "n_bits": int(q.n_bits), prefix + "scale_rows": int(q.delta.numel())}
    if chosen == "rans":
        entry.update({prefix + "levels_coding": "rans", prefix + "rans_chunk": chunk})
    for key, t in (("delta", q.delta), ("zero_point", q.zero_point)):
        entry[f"{prefix}{key}_dtype"], arr = _scale_section(t)
        secs.append((f"{name}.{key}", entry[f"{prefix}{key}_dtype"], arr))
    return [(f"{kind}_{k}", s) for k, s in zip(kinds, secs)], entry, _entropy_bits(levels, q.n_levels)   # as export_quantized's


def _check_decoder_shape(arch, cfg):
    if arch not in ("hnerv", "nerv"):
        raise ValueError(f"unknown arch {arch!r}")
    if cfg.get("out_bias") != "tanh" or cfg.get("dec_acts") != "gelu":
        raise ValueError("the player decodes the shipped decoder only: exact-GELU blocks and a tanh head")


@torch.no_grad()
def write_stream(qnn, path, arch, cfg, embeddings=None, frames=None, bias="soft", coding="packed", chunk=DEFAULT_CHUNK,
                 embedding_bits=None):
    """Write the calibrated `qnn` to `path`.  embeddings: HNeRV's per-frame input embeddings (tensor (N, c, h, w) or the list
    `evaluate()` returned); NeRV stores none and needs `frames`.  bias: 'soft' stores the fp32 bias the evaluated model uses,
    'hard' its integer decision (export.py's module docstring).  coding: 'packed' stores every level tensor at its bit-width,
    'rans' entropy codes every one in chunks of `chunk` symbols, 'auto' codes a tensor only where its four
    coded sections are smaller than its packed words.  -> summary: file size, bytes per kind of section, bpp when the frame
    size is known, the gap to the nominal size `export_quantized` reports, and the bytes of all level sections
    (`coded_level_bytes`) against the histogram entropy of those same tensors (`entropy_level_bytes`).
    embedding_bits (HNeRV only; default None: fp32 embeddings, the file of before): store the embeddings as levels of 2..8
    bits in whichever of EMBED_MODES takes the fewest bytes.  The frames such a file decodes to are those of the
    model on the RESTORED embeddings (summary['embedding_restored']).  A caller that evaluated the model on them passes the
    `QuantisedEmbeddings` it took them from as `embeddings` (quantising a restored tensor a second time derives other scales);
    what is written is decoded again on the GPU and compared with exactly that tensor."""
    from .quantization.quant_layer import QuantModule
    from .quantization.quantizer import AdaRoundQuantizer
    if bias not in ("soft", "hard"):
        raise ValueError(f"bias must be 'soft' or 'hard', got {bias!r}")
    if coding not in CODINGS:
        raise ValueError(f"coding must be one of {CODINGS}, got {coding!r}")
    if coding != "packed":
        _check_chunk(chunk, "write_stream")
    _check_decoder_shape(arch, cfg)
    emb = qemb = None
    if embedding_bits is not None and arch != "hnerv":
        raise ValueError("embedding_bits applies to HNeRV streams: a NeRV stream stores no embeddings")
    if arch == "hnerv":
        if embeddings is None:
            raise ValueError("an HNeRV stream stores the frame embeddings: pass embeddings=")
        if isinstance(embeddings, QuantisedEmbeddings):
            if embedding_bits not in (None, embeddings.bits):
                raise ValueError(f"embeddings were quantised to {embeddings.bits} bits, embedding_bits asks for {embedding_bits}")
            qemb = embeddings
        elif embedding_bits is not None:
            qemb = quantise_embeddings(embeddings, embedding_bits)
        emb = qemb.restored if qemb is not None else (
            torch.cat(list(embeddings), 0) if isinstance(embeddings, (list, tuple)) else embeddings).detach().float()
        frames = emb.shape[0] if frames is None else frames
        if frames != emb.shape[0]:
            raise ValueError(f"{frames} frames but {emb.shape[0]} embeddings")
    elif frames is None:
        raise ValueError("a NeRV stream needs the frame count: pass frames=")
    mods = [m for m in qnn.model.modules() if isinstance(m, QuantModule)]
    layers, sections, nominal_bits, entropy_bits = [], [], 0, 0.0   # sections: [(kind in the size summary, (name, tag, array))]
    for i, m in enumerate(mods):
        wq, bq = m.weight_quantizer, m.bias_quantizer
        if not getattr(wq, "inited", True) or wq.delta is None or bq.delta is None or not m._hip_ok:
            raise ValueError(f"layer {i}: quantisers are not initialised (run one quantised forward first) or the layer is "
                             "not a stride-1 'same' convolution")
        src = m.hadamard_weight if m.hadamard else m.weight.data
        if isinstance(wq, AdaRoundQuantizer) and wq.soft_targets:
            raise ValueError(f"layer {i}: weight quantiser still rounds softly; a stream stores hard decisions")
        lay = dict(shape=list(m.weight.shape), c_in_stored=int(src.shape[1]))
        sides = [(wq, src, f"w{i}", "", "weight")] + ([(bq, m.bias.data, f"b{i}", "bias_", "bias")] if bias == "hard" else [])
        for side in sides:
            secs, entry, e = _layer_side(*side, coding, chunk)
            sections += secs
            lay.update(entry)
            entropy_bits += e
        if bias == "soft":
            sections.append(("bias_soft", (f"b{i}.soft", "f32", bq(m.bias).detach().float().cpu().numpy())))
        layers.append(lay)
        nominal_bits += wq.n_bits * m.weight.numel() + bq.n_bits * m.bias.numel()   # as export_quantized counts them
    header = dict(arch=arch, cfg=cfg, frames=int(frames), hadamard=bool(qnn.hadamard), bias=bias, layers=layers,
                  embedding_shape=None)
    if emb is not None:
        header["embedding_shape"] = list(emb.shape)
        if qemb is None:
            sections.append(("embeddings", ("embeddings", "f32", emb.cpu().numpy())))
        else:
            header["embedding"], secs, emb_sizes = _embedding_stream_sections(qemb, chunk, int(frames), emb.device)
            sections += zip(_EMBED_KINDS, secs)
    header, size = _write_container(path, header, [s for _, s in sections])
    kinds = {}
    for (kind, _), s in zip(sections, header["sections"]):
        kinds[kind] = kinds.get(kind, 0) + _align4(s["bytes"])
    nominal = math.ceil(nominal_bits / 8)
    coded = sum(v for k, v in kinds.items() if k[0] in "wb" and (k.endswith("_levels") or "_rans_" in k))
    entropy = math.ceil(entropy_bits / 8)
    summary = dict(path=path, file_bytes=size, header_bytes=size - sum(kinds.values()), section_bytes=kinds,
                   total_bytes_nominal=nominal, gap_to_nominal_bytes=size - nominal, frames=int(frames), bias=bias,
                   coding=coding, coded_tensors=sum(("levels_coding" in l) + ("bias_levels_coding" in l) for l in layers),
                   coded_level_bytes=coded, entropy_level_bytes=entropy, gap_to_entropy_bytes=coded - entropy,
                   scale_dtypes=[[l["delta_dtype"], l["zero_point_dtype"]] for l in layers])
    if qemb is not None:
        e = header["embedding"]
        summary.update(embedding=dict(bits=e["bits"], coding=e["coding"], temporal=e["temporal"],
                                      mode=smallest_embedding_mode(emb_sizes), mode_bytes=emb_sizes,
                                      bytes=sum(v for k, v in kinds.items() if k.startswith("embedding_"))),
                       embedding_restored=emb)
    h, w = cfg.get("crop_h"), cfg.get("crop_w")
    if frames and h and w:
        summary["bpp"] = size * 8 / (frames * h * w)
    return summary


# ------------------------------------------------------------------------------------------ player
class StreamDecoder:
    """Decode frames from a `.nqv` file alone.  Weights, biases and embeddings are rebuilt once at open; each layer's
    convolution operand is built once (per kernel family, the first time a batch size selects it); `decode` issues plain
    launches only.

    arithmetic='exact' (default) is the live model's arithmetic, bit for bit.  arithmetic='levels'  runs the
    layers the unsplit tiled bf16x3 kernel has on the stored integers instead: y = delta[co] * conv(x, level - zero_point) +
    bias, two MFMAs per product, no rounding of the weights at all; every other layer takes exactly the 'exact' launch.
    `levels_used[B]` lists the layers that took that path at batch size B (filled the first time a B is decoded),
    `levels_ineligible` says why a layer never can.

    arithmetic='half'  runs exactly those layers, with the same records and refusals, as
    y = delta[co] * conv(f16(x), level - zero_point) + bias: the activations rounded once to IEEE half, one F16 MFMA per
    product.  An approximation, about ten times outside the bounds the other two keep and two orders of magnitude below one
    8-bit output step.  A finite activation beyond +-65504 is clamped and raises the decoder's one sticky flag word: `decode`
    never synchronises for it, `saturated()` reads it (one synchronise) and returns a bool."""

    ARITHMETICS = ("exact", "levels", "half")

    def __init__(self, path, device="cuda", arithmetic="exact"):
        if arithmetic not in self.ARITHMETICS:
            raise ValueError(f"arithmetic must be one of {self.ARITHMETICS}, got {arithmetic!r}")
        if not torch.cuda.is_available():
            raise RuntimeError("neuroquant_amd needs an AMD GPU (no CPU path)")
        header, sec = read_container(path)
        self._open_header(path, header, device, arithmetic)
        stored = stored_tensors(header, sec, what=path)   # host validation of every level tensor, before any upload
        stored_emb = embedding_sections(header, sec, what=path)   # ... and of quantised embeddings
        with torch.no_grad():
            self._load_layers(path, sec, stored)
            self._load_embeddings(path, sec, stored_emb)
        self._emb = list(self.embeddings.split(1))   # per-frame views: a decode gathers without a host -> device copy
        self._operands = [dict() for _ in self.weights]   # per layer: 'bf16x3' / 'fp32' operand, built once
        # 'half': the one sticky word every f16 launch of this decoder may raise and none clears
        self._sat = torch.zeros(1, dtype=torch.int32, device=self.device) if self._lv_dtype == "f16" else None
        torch.cuda.synchronize(self.device)

    def _open_header(self, path, header, device, arithmetic):
        """what the header alone decides: the arithmetic's operand dtype, the decoder's geometry and each layer's epilogue"""
        # the operand dtype of the levels path (ops.levels_operand / conv3_forward_levels_raw); None: no such path ('exact')
        self._lv_dtype = {"exact": None, "levels": "bf16", "half": "f16"}[arithmetic]
        if self._lv_dtype is not None and header.get("hadamard"):
            raise ValueError(f"{path}: a Hadamard-domain file stores the levels of the TRANSFORMED weights, not the convolution's: "
                             f"arithmetic={arithmetic!r} does not apply")
        self.arithmetic, self.levels_used = arithmetic, {}
        self.levels_ineligible = {}    # 'levels' / 'half': layer -> why it can never take the path (whatever the batch size)
        self.header, self.device = header, torch.device(device)
        self.arch, self.cfg, self.frames = header["arch"], header["cfg"], int(header["frames"])
        _check_decoder_shape(self.arch, self.cfg)
        cfg = self.cfg
        strides = list(cfg["dec_strides"])
        if len(header["layers"]) != len(strides) + 2:
            raise ValueError(f"{path}: {len(header['layers'])} layers stored, the configuration describes {len(strides) + 2}")
        p = int(np.prod(strides))
        if self.arch == "hnerv":   # models/HNeRV.py / NeRV.py: the channel -> space reshape after layer 0
            self.fc_hw = (int(np.prod(cfg["enc_strides"]) // p),) * 2
        else:
            self.fc_hw = (int(cfg["crop_h"] // p), int(cfg["crop_w"] // p))
        self._r = [1] + [int(s) for s in strides] + [1]
        self._epi = [ops.EPI_PLAIN] + [ops.EPI_PS_GELU] * len(strides) + [ops.EPI_TANH]

    def _dequant(self, sec, st, shape, integers=False):
        """the level tensor `st` dequantised on the GPU by its scale sections -> (tensor, n, delta).  integers: n = level -
        zero_point, the same uploaded arrays decoded once more with a step of one ((float(level) - zp) * 1 is exact); else None"""
        delta, zp = (_upload(sec[f"{st.name}.{k}"], self.device).float() for k in ("delta", "zero_point"))
        dev = _DeviceLevels(st, self.device)
        w = dev.dequant(delta, zp, shape)
        return w, (dev.dequant(torch.ones_like(delta), zp, shape) if integers else None), delta

    def _load_layers(self, path, sec, stored):
        """weights, biases and (arithmetic 'levels' / 'half') the level operands of the layers that are eligible, in layer order"""
        header, on_levels = self.header, self._lv_dtype is not None
        self.weights, self.biases = [], []
        self._levels = [None] * len(header["layers"])   # per layer: (levels operand, delta per output channel) where eligible
        # the level tensors this file stores and the bytes of their sections (unpadded), per coding
        self.level_tensors = {c: sum(st.coding == c for st in stored.values()) for c in ("packed", "rans")}
        self.level_bytes = {c: sum(st.nbytes for st in stored.values() if st.coding == c) for c in ("packed", "rans")}
        for i, lay in enumerate(header["layers"]):
            co, ci, k, k2 = lay["shape"]
            w, n, delta = self._dequant(sec, stored[f"w{i}"], (co, lay["c_in_stored"], k, k2), integers=on_levels)
            if on_levels:
                # eligible: a 3 x 3 / 5 x 5 layer with integer n that bf16 holds exactly and finite steps; the reason a
                # layer is not stays on the decoder.  (The operand is then built without a second look at n: whatever
                # levels_operand still raises is a fault of this code, not a property of the file.)
                why = (f"kernel size {k} x {k2}" if k != k2 or k not in (3, 5) else
                       "a step that is not finite" if not bool(torch.isfinite(delta).all()) else
                       "level - zero_point is not an integer of magnitude <= 256" if not ops.levels_representable(n) else None)
                if why is None:
                    self._levels[i] = (ops.levels_operand(n, checked=True, dtype=self._lv_dtype),
                                       delta.reshape(-1).expand(co).contiguous())
                else:
                    self.levels_ineligible[i] = why
                del n
            if header["hadamard"]:
                w = ops.hadamard_along_channel_weight(w, n_out=ci)
            elif lay["c_in_stored"] != ci:
                raise ValueError(f"{path}: layer {i} stores {lay['c_in_stored']} input channels outside the Hadamard domain")
            if header["bias"] == "soft":
                b = _upload(sec[f"b{i}.soft"], self.device).float()
            else:
                b = self._dequant(sec, stored[f"b{i}"], (co,))[0]
            self.weights.append(w.contiguous())
            self.biases.append(b.contiguous())

    def _load_embeddings(self, path, sec, stored_emb):
        """one embedding per frame: restored from levels, the file's fp32 section, or (NeRV) the position code"""
        self.embedding_info = None   # quantised embeddings: {bits, coding, temporal, bytes (their sections, unpadded)}
        if stored_emb is not None:
            self.embeddings = restore_embeddings(stored_emb, self.device)
            self.embedding_info = dict(bits=stored_emb["bits"], coding=stored_emb["coding"], temporal=stored_emb["temporal"],
                                       bytes=sum(a.nbytes for n_, a in sec.items() if n_.startswith("embeddings.")))
        elif self.arch == "hnerv":
            self.embeddings = _upload(sec["embeddings"], self.device).float().view(self.header["embedding_shape"])
        else:   # NeRV.encode(idx / n) for every frame: elementwise, so a row does not depend on its batch
            from .models._layers import PositionEncoding
            t = torch.arange(self.frames, device=self.device).float() / self.frames
            self.embeddings = PositionEncoding(self.cfg["base"], self.cfg["level"])(t[:, None]).float()
        if self.embeddings.shape[0] != self.frames:
            raise ValueError(f"{path}: {self.embeddings.shape[0]} embeddings for {self.frames} frames")

    def _takes_levels(self, i, x):
        """layer i runs on its integer levels for input x: eligible, bf16x3 precision, and the library offers the shape"""
        cout, cin, k, _ = self.weights[i].shape
        B, _, H, W = x.shape
        return self._levels[i] is not None and ops._use3(None) and ops.conv3_levels_supported(B, cin, H, W, cout, k)

    def _conv(self, i, x):
        """layer i on x: the kernel family ops.conv2d_fused picks in its inference branch, on the cached operand."""
        w, b = self.weights[i], self.biases[i]
        cout, cin, k, _ = w.shape
        B, _, H, W = x.shape
        ops_ = self._operands[i]
        if self._takes_levels(i, x):
            lv = self._levels[i]
            return ops.conv3_forward_levels_raw(x, lv[0], lv[1], b, cout, k, self._epi[i], self._r[i], self._lv_dtype, self._sat)[0]
        if ops._use3(None) and ops.conv3_supported(B, cin, H, W, cout, k):
            if "bf16x3" not in ops_:
                ops_["bf16x3"] = ops.weight_layout3(w)
            return ops.conv3_forward_raw(x, ops_["bf16x3"], b, cout, k, self._epi[i], self._r[i])[0]
        if "fp32" not in ops_:
            ops_["fp32"] = ops.weight_layouts(w, False)[:2]
        wt, dims = ops_["fp32"]
        return ops.conv_forward_raw(x, wt, dims, b, cout, k, self._epi[i], self._r[i])[0]

    def saturated(self):
        """arithmetic='half': True once any launch of this decoder clamped a finite activation beyond the range of IEEE half
        (+-65504); the frames decoded since open are then not the file's.  One synchronise.  Always False otherwise."""
        return self._sat is not None and bool(self._sat.item())

    @torch.no_grad()
    def decode(self, indices, out="float", layout="chw", matrix="bt709", full_range=False):
        """frames `indices` (sequence or tensor of ints) -> (B, 3, H, W) fp32 in [0, 1] (`out='float'`), uint8
        (`out='u8'`; layout 'chw' or 'hwc') or uint8 (B, H * W * 3 / 2) I420 video frames (`out='yuv420'`; `matrix` 'bt709' or
        'bt601', `full_range`: converted from the float frame, so there is one rounding).  One call is one batch: the batch
        size selects the kernels as it does in the live model."""
        if out not in ("float", "u8", "yuv420"):
            raise ValueError(f"out must be 'float', 'u8' or 'yuv420', got {out!r}")
        if out != "u8" and layout != "chw":
            raise ValueError("float and yuv420 frames are planar; layout applies to out='u8'")
        if out == "yuv420" and matrix not in ops.YUV_MATRICES:   # before any launch
            raise ValueError(f"matrix must be one of {sorted(ops.YUV_MATRICES)}, got {matrix!r}")
        idx = [int(i) for i in (indices.reshape(-1).tolist() if isinstance(indices, torch.Tensor) else indices)]
        if not idx or min(idx) < 0 or max(idx) >= self.frames:
            raise IndexError(f"frame indices must lie in [0, {self.frames})")
        x = self._emb[idx[0]] if len(idx) == 1 else torch.cat([self._emb[i] for i in idx])
        taken = None if len(idx) in self.levels_used else []    # the first decode of a batch size records its path
        for i in range(len(self.weights)):
            if taken is not None and self._takes_levels(i, x):
                taken.append(i)
            x = self._conv(i, x)
            if i == 0 and self.fc_hw != (1, 1):
                x = ops._space_from_channels(x, *self.fc_hw).contiguous()
        if taken is not None:
            self.levels_used[len(idx)] = taken
        if out == "yuv420":
            return ops.frames_to_yuv420(x, matrix, full_range)
        return x if out == "float" else ops.frames_to_u8(x, layout)

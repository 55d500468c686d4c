"""Independent numpy restatement of the `.nqv` container, written from that section and importing nothing
from the package's writer or reader: the bit order of the packed levels, the header, a section reader and a writer.

Bit order: level i of a b-bit tensor occupies bits [i*b, (i+1)*b) of the stream; bit j of the stream is bit j % 32 of
little-endian 32-bit word j / 32.  Equivalently: write every level LSB first into one long bit string and cut it into bytes
LSB first -- which is what numpy's packbits / unpackbits do with bitorder='little'.
"""
import json
import struct

import numpy as np

MAGIC = b"NQV1"
DTYPES = {"u16": "<u2", "u32": "<u4", "f16": "<f2", "f32": "<f4"}


def align4(n):
    return (n + 3) // 4 * 4


def packed_words(n, b):
    return -(-(n * b) // 32) if n > 0 and 1 <= b <= 8 else 0


def pack(levels, b):
    """uint8 levels -> uint32 words (zero tail bits)."""
    lv = np.asarray(levels, dtype=np.uint8).reshape(-1)
    bits = np.unpackbits(lv[:, None], axis=1, bitorder="little")[:, :b].reshape(-1)     # level i -> bits i*b .. i*b+b-1
    nw = packed_words(lv.size, b)
    bits = np.concatenate([bits, np.zeros(nw * 32 - bits.size, dtype=np.uint8)])
    return np.packbits(bits, bitorder="little").view("<u4")


def unpack(words, n, b):
    """uint32 words -> the first n levels (uint8)."""
    bits = np.unpackbits(np.asarray(words, dtype="<u4").view(np.uint8), bitorder="little")[:n * b].reshape(n, b)
    return np.packbits(bits, axis=1, bitorder="little").reshape(n)


def write(path, header, sections, version=1):
    """sections: [(name, dtype tag, array)].  -> the header written (with its section table)."""
    table, blobs, pos = [], [], 0
    for name, tag, arr in sections:
        raw = np.asarray(arr).reshape(-1).astype(DTYPES[tag]).tobytes()
        table.append({"name": name, "dtype": tag, "count": int(np.asarray(arr).size), "offset": pos, "bytes": len(raw)})
        blobs.append(raw.ljust(align4(len(raw)), b"\0"))
        pos += len(blobs[-1])
    header = dict(header, version=version, sections=table)
    hj = json.dumps(header).encode("utf-8")
    with open(path, "wb") as f:
        f.write(MAGIC + struct.pack("<I", len(hj)) + hj.ljust(align4(8 + len(hj)) - 8, b"\0") + b"".join(blobs))
    return header


def read(path):
    """-> (header, {name: array}, payload start).  Trusts the file: the validation under test lives in the package."""
    data = open(path, "rb").read()
    assert data[:4] == MAGIC
    (hlen,) = struct.unpack("<I", data[4:8])
    header = json.loads(data[8:8 + hlen].decode("utf-8"))
    start = align4(8 + hlen)
    out = {s["name"]: np.frombuffer(data, DTYPES[s["dtype"]], s["count"], start + s["offset"]) for s in header["sections"]}
    return header, out, start


def dequant(words, delta, zp, shape, b):
    """fp32 (level - zp) * delta with one delta / zp per shape[0] or a single one."""
    n = int(np.prod(shape))
    lv = unpack(words, n, b).astype(np.float32).reshape(shape)
    d, z = np.asarray(delta, dtype=np.float32), np.asarray(zp, dtype=np.float32)
    bshape = (-1,) + (1,) * (len(shape) - 1) if d.size > 1 else (1,) * len(shape)
    return ((lv - z.reshape(bshape)) * d.reshape(bshape)).astype(np.float32)


def hadamard_rows(w):
    """orthonormal Walsh-Hadamard transform along axis 1 (length a power of two), float64 butterflies -> fp32."""
    n = w.shape[1]
    x = w.astype(np.float64).copy()
    h = 1
    while h < n:
        x = x.reshape(w.shape[0], n // (2 * h), 2, h, *w.shape[2:])
        a, b = x[:, :, 0].copy(), x[:, :, 1].copy()
        x[:, :, 0], x[:, :, 1] = a + b, a - b
        x = x.reshape(w.shape)
        h *= 2
    return (x / np.sqrt(n)).astype(np.float32)


def weights_of(path):
    """[(W, b)] fp32 numpy per layer, decoded with this module alone (Hadamard files: transformed back and sliced)."""
    header, sec, _ = read(path)
    out = []
    for i, lay in enumerate(header["layers"]):
        co, ci, k, k2 = lay["shape"]
        W = dequant(sec[f"w{i}.levels"], sec[f"w{i}.delta"].astype(np.float32), sec[f"w{i}.zero_point"].astype(np.float32),
                    (co, lay["c_in_stored"], k, k2), lay["n_bits"])
        if header["hadamard"]:
            W = hadamard_rows(W)[:, :ci]
        if header["bias"] == "soft":
            b = sec[f"b{i}.soft"].astype(np.float32)
        else:
            b = dequant(sec[f"b{i}.levels"], sec[f"b{i}.delta"].astype(np.float32), sec[f"b{i}.zero_point"].astype(np.float32),
                        (co,), lay["bias_n_bits"])
        out.append((np.ascontiguousarray(W), b))
    return header, sec, out

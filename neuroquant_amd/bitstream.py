"""Packed bit-stream container (`.nqv`) of a calibrated model and the GPU player that decodes it.

`write_stream` turns a calibrated `QuantModel` into ONE self-describing file whose size is the nominal bit-rate: the integer
levels of `export._levels`, packed at their bit-width by a HIP kernel, the quantiser scales, the biases and (HNeRV) the frame
embeddings.  `read_container` parses such a file with numpy alone.  `StreamDecoder` opens a file -- no QuantModel, no
checkpoint -- rebuilds every weight bit for bit (unpack + dequantise on the GPU, inverse Hadamard where the file says so),
builds each layer's convolution operand once and then decodes frames with the very launches the no-grad branch of
`models/_decode.run_decoder` issues, so for the same batch size and convolution precision its output equals the live
model's evaluation bit for bit.

The file realises the NOMINAL size (bits x parameters); the levels are not entropy coded and the embeddings stay fp32.
"""
import json
import math
import os
import struct

import numpy as np
import torch

from . import ops

MAGIC = b"NQV1"
VERSION = 1
_DTYPES = {"u32": "<u4", "f16": "<f2", "f32": "<f4"}


def _align4(n):
    return (n + 3) & ~3


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


# ------------------------------------------------------------------------------------------ writer
def _scale_section(t):
    """fp16 when every entry survives the round trip (true after AdaRound's init, quantizer.py:264-265), else fp32."""
    t = t.detach().float().reshape(-1).cpu()
    tag = "f16" if torch.equal(t.half().float(), t) else "f32"
    return tag, t.numpy().astype(_DTYPES[tag])


def _packed(q, x):
    """packed words (numpy uint32) of tensor x under quantiser q.  Unpacks them again on the GPU and compares with q's
    hard-rounded forward bit for bit, so a file that cannot reproduce the model is never written."""
    from .export import _levels
    from .quantization.quantizer import AdaRoundQuantizer
    if isinstance(q, AdaRoundQuantizer):
        hard = ops.adaround_forward(x, q.alpha.data, q.delta.data, q.zero_point, q.n_levels, False)
    else:
        hard = ops.uaq_forward(x, q.delta.data, q.zero_point, q.n_levels)
    words = ops.pack_levels(_levels(q, x), q.n_bits)
    delta, zp = q.delta.detach().float().reshape(-1), q.zero_point.detach().float().reshape(-1)
    if not torch.equal(ops.unpack_dequant(words, delta, zp, x.shape, q.n_bits), hard):
        raise RuntimeError("write_stream: packed levels do not reproduce the quantiser's output")
    return words.cpu().numpy().view(np.uint32)


def _check_decoder_shape(arch, cfg):
    if arch not in ("hnerv", "nerv"):
        raise ValueError(f"unknown arch {arch!r}")
    if cfg.get("out_bias") != "tanh" or cfg.get("dec_acts") != "gelu":
        raise ValueError("the player decodes the shipped decoder only: exact-GELU blocks and a tanh head")


@torch.no_grad()
def write_stream(qnn, path, arch, cfg, embeddings=None, frames=None, bias="soft"):
    """Write the calibrated `qnn` to `path`.  embeddings: HNeRV's per-frame input embeddings (tensor (N, c, h, w) or the list
    `evaluate()` returned); NeRV stores none and needs `frames`.  bias: 'soft' stores the fp32 bias the evaluated model uses,
    'hard' its packed integer decision (export.py's module docstring).  -> summary: file size, bytes per kind of section,
    bpp when the frame size is known, and the gap to the nominal size `export_quantized` reports."""
    from .quantization.quant_layer import QuantModule
    from .quantization.quantizer import AdaRoundQuantizer
    if bias not in ("soft", "hard"):
        raise ValueError(f"bias must be 'soft' or 'hard', got {bias!r}")
    _check_decoder_shape(arch, cfg)
    emb = None
    if arch == "hnerv":
        if embeddings is None:
            raise ValueError("an HNeRV stream stores the frame embeddings: pass embeddings=")
        emb = (torch.cat(list(embeddings), 0) if isinstance(embeddings, (list, tuple)) else embeddings).detach().float()
        frames = emb.shape[0] if frames is None else frames
        if frames != emb.shape[0]:
            raise ValueError(f"{frames} frames but {emb.shape[0]} embeddings")
    elif frames is None:
        raise ValueError("a NeRV stream needs the frame count: pass frames=")
    mods = [m for m in qnn.model.modules() if isinstance(m, QuantModule)]
    layers, sections, nominal_bits = [], [], 0
    for i, m in enumerate(mods):
        wq, bq = m.weight_quantizer, m.bias_quantizer
        if not getattr(wq, "inited", True) or wq.delta is None or bq.delta is None or not m._hip_ok:
            raise ValueError(f"layer {i}: quantisers are not initialised (run one quantised forward first) or the layer is "
                             "not a stride-1 'same' convolution")
        src = m.hadamard_weight if m.hadamard else m.weight.data
        if isinstance(wq, AdaRoundQuantizer) and wq.soft_targets:
            raise ValueError(f"layer {i}: weight quantiser still rounds softly; a stream stores hard decisions")
        lay = dict(shape=list(m.weight.shape), c_in_stored=int(src.shape[1]), n_bits=int(wq.n_bits),
                   scale_rows=int(wq.delta.numel()))
        sections.append((f"w{i}.levels", "u32", _packed(wq, src)))
        for key, t in (("delta", wq.delta), ("zero_point", wq.zero_point)):
            lay[f"{key}_dtype"], arr = _scale_section(t)
            sections.append((f"w{i}.{key}", lay[f"{key}_dtype"], arr))
        if bias == "soft":
            sections.append((f"b{i}.soft", "f32", bq(m.bias).detach().float().cpu().numpy()))
        else:
            lay.update(bias_n_bits=int(bq.n_bits), bias_scale_rows=int(bq.delta.numel()))
            sections.append((f"b{i}.levels", "u32", _packed(bq, m.bias.data)))
            for key, t in (("delta", bq.delta), ("zero_point", bq.zero_point)):
                lay[f"bias_{key}_dtype"], arr = _scale_section(t)
                sections.append((f"b{i}.{key}", lay[f"bias_{key}_dtype"], arr))
        layers.append(lay)
        nominal_bits += wq.n_bits * m.weight.numel() + bq.n_bits * m.bias.numel()   # as export_quantized counts them
    header = dict(arch=arch, cfg=cfg, frames=int(frames), hadamard=bool(qnn.hadamard), bias=bias, layers=layers,
                  embedding_shape=None)
    if emb is not None:
        header["embedding_shape"] = list(emb.shape)
        sections.append(("embeddings", "f32", emb.cpu().numpy()))
    header, size = _write_container(path, header, sections)
    kinds = {}
    for s in header["sections"]:
        kind = "embeddings" if s["name"] == "embeddings" else ("weight_" if s["name"][0] == "w" else "bias_") + s["name"].split(".")[1]
        kinds[kind] = kinds.get(kind, 0) + _align4(s["bytes"])
    nominal = math.ceil(nominal_bits / 8)
    summary = dict(path=path, file_bytes=size, header_bytes=size - sum(kinds.values()), section_bytes=kinds,
                   total_bytes_nominal=nominal, gap_to_nominal_bytes=size - nominal, frames=int(frames), bias=bias,
                   scale_dtypes=[[l["delta_dtype"], l["zero_point_dtype"]] for l in layers])
    h, w = cfg.get("crop_h"), cfg.get("crop_w")
    if frames and h and w:
        summary["bpp"] = size * 8 / (frames * h * w)
    return summary


# ------------------------------------------------------------------------------------------ player
class StreamDecoder:
    """Decode frames from a `.nqv` file alone.  Weights, biases and embeddings are rebuilt once at open; each layer's
    convolution operand is built once (per kernel family, the first time a batch size selects it); `decode` issues plain
    launches only."""

    def __init__(self, path, device="cuda"):
        if not torch.cuda.is_available():
            raise RuntimeError("neuroquant_amd needs an AMD GPU (no CPU path)")
        header, sec = read_container(path)
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

        def up(name):
            a = np.array(sec[name])   # a writable copy; the packed words travel as int32, the dtype ops takes
            return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(self.device)

        self.weights, self.biases = [], []
        with torch.no_grad():
            for i, lay in enumerate(header["layers"]):
                co, ci, k, k2 = lay["shape"]
                w = ops.unpack_dequant(up(f"w{i}.levels"), up(f"w{i}.delta").float(),
                                       up(f"w{i}.zero_point").float(), (co, lay["c_in_stored"], k, k2), lay["n_bits"])
                if header["hadamard"]:
                    w = ops.hadamard_along_channel_weight(w, n_out=ci)
                elif lay["c_in_stored"] != ci:
                    raise ValueError(f"{path}: layer {i} stores {lay['c_in_stored']} input channels outside the Hadamard domain")
                if header["bias"] == "soft":
                    b = up(f"b{i}.soft").float()
                else:
                    b = ops.unpack_dequant(up(f"b{i}.levels"), up(f"b{i}.delta").float(),
                                           up(f"b{i}.zero_point").float(), (co,), lay["bias_n_bits"])
                self.weights.append(w.contiguous())
                self.biases.append(b.contiguous())
            if self.arch == "hnerv":
                self.embeddings = up("embeddings").float().view(header["embedding_shape"])
            else:   # NeRV.encode(idx / n) for every frame: elementwise, so a row does not depend on its batch
                from .models._layers import PositionEncoding
                t = torch.arange(self.frames, device=self.device).float() / self.frames
                self.embeddings = PositionEncoding(cfg["base"], cfg["level"])(t[:, None]).float()
        if self.embeddings.shape[0] != self.frames:
            raise ValueError(f"{path}: {self.embeddings.shape[0]} embeddings for {self.frames} frames")
        self._emb = list(self.embeddings.split(1))   # per-frame views: a decode gathers without a host -> device copy
        self._operands = [dict() for _ in self.weights]   # per layer: 'bf16x3' / 'fp32' operand, built once
        torch.cuda.synchronize(self.device)

    def _conv(self, i, x):
        """layer i on x: the kernel family ops.conv2d_fused picks in its inference branch, on the cached operand."""
        w, b = self.weights[i], self.biases[i]
        cout, cin, k, _ = w.shape
        B, _, H, W = x.shape
        ops_ = self._operands[i]
        if ops._use3(None) and ops.conv3_supported(B, cin, H, W, cout, k):
            if "bf16x3" not in ops_:
                ops_["bf16x3"] = ops.weight_layout3(w)
            return ops.conv3_forward_raw(x, ops_["bf16x3"], b, cout, k, self._epi[i], self._r[i])[0]
        if "fp32" not in ops_:
            ops_["fp32"] = ops.weight_layouts(w, False)[:2]
        wt, dims = ops_["fp32"]
        return ops.conv_forward_raw(x, wt, dims, b, cout, k, self._epi[i], self._r[i])[0]

    @torch.no_grad()
    def decode(self, indices, out="float", layout="chw"):
        """frames `indices` (sequence or tensor of ints) -> (B, 3, H, W) fp32 in [0, 1] (`out='float'`) or uint8
        (`out='u8'`; layout 'chw' or 'hwc').  One call is one batch: the batch size selects the kernels as it does in the
        live model."""
        if out not in ("float", "u8"):
            raise ValueError(f"out must be 'float' or 'u8', got {out!r}")
        if out == "float" and layout != "chw":
            raise ValueError("float frames are planar; layout applies to out='u8'")
        idx = [int(i) for i in (indices.reshape(-1).tolist() if isinstance(indices, torch.Tensor) else indices)]
        if not idx or min(idx) < 0 or max(idx) >= self.frames:
            raise IndexError(f"frame indices must lie in [0, {self.frames})")
        x = self._emb[idx[0]] if len(idx) == 1 else torch.cat([self._emb[i] for i in idx])
        x = self._conv(0, x)
        if self.fc_hw != (1, 1):
            x = ops._space_from_channels(x, *self.fc_hw).contiguous()
        for i in range(1, len(self.weights)):
            x = self._conv(i, x)
        return x if out == "float" else ops.frames_to_u8(x, layout)

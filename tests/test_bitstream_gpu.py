"""Packed bit stream on the GPU: the pack / unpack / 8-bit frame kernels held bit-exact to host restatements at the shapes
where they can go wrong, and the container + player end to end: a file written from a calibrated model, opened alone,
decodes to the live model's evaluation bit for bit; the same file decoded with the numpy restatement of the format
(tests/bitstream_ref.py) and the CPU oracle gives the same PSNR within the bound test_export_quantized already holds."""
import logging
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import bitstream_ref as R
from conftest import BITS, ROOT, T, TINY_HNERV, TINY_NERV, state_dict_from_npz
from oracle import nq_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 64


@pytest.fixture(scope="module")
def ops():
    from neuroquant_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


# ------------------------------------------------------------------------------------------ kernels
SHAPES = [(1, 1), (1, 31), (1, 32), (1, 33), (7, 75), (3, 1), (5, 64), (13, 4097 // 13 + 1), (24, 256 * 9)]


def _raw_pack(lib_, lv, words, n, b):
    from neuroquant_amd import _lib
    _lib.check(lib_.nq_pack_levels(lv.data_ptr(), words.data_ptr(), n, b, torch.cuda.current_stream().cuda_stream), "pack")


def _raw_unpack(lib_, words, delta, zp, w, rows, row_len, b):
    from neuroquant_amd import _lib
    _lib.check(lib_.nq_unpack_dequant(words.data_ptr(), delta.data_ptr(), zp.data_ptr(), w.data_ptr(), rows, row_len, b,
                                      torch.cuda.current_stream().cuda_stream), "unpack")


@pytest.mark.parametrize("b", range(2, 9))
def test_pack_unpack_edge_shapes(ops, b):
    from neuroquant_amd import _lib
    lib_ = _lib.lib()
    g = torch.Generator().manual_seed(100 + b)
    for rows, row_len in SHAPES:
        n = rows * row_len
        lv = torch.randint(0, 2 ** b, (n,), generator=g, dtype=torch.int64).to(torch.uint8)
        delta = torch.rand(rows, generator=g) * 0.1 + 1e-3
        zp = torch.rand(rows, generator=g) * (2 ** b - 1)           # non-integer on purpose
        want_words = R.pack(lv.numpy(), b)
        nw = R.packed_words(n, b)
        assert ops.packed_words(n, b) == nw == len(want_words)
        # pack: into a buffer with sentinels after the end, twice
        lv_d = lv.to(DEV)
        bufs = []
        for _ in range(2):
            buf = torch.full((nw + SENT,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
            _raw_pack(lib_, lv_d, buf, n, b)
            bufs.append(buf.cpu())
        assert torch.equal(bufs[0], bufs[1])
        assert bufs[0][:nw].numpy().view("<u4").tobytes() == want_words.tobytes(), (rows, row_len)
        assert bool((bufs[0][nw:] == 0x5A5A5A5A).all()), (rows, row_len)
        if (rows, row_len) in ((5, 64), (7, 75)):    # a level array that is not 16-byte aligned takes the byte loads
            off = torch.cat([torch.zeros(1, dtype=torch.uint8), lv]).to(DEV)[1:]
            assert off.data_ptr() % 16 != 0
            buf = torch.zeros(nw, dtype=torch.int32, device=DEV)
            _raw_pack(lib_, off, buf, n, b)
            assert torch.equal(buf.cpu(), bufs[0][:nw])
        words = ops.pack_levels(lv_d.view(rows, row_len), b)
        assert words.dtype == torch.int32 and torch.equal(words.cpu(), bufs[0][:nw])
        # unpack + dequantise: exactly nw words allocated (a read past them is out of the tensor), sentinels after the output
        want = (lv.float().view(rows, row_len) - zp[:, None]) * delta[:, None]
        d_d, z_d = delta.to(DEV), zp.to(DEV)
        outs = []
        for _ in range(2):
            out = torch.full((n + SENT,), -12345.0, device=DEV)
            _raw_unpack(lib_, words, d_d, z_d, out, rows, row_len, b)
            outs.append(out.cpu())
        assert torch.equal(outs[0], outs[1])
        assert torch.equal(outs[0][:n].view(rows, row_len), want), (rows, row_len)
        assert bool((outs[0][n:] == -12345.0).all()), (rows, row_len)
        assert torch.equal(ops.unpack_dequant(words, d_d, z_d, (rows, row_len), b).cpu(), want)
        # layer-wise: one scale for the whole tensor
        want1 = (lv.float() - zp[0]) * delta[0]
        assert torch.equal(ops.unpack_dequant(words, d_d[:1], z_d[:1], (n,), b).cpu(), want1)


def test_pack_refuses_levels_that_do_not_fit(ops):
    lv = torch.tensor([0, 3, 4, 1], dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        ops.pack_levels(lv, 2)
    # the kernel itself masks: a stray high bit cannot spill into the neighbours
    from neuroquant_amd import _lib
    words = torch.zeros(1, dtype=torch.int32, device=DEV)
    _raw_pack(_lib.lib(), lv, words, 4, 2)
    assert int(words.cpu()[0]) == (0 | 3 << 2 | 0 << 4 | 1 << 6)


def _u8_ref(x):
    x = torch.where(torch.isnan(x), torch.zeros_like(x), x)
    return (x.clamp(0, 1) * 255).round().to(torch.uint8)


@pytest.mark.parametrize("layout", ("chw", "hwc"))
@pytest.mark.parametrize("shape", [(1, 3, 1, 1), (2, 3, 5, 7), (3, 1, 3, 3), (1, 3, 320, 640)])
def test_frames_to_u8(ops, shape, layout):
    from neuroquant_amd import _lib
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.rand(shape, generator=g)
    special = torch.tensor([0.5, 0.0, 1.0, -0.25, 1.75, float("inf"), float("-inf"), float("nan"), 1.5 / 255, 2.5 / 255])
    flat = x.view(-1)
    k = min(flat.numel(), special.numel())
    pos = torch.randperm(flat.numel(), generator=g)[:k]
    flat[pos] = special[:k]
    if flat.numel() >= special.numel():
        assert float(_u8_ref(torch.tensor([0.5]))[0]) == 128          # 127.5 is exact and rounds to even
    want = _u8_ref(x)
    if layout == "hwc":
        want = want.permute(0, 2, 3, 1).contiguous()
    x_d = x.to(DEV)
    got = ops.frames_to_u8(x_d, layout)
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape)
    assert torch.equal(got.cpu(), want)
    n, C, H, W = shape
    buf = torch.full((x.numel() + SENT,), 0xA5, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().nq_frames_to_u8(x_d.data_ptr(), buf.data_ptr(), n, C, H * W, 0 if layout == "chw" else 1,
                                          torch.cuda.current_stream().cuda_stream), "frames_to_u8")
    buf = buf.cpu()
    assert torch.equal(buf[:x.numel()], want.view(-1)) and bool((buf[x.numel():] == 0xA5).all())


# ------------------------------------------------------------------------------------------ end to end
class _Replay:
    def __init__(self, frames, order, n):
        self.frames, self.order, self.pos, self.n = frames, order, 0, n

    def __len__(self):
        return self.order.shape[1]

    def __iter__(self):
        ep = self.order[self.pos]
        self.pos += 1
        for idx in ep:
            idx_t = torch.as_tensor(idx, dtype=torch.int64, device=DEV)
            yield {"img": self.frames[idx_t], "idx": idx_t, "norm_idx": idx_t.float() / self.n}


def _build(arch, sd):
    from neuroquant_amd.models import HNeRV, NeRV
    model = (HNeRV if arch == "hnerv" else NeRV)(TINY_HNERV if arch == "hnerv" else TINY_NERV)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    return model.to(DEV).eval()


def _quant_model(golden, name, arch, had, bits=BITS, channel_wise=True):
    from neuroquant_amd.quantization import QuantModel
    z = golden(name)
    model = _build(arch, state_dict_from_npz(z, "sd:"))
    qnn = QuantModel(model, hadamard=had, weight_quant_params=dict(n_bits=8, channel_wise=channel_wise, scale_method="max"))
    qnn.set_bitwidth(bits)
    qnn.eval()
    qnn.set_quant_state(True)
    emb = T(z["emb"]).to(DEV)
    with torch.no_grad():
        qnn(emb[:2])
    return z, qnn, emb


@pytest.fixture(scope="module")
def frames(golden):
    return (T(golden("frames_320x640.npz")["frames"]).float() / 255.0).to(DEV)


@pytest.fixture(scope="module")
def hnerv_calibrated(golden, frames):
    """tiny HNeRV, bits [6,5,4,5,5,6,6], the 40-iteration calibration of test_export_quantized; shared, read-only."""
    from neuroquant_amd.quantization import model_reconstruction
    z, qnn, emb = _quant_model(golden, "traj_hnerv.npz", "hnerv", False)
    model_reconstruction(qnn, cali_data=emb, gt=_Replay(frames, z["order"], 8), arch="hnerv", batch_size=2, iters=40,
                         weight=0.01, hadamard=False, b_range=(20, 2), warmup=0.2, lr=0.003)
    qnn.set_quant_state(True)
    return z, qnn, emb


def _live(qnn, emb, B):
    with torch.no_grad():
        return [qnn(emb[j:j + B])[0] for j in range(0, emb.shape[0], B)]


def _assert_plays_back(ops, qnn, emb_of, path, n=8):
    """player output == live evaluation, bit for bit, for B = 1 and B = 2 over all frames; u8 == the torch restatement."""
    from neuroquant_amd.bitstream import StreamDecoder
    dec = StreamDecoder(str(path))
    for B in (1, 2):
        for j in range(0, n, B):
            idx = list(range(j, j + B))
            with torch.no_grad():
                live = qnn(emb_of(idx))[0]
            got = dec.decode(idx)
            assert got.dtype == torch.float32 and torch.equal(got, live), (B, j)
            want8 = _u8_ref(live.cpu())
            assert torch.equal(dec.decode(idx, out="u8").cpu(), want8)
            assert torch.equal(dec.decode(idx, out="u8", layout="hwc").cpu(), want8.permute(0, 2, 3, 1))
    return dec


def _oracle_psnr(z, weights, emb, frames):
    dec = O.Decoder.from_state_dict(state_dict_from_npz(z, "sd:"), "hnerv", [5, 4, 4, 2, 2])
    with torch.no_grad():
        return float(O.psnr_per_frame(dec.forward(emb.cpu(), [(T(W), T(b)) for W, b in weights]), frames.cpu()).double().mean())


def test_hnerv_stream_round_trip(ops, hnerv_calibrated, frames, tmp_path):
    """File sizes (measured on the tiny model, bits [6,5,4,5,5,6,6]) and scale dtypes are printed, not pinned; every equality
    below is."""
    from neuroquant_amd.bitstream import read_container, write_stream
    from neuroquant_amd.export import dequantize, export_quantized
    z, qnn, emb = hnerv_calibrated
    mods = qnn.quant_modules()
    path = tmp_path / "m.nqv"
    s = write_stream(qnn, str(path), "hnerv", dict(TINY_HNERV), embeddings=emb)
    nominal = export_quantized(qnn, str(tmp_path / "q"), frames=8, height=320, width=640)
    size = os.path.getsize(path)
    header, sec, start = R.read(str(path))
    assert read_container(str(path))[0] == header
    assert size == s["file_bytes"] == start + sum(R.align4(x["bytes"]) for x in header["sections"])
    assert s["total_bytes_nominal"] == nominal["total_bytes_nominal"] and s["gap_to_nominal_bytes"] == size - nominal["total_bytes_nominal"]
    assert abs(s["bpp"] - size * 8 / (8 * 320 * 640)) < 1e-12
    lev = sum(x["bytes"] for x in header["sections"] if x["name"].startswith("w") and x["name"].endswith(".levels"))
    assert lev == s["section_bytes"]["weight_levels"] == sum(4 * -(-(m.weight.numel() * b) // 32) for m, b in zip(mods, BITS))
    assert lev <= nominal["total_bytes_nominal"] + 4 * 2 * len(mods)
    print("stream: %d bytes (header %d, sections %s); nominal %d bytes; bpp %.5f" % (
        size, s["header_bytes"], s["section_bytes"], nominal["total_bytes_nominal"], s["bpp"]))
    # scales: bit-equal to the quantiser's, in whichever form the rule chose
    for i, (m, lay) in enumerate(zip(mods, header["layers"])):
        q = m.weight_quantizer
        for key, t in (("delta", q.delta), ("zero_point", q.zero_point)):
            got = sec[f"w{i}.{key}"]
            assert got.dtype == np.dtype(R.DTYPES[lay[f"{key}_dtype"]])
            assert np.array_equal(got.astype(np.float32), t.detach().cpu().numpy().reshape(-1))
        print("layer %d: %d bits, delta %s, zero_point %s" % (i, lay["n_bits"], lay["delta_dtype"], lay["zero_point_dtype"]))
        assert lay["n_bits"] == BITS[i] and lay["shape"] == list(m.weight.shape) and lay["c_in_stored"] == m.weight.shape[1]
    assert np.array_equal(sec["embeddings"].reshape(emb.shape), emb.cpu().numpy())
    # the player, alone
    dec = _assert_plays_back(ops, qnn, lambda idx: emb[idx], path)
    with torch.no_grad():
        psnr_eval = float(ops.frame_psnr(torch.cat(_live(qnn, emb, 1)), frames).double().mean())
        psnr_play = float(ops.frame_psnr(torch.cat([dec.decode([j]) for j in range(8)]), frames).double().mean())
    assert psnr_play == psnr_eval
    # the same file through the numpy reader / unpack and the CPU oracle: summation order only
    _, _, wts = R.weights_of(str(path))
    for (W, b), m in zip(wts, mods):
        with torch.no_grad():
            assert np.array_equal(W, m.weight_quantizer(m.weight).cpu().numpy())
            assert np.array_equal(b, m.bias_quantizer(m.bias).cpu().numpy())
    psnr_ref = _oracle_psnr(z, wts, emb, frames)
    print("evaluated %.4f dB, reference decode of the file %.4f dB" % (psnr_eval, psnr_ref))
    assert abs(psnr_ref - psnr_eval) < 2e-3
    # hard biases: what a pure integer stream carries
    hard = tmp_path / "h.nqv"
    sh = write_stream(qnn, str(hard), "hnerv", dict(TINY_HNERV), embeddings=emb, bias="hard")
    hh, hsec, hstart = R.read(str(hard))
    assert hh["bias"] == "hard" and os.path.getsize(hard) == sh["file_bytes"] == hstart + sum(R.align4(x["bytes"]) for x in hh["sections"])
    lev_h = sum(x["bytes"] for x in hh["sections"] if x["name"].endswith(".levels"))
    assert lev_h <= nominal["total_bytes_nominal"] + 4 * 2 * len(mods)
    from neuroquant_amd.bitstream import StreamDecoder
    dh = StreamDecoder(str(hard))
    with torch.no_grad():
        psnr_hard = float(ops.frame_psnr(torch.cat([dh.decode([j]) for j in range(8)]), frames).double().mean())
    deq = dequantize(str(tmp_path / "q"), bias="hard")
    for (W, b), (W2, b2) in zip(R.weights_of(str(hard))[2], deq):
        assert np.array_equal(W, W2) and np.array_equal(b, b2)
    psnr_hard_ref = _oracle_psnr(z, deq, emb, frames)
    print("hard-bias stream: player %.4f dB, oracle decode of export.dequantize %.4f dB (soft %.4f dB)" % (
        psnr_hard, psnr_hard_ref, psnr_eval))
    assert abs(psnr_hard - psnr_eval) < 0.1
    assert abs(psnr_hard - psnr_hard_ref) < 2e-3


def test_nerv_hadamard_stream_plays_back_bit_for_bit(ops, golden, frames, tmp_path):
    from neuroquant_amd.bitstream import write_stream
    from neuroquant_amd.quantization import model_reconstruction
    z, qnn, emb = _quant_model(golden, "traj_nerv_had.npz", "nerv", True)
    model_reconstruction(qnn, cali_data=emb, gt=_Replay(frames, z["order"], 8), arch="nerv", batch_size=2, iters=16,
                         weight=0.01, opt_mode="mse", hadamard=True, b_range=(20, 2), warmup=0.2, p=2.0, lr=0.003)
    qnn.set_quant_state(True)
    path = tmp_path / "n.nqv"
    s = write_stream(qnn, str(path), "nerv", dict(TINY_NERV), frames=8)
    header, sec, _ = R.read(str(path))
    assert header["hadamard"] is True and header["embedding_shape"] is None and "embeddings" not in sec
    for m, lay in zip(qnn.quant_modules(), header["layers"]):
        assert lay["c_in_stored"] == m.hadamard_weight.shape[1] >= lay["shape"][1] and lay["shape"] == list(m.weight.shape)
    print("nerv+hadamard stream: %d bytes, nominal %d" % (s["file_bytes"], s["total_bytes_nominal"]))

    def emb_of(idx):   # as evaluate() computes it
        return qnn.encode(torch.tensor(idx, device=DEV).float() / 8)
    _assert_plays_back(ops, qnn, emb_of, path)


@pytest.mark.parametrize("channel_wise", (True, False))
@pytest.mark.parametrize("bits", ([2, 3, 4, 6, 4, 4, 2], [8, 7, 3, 5, 2, 8, 7]))
def test_uncalibrated_extreme_widths(ops, golden, tmp_path, bits, channel_wise):
    """UAQ quantisers straight after their 'max' initialisation: delta / zero-point have not been through fp16."""
    from neuroquant_amd.bitstream import write_stream
    z, qnn, emb = _quant_model(golden, "traj_hnerv.npz", "hnerv", False, bits=bits, channel_wise=channel_wise)
    path = tmp_path / "u.nqv"
    s = write_stream(qnn, str(path), "hnerv", dict(TINY_HNERV), embeddings=emb)
    header, sec, _ = R.read(str(path))
    print("uncalibrated %s cw=%s: scale dtypes %s" % (bits, channel_wise, s["scale_dtypes"]))
    for i, (m, lay) in enumerate(zip(qnn.quant_modules(), header["layers"])):
        assert lay["n_bits"] == bits[i] and lay["scale_rows"] == (m.weight.shape[0] if channel_wise else 1)
        for key, t in (("delta", m.weight_quantizer.delta), ("zero_point", m.weight_quantizer.zero_point)):
            assert np.array_equal(sec[f"w{i}.{key}"].astype(np.float32), t.detach().cpu().numpy().reshape(-1))
    _assert_plays_back(ops, qnn, lambda idx: emb[idx], path)


# ------------------------------------------------------------------------------------------ layout of the file, open
@pytest.fixture(scope="module")
def hnerv_uncalibrated(golden):
    """tiny HNeRV, bits [6,5,4,5,5,6,6], quantisers straight after their 'max' initialisation; shared, read-only."""
    _, qnn, emb = _quant_model(golden, "traj_hnerv.npz", "hnerv", False)
    return qnn, emb


RANS_PARTS = ("rans_freq", "rans_states", "rans_offsets", "rans_words")
HEADER_KEYS = {"arch", "cfg", "frames", "hadamard", "bias", "layers", "embedding_shape", "version", "sections"}
LAYER_KEYS = {"shape", "c_in_stored", "n_bits", "scale_rows", "delta_dtype", "zero_point_dtype"}
HARD_KEYS = {"bias_n_bits", "bias_scale_rows", "bias_delta_dtype", "bias_zero_point_dtype"}


def test_section_order_and_header_keys(hnerv_uncalibrated, tmp_path):
    """The order of the sections is part of the format's bytes (the header is written with sorted keys, the sections are
    not sorted): per layer the weight's level sections, its two scales, then the bias; the embeddings last."""
    from neuroquant_amd.bitstream import write_stream
    qnn, emb = hnerv_uncalibrated
    L = len(BITS)

    def names(path, **kw):
        write_stream(qnn, str(path), "hnerv", dict(TINY_HNERV), embeddings=emb, **kw)
        header, _, _ = R.read(str(path))
        return header, [s["name"] for s in header["sections"]]

    header, got = names(tmp_path / "soft.nqv", bias="soft", coding="packed")
    assert got == [f"{t}{i}.{k}" for i in range(L) for t, k in (("w", "levels"), ("w", "delta"), ("w", "zero_point"), ("b", "soft"))
                   ] + ["embeddings"]
    assert set(header) == HEADER_KEYS and all(set(lay) == LAYER_KEYS for lay in header["layers"]) and len(header["layers"]) == L

    header, got = names(tmp_path / "hard.nqv", bias="hard", coding="rans", chunk=64)
    assert got == [f"{t}{i}.{k}" for i in range(L) for t in "wb" for k in RANS_PARTS + ("delta", "zero_point")] + ["embeddings"]
    coded_keys = {"levels_coding", "rans_chunk", "bias_levels_coding", "bias_rans_chunk"}
    assert set(header) == HEADER_KEYS and all(set(lay) == LAYER_KEYS | HARD_KEYS | coded_keys for lay in header["layers"])

    header, got = names(tmp_path / "emb.nqv", bias="soft", coding="packed", embedding_bits=6)
    coded = header["embedding"]["coding"] == "rans"
    assert got == [f"{t}{i}.{k}" for i in range(L) for t, k in (("w", "levels"), ("w", "delta"), ("w", "zero_point"), ("b", "soft"))
                   ] + ["embeddings.delta", "embeddings.zero_point", "embeddings.levels"] + (
                       [f"embeddings.{k}" for k in RANS_PARTS] if coded else [])
    assert set(header) == HEADER_KEYS | {"embedding"} and all(set(lay) == LAYER_KEYS for lay in header["layers"])


def test_open_decodes_each_tensor_from_one_upload_and_refuses_on_the_host(hnerv_uncalibrated, tmp_path):
    """'levels' takes each weight twice from the arrays it uploaded once (its own step, then a step of one): the weights are
    those of 'exact'.  A coded section one word short is refused by the host check, before any kernel."""
    from neuroquant_amd.bitstream import StreamDecoder, write_stream
    qnn, emb = hnerv_uncalibrated
    path = str(tmp_path / "hard.nqv")
    write_stream(qnn, path, "hnerv", dict(TINY_HNERV), embeddings=emb, bias="hard", coding="rans", chunk=64)
    exact, levels = StreamDecoder(path, arithmetic="exact"), StreamDecoder(path, arithmetic="levels")
    assert len(exact.weights) == len(levels.weights) == len(BITS)
    for a, b in zip(exact.weights + exact.biases, levels.weights + levels.biases):
        assert torch.equal(a, b)
    header, sec, _ = R.read(path)
    want = sum(a.nbytes for name, a in sec.items() if name[0] in "wb" and ".rans_" in name)
    for dec in (exact, levels):
        assert dec.level_tensors == {"packed": 0, "rans": 14} and dec.level_bytes == {"packed": 0, "rans": want}

    def refused_one_short(src, victim):
        header, sec, _ = R.read(src)
        assert len(sec[victim]) > 0
        bad = str(tmp_path / "short.nqv")
        head = {k: v for k, v in header.items() if k not in ("version", "sections")}
        R.write(bad, head, [(s["name"], s["dtype"], sec[s["name"]][:-1] if s["name"] == victim else sec[s["name"]])
                            for s in header["sections"]])
        assert len(R.read(bad)[1][victim]) == len(sec[victim]) - 1
        with pytest.raises(ValueError, match=victim.split(".")[0]):
            StreamDecoder(bad)

    # chunks of 64 symbols give a lane one symbol, which never emits a word: every `rans_words` of this file is empty.  The
    # states of w0 lose an entry here; the words of a tensor that has some, in a file of larger chunks, below.
    assert len(sec["w0.rans_words"]) == 0
    refused_one_short(path, "w0.rans_states")
    longer = str(tmp_path / "hard4096.nqv")
    write_stream(qnn, longer, "hnerv", dict(TINY_HNERV), embeddings=emb, bias="hard", coding="rans", chunk=4096)
    refused_one_short(longer, "w1.rans_words")


# ------------------------------------------------------------------------------------------ drivers
def test_drivers_export_and_play_back(tmp_path):
    """calibrate_network --export_stream writes a stream whose playback (a fresh child process running the decode_stream
    command line) reports the PSNR the driver logged for 'Weight quantization w/ opt', to the printed digits; without the
    flag no stream appears."""
    from neuroquant_amd.methods import calibrate_network as cn
    root = logging.getLogger()
    saved = (root.level, list(root.handlers))

    def run(tag, extra):
        args = cn.parse_args(["--arch", "hnerv", "--synthetic", "8", "--batch_size", "2", "--channel_wise", "--init", "max",
                              "--iters_w", "24", "--weight", "0.01", "--b_start", "20", "--b_end", "2", "--warmup", "0.2",
                              "--lr", "0.003", "--precision", "6", "5", "4", "5", "5", "6", "6"] + extra)
        args.outf = str(tmp_path / tag)
        cn.seed_all(903)
        cn.calibrate(args, dict(TINY_HNERV))
        for h in list(root.handlers):          # the driver's own log file: close it before reading
            if h not in saved[1]:
                h.close()
                root.removeHandler(h)
        log = "".join(open(os.path.join(args.outf, f)).read() for f in sorted(os.listdir(args.outf)) if f.endswith(".log"))
        return log, sorted(os.listdir(args.outf))

    try:
        stream = tmp_path / "out" / "model.nqv"
        log, _ = run("with", ["--export_stream", str(stream)])
        log0, files0 = run("without", [])
    finally:
        root.setLevel(saved[0])
        for h in saved[1]:
            if h not in root.handlers:
                root.addHandler(h)
    assert stream.exists() and "bit stream: " in log
    assert "bit stream" not in log0 and not any(f.endswith(".nqv") for f in files0) and len(list(tmp_path.rglob("*.nqv"))) == 1
    logged = re.search(r"Weight quantization w/ opt: best_pred_seen_psnr: ([0-9.]+) \| best_pred_seen_ssim: ([0-9.]+)", log)
    assert logged, log
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "neuroquant_amd.methods.decode_stream", "--stream", str(stream), "--synthetic", "8",
                        "--out", str(tmp_path / "png")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    played = re.search(r"float: PSNR ([0-9.]+) \| MS-SSIM ([0-9.]+)", p.stdout)
    assert played and re.search(r"8-bit: PSNR ([0-9.]+) \| MS-SSIM ([0-9.]+)", p.stdout) and "decode FPS" in p.stdout
    assert played.group(1) == logged.group(1) and played.group(2) == logged.group(2)
    from PIL import Image
    pngs = sorted(os.listdir(tmp_path / "png"))
    assert len(pngs) == 8 and np.asarray(Image.open(tmp_path / "png" / pngs[0])).shape == (320, 640, 3)

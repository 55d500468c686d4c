"""Entropy-coded levels on the GPU: the rANS decode kernel run on streams encoded by the plain-Python restatement
(tests/rans_ref.py) at the shapes where it can go wrong, held bit-exact to the input levels and to the packed path's floats;
and the container + player end to end: rans / auto / packed files of one calibrated model all rebuild the same weights and
play back the live model's evaluation bit for bit."""
import logging
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import rans_ref as R
from conftest import BITS, ROOT, T, TINY_HNERV, TINY_NERV, state_dict_from_npz

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 64
NEW_KEYS = ("levels_coding", "rans_chunk", "bias_levels_coding", "bias_rans_chunk")


@pytest.fixture(scope="module")
def ops():
    from neuroquant_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


# ------------------------------------------------------------------------------------------ kernel
SHAPES = [(1, 1, 64), (1, 63, 64), (1, 64, 64), (1, 65, 64), (7, 75, 64), (13, 316, 128), (3, 1, 64), (24, 2304, 4096)]
KINDS = ("uniform", "peaked", "constant", "rare")


def _levels(kind, n, b, g):
    top = 2 ** b - 1
    if kind == "uniform":
        return torch.randint(0, 2 ** b, (n,), generator=g, dtype=torch.int64)
    if kind == "peaked":
        return torch.clamp(torch.round(torch.randn(n, generator=g) * 1.5 + 2 ** b / 2), 0, top).long()
    lv = torch.full((n,), min(3, top), dtype=torch.int64)
    if kind == "rare" and n > 1:
        lv[n // 3] = 0
    return lv


def _i16(v):
    return torch.from_numpy(np.array(v, dtype=np.uint16).view(np.int16)).to(DEV)


def _i32(v):
    return torch.from_numpy(np.array(v, dtype=np.uint32).view(np.int32)).to(DEV)


def _raw(lib_, words, states, offsets, freq, n, b, chunk, delta, zp, row_len, levels, w):
    from neuroquant_amd import _lib
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(lib_.nq_rans_decode(ptr(words), ptr(states), ptr(offsets), ptr(freq), n, b, chunk, ptr(delta), ptr(zp), row_len,
                                   ptr(levels), ptr(w), torch.cuda.current_stream().cuda_stream), "rans_decode")


@pytest.mark.parametrize("b", range(2, 9))
def test_rans_decode_edge_shapes(ops, b):
    from neuroquant_amd import _lib
    lib_ = _lib.lib()
    g = torch.Generator().manual_seed(200 + b)
    for rows, row_len, chunk in SHAPES:
        n = rows * row_len
        for kind in KINDS:
            lv = _levels(kind, n, b, g)
            freq, states, offsets, words = R.encode(lv.tolist(), b, chunk)
            chunks = -(-n // chunk)
            assert ops.rans_chunks(n, chunk) == chunks == len(offsets) - 1
            if kind == "constant":
                assert not words
            # buffers at exactly their size: a read past them is outside the tensor.  No word at all: one dummy entry, as the
            # entry point refuses a null pointer.
            w_d = _i16(words) if words else torch.zeros(1, dtype=torch.int16, device=DEV)
            s_d, o_d, f_d = _i32(states), _i32(offsets), _i16(freq)
            delta = torch.rand(rows, generator=g) * 0.1 + 1e-3
            zp = torch.rand(rows, generator=g) * (2 ** b - 1)       # non-integer on purpose
            d_d, z_d = delta.to(DEV), zp.to(DEV)
            lv8 = lv.to(torch.uint8)
            want = ops.unpack_dequant(ops.pack_levels(lv8.to(DEV), b), d_d, z_d, (rows, row_len), b).cpu()
            assert torch.equal(want, (lv.float().view(rows, row_len) - zp[:, None]) * delta[:, None])
            tag = (rows, row_len, chunk, kind)
            outs = []
            for _ in range(2):                                      # both outputs, twice
                lo = torch.full((n + SENT,), 0xA5, dtype=torch.uint8, device=DEV)
                wo = torch.full((n + SENT,), -12345.0, device=DEV)
                _raw(lib_, w_d, s_d, o_d, f_d, n, b, chunk, d_d, z_d, row_len, lo, wo)
                outs.append((lo.cpu(), wo.cpu()))
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), tag
            assert torch.equal(outs[0][0][:n], lv8), tag
            assert torch.equal(outs[0][1][:n].view(rows, row_len), want), tag
            assert bool((outs[0][0][n:] == 0xA5).all()) and bool((outs[0][1][n:] == -12345.0).all()), tag
            # each output pointer null in turn (no scales needed for levels alone)
            lo = torch.full((n + SENT,), 0xA5, dtype=torch.uint8, device=DEV)
            _raw(lib_, w_d, s_d, o_d, f_d, n, b, chunk, None, None, row_len, lo, None)
            assert torch.equal(lo.cpu(), outs[0][0]), tag
            wo = torch.full((n + SENT,), -12345.0, device=DEV)
            _raw(lib_, w_d, s_d, o_d, f_d, n, b, chunk, d_d, z_d, row_len, None, wo)
            assert torch.equal(wo.cpu(), outs[0][1]), tag
            # a single scale for the whole tensor
            wo = torch.full((n + SENT,), -12345.0, device=DEV)
            _raw(lib_, w_d, s_d, o_d, f_d, n, b, chunk, d_d[:1], z_d[:1], n, None, wo)
            want1 = ops.unpack_dequant(ops.pack_levels(lv8.to(DEV), b), d_d[:1], z_d[:1], (n,), b).cpu()
            assert torch.equal(wo.cpu()[:n], want1) and bool((wo.cpu()[n:] == -12345.0).all()), tag
            # the ops wrappers (they take the empty word tensor as it is)
            w_ops = _i16(words)
            assert torch.equal(ops.rans_decode(w_ops, s_d, o_d, f_d, n, b, chunk).cpu(), lv8), tag
            assert torch.equal(ops.rans_decode_dequant(w_ops, s_d, o_d, f_d, d_d, z_d, (rows, row_len), b, chunk).cpu(), want), tag


def test_ops_refuse_inconsistent_streams(ops):
    lv = [1, 2, 3, 0] * 1000                     # 16 symbols a lane at 2 bits each: every chunk owns words
    freq, states, offsets, words = R.encode(lv, 2, 1024)
    assert len(offsets) == 5 and offsets[1] > 0
    args = lambda **kw: [_i16(kw.get("words", words)), _i32(kw.get("states", states)), _i32(kw.get("offsets", offsets)),
                         _i16(kw.get("freq", freq))]
    assert ops.rans_decode(*args(), 4000, 2, 1024).cpu().tolist() == lv
    for bad in (dict(states=states[:-1]), dict(offsets=offsets[:-1]), dict(freq=freq + [0] * 4),
                dict(offsets=[1] + offsets[1:]), dict(offsets=offsets[:-1] + [offsets[-1] + 1]),
                dict(offsets=offsets[:1] + [offsets[2] + 1] + offsets[2:]), dict(words=words + [0])):
        with pytest.raises(ValueError):
            ops.rans_decode(*args(**bad), 4000, 2, 1024)
    for n, b, chunk in ((0, 2, 1024), (4000, 0, 1024), (4000, 9, 1024), (4000, 2, 1000), (4000, 2, 0)):
        with pytest.raises(ValueError):
            ops.rans_decode(*args(), n, b, chunk)


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


def _quant_model(golden, name, arch, had):
    from neuroquant_amd.models import HNeRV, NeRV
    from neuroquant_amd.quantization import QuantModel
    z = golden(name)
    model = (HNeRV if arch == "hnerv" else NeRV)(TINY_HNERV if arch == "hnerv" else TINY_NERV)
    missing, unexpected = model.load_state_dict(state_dict_from_npz(z, "sd:"), strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    qnn = QuantModel(model.to(DEV).eval(), hadamard=had, weight_quant_params=dict(n_bits=8, channel_wise=True, scale_method="max"))
    qnn.set_bitwidth(BITS)
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
    """tiny HNeRV, bits [6,5,4,5,5,6,6], 40 calibration iterations; its live evaluation for B = 1 and B = 2.  Shared, read-only."""
    from neuroquant_amd.quantization import model_reconstruction
    z, qnn, emb = _quant_model(golden, "traj_hnerv.npz", "hnerv", False)
    model_reconstruction(qnn, cali_data=emb, gt=_Replay(frames, z["order"], 8), arch="hnerv", batch_size=2, iters=40,
                         weight=0.01, hadamard=False, b_range=(20, 2), warmup=0.2, lr=0.003)
    qnn.set_quant_state(True)
    with torch.no_grad():
        live = {B: [qnn(emb[j:j + B])[0] for j in range(0, 8, B)] for B in (1, 2)}
    return qnn, emb, live


def _assert_plays_back(dec, live):
    for B in (1, 2):
        for k, j in enumerate(range(0, 8, B)):
            got = dec.decode(list(range(j, j + B)))
            assert got.dtype == torch.float32 and torch.equal(got, live[B][k]), (B, j)


def _level_section_bytes(header):
    return sum((s["bytes"] + 3) // 4 * 4 for s in header["sections"] if s["name"].endswith(".levels") or ".rans_" in s["name"])


def test_hnerv_codings_round_trip(ops, hnerv_calibrated, tmp_path):
    """Sizes of the tiny model's files are printed, not pinned; every equality is."""
    from neuroquant_amd.bitstream import DEFAULT_CHUNK, StreamDecoder, read_container, write_stream
    from neuroquant_amd.export import _entropy_bits, _levels
    qnn, emb, live = hnerv_calibrated
    mods = qnn.quant_modules()
    cfg = dict(TINY_HNERV)

    def write(name, **kw):
        path = str(tmp_path / name)
        return path, write_stream(qnn, path, "hnerv", cfg, embeddings=emb, **kw)

    p_default, s_default = write("default.nqv")
    p_packed, s_packed = write("packed.nqv", coding="packed")
    assert open(p_default, "rb").read() == open(p_packed, "rb").read()
    h_packed, sec_packed = read_container(p_packed)
    assert not any(k in lay for lay in h_packed["layers"] for k in NEW_KEYS)
    assert sorted(h_packed) == sorted(["arch", "cfg", "frames", "hadamard", "bias", "layers", "embedding_shape", "version", "sections"])
    assert s_packed["coded_level_bytes"] == _level_section_bytes(h_packed) == s_packed["section_bytes"]["weight_levels"]
    ref = StreamDecoder(p_packed)
    _assert_plays_back(ref, live)
    assert ref.level_bytes["rans"] == 0 and ref.level_bytes["packed"] == s_packed["coded_level_bytes"]
    entropy = sum(_entropy_bits(_levels(m.weight_quantizer, m.weight.data), m.weight_quantizer.n_levels) for m in mods)
    assert s_packed["entropy_level_bytes"] == int(np.ceil(entropy / 8))
    assert s_packed["gap_to_entropy_bytes"] == s_packed["coded_level_bytes"] - s_packed["entropy_level_bytes"]

    files = [write("rans64.nqv", coding="rans", chunk=64), write("rans.nqv", coding="rans"), write("auto.nqv", coding="auto")]
    for (path, s), chunk in zip(files, (64, DEFAULT_CHUNK, DEFAULT_CHUNK)):
        header, sec = read_container(path)
        assert header["version"] == 1 and open(path, "rb").read(4) == b"NQV1" and s["file_bytes"] == os.path.getsize(path)
        coded = [i for i, lay in enumerate(header["layers"]) if lay.get("levels_coding") == "rans"]
        for i, lay in enumerate(header["layers"]):
            if i in coded:
                assert lay["rans_chunk"] == chunk and f"w{i}.levels" not in sec
                assert sec[f"w{i}.rans_freq"].dtype == np.dtype("<u2") and sec[f"w{i}.rans_states"].dtype == np.dtype("<u4")
                assert sec[f"w{i}.rans_offsets"].dtype == np.dtype("<u4") and sec[f"w{i}.rans_words"].dtype == np.dtype("<u2")
            else:
                assert not any(k in lay for k in NEW_KEYS) and np.array_equal(sec[f"w{i}.levels"], sec_packed[f"w{i}.levels"])
        if s["coding"] == "rans":
            assert coded == list(range(len(mods))) and s["coded_tensors"] == len(mods)
            for i, m in enumerate(mods):             # the restatement's reader recovers the quantiser's levels from the file
                want = _levels(m.weight_quantizer, m.weight.data).cpu().numpy().reshape(-1).tolist()
                assert R.read_coded_levels(path, f"w{i}") == want, i
        else:                                        # never larger than packed, tensor by tensor and hence in all
            assert _level_section_bytes(header) <= _level_section_bytes(h_packed)
            for i in range(len(mods)):
                mine = sum((x["bytes"] + 3) // 4 * 4 for x in header["sections"] if x["name"].startswith(f"w{i}.") and
                           (x["name"].endswith(".levels") or ".rans_" in x["name"]))
                assert mine <= (sec_packed[f"w{i}.levels"].nbytes + 3) // 4 * 4
        assert s["coded_level_bytes"] == _level_section_bytes(header)
        assert s["entropy_level_bytes"] == s_packed["entropy_level_bytes"] and s["total_bytes_nominal"] == s_packed["total_bytes_nominal"]
        assert s["gap_to_entropy_bytes"] == s["coded_level_bytes"] - s["entropy_level_bytes"]
        assert sum(v for k, v in s["section_bytes"].items() if "_rans_" in k or k.endswith("_levels")) == s["coded_level_bytes"]
        print("%s chunk %d: file %d bytes, levels %d (packed %d, entropy %d), %d of %d tensors coded" % (
            s["coding"], chunk, s["file_bytes"], s["coded_level_bytes"], s_packed["coded_level_bytes"],
            s["entropy_level_bytes"], len(coded), len(mods)))
        dec = StreamDecoder(path)
        assert dec.level_bytes["packed"] + dec.level_bytes["rans"] <= s["coded_level_bytes"]    # the summary counts padding
        for a, b_ in zip(dec.weights + dec.biases, ref.weights + ref.biases):
            assert torch.equal(a, b_)
        _assert_plays_back(dec, live)
    with pytest.raises(ValueError):
        write("bad.nqv", coding="huffman")
    with pytest.raises(ValueError):
        write("bad.nqv", coding="rans", chunk=100)
    assert not os.path.exists(str(tmp_path / "bad.nqv"))

    # hard biases, coded: plays back equal to the packed hard stream
    p_hp, _ = write("hard_packed.nqv", bias="hard")
    p_hr, s_hr = write("hard_rans.nqv", bias="hard", coding="rans", chunk=128)
    h_hr, sec_hr = read_container(p_hr)
    assert all(lay["bias_levels_coding"] == "rans" and lay["bias_rans_chunk"] == 128 for lay in h_hr["layers"])
    assert s_hr["coded_tensors"] == 2 * len(mods) and not any(n.endswith(".levels") for n in sec_hr)
    for i, m in enumerate(mods):
        assert R.read_coded_levels(p_hr, f"b{i}") == _levels(m.bias_quantizer, m.bias.data).cpu().numpy().reshape(-1).tolist()
    d_hp, d_hr = StreamDecoder(p_hp), StreamDecoder(p_hr)
    for a, b_ in zip(d_hr.weights + d_hr.biases, d_hp.weights + d_hp.biases):
        assert torch.equal(a, b_)
    for B in (1, 2):
        for j in range(0, 8, B):
            assert torch.equal(d_hr.decode(list(range(j, j + B))), d_hp.decode(list(range(j, j + B))))


def test_player_refuses_a_damaged_coded_stream(ops, hnerv_calibrated, tmp_path):
    """StreamDecoder itself (not only the host function the CPU tests call) raises before anything is uploaded."""
    import json
    import struct
    from neuroquant_amd.bitstream import StreamDecoder, write_stream
    qnn, emb, _ = hnerv_calibrated
    path = str(tmp_path / "r.nqv")
    write_stream(qnn, path, "hnerv", dict(TINY_HNERV), embeddings=emb, coding="rans", chunk=64)
    data = bytearray(open(path, "rb").read())
    (hlen,) = struct.unpack("<I", data[4:8])
    header = json.loads(data[8:8 + hlen])
    start = (8 + hlen + 3) // 4 * 4
    s = next(x for x in header["sections"] if x["name"] == "w3.rans_states")
    data[start + s["offset"]:start + s["offset"] + 4] = struct.pack("<I", 65535)      # a state below the bound
    bad = str(tmp_path / "bad.nqv")
    open(bad, "wb").write(bytes(data))
    with pytest.raises(ValueError):
        StreamDecoder(bad)


def test_nerv_hadamard_rans_stream_plays_back_bit_for_bit(ops, golden, frames, tmp_path):
    """the stored tensor is the padded transform-domain one"""
    from neuroquant_amd.bitstream import StreamDecoder, read_container, write_stream
    from neuroquant_amd.quantization import model_reconstruction
    z, qnn, emb = _quant_model(golden, "traj_nerv_had.npz", "nerv", True)
    model_reconstruction(qnn, cali_data=emb, gt=_Replay(frames, z["order"], 8), arch="nerv", batch_size=2, iters=16,
                         weight=0.01, opt_mode="mse", hadamard=True, b_range=(20, 2), warmup=0.2, p=2.0, lr=0.003)
    qnn.set_quant_state(True)
    path = str(tmp_path / "n.nqv")
    s = write_stream(qnn, path, "nerv", dict(TINY_NERV), frames=8, coding="rans", chunk=256)
    header, sec = read_container(path)
    assert header["hadamard"] is True and all(lay["levels_coding"] == "rans" for lay in header["layers"])
    for i, (m, lay) in enumerate(zip(qnn.quant_modules(), header["layers"])):
        n = m.hadamard_weight.numel()
        assert lay["c_in_stored"] == m.hadamard_weight.shape[1] >= lay["shape"][1]
        assert len(sec[f"w{i}.rans_offsets"]) == -(-n // 256) + 1
    print("nerv+hadamard rans stream: %d bytes, levels %d, entropy %d, nominal %d" % (
        s["file_bytes"], s["coded_level_bytes"], s["entropy_level_bytes"], s["total_bytes_nominal"]))
    dec = StreamDecoder(path)
    for B in (1, 2):
        for j in range(0, 8, B):
            idx = list(range(j, j + B))
            with torch.no_grad():
                live = qnn(qnn.encode(torch.tensor(idx, device=DEV).float() / 8))[0]
            assert torch.equal(dec.decode(idx), live), (B, j)


# ------------------------------------------------------------------------------------------ drivers
def test_drivers_export_rans_and_play_back(tmp_path):
    """calibrate_network --export_stream f --stream_coding rans, then the decode_stream command line in a fresh child process:
    the played PSNR / MS-SSIM strings equal the logged ones; both name the coding."""
    from neuroquant_amd.bitstream import read_container
    from neuroquant_amd.methods import calibrate_network as cn
    root = logging.getLogger()
    saved = (root.level, list(root.handlers))
    stream = tmp_path / "out" / "model.nqv"
    try:
        args = cn.parse_args(["--arch", "hnerv", "--synthetic", "8", "--batch_size", "2", "--channel_wise", "--init", "max",
                              "--iters_w", "24", "--weight", "0.01", "--b_start", "20", "--b_end", "2", "--warmup", "0.2",
                              "--lr", "0.003", "--precision", "6", "5", "4", "5", "5", "6", "6",
                              "--export_stream", str(stream), "--stream_coding", "rans"])
        assert cn.parse_args(["--arch", "hnerv"]).stream_coding == "packed"
        args.outf = str(tmp_path / "run")
        cn.seed_all(903)
        cn.calibrate(args, dict(TINY_HNERV))
        for h in list(root.handlers):
            if h not in saved[1]:
                h.close()
                root.removeHandler(h)
        log = "".join(open(os.path.join(args.outf, f)).read() for f in sorted(os.listdir(args.outf)) if f.endswith(".log"))
    finally:
        root.setLevel(saved[0])
        for h in saved[1]:
            if h not in root.handlers:
                root.addHandler(h)
    line = next(ln for ln in log.splitlines() if "bit stream: " in ln)
    assert "coding rans" in line and re.search(r"gap to entropy -?[0-9]+ bytes", line), line
    header, _ = read_container(str(stream))
    assert all(lay["levels_coding"] == "rans" for lay in header["layers"])
    logged = re.search(r"Weight quantization w/ opt: best_pred_seen_psnr: ([0-9.]+) \| best_pred_seen_ssim: ([0-9.]+)", log)
    assert logged, log
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "neuroquant_amd.methods.decode_stream", "--stream", str(stream), "--synthetic", "8"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    played = re.search(r"float: PSNR ([0-9.]+) \| MS-SSIM ([0-9.]+)", p.stdout)
    assert played and played.group(1) == logged.group(1) and played.group(2) == logged.group(2)
    named = re.search(r"levels: rans ([0-9]+) bytes in ([0-9]+) tensors, packed ([0-9]+) bytes in ([0-9]+) tensors", p.stdout)
    assert named and int(named.group(2)) == len(header["layers"]) and int(named.group(3)) == 0 and int(named.group(1)) > 0

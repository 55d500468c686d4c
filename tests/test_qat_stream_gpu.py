"""QAT baselines to the bit stream: ops.qat_levels / ops.qat_restore (csrc/qat_stream.hip) against the trainer's
own quantiser ops.qat_weight(noise=False) and the existing packer, and a QAT-trained tiny HNeRV written by write_qat_stream and
played back by StreamDecoder.  Every comparison is exact.  "Bit for bit" is taken on the int32 view after `+ 0.0`, which only
turns the quantiser's -0 (a negative weight below the first step) into the +0 that symbol 0 restores to (§30.3)."""
import functools

import numpy as np
import pytest
import torch

from conftest import TINY_HNERV

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 1), (5, 3, 3), (65, 8, 3), (130, 7, 5), (16, 16, 1)]   # (C_out, C_in, k): the table of test_qat_gpu.py
TABLE = [(m, b, f) for m in ("ffnerv", "hinerv") for b in (2, 3, 5, 8) for f in ("packed", "symbols")]


@functools.lru_cache(None)
def tensors():
    """w ~ 0.5 N(0, 1) per shape with a tie for column 1's maximum (its row and the last) and a column of zeros (column 2)"""
    rng = np.random.default_rng(11)
    out = []
    for cout, cin, k in SHAPES:
        w = (0.5 * rng.standard_normal((cout, cin * k * k))).astype(np.float32)
        w[-1, 1] = -np.abs(w[:, 1]).max()
        w[:, 2] = 0
        out.append(torch.from_numpy(w.reshape(cout, cin, k, k)).cuda())
    return out


def same_bits(a, b):
    return a.shape == b.shape and torch.equal((a + 0.0).view(torch.int32), (b + 0.0).view(torch.int32))


def there_and_back(ops, ws, bits, mode, form):
    held = ops.qat_levels(ws, bits, mode, form)
    return ops.qat_restore([s for s, _ in held], [w.shape for w in ws], bits, mode, [sc for _, sc in held], form)


@pytest.mark.parametrize("mode,bits,form", TABLE)
def test_restore_equals_the_quantiser(mode, bits, form):
    from neuroquant_amd import ops
    ws = tensors()
    want = ops.qat_weight(ws, bits, mode, noise=False)
    for i, (w, y, got) in enumerate(zip(ws, want, there_and_back(ops, ws, bits, mode, form))):
        assert same_bits(got, y), SHAPES[i]
        assert same_bits(there_and_back(ops, [w], bits, mode, form)[0], y), SHAPES[i]      # one tensor at a time


@pytest.mark.parametrize("mode,bits", sorted({t[:2] for t in TABLE}))
def test_packed_words_are_the_packers(mode, bits):
    from neuroquant_amd import ops
    ws = tensors()
    packed, symbols = ops.qat_levels(ws, bits, mode, "packed"), ops.qat_levels(ws, bits, mode, "symbols")
    stats = ops.qat_stats(ops.qat_weight_raw(ws, bits, "hinerv")[1], ws)
    for i, ((words, sc), (sym, sc2)) in enumerate(zip(packed, symbols)):
        assert int(sym.max()) <= (2 * (2 ** (bits - 1) - 1) if mode == "ffnerv" else 2 ** bits - 1), SHAPES[i]
        assert torch.equal(words, ops.pack_levels(sym, bits)), SHAPES[i]
        assert (sc is None and sc2 is None) if mode == "ffnerv" else (torch.equal(sc, stats[i][0]) and torch.equal(sc2, sc)), SHAPES[i]


@pytest.mark.parametrize("mode", ["ffnerv", "hinerv"])
def test_tiny_hnerv_round_trip(mode, tmp_path):
    from neuroquant_amd import objective
    from neuroquant_amd.bitstream import StreamDecoder, read_container, write_qat_stream
    from neuroquant_amd.methods import regress
    args = regress.parse_args(["--arch", "hnerv", "--qat", mode, "--qat_bits", "6"])
    torch.manual_seed(1)
    model = regress.build_model(args, TINY_HNERV, "cuda")
    frames = torch.rand(3, 3, 320, 640, generator=torch.Generator().manual_seed(3)).cuda()
    regress.train_step(model, torch.optim.SGD(model.parameters(), lr=1e-2), {"img": frames[:2]}, args, objective.of_params(None))
    model.eval()
    with torch.no_grad():
        emb = model.encode(frames)
        live = [model.decode(emb[i:i + 1])[0] for i in range(3)]
    played = {}
    for coding in ("packed", "rans"):
        path = str(tmp_path / f"{coding}.nqv")
        s = write_qat_stream(model, path, "hnerv", dict(TINY_HNERV), mode, 6, embeddings=emb, coding=coding, chunk=64)
        header = read_container(path)[0]
        assert header["weight_quantiser"] == dict(mode=mode, bits=[6] * 7) and s["coded_tensors"] == (7 if coding == "rans" else 0)
        dec = StreamDecoder(path)
        played[coding] = [dec.decode([i]) for i in range(3)]
        assert all(torch.equal(a, b) for a, b in zip(played[coding], live)), coding
        with pytest.raises(ValueError):
            StreamDecoder(path, arithmetic="levels")
    assert all(torch.equal(a, b) for a, b in zip(played["packed"], played["rans"]))
    assert not torch.equal(live[0], live[1])


def test_write_stream_is_the_file_of_before(golden, tmp_path):
    """a calibrated model's file carries no weight_quantiser field and is, byte for byte, its own header and sections written
    again by the container writer with that field absent"""
    from neuroquant_amd import bitstream
    from test_bitstream_gpu import _quant_model
    _, qnn, emb = _quant_model(golden, "traj_hnerv.npz", "hnerv", False)
    a, b = str(tmp_path / "a.nqv"), str(tmp_path / "b.nqv")
    bitstream.write_stream(qnn, a, "hnerv", dict(TINY_HNERV), embeddings=emb, coding="auto", chunk=64)
    header, sec = bitstream.read_container(a)
    assert bitstream.QAT_FIELD not in header and bitstream.qat_entry(header) is None
    plain = {k: v for k, v in header.items() if k not in (bitstream.QAT_FIELD, "version", "sections")}
    bitstream._write_container(b, plain, [(s["name"], s["dtype"], sec[s["name"]]) for s in header["sections"]])
    assert open(a, "rb").read() == open(b, "rb").read()

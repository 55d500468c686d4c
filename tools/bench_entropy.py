#!/usr/bin/env python3
"""Sizes and open times of the entropy-coded bit stream against the packed one, over the chunk size.

    python tools/bench_entropy.py [--out profiles/entropy.json] [--opens 15] [--frames 16] [--parent FILE]

Two models, the same measurements on each.  "random_init" is the one tools/bench_player.py builds and times: a RANDOMLY
INITIALISED HNeRV-3M wrapped in QuantModel (bits 6 5 4 5 5 6 6, channel-wise, 'max' scales) and calibrated for a few iterations
on synthetic frames; that tool loads no checkpoint.  Weights straight from an initialiser need not have the histogram of
trained ones, so "trained" repeats everything on the committed trained HNeRV-3M decoder of the test suite
(tests/golden/hnerv3m_bunny8real_f16.npz, eight real frames), which is the model whose sizes mean something.

Per chunk = 4096 ... 262144: file bytes for coding packed / rans / auto, coded level bytes against the histogram entropy, the
StreamDecoder open time of each file (host clock around read + validate + upload + decode + synchronise; median, min and max
over --opens opens, the three files taking turns) and decode frames/s at B = 1 (host clock around 4 sweeps over all frames,
median of 5 windows).  --parent FILE times the StreamDecoder of another copy of neuroquant_amd/bitstream.py (the parent
commit's) on the packed file and on the first coded one (coding rans, chunk 4096) in the same run, taking turns with the
current one.  Prints ONE JSON object and writes it to --out.  Needs the GPU.

    python tools/bench_entropy.py --encoder [--out profiles/rans_encode.json] [--repeats 7] [--parent FILE]

times the encoders instead, on the trained model only: `ops.rans_encode` against `bitstream.rans_encode` per
tensor at chunk 4096 / 32768 / 262144, `write_stream` with encoder "gpu" and "host" for coding rans and auto, and the default
packed export (with --parent: against the parent commit's bitstream.py, taking turns)."""
import argparse
import importlib.util
import json
import logging
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_player import BITS, HNERV_3M, build_model, sweep_fps  # noqa: E402

CHUNKS = [4096 << k for k in range(7)]


def stats(v, digits=3):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def time_opens(makers, paths, opens):
    """ms per open, the candidates taking turns; makers: {name: StreamDecoder class}, paths: {name: file}"""
    t = {k: [] for k in makers}
    for k in makers:                                  # warm-up: kernels loaded, allocator primed
        makers[k](paths[k])
    for _ in range(opens):
        for k in makers:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            makers[k](paths[k])                       # ends with a device synchronise
            t[k].append((time.perf_counter() - t0) * 1e3)
    return {k: stats(v) for k, v in t.items()}


def decode_fps(dec, n, windows=5, passes=4):
    def play(j, B):
        dec.decode([j])
    sweep_fps(play, n, 1, 1)
    return stats([sweep_fps(play, n, 1, passes) for _ in range(windows)], 1)


def load_parent(path):
    """another copy of bitstream.py as a module inside the package (its relative imports resolve against this tree)"""
    spec = importlib.util.spec_from_file_location("neuroquant_amd._bitstream_parent", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.StreamDecoder


def build_trained(iters):
    """the committed trained HNeRV-3M decoder (tests/golden/hnerv3m_bunny8real_f16.npz, the eight real Bunny crops), same
    bits and 'max' scales, calibrated for `iters` iterations in the order tools/precision_gate.py replays"""
    import precision_gate as pg
    from neuroquant_amd.quantization import QuantModel, model_reconstruction
    from neuroquant_amd.utils import CacheLoader, FrameCache
    model, emb, _ = pg.load_fixture_checkpoint("hnerv3m_bunny8real_f16.npz", "cuda")
    frames = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "bunny8_640x1280.npz"))["frames"]).to("cuda")
    qnn = QuantModel(model, hadamard=False, weight_quant_params=dict(n_bits=8, channel_wise=True, scale_method="max")).to("cuda")
    qnn.set_bitwidth(BITS)
    qnn.eval()
    qnn.set_quant_state(True)
    with torch.no_grad():
        qnn(emb[:2])
    model_reconstruction(qnn, cali_data=emb, gt=CacheLoader(FrameCache(frames), list(range(8)), 2, seed=903), arch="hnerv",
                         batch_size=2, iters=iters, weight=0.01, opt_mode="mse", hadamard=False, b_range=(20, 2), warmup=0.2,
                         p=2.0, lr=0.003)
    qnn.set_quant_state(True)
    qnn.eval()
    return qnn, emb


def measure(qnn, emb, opens, parent, tmp, tag):
    from neuroquant_amd.bitstream import StreamDecoder, write_stream
    n = emb.shape[0]
    packed = os.path.join(tmp, tag + "_packed.nqv")
    sp = write_stream(qnn, packed, "hnerv", dict(HNERV_3M), embeddings=emb)
    ref = StreamDecoder(packed)
    res = dict(frames=n, levels=int(sum(w.numel() for w in ref.weights)), total_bytes_nominal=sp["total_bytes_nominal"],
               entropy_level_bytes=sp["entropy_level_bytes"], packed_file_bytes=sp["file_bytes"],
               packed_level_bytes=sp["coded_level_bytes"], chunks=[])
    versus = {"parent": load_parent(parent), "current": StreamDecoder} if parent else None
    if versus:
        res["packed_open_ms_parent_vs_current"] = time_opens(versus, dict.fromkeys(versus, packed), opens)
    res["packed_decode_fps_B1"] = decode_fps(ref, n)
    for chunk in CHUNKS:
        paths, row = {"packed": packed}, {"chunk": chunk}
        for coding in ("rans", "auto"):
            paths[coding] = os.path.join(tmp, "%s_%s_%d.nqv" % (tag, coding, chunk))
            t0 = time.perf_counter()
            s = write_stream(qnn, paths[coding], "hnerv", dict(HNERV_3M), embeddings=emb, coding=coding, chunk=chunk)
            row[coding] = {"file_bytes": s["file_bytes"], "coded_level_bytes": s["coded_level_bytes"],
                           "gap_to_entropy_bytes": s["gap_to_entropy_bytes"], "coded_tensors": s["coded_tensors"],
                           "level_bytes_over_packed": round(s["coded_level_bytes"] / sp["coded_level_bytes"], 5),
                           "level_bytes_over_entropy": round(s["coded_level_bytes"] / s["entropy_level_bytes"], 5),
                           "file_bytes_over_packed": round(s["file_bytes"] / sp["file_bytes"], 5),
                           "write_seconds": round(time.perf_counter() - t0, 2)}
        if versus and chunk == CHUNKS[0]:   # the first coded file: every tensor through the rANS upload and decode
            res["rans_open_ms_parent_vs_current"] = time_opens(versus, dict.fromkeys(versus, paths["rans"]), opens)
        row["open_ms"] = time_opens({k: StreamDecoder for k in paths}, paths, opens)
        for coding in ("rans", "auto"):
            dec = StreamDecoder(paths[coding])
            row[coding]["weights_bit_identical_to_packed"] = all(torch.equal(x, y) for x, y in zip(dec.weights, ref.weights))
            row[coding]["decode_fps_B1"] = decode_fps(dec, n)
        res["chunks"].append(row)
    return res


ENCODER_CHUNKS = [4096, 32768, 262144]


def _host_ms(fn, repeats):
    """ms per call of fn, host clock around work that ends synchronised; one untimed call first"""
    fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def write_stream_(qnn, path, cfg, emb, **kw):
    from neuroquant_amd.bitstream import write_stream
    return write_stream(qnn, path, "hnerv", cfg, embeddings=emb, **kw)


def measure_encoders(qnn, emb, repeats, parent, tmp):
    """--encoder: the HIP rANS encoder against the host one on the trained model's level tensors.  Per chunk and
    tensor: ops.rans_encode (levels already on the device; includes its 4-byte read-back) against bitstream.rans_encode
    including the copy of the levels to the host, the two taking turns; write_stream wall time with both encoders for coding
    rans and auto; and the default packed export, against the parent commit's bitstream.py where --parent names one."""
    from neuroquant_amd import bitstream, ops
    from neuroquant_amd.export import _levels
    mods = qnn.quant_modules()
    tensors = [(_levels(m.weight_quantizer, m.hadamard_weight if m.hadamard else m.weight.data).reshape(-1).contiguous(),
                int(m.weight_quantizer.n_bits)) for m in mods]
    res = dict(levels=[int(t.numel()) for t, _ in tensors], bits=[b for _, b in tensors], repeats=repeats, chunks=[])
    cfg = dict(HNERV_3M)
    for chunk in ENCODER_CHUNKS:
        row, tot = dict(chunk=chunk, tensors=[]), {"gpu": [0.0] * repeats, "host": [0.0] * repeats}
        for i, (lv, b) in enumerate(tensors):
            got = [t.cpu().numpy() for t in ops.rans_encode(lv, b, chunk)]
            want = bitstream.rans_encode(lv.cpu().numpy(), b, chunk)
            same = all(np.array_equal(g.view(w.dtype), w) for g, w in zip(got, want))
            t = {"gpu": [], "host": []}
            for _ in range(repeats + 1):                      # the two encoders take turns; the first round is the warm-up
                t["gpu"].append(_host_ms(lambda: ops.rans_encode(lv, b, chunk), 1)[0])
                t["host"].append(_host_ms(lambda: bitstream.rans_encode(lv.cpu().numpy(), b, chunk), 1)[0])
            for k in tot:
                tot[k] = [x + y for x, y in zip(tot[k], t[k][1:])]
            row["tensors"].append(dict(tensor="w%d" % i, levels=int(lv.numel()), n_bits=b, words=int(want[3].size),
                                       identical=bool(same), gpu_ms=stats(t["gpu"][1:]), host_ms=stats(t["host"][1:])))
        row["total_gpu_ms"], row["total_host_ms"] = stats(tot["gpu"]), stats(tot["host"])
        row["write_stream_ms"] = {}
        for coding in ("rans", "auto"):
            t = {"gpu": [], "host": []}
            for _ in range(repeats + 1):
                for enc in t:
                    path = os.path.join(tmp, "enc_%s_%s_%d.nqv" % (coding, enc, chunk))
                    t[enc].append(_host_ms(lambda: write_stream_(qnn, path, cfg, emb, coding=coding, chunk=chunk, encoder=enc), 1)[0])
            same = open(os.path.join(tmp, "enc_%s_gpu_%d.nqv" % (coding, chunk)), "rb").read() == \
                open(os.path.join(tmp, "enc_%s_host_%d.nqv" % (coding, chunk)), "rb").read()
            row["write_stream_ms"][coding] = dict(gpu=stats(t["gpu"][1:]), host=stats(t["host"][1:]), files_identical=bool(same))
        res["chunks"].append(row)
    # the default export launches nothing new
    writers = {"current": bitstream.write_stream}
    if parent:
        spec = importlib.util.spec_from_file_location("neuroquant_amd._bitstream_parent", parent)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        writers["parent"] = mod.write_stream
    t = {k: [] for k in writers}
    for _ in range(3 * repeats + 1):
        for k, w in writers.items():
            path = os.path.join(tmp, "packed_%s.nqv" % k)
            t[k].append(_host_ms(lambda: w(qnn, path, "hnerv", cfg, embeddings=emb), 1)[0])
    res["packed_write_stream_ms"] = {k: stats(v[1:]) for k, v in t.items()}
    return res


def main(argv):
    if "--encoder" in argv:
        ap = argparse.ArgumentParser()
        ap.add_argument("--encoder", action="store_true", help="time the HIP rANS encoder against the host one (DESIGN.md §26)")
        ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rans_encode.json"))
        ap.add_argument("--repeats", type=int, default=7)
        ap.add_argument("--parent", default=None, help="the parent commit's neuroquant_amd/bitstream.py: its packed export is timed too")
        a = ap.parse_args(argv)
        if not torch.cuda.is_available():
            raise SystemExit("bench_entropy needs the GPU (nothing is measured without one)")
        logging.getLogger().setLevel(logging.WARNING)
        with tempfile.TemporaryDirectory() as tmp:
            qnn, emb = build_trained(48)
            res = dict(device=torch.cuda.get_device_name(0), model="HNeRV-3M 640x1280, tests/golden/hnerv3m_bunny8real_f16.npz, 48 "
                       "calibration iterations", timing="host clock, synchronised before and after each call; ms; median / min / max",
                       **measure_encoders(qnn, emb, a.repeats, a.parent, tmp))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
        print(json.dumps(res))
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "entropy.json"))
    ap.add_argument("--opens", type=int, default=15)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--parent", default=None, help="another copy of neuroquant_amd/bitstream.py whose StreamDecoder is timed too")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_entropy needs the GPU (nothing is measured without one)")
    logging.getLogger().setLevel(logging.WARNING)
    from neuroquant_amd import ops
    from neuroquant_amd.bitstream import DEFAULT_CHUNK
    res = {"device": torch.cuda.get_device_name(0), "conv_precision": ops.get_conv_precision(), "opens_per_file": a.opens,
           "default_chunk": DEFAULT_CHUNK, "bits": BITS}
    with tempfile.TemporaryDirectory() as tmp:
        qnn, emb = build_model(a.frames, a.iters)
        res["random_init"] = dict(model="HNeRV-3M 640x1280 as tools/bench_player.py builds it: randomly initialised, %d calibration "
                                  "iterations on %d synthetic frames" % (a.iters, a.frames), **measure(qnn, emb, a.opens, a.parent, tmp, "rnd"))
        del qnn, emb
        qnn, emb = build_trained(48)
        res["trained"] = dict(model="HNeRV-3M 640x1280, the committed trained decoder tests/golden/hnerv3m_bunny8real_f16.npz, "
                              "48 calibration iterations on the eight real Bunny crops", **measure(qnn, emb, a.opens, a.parent, tmp, "trn"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])

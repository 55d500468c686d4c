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
current one.  Prints ONE JSON object and writes it to --out.  Needs the GPU."""
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


def main(argv):
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

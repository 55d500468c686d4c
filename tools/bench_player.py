#!/usr/bin/env python3
"""Times the bit-stream player (neuroquant_amd/bitstream.py) at HNeRV-3M, 640 x 1280, B = 1 and B = 2, against
`qnn.decode` in eval mode on the same live model in the same process, plus the open time of the file and ops.frames_to_u8.

    python tools/bench_player.py [--out profiles/player.json] [--repeats 9] [--frames 16] [--passes 4]

The model is a randomly initialised HNeRV-3M wrapped in QuantModel (bits 6 5 4 5 5 6 6, channel-wise) and calibrated for a
few iterations on synthetic frames, so its quantisers are the AdaRound ones a real export carries; timing does not depend
on the weights' values.  frames/s: host clock around `passes` sweeps over all frames, ended by a device synchronise;
median over `repeats` windows, player and baseline alternating, after a warm-up of both at that batch size.  The baseline
is timed twice: as shipped (decode() synchronises after every call in eval mode) and with that synchronise switched off
(model.sync_decode = False), which is the like-for-like figure the expectation is held against.  frames_to_u8: HIP events
around 200 calls.  Prints ONE JSON object and writes it to --out.  Needs the GPU: there is nothing to measure without one."""
import argparse
import json
import logging
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neuroquant_amd import ops  # noqa: E402

HNERV_3M = dict(crop_h=640, crop_w=1280, diff_enc=False, stage_block=1, enc_strides=[5, 4, 4, 2, 2],
                enc_channel=[64, 64, 64, 64, 16], channel_reduce=1.2, channel_lbound=12, dec_in_channel=92,
                dec_kernels=[1, 3, 5, 5, 5], dec_strides=[5, 4, 4, 2, 2], dec_norm="none", dec_acts="gelu", out_bias="tanh")
BITS = [6, 5, 4, 5, 5, 6, 6]


def build_model(n_frames, iters):
    from neuroquant_amd.models import HNeRV
    from neuroquant_amd.quantization import QuantModel, model_reconstruction
    from neuroquant_amd.utils import CacheLoader, FrameCache, synthetic_frames
    torch.manual_seed(903)
    model = HNeRV(HNERV_3M).to("cuda").eval()
    cache = FrameCache(synthetic_frames(n_frames, 640, 1280, device="cuda"))
    with torch.no_grad():
        emb = torch.cat([model.encode(cache.batch(torch.tensor([i], device="cuda"))) for i in range(n_frames)])
    qnn = QuantModel(model, hadamard=False, weight_quant_params=dict(n_bits=8, channel_wise=True, scale_method="max")).to("cuda")
    qnn.set_bitwidth(BITS)
    qnn.eval()
    qnn.set_quant_state(True)
    with torch.no_grad():
        qnn(emb[:2])
    model_reconstruction(qnn, cali_data=emb, gt=CacheLoader(cache, list(range(n_frames)), 2, seed=903), arch="hnerv",
                         batch_size=2, iters=iters, weight=0.01, opt_mode="mse", hadamard=False, b_range=(20, 2), warmup=0.2,
                         p=2.0, lr=0.003)
    qnn.set_quant_state(True)
    qnn.eval()
    return qnn, emb


def sweep_fps(fn, n, B, passes):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(passes):
        for j in range(0, n, B):
            fn(j, B)
    torch.cuda.synchronize()
    return passes * n / (time.perf_counter() - t0)


def med(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def bench_u8(B, layout, repeats, calls=200):
    x = torch.rand(B, 3, 640, 1280, device="cuda")
    fn = lambda: ops.frames_to_u8(x, layout)
    for _ in range(20):
        fn()
    t = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls):
            fn()
        e.record()
        torch.cuda.synchronize()
        t.append(s.elapsed_time(e) * 1e3 / calls)
    us = statistics.median(t)
    nbytes = x.numel() * 5                       # 4 bytes read + 1 written per element
    return {"B": B, "layout": layout, "us_per_call": round(us, 2), "us_min_max": [round(min(t), 2), round(max(t), 2)],
            "algorithmic_bytes": nbytes, "GB_per_s": round(nbytes / us / 1e3, 1),
            "note": "back-to-back calls on one stream: launch gaps included"}


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "player.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--iters", type=int, default=16)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_player needs the GPU (nothing is measured without one)")
    logging.getLogger().setLevel(logging.WARNING)
    from neuroquant_amd.bitstream import StreamDecoder, write_stream
    qnn, emb = build_model(a.frames, a.iters)
    n = a.frames
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "hnerv3m.nqv")
        summary = write_stream(qnn, path, "hnerv", dict(HNERV_3M), embeddings=emb)
        opens = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec = StreamDecoder(path)            # read + upload + unpack (+ synchronise)
            opens.append((time.perf_counter() - t0) * 1e3)
        dec = StreamDecoder(path)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first = dec.decode([0])                  # builds the operands B = 1 selects, then decodes
        torch.cuda.synchronize()
        first_ms = (time.perf_counter() - t0) * 1e3
    res = {"device": torch.cuda.get_device_name(0), "model": "HNeRV-3M 640x1280, bits 6 5 4 5 5 6 6 channel-wise",
           "conv_precision": ops.get_conv_precision(), "frames": n, "passes_per_window": a.passes, "repeats": a.repeats,
           "file_bytes": summary["file_bytes"], "total_bytes_nominal": summary["total_bytes_nominal"],
           "open_ms": med(opens), "first_decode_ms_including_operand_layouts": round(first_ms, 2), "decode": [],
           "frames_to_u8": [bench_u8(B, lay, a.repeats) for B in (1, 2, 8) for lay in ("chw", "hwc")]}
    with torch.no_grad():
        assert torch.equal(first, qnn(emb[:1])[0])
        for B in (1, 2):
            def play(j, B):
                dec.decode(list(range(j, j + B)))

            def play_u8(j, B):
                dec.decode(list(range(j, j + B)), out="u8", layout="hwc")

            def live(j, B):
                qnn.decode(emb[j:j + B])

            same = all(torch.equal(dec.decode(list(range(j, j + B))), qnn(emb[j:j + B])[0]) for j in range(0, n, B))
            t = {k: [] for k in ("player", "player_u8_hwc", "live_as_shipped", "live_no_sync")}
            for k in range(2 + a.repeats):       # two warm-up rounds, then alternating windows
                row = {}
                row["player"] = sweep_fps(play, n, B, a.passes)
                qnn.model.sync_decode = None
                row["live_as_shipped"] = sweep_fps(live, n, B, a.passes)
                row["player_u8_hwc"] = sweep_fps(play_u8, n, B, a.passes)
                qnn.model.sync_decode = False
                row["live_no_sync"] = sweep_fps(live, n, B, a.passes)
                qnn.model.sync_decode = None
                if k >= 2:
                    for key, v in row.items():
                        t[key].append(v)
            entry = {"B": B, "bit_identical_to_live_decode": bool(same), "fps": {k: med(v) for k, v in t.items()}}
            entry["player_over_live_no_sync"] = round(entry["fps"]["player"]["median"] / entry["fps"]["live_no_sync"]["median"], 3)
            entry["player_over_live_as_shipped"] = round(entry["fps"]["player"]["median"] / entry["fps"]["live_as_shipped"]["median"], 3)
            res["decode"].append(entry)
    res["expectation"] = "player frames/s >= live qnn.decode frames/s (same convolution launches, strictly fewer others)"
    res["expectation_met"] = all(e["player_over_live_no_sync"] >= 1.0 and e["bit_identical_to_live_decode"] for e in res["decode"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])

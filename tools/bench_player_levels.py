#!/usr/bin/env python3
"""Times the bit-stream player's two arithmetics against each other: `exact` (the live model's bf16x3 launches)
and `levels` (integer-level convolutions, two MFMAs per product, on the layers the unsplit tiled kernel has) on the model and
file of tools/bench_player.py -- HNeRV-3M, 640 x 1280, bits 6 5 4 5 5 6 6 channel-wise -- in ONE process that holds both decoders
on the same file.

    python tools/bench_player_levels.py [--out profiles/player_levels.json] [--repeats 9] [--frames 16] [--passes 4]

frames/s: host clock around `passes` sweeps over all frames, ended by a device synchronise; median over `repeats` windows with
min / max kept, the two decoders alternating, after two warm-up rounds at that batch size; B = 1 and B = 2, float output.
Per layer (dec3 .. dec5): HIP events around `calls` back-to-back launches of that layer on its own recorded input, again
alternating, median of `repeats`.  Also: open time of both decoders, `levels_used`, the largest |difference| of the decoded
frames.  Prints ONE JSON object and writes it to --out.  Needs the GPU."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_player import HNERV_3M, build_model, med, sweep_fps  # noqa: E402
from neuroquant_amd import ops  # noqa: E402

BIG = (3, 4, 5)   # dec3, dec4, dec5: 98 % of the forward FLOPs


def layer_us(decs, i, x, repeats, calls):
    """{name: us per launch of layer i on x} -- events around `calls` launches, decoders alternating inside every repeat"""
    t = {k: [] for k in decs}
    for d in decs.values():
        for _ in range(10):
            d._conv(i, x)
    for _ in range(repeats):
        for k, d in decs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(calls):
                d._conv(i, x)
            e.record()
            torch.cuda.synchronize()
            t[k].append(s.elapsed_time(e) * 1e3 / calls)
    return {k: med(v) for k, v in t.items()}


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "player_levels.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--calls", type=int, default=50)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_player_levels needs the GPU (nothing is measured without one)")
    logging.getLogger().setLevel(logging.WARNING)
    from neuroquant_amd.bitstream import StreamDecoder, write_stream
    qnn, emb = build_model(a.frames, a.iters)
    n = a.frames
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "hnerv3m.nqv")
        summary = write_stream(qnn, path, "hnerv", dict(HNERV_3M), embeddings=emb)
        opens = {"exact": [], "levels": []}
        for _ in range(5):
            for arith in opens:                   # read + upload + unpack (levels: + the integer tensors and their operands)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                StreamDecoder(path, arithmetic=arith)
                opens[arith].append((time.perf_counter() - t0) * 1e3)
        decs = {arith: StreamDecoder(path, arithmetic=arith) for arith in ("exact", "levels")}
    res = {"device": torch.cuda.get_device_name(0), "model": "HNeRV-3M 640x1280, bits 6 5 4 5 5 6 6 channel-wise",
           "conv_precision": ops.get_conv_precision(), "frames": n, "passes_per_window": a.passes, "repeats": a.repeats,
           "calls_per_event_pair": a.calls, "file_bytes": summary["file_bytes"],
           "open_ms": {k: med(v) for k, v in opens.items()}, "decode": []}
    with torch.no_grad():
        for B in (1, 2):
            inputs, orig = {}, decs["exact"]._conv

            def spy(i, x):
                inputs[i] = x
                return orig(i, x)

            decs["exact"]._conv = spy
            decs["exact"].decode(list(range(B)))
            del decs["exact"]._conv               # back to the class's method
            same_live = all(torch.equal(decs["exact"].decode(list(range(j, j + B))), qnn(emb[j:j + B])[0]) for j in range(0, n, B))
            diff = max(float((decs["exact"].decode(list(range(j, j + B))) - decs["levels"].decode(list(range(j, j + B)))).abs().max())
                       for j in range(0, n, B))
            t = {k: [] for k in decs}
            for k in range(2 + a.repeats):        # two warm-up rounds, then alternating windows
                row = {name: sweep_fps(lambda j, B, d=d: d.decode(list(range(j, j + B))), n, B, a.passes) for name, d in decs.items()}
                if k >= 2:
                    for name, v in row.items():
                        t[name].append(v)
            fps = {k: med(v) for k, v in t.items()}
            layers = {}
            for i in BIG:
                cout, cin, kk, _ = decs["exact"].weights[i].shape
                us = layer_us(decs, i, inputs[i], a.repeats, a.calls)
                layers[f"dec{i}"] = {"shape": [B, cin, inputs[i].shape[2], inputs[i].shape[3], cout, kk],
                                     "on_levels_path": i in decs["levels"].levels_used[B], "us_per_launch": us,
                                     "levels_over_exact": round(us["levels"]["median"] / us["exact"]["median"], 4)}
            spread = max((f["max"] - f["min"]) / f["median"] for f in fps.values())
            gain = fps["levels"]["median"] / fps["exact"]["median"] - 1.0
            res["decode"].append({"B": B, "levels_used": decs["levels"].levels_used[B], "exact_bit_identical_to_live_model": bool(same_live),
                                  "max_abs_difference_levels_vs_exact": diff, "fps": fps, "levels_over_exact": round(1.0 + gain, 4),
                                  "largest_window_spread": round(spread, 4), "gain_exceeds_spread": bool(gain > spread),
                                  "layers": layers})
    res["expectation"] = "levels frames/s > exact frames/s at B = 1 and B = 2 by more than the windows' spread"
    res["expectation_met"] = all(e["gain_exceeds_spread"] for e in res["decode"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])

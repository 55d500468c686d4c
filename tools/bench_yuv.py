#!/usr/bin/env python3
"""Times the 8-bit YUV 4:2:0 conversions (neuroquant_amd/csrc/yuv.hip) at 640 x 1280, B = 1, 2 and 8, against
ops.frames_to_u8(..., 'chw') on the same tensors in the same process, and the bit-stream player with out='yuv420' against
out='u8' at HNeRV-3M, B = 1 and 2.

    python tools/bench_yuv.py [--out profiles/yuv.json] [--repeats 9] [--calls 200] [--frames 16] [--passes 4]

Kernels: HIP events around `calls` back-to-back calls on one stream (launch gaps included: at these sizes a call moves a few
MB), median over `repeats` windows; the three kernels alternate inside every repeat, after a warm-up of each.  The yardstick
is frames_to_u8 'chw', which reads the same floats and writes twice the bytes.  Player: host clock around `passes` sweeps
over all frames, ended by a device synchronise (tools/bench_player.py's method and model), the two outputs alternating.
Prints ONE JSON object and writes it to --out.  Needs the GPU: there is nothing to measure without one."""
import argparse
import json
import logging
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from neuroquant_amd import ops  # noqa: E402
from bench_player import HNERV_3M, build_model, med, sweep_fps  # noqa: E402

H, W = 640, 1280


def window_us(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / calls


def bench_kernels(B, repeats, calls):
    x = torch.rand(B, 3, H, W, device="cuda")
    yuv = ops.frames_to_yuv420(x)
    px = B * H * W
    fns = {"frames_to_yuv420": (lambda: ops.frames_to_yuv420(x), px * 12 + px * 3 // 2),       # bytes read + written
           "yuv420_to_rgb_u8": (lambda: ops.yuv420_to_rgb_u8(yuv, H, W), px * 3 // 2 + px * 3),
           "frames_to_u8_chw": (lambda: ops.frames_to_u8(x, "chw"), px * 12 + px * 3)}
    for fn, _ in fns.values():
        for _ in range(20):
            fn()
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, (fn, _) in fns.items():
            t[k].append(window_us(fn, calls))
    row = {"B": B, "note": "back-to-back calls on one stream: launch gaps included"}
    for k, (_, nbytes) in fns.items():
        us = statistics.median(t[k])
        row[k] = {"us_per_call": round(us, 2), "us_min_max": [round(min(t[k]), 2), round(max(t[k]), 2)],
                  "algorithmic_bytes": nbytes, "GB_per_s": round(nbytes / us / 1e3, 1)}
    row["frames_to_yuv420_over_frames_to_u8_chw_time"] = round(row["frames_to_yuv420"]["us_per_call"] /
                                                             row["frames_to_u8_chw"]["us_per_call"], 3)
    return row


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--iters", type=int, default=16)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_yuv needs the GPU (nothing is measured without one)")
    logging.getLogger().setLevel(logging.WARNING)
    from neuroquant_amd.bitstream import StreamDecoder, write_stream
    res = {"device": torch.cuda.get_device_name(0), "size": "%dx%d" % (W, H), "calls_per_window": a.calls, "repeats": a.repeats,
           "kernels": [bench_kernels(B, a.repeats, a.calls) for B in (1, 2, 8)], "player": []}
    qnn, emb = build_model(a.frames, a.iters)
    n = a.frames
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "hnerv3m.nqv")
        write_stream(qnn, path, "hnerv", dict(HNERV_3M), embeddings=emb)
        dec = StreamDecoder(path)
    with torch.no_grad():
        for B in (1, 2):
            outs = {"float": lambda j, B: dec.decode(list(range(j, j + B))),
                    "u8": lambda j, B: dec.decode(list(range(j, j + B)), out="u8"),
                    "yuv420": lambda j, B: dec.decode(list(range(j, j + B)), out="yuv420")}
            same = all(torch.equal(dec.decode(list(range(j, j + B)), out="yuv420"),
                                   ops.frames_to_yuv420(dec.decode(list(range(j, j + B))))) for j in range(0, n, B))
            t = {k: [] for k in outs}
            for k in range(2 + a.repeats):       # two warm-up rounds, then alternating windows
                row = {key: sweep_fps(fn, n, B, a.passes) for key, fn in outs.items()}
                if k >= 2:
                    for key, v in row.items():
                        t[key].append(v)
            entry = {"B": B, "yuv420_equals_conversion_of_float": bool(same), "fps": {k: med(v) for k, v in t.items()}}
            entry["yuv420_over_u8"] = round(entry["fps"]["yuv420"]["median"] / entry["fps"]["u8"]["median"], 3)
            res["player"].append(entry)
    res["model"] = "HNeRV-3M 640x1280, bits 6 5 4 5 5 6 6 channel-wise"
    res["yardstick"] = "frames_to_u8 'chw' in the same run: the same floats read, twice the bytes written"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])

#!/usr/bin/env python3
"""Times the bit-stream player's three arithmetics against each other: `exact` (the live model's bf16x3
launches), `levels` (integer weights, two BF16 MFMAs per product) and `half` (integer weights against half-precision activations,
one F16 MFMA per product) on the model and file of tools/bench_player.py -- HNeRV-3M, 640 x 1280, bits 6 5 4 5 5 6 6
channel-wise -- in ONE process that holds all three decoders on the same file.

    python tools/bench_player_half.py [--out profiles/player_half.json] [--repeats 9] [--frames 16] [--passes 4] [--trained_iters 16]

frames/s: host clock around `passes` sweeps over all frames, ended by a device synchronise; median over `repeats` windows with
min / max kept, the three decoders alternating, after two warm-up rounds at that batch size; B = 1 and B = 2, float output.
Per layer (dec3 .. dec5): HIP events around `calls` back-to-back launches of that layer on its own recorded input, again
alternating, median of `repeats`.  `half` counts as faster than another arithmetic where the gap exceeds the largest window
spread of the run.  Also: open times, `levels_used`, the saturation flag, and -- on the committed TRAINED HNeRV-3M decoder
(tests/golden/hnerv3m_bunny8real_f16.npz on the eight real crops) -- the largest |half - exact| over the decoded frames and the
PSNR of all three.  Prints ONE JSON object and writes it to --out.  Needs the GPU."""
import argparse
import json
import logging
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_player import HNERV_3M, build_model, med, sweep_fps  # noqa: E402
from bench_player_levels import BIG, layer_us  # noqa: E402
from neuroquant_amd import ops  # noqa: E402

ARITH = ("exact", "levels", "half")
EXTRAPOLATED = 0.75   # half / levels per launch on dec3-dec5, from a line through the bf16x3 and levels times (3 and 2 MFMAs)


def trained_accuracy(iters, tmp):
    """the three arithmetics on the trained fixture: PSNR per arithmetic, largest |half - exact| and |levels - exact|, B = 1"""
    from bench_entropy import build_trained
    from neuroquant_amd.bitstream import StreamDecoder, write_stream
    qnn, emb = build_trained(iters)
    gt = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "bunny8_640x1280.npz"))["frames"]).to("cuda").float() / 255.0
    path = os.path.join(tmp, "trained.nqv")
    write_stream(qnn, path, "hnerv", dict(HNERV_3M), embeddings=emb)
    n = emb.shape[0]
    out = {}
    with torch.no_grad():
        for arith in ARITH:
            d = StreamDecoder(path, arithmetic=arith)
            out[arith] = (torch.cat([d.decode([j]) for j in range(n)]), d.saturated())
    psnr = {k: float(ops.frame_psnr(v[0], gt).double().mean()) for k, v in out.items()}
    return {"model": "tests/golden/hnerv3m_bunny8real_f16.npz on tests/golden/bunny8_640x1280.npz, bits 6 5 4 5 5 6 6, "
                     f"{iters} calibration iterations", "frames": n, "psnr_db": psnr,
            "half_minus_exact_db": psnr["half"] - psnr["exact"], "levels_minus_exact_db": psnr["levels"] - psnr["exact"],
            "max_abs_half_minus_exact": float((out["half"][0] - out["exact"][0]).abs().max()),
            "max_abs_levels_minus_exact": float((out["levels"][0] - out["exact"][0]).abs().max()),
            "one_8bit_step": 1.0 / 255.0, "saturated": bool(out["half"][1])}


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "player_half.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--trained_iters", type=int, default=16)
    ap.add_argument("--calls", type=int, default=50)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_player_half needs the GPU (nothing is measured without one)")
    logging.getLogger().setLevel(logging.WARNING)
    from neuroquant_amd.bitstream import StreamDecoder, write_stream
    qnn, emb = build_model(a.frames, a.iters)
    n = a.frames
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "hnerv3m.nqv")
        summary = write_stream(qnn, path, "hnerv", dict(HNERV_3M), embeddings=emb)
        opens = {k: [] for k in ARITH}
        for _ in range(5):
            for arith in opens:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                StreamDecoder(path, arithmetic=arith)
                opens[arith].append((time.perf_counter() - t0) * 1e3)
        decs = {arith: StreamDecoder(path, arithmetic=arith) for arith in ARITH}
        trained = trained_accuracy(a.trained_iters, tmp)
    res = {"device": torch.cuda.get_device_name(0), "model": "HNeRV-3M 640x1280, bits 6 5 4 5 5 6 6 channel-wise",
           "conv_precision": ops.get_conv_precision(), "frames": n, "passes_per_window": a.passes, "repeats": a.repeats,
           "calls_per_event_pair": a.calls, "file_bytes": summary["file_bytes"],
           "open_ms": {k: med(v) for k, v in opens.items()}, "trained_fixture": trained, "decode": []}
    with torch.no_grad():
        for B in (1, 2):
            inputs, orig = {}, decs["exact"]._conv

            def spy(i, x):
                inputs[i] = x
                return orig(i, x)

            decs["exact"]._conv = spy
            decs["exact"].decode(list(range(B)))
            del decs["exact"]._conv               # back to the class's method
            frames = {k: torch.cat([d.decode(list(range(j, j + B))) for j in range(0, n, B)]) for k, d in decs.items()}
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
                spread_l = max((u["max"] - u["min"]) / u["median"] for u in us.values())
                h_l, h_e = us["half"]["median"] / us["levels"]["median"], us["half"]["median"] / us["exact"]["median"]
                layers[f"dec{i}"] = {"shape": [B, cin, inputs[i].shape[2], inputs[i].shape[3], cout, kk],
                                     "on_half_path": i in decs["half"].levels_used[B], "us_per_launch": us,
                                     "levels_over_exact": round(us["levels"]["median"] / us["exact"]["median"], 4),
                                     "half_over_exact": round(h_e, 4), "half_over_levels": round(h_l, 4),
                                     "extrapolated_half_over_levels": EXTRAPOLATED, "largest_spread": round(spread_l, 4),
                                     "half_faster_than_levels": bool(1.0 - h_l > spread_l)}
            spread = max((f["max"] - f["min"]) / f["median"] for f in fps.values())
            over_l, over_e = fps["half"]["median"] / fps["levels"]["median"], fps["half"]["median"] / fps["exact"]["median"]
            res["decode"].append({"B": B, "levels_used": {k: d.levels_used[B] for k, d in decs.items()},
                                  "max_abs_half_minus_exact": float((frames["half"] - frames["exact"]).abs().max()),
                                  "max_abs_levels_minus_exact": float((frames["levels"] - frames["exact"]).abs().max()),
                                  "fps": fps, "half_over_levels": round(over_l, 4), "half_over_exact": round(over_e, 4),
                                  "levels_over_exact": round(fps["levels"]["median"] / fps["exact"]["median"], 4),
                                  "largest_window_spread": round(spread, 4),
                                  "half_faster_than_levels": bool(over_l - 1.0 > spread),
                                  "half_faster_than_exact": bool(over_e - 1.0 > spread), "layers": layers})
    res["saturated"] = bool(decs["half"].saturated())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])

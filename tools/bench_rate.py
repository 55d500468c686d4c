#!/usr/bin/env python3
"""Measures the rate term of the calibration (nq_level_rate, neuroquant_amd/csrc/rate.hip) on the GPU:

  default_path  with --parent_tree DIR (a built checkout of the parent commit): bench.py's headline it/s of this tree against
                that one, alternating child processes, and the spread of the repeated parent runs it has to sit inside
  kernels       ops.level_rate_raw over the seven weight tensors of HNeRV-3M at bits 6 5 4 5 5 6 6 (one call = four launches),
                with and without the gradient; with --trace the median duration of each of the four launches from a
                `rocprofv3 --kernel-trace` run of a fresh child process
  iteration     it/s of captured calibration iterations of the HNeRV-3M headline shape at B = 2 with the term off (the fused
                parameter side), off with NQ_FUSED_ADAM=0 (the unfused side the term rides on) and on, alternating
  effect        2000-iteration calibrations of the trained HNeRV-3M fixture at bits 6 5 4 5 5 6 6 for lambda = 0 and several
                positive values: bytes of the `rans` file, coded_level_bytes, entropy_level_bytes, R_hard / 8, PSNR, MS-SSIM

    python tools/bench_rate.py [--out profiles/rate.json] [--parent_tree DIR] [--trace] [--lambdas 0.1 1 10 100]
                               [--skip kernels,iteration,effect]

Kernels: HIP events around `calls` back-to-back calls on one stream (launch gaps and the wrapper's allocations included), median
over `repeats` windows.  Iterations: host clock between two device synchronisations.  Recorded, not asserted; ONE run per
lambda.  Sections measured by an earlier call are kept.  Prints ONE JSON object and writes it to --out.  Needs the GPU."""
import argparse
import collections
import csv
import glob
import json
import logging
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench import HNERV_3M  # noqa: E402
from bench_msssim_loss import calibrate  # noqa: E402
from bench_ssim_calib import headline, metrics, spread  # noqa: E402
from bench_yuv_loss import BITS, fixture, quantised, window_us  # noqa: E402
from neuroquant_amd import ops  # noqa: E402

TRACE_CALLS = 60


def weight_items(qnn):
    """[(x, alpha, delta, zp, n_levels)] of the decoder's weight quantisers, alpha as AdaRound initialises it"""
    items = []
    for m in qnn.quant_modules():
        wq = m.weight_quantizer
        d, z, a = ops.adaround_init(m.org_weight.data, wq.delta.data, wq.zero_point)
        items.append((m.org_weight.data, a, d, z, wq.n_levels))
    return items


def bench_kernels(items, repeats, calls):
    das = [torch.zeros_like(it[0]) for it in items]
    fns = {"level_rate": lambda: ops.level_rate_raw(items, 1e-7, dalphas=das),
           "level_rate_no_gradient": lambda: ops.level_rate_raw(items, 1e-7)}
    for fn in fns.values():
        for _ in range(20):
            fn()
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t[k].append(window_us(fn, calls))
    row = {"tensors": [[list(it[0].shape), it[4]] for it in items], "elements": sum(it[0].numel() for it in items),
           "launches_per_call": ops.LEVEL_RATE_LAUNCHES,
           "note": "back-to-back calls of the ops wrapper on one stream: launch gaps and allocations included"}
    for k in fns:
        row[k] = {"us_per_call": round(statistics.median(t[k]), 2), "us_min_max": [round(min(t[k]), 2), round(max(t[k]), 2)]}
    row["us_per_launch"] = round(row["level_rate"]["us_per_call"] / ops.LEVEL_RATE_LAUNCHES, 2)
    return row


def trace_child():
    model, emb, _ = fixture()
    items = weight_items(quantised(model, emb))
    das = [torch.zeros_like(it[0]) for it in items]
    for _ in range(TRACE_CALLS):
        ops.level_rate_raw(items, 1e-7, dalphas=das)
    torch.cuda.synchronize()


def launch_trace():
    """this script as a fresh child under rocprofv3 --kernel-trace: the median duration of each of the four launches"""
    with tempfile.TemporaryDirectory() as d:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable,
                        os.path.abspath(__file__), "--trace_child"], check=True, capture_output=True, text=True, timeout=300)
        with open(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]) as fh:
            rows = list(csv.DictReader(fh))
    by = collections.defaultdict(list)
    for r in rows:
        m = re.search(r"rate_(hist|finish|pass|sum)_kernel", r["Kernel_Name"])
        if m:
            by[(m.group(0), int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]))].append(
                (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = [{"kernel": k[0], "workgroups": k[1], "launches": len(v), "median_us": round(statistics.median(v[len(v) // 3:]), 2)}
           for k, v in by.items()]
    return {"what": "rocprofv3 --kernel-trace of %d nq_level_rate calls with gradient over the seven HNeRV-3M weight tensors, in a "
                    "process of its own: median duration per launch over the last two thirds of the calls, us" % TRACE_CALLS,
            "launches": out, "sum_of_medians_us": round(sum(r["median_us"] for r in out), 2)}


def iteration_rate(model, emb, frames, steps, objective, first=200):
    """it/s over iterations first .. steps of one calibration planned for steps + 100 and cut at `steps` (all of phase 2)"""
    assert 0.05 * (steps + 100) / 100 < 1 and first < steps
    marks = {}

    def hook(done):
        if done in (first, steps):
            torch.cuda.synchronize()
            marks[done] = time.perf_counter()

    before = ops.level_rate_launches
    calibrate(quantised(model, emb), emb, frames, steps + 100, objective, epoch_batches=100, hook=hook, max_steps=steps)
    assert (ops.level_rate_launches > before) == ("rate" in objective)
    return (steps - first) / (marks[steps] - marks[first])


def effect_row(model, emb, frames, iters, lam, pixels):
    from neuroquant_amd.bitstream import write_stream
    from neuroquant_amd.methods.calibrate_network import hard_level_rate
    objective = dict(rate=dict(weight=lam, pixels=pixels)) if lam > 0 else {}
    qnn = calibrate(quantised(model, emb), emb, frames, iters, objective)
    row = metrics(qnn, emb, frames)
    with tempfile.TemporaryDirectory() as d:
        s = write_stream(qnn, os.path.join(d, "model.nqv"), "hnerv", dict(HNERV_3M), frames=int(frames.shape[0]), embeddings=emb,
                         coding="rans")
    row.update(file_bytes=s["file_bytes"], coded_level_bytes=s["coded_level_bytes"], entropy_level_bytes=s["entropy_level_bytes"],
               r_hard_bytes=round(hard_level_rate(qnn, False) / 8, 1))
    return row


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--rate_repeats", type=int, default=3)
    ap.add_argument("--lambdas", type=float, nargs="+", default=[0.1, 1.0, 10.0, 100.0])
    ap.add_argument("--parent_tree", default=None, help="a built checkout of the parent commit: bench.py there against bench.py here")
    ap.add_argument("--headline_steps", type=int, default=600)
    ap.add_argument("--trace", action="store_true", help="also trace the four launches with rocprofv3 (a child process)")
    ap.add_argument("--trace_child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--skip", default="", help="comma-separated: kernels, iteration, effect")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_rate needs the GPU (nothing is measured without one)")
    if a.trace_child:
        return trace_child()
    logging.getLogger().setLevel(logging.WARNING)
    skip = set(filter(None, a.skip.split(",")))
    res = {"device": torch.cuda.get_device_name(0), "calls_per_window": a.calls, "repeats": a.repeats}
    if os.path.exists(a.out):                    # sections measured by an earlier call are kept
        with open(a.out) as fh:
            res = dict(json.load(fh), **res)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")

    if a.parent_tree:                            # before this process opens the GPU for long: child processes, alternating
        runs = {"this_tree": [], "parent": []}
        for _ in range(a.rate_repeats):
            runs["this_tree"].append(headline(ROOT, a.headline_steps, 100))
            runs["parent"].append(headline(a.parent_tree, a.headline_steps, 100))
        res["default_path"] = {"what": "bench.py --gpus 1 --steps %d --warmup 100 (headline `value`), fresh processes, alternating"
                                       % a.headline_steps,
                               "it_per_s": {k: spread(v) for k, v in runs.items()}, "runs": runs,
                               "parent_run_to_run_spread": round((max(runs["parent"]) - min(runs["parent"])) / statistics.median(runs["parent"]), 4),
                               "this_tree_over_parent": round(statistics.median(runs["this_tree"]) / statistics.median(runs["parent"]), 4)}
        save()
    if a.trace:                                  # a child process too, and before this one opens the GPU
        res["launch_trace"] = launch_trace()
        save()
    model, emb, frames = fixture()
    pixels = int(frames.shape[0] * frames.shape[2] * frames.shape[3])
    if "kernels" not in skip:
        res["kernels"] = bench_kernels(weight_items(quantised(model, emb)), a.repeats, a.calls)
        save()
    if "iteration" not in skip:
        rates = {"off": [], "off_unfused": [], "on": []}
        for _ in range(a.rate_repeats):          # alternating
            for name in rates:
                os.environ["NQ_FUSED_ADAM"] = "0" if name == "off_unfused" else "1"
                rates[name].append(iteration_rate(model, emb, frames, a.steps, dict(rate=dict(weight=1.0, pixels=pixels)) if name == "on" else {}))
        os.environ.pop("NQ_FUSED_ADAM", None)
        med = {k: statistics.median(v) for k, v in rates.items()}
        res["iteration"] = {"model": "HNeRV-3M 640x1280 (trained fixture), B = 2, bits 6 5 4 5 5 6 6, captured iterations",
                            "iterations_timed": a.steps - 200, "it_per_s": {k: spread(v) for k, v in rates.items()},
                            "on_over_off": round(med["on"] / med["off"], 4), "on_over_off_unfused": round(med["on"] / med["off_unfused"], 4),
                            "note": "off: d(alpha) + regulariser + Adam in one launch; off_unfused (NQ_FUSED_ADAM=0): the two launches "
                                    "the term rides on; on: those two and the four launches of nq_level_rate between them"}
        save()
    if "effect" not in skip:
        rows = res.get("effect", {}).get("rows", {})
        for lam in [0.0] + [v for v in a.lambdas if v > 0]:
            rows["lambda_%g" % lam] = effect_row(model, emb, frames, a.iters, lam, pixels)
            res["effect"] = {"model": "tests/golden/hnerv3m_bunny8real_f16.npz on tests/golden/bunny8_640x1280.npz, bits %s, channel-wise "
                                      "'max' scales, %d iterations, B = 2, weight 0.01, lr 0.003, warmup 0.2, l2 objective; P = %d pixels"
                                      % (" ".join(map(str, BITS)), a.iters, pixels),
                             "rows": rows, "note": "file written with coding 'rans' and fp32 embeddings; PSNR / MS-SSIM: means over the "
                                                   "eight frames; ONE run per lambda"}
            save()
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])

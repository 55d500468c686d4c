#!/usr/bin/env python3
"""Measures the MSE + MS-SSIM objective (nq_msssim_loss, neuroquant_amd/csrc/msssim_loss.hip) on the GPU:

  kernels    nq_msssim_loss with gradient (11 launches) and forward only (6) beside nq_ssim_loss, nq_l2_loss and the forward-only
             nq_ms_ssim on the same tensors in the same process, at (2, 3, 640, 1280) and (2, 3, 960, 1920)
  iteration  it/s of captured calibration iterations of the HNeRV-3M headline shape at B = 2 with `l2`, `Fusion5` and `msssim`,
             alternating; with --parent_tree DIR (a built checkout of the parent commit) also bench.py's headline it/s of this
             tree against that one, alternating child processes: the default path did not move
  trainer    steps/s of the trainer's step on HNeRV-3M (640 x 1280), B = 2, with `l2` against `msssim`, alternating
  trace      with --trace: the median duration of each of the eleven launches at (2, 3, 640, 1280), from a `rocprofv3
             --kernel-trace` run of a fresh child process (60 calls, the last 40 counted): `launch_trace`
  effect     2000-iteration calibrations at bits 6 5 4 5 5 6 6 with `l2`, `Fusion5`, `ssim`, `msssim` (0, 1) and (0.7, 0.3) on the
             trained HNeRV-3M fixture and its eight real frames: PSNR, MS-SSIM and single-scale SSIM, means over the frames

    python tools/bench_msssim_loss.py [--out profiles/msssim_loss.json] [--repeats 9] [--calls 200] [--iters 2000] [--steps 1000]
                                      [--parent_tree DIR] [--trace] [--skip kernels,iteration,trainer,effect]

Kernels: HIP events around `calls` back-to-back calls on one stream (launch gaps and the wrappers' allocations included, the
same for every candidate), median over `repeats` windows, candidates alternating inside every repeat after a warm-up of each.
Iterations and steps: host clock between two device synchronisations.  Recorded, not asserted.  Sections measured by an earlier
call are kept.  Prints ONE JSON object and writes it to --out.  Needs the GPU: there is nothing to measure without one."""
import argparse
import json
import logging
import os
import collections
import csv
import glob
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
from bench_ssim_calib import headline, metrics, spread  # noqa: E402
from bench_ssim_loss import train  # noqa: E402
from bench_yuv_loss import BITS, fixture, quantised, window_us  # noqa: E402
from neuroquant_amd import ops  # noqa: E402

OBJECTIVES = {"l2": {}, "Fusion5": dict(ssim=dict(w_mse=0.7, w_ssim=0.3)), "ssim": dict(ssim=dict(w_mse=0.0, w_ssim=1.0)),
              "msssim": dict(msssim=dict(w_mse=0.0, w_ms=1.0)), "msssim_0.7_0.3": dict(msssim=dict(w_mse=0.7, w_ms=0.3))}


def bench_kernels(frames_u8, size, repeats, calls):
    g = torch.Generator(device="cuda").manual_seed(size[0])
    tgt = ops.gather_frames_u8(frames_u8, torch.tensor([5, 2], device="cuda"))
    if tuple(tgt.shape[2:]) != size:
        tgt = torch.nn.functional.interpolate(tgt, size=size, mode="bilinear", align_corners=False).clamp_(0, 1).contiguous()
    pred = (tgt + 0.05 * torch.randn(tgt.shape, device="cuda", generator=g)).clamp_(0.01, 0.99)
    fns = {"msssim_loss": lambda: ops.ms_ssim_loss_raw(pred, tgt, 0.7, 0.3),
           "msssim_loss_forward_only": lambda: ops.ms_ssim_loss_raw(pred, tgt, 0.7, 0.3, want_grad=False),
           "ms_ssim_metric": lambda: ops.ms_ssim(pred, tgt),
           "ssim_loss": lambda: ops.ssim_loss_raw(pred, tgt, 0.7, 0.3),
           "ssim_loss_forward_only": lambda: ops.ssim_loss_raw(pred, tgt, 0.7, 0.3, want_grad=False),
           "l2_loss": lambda: ops.l2_loss_and_grad(pred, tgt)}
    for fn in fns.values():
        for _ in range(20):
            fn()
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t[k].append(window_us(fn, calls))
    row = {"shape": list(pred.shape), "inputs": "real Bunny crops (bilinearly resized where the shape differs) and their noisy (sigma "
                                                "0.05) versions, weights (0.7, 0.3)",
           "note": "back-to-back calls of the ops wrapper on one stream: launch gaps and allocations included",
           "launches": {"msssim_loss": ops.MSSSIM_LOSS_LAUNCHES, "msssim_loss_forward_only": 6, "ssim_loss": 3}}
    for k in fns:
        row[k] = {"us_per_call": round(statistics.median(t[k]), 2), "us_min_max": [round(min(t[k]), 2), round(max(t[k]), 2)]}
    us = lambda k: row[k]["us_per_call"]
    row["msssim_loss_us_per_launch"] = round(us("msssim_loss") / ops.MSSSIM_LOSS_LAUNCHES, 2)
    row["msssim_loss_over_ssim_loss_time"] = round(us("msssim_loss") / us("ssim_loss"), 2)
    row["msssim_loss_over_l2_loss_time"] = round(us("msssim_loss") / us("l2_loss"), 2)
    return row


TRACE_CALLS = 60


def trace_child():
    """what the traced child process runs: TRACE_CALLS nq_msssim_loss calls with gradient on the inputs of bench_kernels"""
    import numpy as np
    frames = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "bunny8_640x1280.npz"))["frames"]).to("cuda")
    tgt = ops.gather_frames_u8(frames, torch.tensor([5, 2], device="cuda"))
    g = torch.Generator(device="cuda").manual_seed(640)
    pred = (tgt + 0.05 * torch.randn(tgt.shape, device="cuda", generator=g)).clamp_(0.01, 0.99)
    for _ in range(TRACE_CALLS):
        ops.ms_ssim_loss_raw(pred, tgt, 0.7, 0.3)
    torch.cuda.synchronize()


def launch_trace():
    """-> the `launch_trace` section: this script as a fresh child under rocprofv3 --kernel-trace, its CSV grouped by (kernel,
    grid): one row per launch of a call, the median over the last two thirds of the calls"""
    with tempfile.TemporaryDirectory() as d:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable,
                        os.path.abspath(__file__), "--trace_child"], check=True, capture_output=True, text=True, timeout=300)
        with open(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]) as fh:
            rows = list(csv.DictReader(fh))
    by = collections.defaultdict(list)
    for r in rows:
        m = re.search(r"msl_\w+(<[^>]*>)?", r["Kernel_Name"])
        if m:
            key = (m.group(0), int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]), int(r["Grid_Size_Y"]))
            by[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = [{"kernel": k[0], "workgroups_x": k[1], "planes": k[2], "launches": len(v),
            "median_us": round(statistics.median(v[len(v) // 3:]), 2)} for k, v in by.items()]
    out.sort(key=lambda r: (r["kernel"], -r["workgroups_x"]))
    return {"what": "rocprofv3 --kernel-trace of %d nq_msssim_loss calls with gradient at (2, 3, 640, 1280), weights (0.7, 0.3), in a "
                    "process of its own: median duration per launch over the last two thirds of the calls, us" % TRACE_CALLS,
            "launches": out, "sum_of_medians_us": round(sum(r["median_us"] for r in out), 2)}


def calibrate(qnn, emb, frames, iters, objective, epoch_batches=None, hook=None, max_steps=None):
    from neuroquant_amd.quantization import model_reconstruction
    from neuroquant_amd.utils import CacheLoader, FrameCache
    loader = CacheLoader(FrameCache(frames), list(range(frames.shape[0])), 2, seed=903, epoch_batches=epoch_batches)
    model_reconstruction(qnn, cali_data=emb, gt=loader, arch="hnerv", batch_size=2, iters=iters, weight=0.01, opt_mode="mse",
                         hadamard=False, b_range=(20, 2), warmup=0.2, p=2.0, lr=0.003, step_hook=hook, max_steps=max_steps,
                         **objective)
    qnn.set_quant_state(True)
    qnn.eval()
    return qnn


def iteration_rate(model, emb, frames, steps, objective, first=200):
    """it/s over iterations first .. steps of one calibration planned for steps + 100 and cut at `steps` (all of phase 2)"""
    assert 0.05 * (steps + 100) / 100 < 1 and first < steps
    marks = {}

    def hook(done):
        if done in (first, steps):
            torch.cuda.synchronize()
            marks[done] = time.perf_counter()

    before = ops.msssim_loss_head_launches
    calibrate(quantised(model, emb), emb, frames, steps + 100, objective, epoch_batches=100, hook=hook, max_steps=steps)
    assert (ops.msssim_loss_head_launches > before) == ("msssim" in objective)
    return (steps - first) / (marks[steps] - marks[first])


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msssim_loss.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--rate_repeats", type=int, default=3)
    ap.add_argument("--trainer_steps", type=int, default=150)
    ap.add_argument("--parent_tree", default=None, help="a built checkout of the parent commit: bench.py there against bench.py here")
    ap.add_argument("--headline_steps", type=int, default=600)
    ap.add_argument("--trace", action="store_true", help="also trace the eleven launches with rocprofv3 (a child process)")
    ap.add_argument("--trace_child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--skip", default="", help="comma-separated: kernels, iteration, trainer, effect")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_msssim_loss needs the GPU (nothing is measured without one)")
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
        res["default_path"] = {"what": "bench.py --gpus 1 --steps %d --warmup 100 (headline `value`, l2), fresh processes, alternating"
                                       % a.headline_steps,
                               "it_per_s": {k: spread(v) for k, v in runs.items()},
                               "this_tree_over_parent": round(statistics.median(runs["this_tree"]) / statistics.median(runs["parent"]), 4)}
        save()
    if a.trace:                                  # a child process too, and before this one opens the GPU
        res["launch_trace"] = launch_trace()
        save()
    model, emb, frames = fixture()
    if "kernels" not in skip:
        res["kernels"] = [bench_kernels(frames, size, a.repeats, a.calls) for size in ((640, 1280), (960, 1920))]
        save()
    if "iteration" not in skip:
        rates = {"l2": [], "Fusion5": [], "msssim": []}
        for _ in range(a.rate_repeats):          # alternating
            for name in rates:
                rates[name].append(iteration_rate(model, emb, frames, a.steps, OBJECTIVES[name]))
        med = {k: statistics.median(v) for k, v in rates.items()}
        res["iteration"] = {"model": "HNeRV-3M 640x1280 (trained fixture), B = 2, bits 6 5 4 5 5 6 6, captured iterations",
                            "iterations_timed": a.steps - 200, "it_per_s": {k: spread(v) for k, v in rates.items()},
                            "msssim_over_l2": round(med["msssim"] / med["l2"], 4),
                            "msssim_over_Fusion5": round(med["msssim"] / med["Fusion5"], 4),
                            "note": "l2 computes its loss behind the head convolution (nq_head_forward_loss); Fusion5 runs the head "
                                    "convolution and nq_ssim_loss_head (three launches); msssim runs the head convolution, the frame "
                                    "gather, nq_msssim_loss (eleven launches), nq_tanh_out_backward and nq_channel_sum"}
        save()
    if "trainer" not in skip:
        rates = {"l2": [], "msssim": []}
        for _ in range(a.rate_repeats):
            for name in rates:
                rates[name].append(train(HNERV_3M, frames, name, a.trainer_steps, first=20)[1])
        res["trainer"] = {"note": "HNeRV-3M 640x1280: model + step_loss + backward + Adam at B = 2, steps 20 .. %d of a run, %d runs "
                                  "per loss, alternating" % (a.trainer_steps, a.rate_repeats),
                          "steps_per_s": {k: spread(v) for k, v in rates.items()},
                          "msssim_over_l2": round(statistics.median(rates["msssim"]) / statistics.median(rates["l2"]), 4)}
        save()
    if "effect" not in skip:
        effect = res.get("effect", {}).get("metrics", {})
        effect.update({"full_precision": metrics(model, emb, frames),
                       "quantised_before_calibration": metrics(quantised(model, emb), emb, frames)})
        for name, objective in OBJECTIVES.items():
            effect["calibrated_" + name] = metrics(calibrate(quantised(model, emb), emb, frames, a.iters, objective), emb, frames)
            res["effect"] = {"model": "tests/golden/hnerv3m_bunny8real_f16.npz on tests/golden/bunny8_640x1280.npz, bits %s, "
                                      "channel-wise 'max' scales, %d iterations, B = 2, weight 0.01, lr 0.003, warmup 0.2"
                                      % (" ".join(map(str, BITS)), a.iters),
                             "metrics": effect, "note": "means over the eight frames; ONE run per objective"}
            save()
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])

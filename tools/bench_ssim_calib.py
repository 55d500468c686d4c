#!/usr/bin/env python3
"""Measures the calibration's MSE + SSIM objective (nq_ssim_loss_head, neuroquant_amd/csrc/ssim_loss.hip) on the GPU:

  kernels    nq_ssim_loss_head in head mode with a uint8-cache target beside nq_ssim_loss (float target, image gradient), the
             unfused chain it replaces (frame gather + nq_ssim_loss + nq_tanh_out_backward + nq_channel_sum) and
             nq_l2_loss_tanh_head, on the same tensors in the same process, at (B, 3, 640, 1280), B = 2, 1
  iteration  it/s of captured calibration iterations of the HNeRV-3M headline shape at B = 2 with `l2` against `Fusion5`,
             alternating; with --parent_tree DIR (a built checkout of the parent commit) also bench.py's headline it/s of this
             tree against that one, alternating child processes: the default path did not move
  effect     2000-iteration calibrations at bits 6 5 4 5 5 6 6 with `l2`, `Fusion5` and `ssim` on the trained HNeRV-3M fixture
             and its eight real frames: PSNR, MS-SSIM and single-scale SSIM, means over the frames

    python tools/bench_ssim_calib.py [--out profiles/ssim_calib.json] [--repeats 9] [--calls 200] [--iters 2000] [--steps 1200]
                                     [--parent_tree DIR] [--skip kernels,iteration,effect]

Kernels: HIP events around `calls` back-to-back calls on one stream (launch gaps and the wrappers' allocations included, the
same for every candidate), median over `repeats` windows, candidates alternating inside every repeat after a warm-up of each.
Iterations: host clock between two device synchronisations, 200 iterations into the run and at its end.  Recorded, not asserted.
Prints ONE JSON object and writes it to --out.  Needs the GPU: there is nothing to measure without one."""
import argparse
import ctypes
import json
import logging
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_yuv_loss import BITS, fixture, quantised, window_us  # noqa: E402
from neuroquant_amd import _lib as L  # noqa: E402
from neuroquant_amd import ops  # noqa: E402
from neuroquant_amd.methods.calibrate_network import SSIM_LOSSES  # noqa: E402

OBJECTIVES = {"l2": None, **{k: dict(w_mse=v[0], w_ssim=v[1]) for k, v in SSIM_LOSSES.items() if k in ("Fusion5", "ssim")}}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def unfused_chain(pred, cache, idx, w):
    """what the head-mode call replaces: a float copy of the target, the image gradient, the tanh backward, the channel sums"""
    lib = L.lib()
    tgt = ops.gather_frames_u8(cache, idx)
    loss3, grad = ops.ssim_loss_raw(pred, tgt, *w)
    dconv, db, ws = torch.empty_like(grad), torch.empty(pred.shape[1], device="cuda"), torch.empty(512 * pred.shape[1], device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    L.check(lib.nq_tanh_out_backward(_ptr(grad), _ptr(pred), _ptr(dconv), grad.numel(), st), "tanh_out_backward")
    L.check(lib.nq_channel_sum(_ptr(dconv), _ptr(db), _ptr(ws), pred.shape[0], pred.shape[1], pred.shape[2] * pred.shape[3], st),
            "channel_sum")
    return loss3, dconv, db


def bench_kernels(frames_u8, B, repeats, calls):
    g = torch.Generator(device="cuda").manual_seed(B)
    idx = torch.tensor([5, 2], device="cuda")[:B]
    tgt = ops.gather_frames_u8(frames_u8, idx)
    pred = (tgt + 0.05 * torch.randn(tgt.shape, device="cuda", generator=g)).clamp_(0.01, 0.99)
    w = SSIM_LOSSES["Fusion5"]
    fns = {"ssim_loss_head_u8": lambda: ops.ssim_loss_head_raw(pred, cache_u8=frames_u8, idx=idx, w_mse=w[0], w_ssim=w[1], head=True),
           "ssim_loss_head_f32": lambda: ops.ssim_loss_head_raw(pred, tgt=tgt, w_mse=w[0], w_ssim=w[1], head=True),
           "ssim_loss_image_u8": lambda: ops.ssim_loss_head_raw(pred, cache_u8=frames_u8, idx=idx, w_mse=w[0], w_ssim=w[1], head=False),
           "ssim_loss": lambda: ops.ssim_loss_raw(pred, tgt, *w),
           "unfused_chain_u8": lambda: unfused_chain(pred, frames_u8, idx, w),
           "l2_loss_tanh_head_u8": lambda: ops.l2_loss_tanh_head_raw(pred, cache_u8=frames_u8, idx=idx)}
    for fn in fns.values():
        assert fn() is not None
        for _ in range(20):
            fn()
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t[k].append(window_us(fn, calls))
    row = {"shape": list(pred.shape), "inputs": "real Bunny crops (frames 5, 2 of the cache) and their noisy (sigma 0.05) versions, Fusion5",
           "note": "back-to-back calls of the ops wrapper on one stream: launch gaps and allocations included"}
    for k in fns:
        row[k] = {"us_per_call": round(statistics.median(t[k]), 2), "us_min_max": [round(min(t[k]), 2), round(max(t[k]), 2)]}
    us = lambda k: row[k]["us_per_call"]
    row["head_u8_over_ssim_loss_time"] = round(us("ssim_loss_head_u8") / us("ssim_loss"), 3)
    row["head_u8_over_unfused_chain_time"] = round(us("ssim_loss_head_u8") / us("unfused_chain_u8"), 3)
    row["head_u8_over_l2_head_time"] = round(us("ssim_loss_head_u8") / us("l2_loss_tanh_head_u8"), 2)
    return row


def calibrate(qnn, emb, frames, iters, ssim, epoch_batches=None, hook=None, max_steps=None):
    from neuroquant_amd.quantization import model_reconstruction
    from neuroquant_amd.utils import CacheLoader, FrameCache
    loader = CacheLoader(FrameCache(frames), list(range(frames.shape[0])), 2, seed=903, epoch_batches=epoch_batches)
    model_reconstruction(qnn, cali_data=emb, gt=loader, arch="hnerv", batch_size=2, iters=iters, weight=0.01, opt_mode="mse",
                         hadamard=False, b_range=(20, 2), warmup=0.2, p=2.0, lr=0.003, step_hook=hook, max_steps=max_steps, ssim=ssim)
    qnn.set_quant_state(True)
    qnn.eval()
    return qnn


def iteration_rate(model, emb, frames, steps, ssim, first=200):
    """it/s over iterations first .. steps of one calibration planned for steps + 100 and cut at `steps` (all of phase 2)"""
    assert 0.05 * (steps + 100) / 100 < 1 and first < steps
    marks = {}

    def hook(done):
        if done in (first, steps):
            torch.cuda.synchronize()
            marks[done] = time.perf_counter()

    before = ops.ssim_loss_head_launches
    calibrate(quantised(model, emb), emb, frames, steps + 100, ssim, epoch_batches=100, hook=hook, max_steps=steps)
    assert (ops.ssim_loss_head_launches > before) == (ssim is not None)
    return (steps - first) / (marks[steps] - marks[first])


def headline(tree, steps, warmup):
    """bench.py's headline it/s of the checkout at `tree`, in a fresh child process"""
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--repeats", "1",
           "--no-cpu-baseline", "--no-fp32", "--no-phase1", "--no-nerv", "--no-trained", "--no-uvg"]
    out = subprocess.run(cmd, cwd=tree, check=True, capture_output=True, text=True, timeout=600).stdout
    return float(json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])["value"])


@torch.no_grad()
def metrics(net, emb, frames):
    psnr, msssim, ssim = [], [], []
    for i in range(frames.shape[0]):
        gt = ops.gather_frames_u8(frames, torch.tensor([i], device="cuda"))
        out = net.decode(emb[i:i + 1])[0]
        psnr.append(ops.frame_psnr(out, gt))
        msssim.append(ops.ms_ssim(out, gt))
        ssim.append(ops.ssim(out, gt))
    return {"psnr": round(float(torch.cat(psnr).mean()), 4), "ms_ssim": round(float(torch.cat(msssim).mean()), 5),
            "ssim": round(float(torch.cat(ssim).mean()), 5)}


def spread(v, digits=1):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_calib.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--rate_repeats", type=int, default=3)
    ap.add_argument("--parent_tree", default=None, help="a built checkout of the parent commit: bench.py there against bench.py here")
    ap.add_argument("--headline_steps", type=int, default=600)
    ap.add_argument("--skip", default="", help="comma-separated: kernels, iteration, effect")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_ssim_calib needs the GPU (nothing is measured without one)")
    logging.getLogger().setLevel(logging.WARNING)
    skip = set(filter(None, a.skip.split(",")))
    res = {"device": torch.cuda.get_device_name(0), "calls_per_window": a.calls, "repeats": a.repeats}
    if os.path.exists(a.out):                    # sections measured by an earlier call are kept
        with open(a.out) as fh:
            res = dict(json.load(fh), **res)
    if a.parent_tree:                            # before this process opens the GPU for long: child processes, alternating
        runs = {"this_tree": [], "parent": []}
        for _ in range(a.rate_repeats):
            runs["this_tree"].append(headline(ROOT, a.headline_steps, 100))
            runs["parent"].append(headline(a.parent_tree, a.headline_steps, 100))
        res["default_path"] = {"what": "bench.py --gpus 1 --steps %d --warmup 100 (headline `value`, l2), fresh processes, alternating"
                                       % a.headline_steps,
                               "it_per_s": {k: spread(v) for k, v in runs.items()},
                               "this_tree_over_parent": round(statistics.median(runs["this_tree"]) / statistics.median(runs["parent"]), 4)}
    model, emb, frames = fixture()
    if "kernels" not in skip:
        res["kernels"] = [bench_kernels(frames, B, a.repeats, a.calls) for B in (2, 1)]
    if "iteration" not in skip:
        rates = {"l2": [], "Fusion5": []}
        for _ in range(a.rate_repeats):          # alternating
            for name in rates:
                rates[name].append(iteration_rate(model, emb, frames, a.steps, OBJECTIVES[name]))
        res["iteration"] = {"model": "HNeRV-3M 640x1280 (trained fixture), B = 2, bits 6 5 4 5 5 6 6, captured iterations",
                            "iterations_timed": a.steps - 200, "it_per_s": {k: spread(v) for k, v in rates.items()},
                            "Fusion5_over_l2": round(statistics.median(rates["Fusion5"]) / statistics.median(rates["l2"]), 4),
                            "note": "l2 computes its loss behind the head convolution (nq_head_forward_loss); Fusion5 runs the head "
                                    "convolution and nq_ssim_loss_head (three launches) after it"}
    if "effect" not in skip:
        effect = {"full_precision": metrics(model, emb, frames), "quantised_before_calibration": metrics(quantised(model, emb), emb, frames)}
        for name, ssim in OBJECTIVES.items():
            effect["calibrated_" + name] = metrics(calibrate(quantised(model, emb), emb, frames, a.iters, ssim), emb, frames)
        res["effect"] = {"model": "tests/golden/hnerv3m_bunny8real_f16.npz on tests/golden/bunny8_640x1280.npz, bits %s, "
                                  "channel-wise 'max' scales, %d iterations, B = 2, weight 0.01, lr 0.003, warmup 0.2"
                                  % (" ".join(map(str, BITS)), a.iters),
                         "metrics": effect, "note": "means over the eight frames; one run per objective"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])

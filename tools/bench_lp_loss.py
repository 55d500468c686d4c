#!/usr/bin/env python3
"""Measures the absolute-error loss (neuroquant_amd/csrc/lp_loss.hip) on the GPU:

  kernels      per call at (2, 3, 640, 1280): nq_lp_loss with p = 1 in image and head mode, float and uint8-cache target, beside
               nq_l2_loss and nq_l2_loss_tanh_head; p = 3.5 against p = 1; nq_ssim_loss alone against nq_ssim_loss followed by the
               accumulate-mode L1 launch (what that extra pass costs: the number a fused L1 + SSIM gather has to beat)
  trainer      HNeRV-3M steps/s of the trainer's step with `l2`, `Fusion5`, `lp` (p = 1: the reference's l1) and the Fusion6
               weights through ops.ssim_loss(w_l1=)
  calibration  HNeRV-3M phase-2 it/s of model_reconstruction with p = 2 (the default path) and p = 1
  default      with --parent_tree DIR (a built checkout of the parent commit): bench.py of both trees, alternating

    python tools/bench_lp_loss.py [--out profiles/lp_loss.json] [--runs 3] [--calls 200] [--steps 120] [--parent_tree DIR]

Every arm runs `runs` times, the arms alternating inside a run; the median and the range are reported.  Kernels: HIP events
around `calls` back-to-back calls of the ops wrapper on one stream (launch gaps and the wrapper's allocations included, the same
for every arm).  Trainer and calibration: host clock between two device synchronisations, 20 steps into a run and at its end.
Recorded, not asserted.  Prints ONE JSON object and writes it to --out.  Needs the GPU."""
import argparse
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
from bench import BITS, HNERV_3M, build_model  # noqa: E402
from neuroquant_amd import ops  # noqa: E402
from neuroquant_amd.methods import regress  # noqa: E402
from neuroquant_amd.methods.calibrate_network import seed_all  # noqa: E402
from neuroquant_amd.models import HNeRV  # noqa: E402
from neuroquant_amd.quantization import QuantModel, model_reconstruction  # noqa: E402
from neuroquant_amd.utils import CacheLoader, FrameCache  # noqa: E402


def spread(v, nd=2):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def window_us(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / calls


def bench_kernels(frames_u8, runs, calls):
    idx = torch.tensor([1, 0], device="cuda")
    tgt = ops.gather_frames_u8(frames_u8, idx)
    g = torch.Generator(device="cuda").manual_seed(2)
    pred = (tgt + 0.05 * torch.randn(tgt.shape, device="cuda", generator=g)).clamp_(0.01, 0.99)

    def ssim_plus_l1():
        loss3, grad = ops.ssim_loss_raw(pred, tgt, 0.0, 0.3)
        ops.lp_loss_raw(pred, tgt=tgt, w_abs=0.7, into=(loss3, grad, None))

    fns = {"l2_loss": lambda: ops.l2_loss_and_grad(pred, tgt),
           "l2_loss_tanh_head_cache": lambda: ops.l2_loss_tanh_head_raw(pred, cache_u8=frames_u8, idx=idx),
           "lp_p1_image": lambda: ops.lp_loss_raw(pred, tgt=tgt),
           "lp_p1_image_cache": lambda: ops.lp_loss_raw(pred, cache_u8=frames_u8, idx=idx),
           "lp_p1_head": lambda: ops.lp_loss_raw(pred, tgt=tgt, head=True),
           "lp_p1_head_cache": lambda: ops.lp_loss_raw(pred, cache_u8=frames_u8, idx=idx, head=True),
           "lp_p3.5_image": lambda: ops.lp_loss_raw(pred, tgt=tgt, p=3.5),
           "lp_p1_plus_mse_image": lambda: ops.lp_loss_raw(pred, tgt=tgt, w_abs=0.3, w_mse=0.7),
           "ssim_loss": lambda: ops.ssim_loss_raw(pred, tgt, 0.0, 0.3),
           "ssim_loss_then_l1_accumulate": ssim_plus_l1}
    for fn in fns.values():
        for _ in range(20):
            fn()
    t = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            t[k].append(window_us(fn, calls))
    row = {"shape": list(pred.shape), "us_per_call": {k: spread(v) for k, v in t.items()},
           "note": "back-to-back calls of the ops wrapper on one stream: launch gaps and allocations included"}
    med = {k: statistics.median(v) for k, v in t.items()}
    row["l1_accumulate_pass_us"] = round(med["ssim_loss_then_l1_accumulate"] - med["ssim_loss"], 2)
    row["p3.5_over_p1"] = round(med["lp_p3.5_image"] / med["lp_p1_image"], 3)
    row["lp_p1_head_cache_over_l2_tanh_head_cache"] = round(med["lp_p1_head_cache"] / med["l2_loss_tanh_head_cache"], 3)
    return row


def train_rate(frames_u8, loss, steps, first=20, seed=903):
    """steps/s over steps first .. steps of the trainer's step at B = 2; loss = a config's `loss:` or a callable(img_out, img)"""
    seed_all(seed)
    args = regress.parse_args(["--arch", "hnerv"])
    args.lr = 1e-3
    params = None if callable(loss) else regress.loss_params(args, dict(HNERV_3M, loss=loss))
    loader = CacheLoader(FrameCache(frames_u8), list(range(frames_u8.shape[0])), 2, seed=seed)
    model = HNeRV(HNERV_3M).to("cuda").train()
    opt = torch.optim.Adam(model.parameters(), weight_decay=0.)
    done, marks = 0, {}
    while done < steps:
        for sample in loader:
            img = sample["img"]
            img_out, _, _ = model(img)
            step = loss(img_out, img) if callable(loss) else regress.step_loss(img_out, img, params)
            opt.zero_grad(set_to_none=True)
            step.backward()
            opt.step()
            done += 1
            if done in (first, steps):
                torch.cuda.synchronize()
                marks[done] = time.perf_counter()
            if done == steps:
                break
    return (steps - first) / (marks[steps] - marks[first])


def calib_rate(frames_u8, p, steps, first=20):
    """phase-2 it/s of model_reconstruction(p=p) on the seeded HNeRV-3M of bench.py at B = 2, from the uint8 frame cache"""
    model = build_model().to("cuda")
    cache = FrameCache(frames_u8)
    with torch.no_grad():
        emb = torch.cat([model.encode(cache.batch(torch.tensor([i], device="cuda"))) for i in range(len(cache))])
    qnn = QuantModel(model, hadamard=False, weight_quant_params=dict(n_bits=8, channel_wise=True, scale_method="max"))
    qnn.set_bitwidth(BITS)
    qnn.eval()
    qnn.set_quant_state(True)
    with torch.no_grad():
        qnn(emb[:2])
    loader = CacheLoader(cache, list(range(len(cache))), 2, seed=903, epoch_batches=steps + 1)
    marks = {}

    def hook(done):
        if done in (first, steps) and done not in marks:
            torch.cuda.synchronize()
            marks[done] = time.perf_counter()

    model_reconstruction(qnn, cali_data=emb, gt=loader, arch="hnerv", batch_size=2, iters=len(loader), hadamard=False, warmup=0.0,
                         max_steps=steps, step_hook=hook, weight=0.01, b_range=(20, 2), lr=0.003, p=p)
    hook(steps)
    return (steps - first) / (marks[steps] - marks[first])


def bench_py(tree, steps, warmup):
    """it/s of `bench.py --gpus 1` in `tree`, a fresh child process -> its JSON result line"""
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                         capture_output=True, text=True, timeout=600, check=True).stdout
    return json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_loss.json"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--parent_tree", default=None, help="a built checkout of the parent commit: bench.py of both trees, alternating")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_lp_loss needs the GPU (nothing is measured without one)")
    logging.getLogger().setLevel(logging.WARNING)
    frames = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "bunny8_640x1280.npz"))["frames"]).to("cuda")
    res = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "calls_per_window": a.calls,
           "kernels": bench_kernels(frames, a.runs, a.calls)}
    fusion6 = lambda out, img: ops.ssim_loss(out, img, 0.0, 0.3, w_l1=0.7)
    arms = {"l2": "l2", "Fusion5": "Fusion5", "lp_p1 (l1)": "lp", "ssim_loss(0, 0.3, w_l1=0.7) (Fusion6)": fusion6}
    rates = {k: [] for k in arms}
    for _ in range(a.runs):
        for k, loss in arms.items():
            rates[k].append(train_rate(frames, loss, a.steps))
    res["trainer_hnerv3m_steps_per_s"] = {k: spread(v, 1) for k, v in rates.items()}
    crates = {"p=2": [], "p=1": []}
    for _ in range(a.runs):
        for k, p in (("p=2", 2.0), ("p=1", 1.0)):
            crates[k].append(calib_rate(frames, p, a.steps))
    res["calibration_hnerv3m_phase2_it_per_s"] = {k: spread(v, 1) for k, v in crates.items()}
    if a.parent_tree:
        runs = {"this": [], "parent": []}
        for _ in range(a.runs):
            for k, tree in (("this", ROOT), ("parent", a.parent_tree)):
                runs[k].append(bench_py(tree, 200, 20))
        key = next(k for k in ("it_per_s", "iters_per_s", "value") if k in runs["this"][0])
        res["default_path_bench_py"] = {k: spread([r[key] for r in v], 1) for k, v in runs.items()}
        res["default_path_bench_py"]["metric"] = key
    else:
        res["default_path_bench_py"] = "not measured (no --parent_tree)"
    res["not_done"] = "the L1 term is a pass of its own behind the SSIM / MS-SSIM launches; folding it into their gathers would save " \
                      "l1_accumulate_pass_us per call"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])

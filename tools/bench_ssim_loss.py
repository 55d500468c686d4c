#!/usr/bin/env python3
"""Measures the MSE + SSIM training loss (neuroquant_amd/csrc/ssim_loss.hip) on the GPU:

  kernels   nq_ssim_loss (forward + backward, and the forward alone) beside nq_l2_loss and nq_yuv420_loss on the same tensors
            in the same process, at (B, 3, 640, 1280), B = 1, 2
  trainer   steps/s of the trainer's step (methods/regress.py: model, step_loss, backward, Adam) with `l2` against `Fusion5`
            on a tiny HNeRV (320 x 640) and on HNeRV-3M (640 x 1280), B = 2, alternating, in the same process
  effect    HNeRV-3M trained from the same seed for the same number of steps on the eight real Bunny crops with `l2` and with
            `Fusion5`: PSNR, MS-SSIM and SSIM, means over the eight frames

    python tools/bench_ssim_loss.py [--out profiles/ssim_loss.json] [--repeats 9] [--calls 200] [--rate_steps 150] [--steps 800]

Kernels: HIP events around `calls` back-to-back calls of the ops wrapper on one stream (launch gaps and the wrapper's
allocations included, the same for every candidate), median over `repeats` windows, candidates alternating inside every repeat
after a warm-up of each.  Trainer: host clock between two device synchronisations, 20 steps into the run and at its end.
Recorded, not asserted.  Prints ONE JSON object and writes it to --out.  Needs the GPU: there is nothing to measure without one."""
import argparse
import json
import logging
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import HNERV_3M  # noqa: E402
from neuroquant_amd import ops  # noqa: E402
from neuroquant_amd.methods import regress  # noqa: E402
from neuroquant_amd.methods.calibrate_network import seed_all  # noqa: E402
from neuroquant_amd.models import HNeRV  # noqa: E402
from neuroquant_amd.utils import CacheLoader, FrameCache  # noqa: E402

TINY = dict(crop_h=320, crop_w=640, diff_enc=False, stage_block=1, enc_strides=[5, 4, 4, 2, 2], enc_channel=[16, 16, 16, 16, 8],
            channel_reduce=1.2, channel_lbound=6, dec_in_channel=12, dec_kernels=[1, 3, 5, 5, 5], dec_strides=[5, 4, 4, 2, 2],
            dec_norm="none", dec_acts="gelu", out_bias="tanh")
YUV = dict(matrix="bt709", full_range=False, weights=(6.0, 1.0, 1.0))
LR = 1e-3


def window_us(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / calls


def bench_kernels(frames_u8, B, repeats, calls):
    g = torch.Generator(device="cuda").manual_seed(B)
    tgt = ops.gather_frames_u8(frames_u8, torch.arange(B, device="cuda"))
    pred = (tgt + 0.05 * torch.randn(tgt.shape, device="cuda", generator=g)).clamp_(0.01, 0.99)
    fns = {"ssim_loss_fusion5": lambda: ops.ssim_loss_raw(pred, tgt, 0.7, 0.3),
           "ssim_loss_fusion5_forward_only": lambda: ops.ssim_loss_raw(pred, tgt, 0.7, 0.3, want_grad=False),
           "l2_loss": lambda: ops.l2_loss_and_grad(pred, tgt),
           "yuv420_loss": lambda: ops.yuv420_loss_raw(pred, tgt=tgt, head=False, **YUV)}
    for fn in fns.values():
        for _ in range(20):
            fn()
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t[k].append(window_us(fn, calls))
    row = {"shape": list(pred.shape), "inputs": "real Bunny crops and their noisy (sigma 0.05) versions",
           "note": "back-to-back calls of the ops wrapper on one stream: launch gaps and allocations included"}
    for k in fns:
        row[k] = {"us_per_call": round(statistics.median(t[k]), 2), "us_min_max": [round(min(t[k]), 2), round(max(t[k]), 2)]}
    row["ssim_loss_over_l2_loss_time"] = round(row["ssim_loss_fusion5"]["us_per_call"] / row["l2_loss"]["us_per_call"], 2)
    return row


def train(cfg, frames_u8, loss_name, steps, seed=903, first=None):
    """`steps` trainer steps at B = 2 from `seed` -> (model, steps/s over steps first .. steps or None)"""
    seed_all(seed)
    args = regress.parse_args(["--arch", "hnerv"])
    args.lr = LR
    params = regress.loss_params(args, dict(cfg, loss=loss_name))
    loader = CacheLoader(FrameCache(frames_u8), list(range(frames_u8.shape[0])), 2, seed=seed)
    model = HNeRV(cfg).to("cuda").train()
    opt = torch.optim.Adam(model.parameters(), weight_decay=0.)
    done, marks = 0, {}
    while done < steps:
        for sample in loader:
            regress.adjust_lr(opt, done / steps, args)
            img = sample["img"]
            img_out, _, _ = model(img)
            loss = regress.step_loss(img_out, img, params)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            done += 1
            if done in (first, steps):
                torch.cuda.synchronize()
                marks[done] = time.perf_counter()
            if done == steps:
                break
    rate = (steps - first) / (marks[steps] - marks[first]) if first else None
    return model, rate


@torch.no_grad()
def metrics(model, frames_u8):
    model.eval()
    psnr, msssim, ssim = [], [], []
    for i in range(frames_u8.shape[0]):
        gt = ops.gather_frames_u8(frames_u8, torch.tensor([i], device="cuda"))
        out = model(gt)[0]
        psnr.append(ops.frame_psnr(out, gt))
        msssim.append(ops.ms_ssim(out, gt))
        ssim.append(ops.ssim(out, gt))
    return {"psnr": round(float(torch.cat(psnr).mean()), 4), "ms_ssim": round(float(torch.cat(msssim).mean()), 5),
            "ssim": round(float(torch.cat(ssim).mean()), 5)}


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_loss.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rate_steps", type=int, default=150)
    ap.add_argument("--rate_repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=800)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_ssim_loss needs the GPU (nothing is measured without one)")
    logging.getLogger().setLevel(logging.WARNING)
    frames = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "bunny8_640x1280.npz"))["frames"]).to("cuda")
    res = {"device": torch.cuda.get_device_name(0), "calls_per_window": a.calls, "repeats": a.repeats,
           "kernels": [bench_kernels(frames, B, a.repeats, a.calls) for B in (1, 2)]}
    res["trainer"] = {"note": "model + step_loss + backward + Adam at B = 2, steps 20 .. %d of a run, %d runs per loss, alternating"
                              % (a.rate_steps, a.rate_repeats)}
    for name, cfg, data in (("tiny_320x640", TINY, frames[:, :, :320, :640].contiguous()), ("hnerv3m_640x1280", HNERV_3M, frames)):
        rates = {"l2": [], "Fusion5": []}
        for _ in range(a.rate_repeats):
            for loss_name in rates:
                rates[loss_name].append(train(cfg, data, loss_name, a.rate_steps, first=20)[1])
        res["trainer"][name] = {"steps_per_s": {k: {"median": round(statistics.median(v), 1), "min": round(min(v), 1),
                                                    "max": round(max(v), 1)} for k, v in rates.items()},
                                "Fusion5_over_l2": round(statistics.median(rates["Fusion5"]) / statistics.median(rates["l2"]), 4)}
    res["effect"] = {"model": "HNeRV-3M from seed 903 on tests/golden/bunny8_640x1280.npz, %d steps, B = 2, Adam, lr %g, "
                              "cosine_0.1_1_0.1; means over the eight training frames; one run per loss" % (a.steps, LR),
                     "metrics": {loss_name: metrics(train(HNERV_3M, frames, loss_name, a.steps)[0], frames)
                                 for loss_name in ("l2", "Fusion5")}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])

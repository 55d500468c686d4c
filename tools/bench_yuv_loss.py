#!/usr/bin/env python3
"""Measures the YUV 4:2:0 objective (neuroquant_amd/csrc/yuv_loss.hip) on the GPU:

  kernels    nq_yuv420_loss in both gradient modes and both target forms against nq_l2_loss_tanh_head on the same tensors in
             the same process, at (2, 3, 640, 1280) and (2, 3, 960, 1920), with the bytes the algorithm moves over the time
  iteration  calibration it/s of the trained HNeRV-3M at B = 2 with loss_domain 'yuv420' against 'rgb' (which runs the loss
             behind the head convolution, one launch the YUV path gives up), alternating, in the same process
  effect     2000-iteration calibrations at bits 6 5 4 5 5 6 6 in both domains on the trained HNeRV-3M fixture and its eight
             frames: RGB PSNR, MS-SSIM and PSNR-Y / U / V / 6:1:1 of each

    python tools/bench_yuv_loss.py [--out profiles/yuv_loss.json] [--repeats 9] [--calls 500] [--iters 2000] [--steps 1200]

Kernels: HIP events around `calls` back-to-back calls of the ops wrapper on one stream (launch gaps and the wrapper's four
allocations included, the same for every candidate), median over `repeats` windows, candidates alternating inside every
repeat after a warm-up of each.  Iteration: host clock between two device synchronisations, 200 iterations into the run and
at its end.  Prints ONE JSON object and writes it to --out.  Needs the GPU: there is nothing to measure without one."""
import argparse
import copy
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from neuroquant_amd import ops  # noqa: E402

BITS = [6, 5, 4, 5, 5, 6, 6]
YUV = dict(matrix="bt709", full_range=False, weights=(6.0, 1.0, 1.0))


def window_us(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / calls


def bench_kernels(B, H, W, repeats, calls):
    g = torch.Generator(device="cuda").manual_seed(H + W)
    cache = torch.randint(0, 256, (8, 3, H, W), device="cuda", dtype=torch.uint8, generator=g)
    idx = torch.tensor([5, 2], device="cuda")[:B]
    tgt = ops.gather_frames_u8(cache, idx)
    pred = (tgt + 0.05 * torch.randn(tgt.shape, device="cuda", generator=g)).clamp_(0.01, 0.99)
    n = pred.numel()
    f32, u8 = 12 * n, 9 * n                     # pred + target read, gradient written; the sums are a few KB
    fns = {"yuv420_loss_image_f32": (lambda: ops.yuv420_loss_raw(pred, tgt=tgt, head=False, **YUV), f32),
           "yuv420_loss_head_f32": (lambda: ops.yuv420_loss_raw(pred, tgt=tgt, head=True, **YUV), f32),
           "yuv420_loss_head_u8": (lambda: ops.yuv420_loss_raw(pred, cache_u8=cache, idx=idx, head=True, **YUV), u8),
           "l2_loss_tanh_head_f32": (lambda: ops.l2_loss_tanh_head_raw(pred, tgt=tgt), f32),
           "l2_loss_tanh_head_u8": (lambda: ops.l2_loss_tanh_head_raw(pred, cache_u8=cache, idx=idx), u8)}
    for fn, _ in fns.values():
        assert fn() is not None
        for _ in range(20):
            fn()
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, (fn, _) in fns.items():
            t[k].append(window_us(fn, calls))
    row = {"shape": [B, 3, H, W], "note": "back-to-back calls of the ops wrapper on one stream: launch gaps and allocations included"}
    for k, (_, nbytes) in fns.items():
        us = statistics.median(t[k])
        row[k] = {"us_per_call": round(us, 2), "us_min_max": [round(min(t[k]), 2), round(max(t[k]), 2)],
                  "algorithmic_bytes": nbytes, "GB_per_s": round(nbytes / us / 1e3, 1)}
    for form in ("f32", "u8"):
        row["yuv420_head_over_l2_head_time_" + form] = round(row["yuv420_loss_head_" + form]["us_per_call"] /
                                                             row["l2_loss_tanh_head_" + form]["us_per_call"], 3)
    return row


def fixture():
    import precision_gate as pg
    model, emb, _ = pg.load_fixture_checkpoint("hnerv3m_bunny8real_f16.npz", "cuda")
    frames = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "bunny8_640x1280.npz"))["frames"]).to("cuda")
    return model, emb, frames


def quantised(model, emb):
    from neuroquant_amd.quantization import QuantModel
    qnn = QuantModel(copy.deepcopy(model), hadamard=False, weight_quant_params=dict(n_bits=8, channel_wise=True, scale_method="max")).to("cuda")
    qnn.set_bitwidth(BITS)
    qnn.eval()
    qnn.set_quant_state(True)
    with torch.no_grad():
        qnn(emb[:2])
    return qnn


def calibrate(qnn, emb, frames, iters, domain, epoch_batches=None, hook=None, max_steps=None):
    from neuroquant_amd.quantization import model_reconstruction
    from neuroquant_amd.utils import CacheLoader, FrameCache
    loader = CacheLoader(FrameCache(frames), list(range(frames.shape[0])), 2, seed=903, epoch_batches=epoch_batches)
    model_reconstruction(qnn, cali_data=emb, gt=loader, arch="hnerv", batch_size=2, iters=iters, weight=0.01, opt_mode="mse",
                         hadamard=False, b_range=(20, 2), warmup=0.2, p=2.0, lr=0.003, step_hook=hook, max_steps=max_steps,
                         loss_domain=domain, yuv=YUV if domain == "yuv420" else None)
    qnn.set_quant_state(True)
    qnn.eval()
    return qnn


def iteration_rate(model, emb, frames, steps, domain, first=200):
    """it/s over iterations first .. steps of one calibration planned for steps + 100 and cut at `steps` (all of phase 2:
    0.05 * (steps + 100) / 100 rounds to no phase-1 epoch)"""
    assert 0.05 * (steps + 100) / 100 < 1 and first < steps
    marks = {}

    def hook(done):
        if done in (first, steps):
            torch.cuda.synchronize()
            marks[done] = time.perf_counter()

    before = ops.yuv420_loss_launches
    calibrate(quantised(model, emb), emb, frames, steps + 100, domain, epoch_batches=100, hook=hook, max_steps=steps)
    assert (ops.yuv420_loss_launches > before) == (domain == "yuv420")
    return (steps - first) / (marks[steps] - marks[first])


@torch.no_grad()
def metrics(net, emb, frames):
    h, w = frames.shape[-2:]
    psnr, ssim, yuv = [], [], []
    for i in range(frames.shape[0]):
        gt = ops.gather_frames_u8(frames, torch.tensor([i], device="cuda"))
        out = net.decode(emb[i:i + 1])[0]
        psnr.append(ops.frame_psnr(out, gt))
        ssim.append(ops.ms_ssim(out, gt))
        yuv.append(ops.yuv420_psnr(ops.frames_to_yuv420(out, YUV["matrix"], YUV["full_range"]),
                                   ops.frames_to_yuv420(gt, YUV["matrix"], YUV["full_range"]), h, w))
    p = torch.cat(yuv).cpu()
    loss4 = ops.yuv420_loss_raw(torch.cat([net.decode(emb[i:i + 1])[0] for i in range(2)]), cache_u8=frames,
                                idx=torch.arange(2, device="cuda"), **YUV)[0].cpu()
    return {"psnr_rgb": round(float(torch.cat(psnr).mean()), 4), "ms_ssim": round(float(torch.cat(ssim).mean()), 5),
            "psnr_y": round(float(p[:, 0].mean()), 4), "psnr_u": round(float(p[:, 1].mean()), 4),
            "psnr_v": round(float(p[:, 2].mean()), 4),
            "psnr_yuv_611": round(float(((6 * p[:, 0] + p[:, 1] + p[:, 2]) / 8).mean()), 4),
            "unrounded_plane_psnr_frames_0_1": [round(float(-10 * torch.log10(v)), 4) for v in loss4[1:]]}


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_loss.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--rate_repeats", type=int, default=3)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_yuv_loss needs the GPU (nothing is measured without one)")
    logging.getLogger().setLevel(logging.WARNING)
    res = {"device": torch.cuda.get_device_name(0), "calls_per_window": a.calls, "repeats": a.repeats, "objective": YUV,
           "kernels": [bench_kernels(2, H, W, a.repeats, a.calls) for H, W in ((640, 1280), (960, 1920))]}
    model, emb, frames = fixture()
    rates = {"rgb": [], "yuv420": []}
    for _ in range(a.rate_repeats):              # alternating
        for domain in rates:
            rates[domain].append(iteration_rate(model, emb, frames, a.steps, domain))
    res["iteration"] = {"model": "HNeRV-3M 640x1280 (trained fixture), B = 2, bits 6 5 4 5 5 6 6, captured iterations",
                        "iterations_timed": a.steps - 200,
                        "it_per_s": {k: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
                                     for k, v in rates.items()},
                        "yuv420_over_rgb": round(statistics.median(rates["yuv420"]) / statistics.median(rates["rgb"]), 4),
                        "note": "rgb computes its loss behind the head convolution (nq_head_forward_loss); yuv420 runs the head "
                                "convolution and nq_yuv420_loss as two launches"}
    effect = {"full_precision": metrics(model, emb, frames), "quantised_before_calibration": metrics(quantised(model, emb), emb, frames)}
    for domain in ("rgb", "yuv420"):
        effect["calibrated_" + domain] = metrics(calibrate(quantised(model, emb), emb, frames, a.iters, domain), emb, frames)
    res["effect"] = {"model": "tests/golden/hnerv3m_bunny8real_f16.npz on tests/golden/bunny8_640x1280.npz, bits 6 5 4 5 5 6 6, "
                              "channel-wise 'max' scales, %d iterations, B = 2, weight 0.01, lr 0.003, warmup 0.2" % a.iters,
                     "metrics": effect,
                     "note": "means over the eight frames; the 4:2:0 planes of the ground truth are those of the cached RGB frames"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])

#!/usr/bin/env python3
"""Times ops.ms_ssim (neuroquant_amd/csrc/msssim.hip) against the same arithmetic composed from PyTorch ops on the GPU
(grouped F.conv2d along H then W, F.avg_pool2d -- what a user would have to write without the kernel; the composition
lives only in this tool), and evaluate() of the drivers on 8 frames of HNeRV-3M with and without the MS-SSIM call.

    python tools/bench_msssim.py [--out profiles/msssim.json] [--repeats 9] [--calls 50]

Per shape: median over `repeats` windows of `calls` calls each, HIP events on the stream, after a warm-up of both paths.
Prints ONE JSON object and writes it to --out.  Needs the GPU: there is nothing to measure without one."""
import argparse
import json
import logging
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from neuroquant_amd import ops  # noqa: E402

SHAPES = [(1, 640, 1280), (8, 640, 1280), (1, 960, 1920)]
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
LAUNCHES = 6   # one per scale + the finishing launch (nq_ms_ssim)


def torch_ms_ssim(X, Y, g):
    """the definition of ops.ms_ssim from PyTorch ops; g: the (11,) window on the device."""
    c = X.shape[1]
    gh, gw = g.view(1, 1, -1, 1).expand(c, 1, -1, 1), g.view(1, 1, 1, -1).expand(c, 1, 1, -1)

    def filt(a):
        return F.conv2d(F.conv2d(a, gh, groups=c), gw, groups=c)

    vals = []
    for s in range(5):
        mu1, mu2 = filt(X), filt(Y)
        s1, s2, s12 = filt(X * X) - mu1 * mu1, filt(Y * Y) - mu2 * mu2, filt(X * Y) - mu1 * mu2
        cs_map = (2 * s12 + 0.03 ** 2) / (s1 + s2 + 0.03 ** 2)
        if s < 4:
            vals.append(torch.relu(cs_map.flatten(2).mean(-1)))
            pad = (X.shape[2] % 2, X.shape[3] % 2)
            X, Y = F.avg_pool2d(X, 2, padding=pad), F.avg_pool2d(Y, 2, padding=pad)
        else:
            ssim_map = (2 * mu1 * mu2 + 0.01 ** 2) / (mu1 * mu1 + mu2 * mu2 + 0.01 ** 2) * cs_map
            vals.append(torch.relu(ssim_map.flatten(2).mean(-1)))
    w = torch.tensor(WEIGHTS, device=X.device).view(-1, 1, 1)
    return torch.prod(torch.stack(vals) ** w, 0).mean(1)


def algorithmic_bytes(f, c, h, w):
    """every scale's two images read once + the pooled images of scales 2-5 written once."""
    rd = wr = 0
    for s in range(5):
        rd += 2 * f * c * h * w * 4
        h, w = (h + 1) // 2, (w + 1) // 2
        if s < 4:
            wr += 2 * f * c * h * w * 4
    return rd + wr


def window_us(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / calls


def bench_shape(f, h, w, repeats, calls):
    gen = torch.Generator(device="cuda").manual_seed(903)
    from neuroquant_amd.utils import synthetic_frames
    Y = synthetic_frames(f, h, w, device="cuda").float() / 255.0
    X = (Y + 0.014 * torch.randn(Y.shape, device="cuda", generator=gen)).clamp(0, 1)
    coords = torch.arange(11, dtype=torch.float32, device="cuda") - 5
    g = torch.exp(-(coords ** 2) / (2 * 1.5 ** 2))
    g = g / g.sum()
    hip, ref = (lambda: ops.ms_ssim(X, Y)), (lambda: torch_ms_ssim(X, Y, g))
    diff = (hip() - ref()).abs().max().item()
    for fn in (hip, ref):
        window_us(fn, 10)
    t_hip, t_ref = [], []
    for _ in range(repeats):                     # alternating windows: both see the same neighbours on the machine
        t_hip.append(window_us(hip, calls))
        t_ref.append(window_us(ref, calls))
    us_hip, us_ref = statistics.median(t_hip), statistics.median(t_ref)
    nbytes = algorithmic_bytes(f, 3, h, w)
    return {"frames": f, "H": h, "W": w, "hip_us_per_call": round(us_hip, 2), "torch_ops_us_per_call": round(us_ref, 2),
            "torch_over_hip": round(us_ref / us_hip, 2), "hip_us_min_max": [round(min(t_hip), 2), round(max(t_hip), 2)],
            "torch_ops_us_min_max": [round(min(t_ref), 2), round(max(t_ref), 2)],
            "algorithmic_bytes": nbytes, "hip_TB_per_s": round(nbytes / us_hip / 1e6, 3),
            "launches_per_call": LAUNCHES, "max_abs_diff_hip_vs_torch_ops": diff}


def bench_evaluate(repeats):
    """ms per evaluated frame of calibrate_network.evaluate() on 8 frames of HNeRV-3M (decode, PSNR, the encoder and the
    frame gather included), with ops.ms_ssim and with the call replaced by a constant (the evaluation as it was before
    MS-SSIM was reported)."""
    import types
    import precision_gate as pg
    from neuroquant_amd.methods import calibrate_network as cn
    from neuroquant_amd.utils import FrameCache
    model, _, _ = pg.load_fixture_checkpoint("hnerv3m_bunny8real_f16.npz", "cuda")
    cache = FrameCache(pg.bunny_real_640("cuda", 8))
    args = types.SimpleNamespace(arch="hnerv", print_freq=50, val_ind_list=[])
    real, const = ops.ms_ssim, torch.ones(1, device="cuda")

    def run(with_ssim):
        ops.ms_ssim = real if with_ssim else (lambda out, gt: const)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cn.evaluate(model, cache, args, pg.HNERV_3M)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / len(cache)
        finally:
            ops.ms_ssim = real

    for k in range(3):
        run(True), run(False)
    t_with, t_without = [], []
    for _ in range(repeats):
        t_with.append(run(True))
        t_without.append(run(False))
    a, b = statistics.median(t_with), statistics.median(t_without)
    return {"frames": len(cache), "ms_per_frame_with_msssim": round(a, 4), "ms_per_frame_without": round(b, 4),
            "with_over_without": round(a / b, 4), "with_min_max": [round(min(t_with), 4), round(max(t_with), 4)],
            "without_min_max": [round(min(t_without), 4), round(max(t_without), 4)]}


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msssim.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_msssim needs the GPU (nothing is measured without one)")
    logging.getLogger().setLevel(logging.WARNING)
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "calls_per_window": a.calls,
           "ms_ssim": [bench_shape(f, h, w, a.repeats, a.calls) for f, h, w in SHAPES],
           "evaluate_hnerv3m": bench_evaluate(a.repeats)}
    res["faster_than_torch_ops_at_all_shapes"] = all(r["torch_over_hip"] > 1 for r in res["ms_ssim"])
    res["evaluate_within_1.25x"] = res["evaluate_hnerv3m"]["with_over_without"] <= 1.25
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main(sys.argv[1:])

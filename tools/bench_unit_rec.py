#!/usr/bin/env python3
"""nq_unit_rec_loss against the unfused chain it replaces (ops.lp_loss_raw image-mode gradient + nq_ps_gelu_backward), lp p = 2, at
the dec5 block (2, 37, 640, 1280) r = 2, the dec4 block (2, 44, 320, 640) r = 2 and the head (2, 3, 640, 1280) r = 1 of HNeRV-3M;
the fisher modes at the dec5 block.  -> profiles/unit_rec.json.  Per shape: 5 batches of 20 back-to-back calls between two HIP
events after 10 warm-up calls; the median batch mean and the range over batches are recorded, in microseconds, with the bytes the
fused kernel must move (reads of pred / tgt / z (/ fisher), one write of dconv) and the bandwidth that implies.  Not measured
here: it/s per unit of a calibration, the network-wise rate against the parent commit, PSNR of equal-iteration calibrations.

    python tools/bench_unit_rec.py [--out profiles/unit_rec.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuroquant_amd import _lib as L, ops  # noqa: E402

SHAPES = [("dec5", 2, 37, 320, 640, 2), ("dec4", 2, 44, 160, 320, 2), ("head", 2, 3, 640, 1280, 1)]   # B, C, conv H, W, r


def timed(fn, warm=10, reps=20, batches=5):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(batches):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) * 1e3 / reps)
    return dict(us=round(statistics.median(out), 2), min=round(min(out), 2), max=round(max(out), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "unit_rec.json"))
    args = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), method="5 batches x 20 calls between HIP events, 10 warm-up calls; median (min - max) us",
               cases=[])
    for name, B, C, H, W, r in SHAPES:
        full = (B, C, H * r, W * r)
        pred, tgt, z = (torch.randn(full, device="cuda") for _ in range(3))
        fisher = torch.rand(full, device="cuda") + 1
        zz = z if r > 1 else None
        mb = pred.numel() * 4 / 1e6

        def chain():
            g = ops.lp_loss_raw(pred, tgt=tgt, p=2.0, scale=float(C))[1]
            if r > 1:
                d = torch.empty((B, C * r * r, H, W), device="cuda")
                L.check(L.lib().nq_ps_gelu_backward(ops._p(g), ops._p(z), ops._p(d), B, C, H, W, r, ops._stream()))
        case = dict(name=name, shape=list(full), r=r, tensor_MB=round(mb, 1), unfused_chain=timed(chain))
        modes = [("lp", 2.0), ("lp", 1.0)] + ([("fisher_diag", 2.0), ("fisher_full", 2.0)] if name == "dec5" else [])
        for mode, p in modes:
            f = fisher if mode != "lp" else None
            t = timed(lambda: ops.unit_rec_loss(pred, tgt, mode, p, fisher=f, z=zz, r=r))
            passes = 3 + (zz is not None) + (f is not None) + (mode == "fisher_full") * 3
            t["GB_per_s"] = round(passes * mb / t["us"] * 1e3, 1)     # MB / us = TB / s
            case[f"{mode}_p{p:g}"] = t
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
    res["not_measured"] = ["it/s per unit of HNeRV-3M", "network-wise rate against the parent commit",
                           "PSNR / MS-SSIM of equal-iteration network / block / layer calibrations"]
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

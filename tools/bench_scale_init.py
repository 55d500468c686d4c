#!/usr/bin/env python3
"""Measures scale init by search (nq_scale_init_search / nq_scale_init_gaussian, neuroquant_amd/csrc/scale_init.hip, DESIGN.md
§25) on the GPU, on the trained HNeRV-3M fixture (seven weight tensors and their biases):

  default_path  with --parent_tree DIR (a built checkout of the parent commit): bench.py's headline it/s of this tree against
                that one, alternating child processes (--init max issues no new launch)
  init          ops.scale_init over all weights and biases per method, channel-wise and layer-wise, at 4 bits; the reference's
                per-channel loop over ten candidates restated in torch ops on the same GPU (channel-wise 'mse', ONE run); the
                first forward of a QuantModel (what the driver logs as `Init time`) per method
  table         bit_assign.perturbation_table over the widths 2..8 (49 sets of scales) with --init mse against max
  quality       PSNR / MS-SSIM of the quantised model straight after init ("w/o opt") and, with --iters N > 0, after N
                calibration iterations, for the four methods at bits 6 5 4 5 5 6 6, uniform 4 and uniform 3; ONE run each

    python tools/bench_scale_init.py [--out profiles/scale_init.json] [--parent_tree DIR] [--iters 2000] [--skip init,table,quality]

Host clock between two device synchronisations (a searched init ends with one host read).  Recorded, not asserted.  Sections
measured by an earlier call are kept.  Prints ONE JSON object and writes it to --out.  Needs the GPU."""
import argparse
import copy
import json
import logging
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_ssim_calib import headline, metrics, spread  # noqa: E402
from bench_yuv_loss import fixture  # noqa: E402
from neuroquant_amd import ops  # noqa: E402

METHODS = ("max", "mse", "l1", "gaussian")
SETTINGS = {"6545566": [6, 5, 4, 5, 5, 6, 6], "uniform4": [4] * 7, "uniform3": [3] * 7}


def clock_ms(fn, repeats):
    t = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


def torch_loop_mse(x, n_levels):
    """the reference's search (quantizer.py:139-140, 170-186, 227-234) in torch ops on the device: a Python loop over channels"""
    eps = torch.tensor(1e-8, device=x.device)
    out = []
    for c in range(x.shape[0]):
        r = x[c]
        x_max, x_min, best = r.max(), r.min(), 1e10
        for i in range(10):
            hi, lo = x_max * (1.0 - i * 0.05), x_min * (1.0 - i * 0.05)
            d = torch.max((hi - lo) / (n_levels - 1), eps)
            z = (-lo / d).round()
            xq = (torch.clamp(torch.round(r / d) + z, 0, n_levels - 1) - z) * d
            score = (r - xq).abs().pow(3.5).mean()
            if score < best:
                best, keep = score, (d, z)
        out.append(keep)
    return out


def quantised(model, emb, bits, method):
    from neuroquant_amd.quantization import QuantModel
    qnn = QuantModel(copy.deepcopy(model), hadamard=False, weight_quant_params=dict(n_bits=8, channel_wise=True, scale_method=method)).to("cuda")
    qnn.set_bitwidth(bits)
    qnn.eval()
    qnn.set_quant_state(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        qnn(emb[:2])
    torch.cuda.synchronize()
    return qnn, (time.perf_counter() - t0) * 1e3


def calibrate(qnn, emb, frames, iters):
    from neuroquant_amd.quantization import model_reconstruction
    from neuroquant_amd.utils import CacheLoader, FrameCache
    loader = CacheLoader(FrameCache(frames), list(range(frames.shape[0])), 2, seed=903)
    model_reconstruction(qnn, cali_data=emb, gt=loader, arch="hnerv", batch_size=2, iters=iters, weight=0.01, opt_mode="mse",
                         hadamard=False, b_range=(20, 2), warmup=0.2, p=2.0, lr=0.003)
    qnn.set_quant_state(True)
    qnn.eval()
    return qnn


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scale_init.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--iters", type=int, default=2000, help="calibration iterations of the quality rows; 0: straight after init only")
    ap.add_argument("--settings", nargs="+", default=list(SETTINGS), choices=list(SETTINGS))
    ap.add_argument("--parent_tree", default=None, help="a built checkout of the parent commit: bench.py there against bench.py here")
    ap.add_argument("--headline_steps", type=int, default=600)
    ap.add_argument("--rate_repeats", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma-separated: init, table, quality")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_scale_init needs the GPU (nothing is measured without one)")
    logging.getLogger().setLevel(logging.WARNING)
    skip = set(filter(None, a.skip.split(",")))
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            res = dict(json.load(fh), **res)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")

    if a.parent_tree:                            # child processes, alternating, before this process opens the GPU for long
        runs = {"this_tree": [], "parent": []}
        for _ in range(a.rate_repeats):
            runs["this_tree"].append(headline(ROOT, a.headline_steps, 100))
            runs["parent"].append(headline(a.parent_tree, a.headline_steps, 100))
        res["default_path"] = {"what": "bench.py --gpus 1 --steps %d --warmup 100 (headline `value`), fresh processes, alternating"
                                       % a.headline_steps,
                               "it_per_s": {k: spread(v) for k, v in runs.items()}, "runs": runs,
                               "this_tree_over_parent": round(statistics.median(runs["this_tree"]) / statistics.median(runs["parent"]), 4)}
        save()
    model, emb, frames = fixture()
    from neuroquant_amd.methods import bit_assign
    convs = bit_assign.decoder_convs(model)
    tensors = [m.weight.data for m in convs] + [m.bias.data for m in convs]
    if "init" not in skip:
        row = {"tensors": [list(t.shape) for t in tensors], "elements": sum(t.numel() for t in tensors), "n_levels": 16,
               "note": "all weights and biases, one ops.scale_init call each; host clock, the host read of a searched init included"}
        for cw in (True, False):
            for method in METHODS:
                fn = lambda: [ops.scale_init(t, 16, cw, method) for t in tensors]      # noqa: E731
                fn()
                row["%s_%s" % ("channel_wise" if cw else "layer_wise", method)] = clock_ms(fn, a.repeats)
        ws = [m.weight.data for m in convs]
        torch_loop_mse(ws[0], 16)
        row["channel_wise_mse_torch_loop"] = dict(clock_ms(lambda: [torch_loop_mse(w, 16) for w in ws], 1), runs=1,
                                                  note="weights only: the reference's per-channel loop in torch ops, same GPU")
        row["channel_wise_mse_weights_only"] = clock_ms(lambda: [ops.scale_init(w, 16, True, "mse") for w in ws], a.repeats)
        first = {}
        for m in METHODS:
            quantised(model, emb, SETTINGS["uniform4"], m)                       # warm-up: the method's first launches in this process
            first[m] = round(quantised(model, emb, SETTINGS["uniform4"], m)[1], 2)
        row["quant_model_first_forward_ms"] = first
        res["init"] = row
        save()
    if "table" not in skip:
        row = {"what": "bit_assign.perturbation_table, widths 2..8, channel-wise: 49 sets of scales, fake-quantised weights, histograms"}
        for method in ("max", "mse"):
            args = types.SimpleNamespace(channel_wise=True, hadamard=False, init=method)
            bit_assign.perturbation_table(model, list(range(2, 9)), args)
            row[method] = clock_ms(lambda: bit_assign.perturbation_table(model, list(range(2, 9)), args), 3)
        res["table"] = row
        save()
    if "quality" not in skip:
        rows = res.get("quality", {}).get("rows", {})
        for name in a.settings:
            for method in METHODS:
                qnn, _ = quantised(model, emb, SETTINGS[name], method)
                r = rows.setdefault("%s_%s" % (name, method), {})
                r["without_opt"] = metrics(qnn, emb, frames)
                if a.iters > 0:
                    r["after_%d" % a.iters] = metrics(calibrate(qnn, emb, frames, a.iters), emb, frames)
                res["quality"] = {"model": "tests/golden/hnerv3m_bunny8real_f16.npz on tests/golden/bunny8_640x1280.npz, channel-wise, B = 2, "
                                           "weight 0.01, lr 0.003, warmup 0.2, l2 objective", "rows": rows,
                                  "note": "PSNR / MS-SSIM: means over the eight frames; ONE run each"}
                save()
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])

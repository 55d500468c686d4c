"""Measures the QAT baselines' way to the bit stream (ops.qat_levels / ops.qat_restore, csrc/qat_stream.hip; bitstream.write_qat_stream
and the player's open) -> profiles/qat_stream.json.  All on the seven decoder weights of HNeRV-3M at `--bits`.

  kernels   one qat_levels call and one qat_restore call over the seven tensors, forms 'packed' and 'symbols', modes 'ffnerv' and
            'hinerv', against the same arithmetic on PyTorch ops tensor by tensor (symbols and restore; PyTorch has no packer, so
            its side of 'packed' is the symbol arithmetic followed by ops.pack_levels), alternating inside every repeat
  export    write_qat_stream of a freshly initialised HNeRV-3M with 8 frame embeddings, coding 'packed' and 'rans': host seconds
            (device work, the copies to the host, the host rANS encoder and the file write) and file bytes; ONE run each
  open      StreamDecoder(path) of those files and of a calibrated model's file of the same shape and widths (write_stream, max
            scales, no calibration): host seconds between two synchronisations, median of `--opens`

    python tools/bench_qat_stream.py [--out profiles/qat_stream.json] [--repeats 9] [--calls 50] [--opens 5] [--bits 6]

Kernels: HIP events around `calls` back-to-back calls on one stream (launch gaps and allocations included, the same for both sides),
median over `repeats` windows after a warm-up of each; microseconds per CALL.  Recorded, not asserted.  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v, digits=1):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits), "runs": len(v)}


def torch_symbols(w, bits, mode):
    """-> (uint8 symbols, column scales or None) on PyTorch ops"""
    import torch
    if mode == "ffnerv":
        t, n = torch.tanh(w), 2 ** (bits - 1) - 1
        return (torch.floor(t.abs() * float(n)) * torch.sign(t) + n).to(torch.uint8), None
    w2 = w.reshape(w.shape[0], -1)
    s = 2 * w2.abs().max(dim=0)[0] / (2. ** bits - 1.) + 1e-6
    return (torch.round(w2 / s).clamp(-2 ** (bits - 1), 2 ** (bits - 1) - 1) + 2 ** (bits - 1)).to(torch.uint8), s


def torch_restore(sym, scale, shape, bits, mode):
    if mode == "ffnerv":
        n = 2 ** (bits - 1) - 1
        return ((sym.float() - n) / float(n)).reshape(shape)
    return ((sym.float() - 2 ** (bits - 1)).reshape(shape[0], -1) * scale).reshape(shape)


def bench_kernels(ws, mode, bits, repeats, calls):
    import torch
    from neuroquant_amd import ops
    shapes = [w.shape for w in ws]
    held = {f: ops.qat_levels(ws, bits, mode, f) for f in ops.QAT_FORMS}
    tsym = [torch_symbols(w, bits, mode) for w in ws]
    sides = {
        "hip_levels_packed": lambda: ops.qat_levels(ws, bits, mode, "packed"),
        "hip_levels_symbols": lambda: ops.qat_levels(ws, bits, mode, "symbols"),
        "torch_levels_symbols": lambda: [torch_symbols(w, bits, mode) for w in ws],
        "torch_levels_then_pack": lambda: [ops.pack_levels(torch_symbols(w, bits, mode)[0], bits) for w in ws],
        "hip_restore_packed": lambda: ops.qat_restore([s for s, _ in held["packed"]], shapes, bits, mode, [c for _, c in held["packed"]], "packed"),
        "hip_restore_symbols": lambda: ops.qat_restore([s for s, _ in held["symbols"]], shapes, bits, mode, [c for _, c in held["symbols"]], "symbols"),
        "torch_restore_symbols": lambda: [torch_restore(s, c, sh, bits, mode) for (s, c), sh in zip(tsym, shapes)],
    }

    def window_us(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        with torch.no_grad():
            for _ in range(calls):
                fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / calls

    t = {k: [] for k in sides}
    for r in range(repeats + 1):                          # the first round warms up
        for k, v in t.items():
            us = window_us(sides[k])
            if r:
                v.append(us)
    return {"us_per_call": {k: spread(v) for k, v in t.items()}}


def timed_open(path, opens):
    import torch
    from neuroquant_amd.bitstream import StreamDecoder
    out = []
    for _ in range(opens + 1):                            # the first open warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        StreamDecoder(path)                               # synchronises before it returns
        out.append((time.perf_counter() - t0) * 1e3)
    return spread(out[1:], 2)


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qat_stream.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--opens", type=int, default=5)
    ap.add_argument("--bits", type=int, default=6)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_qat_stream needs the GPU (nothing is measured without one)")
    from bench import HNERV_3M
    from neuroquant_amd import bitstream
    from neuroquant_amd.methods import regress
    from neuroquant_amd.quantization import QuantModel
    cfg = dict(HNERV_3M)
    res = {"device": torch.cuda.get_device_name(0), "bits": a.bits,
           "not_measured": "the trainer's steps/s without --export_stream against the parent commit (that path runs no new code: "
                           "qat.hip's arithmetic moved to a shared header unchanged); any PSNR at equal bytes; a NeRV file",
           "kernels": {"calls_per_window": a.calls, "repeats": a.repeats,
                       "note": "one call over the seven HNeRV-3M decoder weights, back-to-back on one stream, allocations and launch "
                               "gaps included; hinerv levels include the column-statistics launch"},
           "export": {"note": "ONE run each: host seconds of write_qat_stream (8 embeddings, host rANS encoder, chunk 32768) and file bytes"},
           "open": {"note": "host milliseconds of StreamDecoder(path), median of %d after one warm-up" % a.opens}}
    emb = None

    def save():                                           # after each part: a later part that fails loses nothing measured
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)

    with tempfile.TemporaryDirectory() as tmp:
        for mode in ("ffnerv", "hinerv"):
            torch.manual_seed(0)
            model = regress.build_model(regress.parse_args(["--arch", "hnerv", "--qat", mode, "--qat_bits", str(a.bits)]), cfg, "cuda").eval()
            ws = [p.detach() for n, p in model.named_parameters() if not n.startswith("encoder") and p.dim() == 4]
            res["elements"] = sum(w.numel() for w in ws)
            res["kernels"][mode] = bench_kernels(ws, mode, a.bits, a.repeats, a.calls)
            with torch.no_grad():
                emb = model.encode(torch.rand(8, 3, cfg["crop_h"], cfg["crop_w"], device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)))
            for coding in ("packed", "rans"):
                path = os.path.join(tmp, f"{mode}_{coding}.nqv")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s = bitstream.write_qat_stream(model, path, "hnerv", cfg, mode, a.bits, embeddings=emb, coding=coding)
                res["export"][f"{mode}_{coding}"] = {"seconds": round(time.perf_counter() - t0, 3), "file_bytes": s["file_bytes"],
                                                     "nominal_bytes": s["total_bytes_nominal"]}
                res["open"][f"{mode}_{coding}"] = timed_open(path, a.opens)
        save()
        model.weight_qat = None
        qnn = QuantModel(model, hadamard=False, weight_quant_params=dict(n_bits=8, channel_wise=True, scale_method="max"))
        qnn.set_bitwidth([a.bits] * 7)
        qnn.eval()
        qnn.set_quant_state(True)
        with torch.no_grad():
            qnn(emb[:2])
        for coding in ("packed", "rans"):
            path = os.path.join(tmp, f"calibrated_{coding}.nqv")
            s = bitstream.write_stream(qnn, path, "hnerv", cfg, embeddings=emb, coding=coding)
            res["open"][f"calibrated_{coding}"] = dict(timed_open(path, a.opens), file_bytes=s["file_bytes"])
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])

#!/usr/bin/env python3
"""Sizes, quality and open times of quantised, temporally coded frame embeddings on the committed trained
HNeRV-3M decoder (tests/golden/hnerv3m_bunny8real_f16.npz, eight consecutive real Bunny frames, bits 6 5 4 5 5 6 6).

    python tools/bench_embeddings.py [--out profiles/embeddings.json] [--opens 15] [--iters 2000]

For embedding bits 4 ... 8: the section bytes of the three layouts and the one `write_stream` keeps; the PSNR of the
full-precision model and of the quantised, not yet calibrated model ('w/o opt') on the restored embeddings against the same
two figures on the fp32 embeddings (HIP path, B = 1, mean over the eight frames); the StreamDecoder open time of the file
against the file with fp32 embeddings (host clock around read + validate + upload + decode + synchronise; median, min and max
over --opens opens, the two files taking turns after a warm-up of both).  Then one --iters calibration on fp32, 8-bit and
6-bit embeddings, same seed and batch order, and the PSNR each ends at.

Eight frames is all the fixture holds: the sizes a 132-frame or a 600-frame clip would take are EXTRAPOLATED from the bits per
value measured here and say so in the output.  Prints ONE JSON object and writes it to --out.  Needs the GPU."""
import argparse
import json
import logging
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_entropy import time_opens  # noqa: E402
from bench_player import BITS, HNERV_3M  # noqa: E402


def fixture():
    import precision_gate as pg
    model, emb, _ = pg.load_fixture_checkpoint("hnerv3m_bunny8real_f16.npz", "cuda")
    return model, emb, pg.bunny_real_640("cuda", 8)


def quant_model(model):
    from neuroquant_amd.quantization import QuantModel
    qnn = QuantModel(model, hadamard=False, weight_quant_params=dict(n_bits=8, channel_wise=True, scale_method="max")).to("cuda")
    qnn.set_bitwidth(BITS)
    qnn.eval()
    qnn.set_quant_state(True)
    return qnn


@torch.no_grad()
def psnr(net, emb, gt):
    from neuroquant_amd import ops
    return float(torch.cat([ops.frame_psnr(net(emb[i:i + 1])[0], gt[i:i + 1]) for i in range(emb.shape[0])]).double().mean())


def calibrated_psnr(emb, frames_u8, gt, iters):
    """a fresh copy of the fixture calibrated for `iters` iterations on `emb` (seed 903, B = 2) -> final PSNR on `emb`"""
    from neuroquant_amd.quantization import model_reconstruction
    from neuroquant_amd.utils import CacheLoader, FrameCache
    torch.manual_seed(903)
    qnn = quant_model(fixture()[0])
    with torch.no_grad():
        qnn(emb[:2])
    model_reconstruction(qnn, cali_data=emb, gt=CacheLoader(FrameCache(frames_u8), list(range(emb.shape[0])), 2, seed=903),
                         arch="hnerv", batch_size=2, iters=iters, weight=0.01, opt_mode="mse", hadamard=False, b_range=(20, 2),
                         warmup=0.2, p=2.0, lr=0.003)
    qnn.set_quant_state(True)
    qnn.eval()
    return round(psnr(qnn, emb, gt), 4)


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "embeddings.json"))
    ap.add_argument("--opens", type=int, default=15)
    ap.add_argument("--iters", type=int, default=2000)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_embeddings needs the GPU (nothing is measured without one)")
    logging.getLogger().setLevel(logging.WARNING)
    from neuroquant_amd import ops
    from neuroquant_amd.bitstream import StreamDecoder, encode_embeddings, quantise_embeddings, write_stream
    fp_model = fixture()[0]                 # QuantModel wraps its model in place: the full-precision figures need their own copy
    model, emb, frames_u8 = fixture()
    gt = frames_u8.float() / 255.0
    n, values = emb.shape[0], emb[0].numel()
    qnn = quant_model(model)
    with torch.no_grad():
        qnn(emb[:2])
    res = {"device": torch.cuda.get_device_name(0), "conv_precision": ops.get_conv_precision(), "bits": BITS,
           "model": "HNeRV-3M 640x1280, the committed trained decoder tests/golden/hnerv3m_bunny8real_f16.npz on the eight real "
                    "Bunny crops tests/golden/bunny8_640x1280.npz; quantisers straight after their 'max' initialisation",
           "frames": n, "values_per_frame": values, "fp32_embedding_bytes": 4 * emb.numel(), "opens_per_file": a.opens,
           "psnr_fp32_embeddings": {"fp": round(psnr(fp_model.decode, emb, gt), 4), "q_noopt": round(psnr(qnn, emb, gt), 4)},
           "embedding_bits": []}
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, "fp32.nqv")
        sb = write_stream(qnn, base, "hnerv", dict(HNERV_3M), embeddings=emb)
        res["fp32_file_bytes"] = sb["file_bytes"]
        for b in range(4, 9):
            q = quantise_embeddings(emb, b)
            path = os.path.join(tmp, "e%d.nqv" % b)
            s = write_stream(qnn, path, "hnerv", dict(HNERV_3M), embeddings=q)
            e = s["embedding"]
            dec = StreamDecoder(path)
            # the temporal layout, kept or not: its 16-bit words grow with the frames, everything else (scales, frame 0, the
            # frequency table, one chunk's states and offsets) does not
            words = next(4 * ((arr.nbytes + 3) // 4) for name, _, arr in encode_embeddings(q, b, "temporal")[1] if name.endswith("rans_words"))
            fixed = e["mode_bytes"]["temporal"] - words
            # ... and the histogram entropy of the differences of frames 1..7: eight frames leave 14 symbols per lane, so a good
            # part of what they cost sits in the 64 final states, not in the words
            res_sym = ops.embed_symbols(q.source, q.delta, q.zero_point, b, True)[1][1:].reshape(-1).long()
            p = torch.bincount(res_sym, minlength=2 ** b).double() / res_sym.numel()
            bpv = float(-(p[p > 0] * p[p > 0].log2()).sum())
            row = {"bits": b, "mode_bytes": e["mode_bytes"], "mode": e["mode"], "embedding_section_bytes": e["bytes"],
                   "file_bytes": s["file_bytes"], "file_bytes_saved": sb["file_bytes"] - s["file_bytes"],
                   "restored_bit_identical_in_player": bool(torch.equal(dec.embeddings, q.restored)),
                   "psnr": {"fp": round(psnr(fp_model.decode, q.restored, gt), 4), "q_noopt": round(psnr(qnn, q.restored, gt), 4)},
                   "open_ms": time_opens({"fp32": StreamDecoder, "quantised": StreamDecoder}, {"fp32": base, "quantised": path},
                                         a.opens),
                   "temporal_word_bytes": words, "temporal_fixed_bytes": fixed,
                   "temporal_residual_entropy_bits_per_value": round(bpv, 3),
                   "extrapolated_not_measured": {
                       "note": "EXTRAPOLATED from eight frames, NOT measured on a long clip: the temporal layout at the histogram "
                               "entropy of the differences of frames 1..7 on every later frame, the fixed part (scales, frame 0, frequency "
                               "table, states and offsets of one chunk) once",
                       "bunny_132_frames_bytes": int(round(fixed + bpv * 131 * values / 8)),
                       "bunny_132_frames_fp32_bytes": 132 * values * 4,
                       "uvg_600_frames_bytes": int(round(fixed + bpv * 599 * values / 8)),
                       "uvg_600_frames_fp32_bytes": 600 * values * 4}}
            res["embedding_bits"].append(row)
    res["calibration"] = {"iters": a.iters, "note": "a fresh copy of the fixture per run, seed 903, B = 2, the same batch order; "
                                                    "PSNR of the calibrated model on the embeddings it was calibrated on",
                          "fp32": calibrated_psnr(emb, frames_u8, gt, a.iters)}
    for b in (8, 6):
        res["calibration"]["%d_bit" % b] = calibrated_psnr(quantise_embeddings(emb, b).restored, frames_u8, gt, a.iters)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])

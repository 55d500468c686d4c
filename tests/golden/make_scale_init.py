#!/usr/bin/env python3
"""scale_init.npz: UniformAffineQuantizer.init_quantization_scale of the REAL reference (quantization/quantizer.py:127-225,
imported read-only on the CPU, python -B) for scale_method 'mse' / 'l1' / 'gaussian' -- what tests/scale_init_ref.py restates
and csrc/scale_init.hip computes.  Only DATA is written: the inputs and the reference's (delta, zero_point).

  inputs   w27 (32, 3, 3, 3), w144 (32, 16, 3, 3): channel-wise weights, rows of 27 and 144 elements (normal x 0.05 x a per-row
           factor in [1, 4]); bias (96,): a 1-D tensor under channel_wise=True; layer (8, 4, 3, 3): a layer-wise tensor
  results  '<method>/<bits>/<input>/delta', '.../zp' for bits 2, 3, 4, 8
  gaussian_delta_rel  the largest relative deviation of the restatement's gaussian delta from the reference's over every
           case here (the reference takes mean and variance in fp32, the definition in double); the test allows twice that

    python3 -B tests/golden/make_scale_init.py
"""
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)

import numpy as np
import torch

import _ref_stubs

_ref_stubs.install()

from quantization.quantizer import UniformAffineQuantizer  # noqa: E402

import scale_init_ref as S  # noqa: E402

warnings.filterwarnings("ignore")
torch.set_num_threads(1)

METHODS = ("mse", "l1", "gaussian")
BITS = (2, 3, 4, 8)


def main():
    g = torch.Generator().manual_seed(2510)

    def rows(*shape):
        w = torch.randn(*shape, generator=g) * 0.05
        return w * (1 + 3 * torch.rand(shape[0], *([1] * (len(shape) - 1)), generator=g))

    inputs = {"w27": (rows(32, 3, 3, 3), True), "w144": (rows(32, 16, 3, 3), True),
              "bias": (torch.randn(96, generator=g) * 0.1, True), "layer": (rows(8, 4, 3, 3), False)}
    out = {name: t.numpy().copy() for name, (t, _) in inputs.items()}
    worst = 0.0
    for method in METHODS:
        for bits in BITS:
            for name, (t, cw) in inputs.items():
                q = UniformAffineQuantizer(n_bits=bits, channel_wise=cw, scale_method=method)
                d, z = q.init_quantization_scale(t.clone(), cw)
                d, z = np.asarray(d.detach().numpy(), np.float32), np.asarray(z.detach().numpy(), np.float32)
                out[f"{method}/{bits}/{name}/delta"], out[f"{method}/{bits}/{name}/zp"] = d, z
                rd, rz = S.scale_init(t.numpy(), 2 ** bits, cw, method)
                assert rd.shape == d.shape and rz.shape == z.shape, (method, bits, name, rd.shape, d.shape)
                same = int(((rd == d) & (rz == z)).sum())
                if method == "gaussian":
                    worst = max(worst, float(np.max(np.abs(rd.astype(np.float64) - d) / d)))
                print(f"{method:9s} {bits} bits {name:6s}: restatement bit-equal on {same} of {d.size} rows")
    out["gaussian_delta_rel"] = np.float64(worst)
    path = os.path.join(HERE, "scale_init.npz")
    np.savez_compressed(path, **out)
    print(f"gaussian: largest relative deviation of delta {worst:.3e}")
    print(f"wrote scale_init.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()

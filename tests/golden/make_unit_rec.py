#!/usr/bin/env python3
"""unit_rec.npz: calib_block.LossFunction of the REAL reference (calib_block.py:49-88, imported read-only on the CPU) with
round_loss='none' -- what tests/unit_rec_ref.loss restates.  Only DATA is written: one random (2, 3, 6, 10) triple pred / tgt /
grad (|g| + 1) in float64 and the reference's values.     python3 -B tests/golden/make_unit_rec.py"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference")

import numpy as np
import torch

import _ref_stubs
_ref_stubs.install()
from quantization.calib_block import LossFunction  # noqa: E402


def main():
    g = torch.Generator().manual_seed(3311)
    pred, tgt = (torch.randn(2, 3, 6, 10, generator=g, dtype=torch.float64) for _ in range(2))
    grad = torch.randn(2, 3, 6, 10, generator=g, dtype=torch.float64).abs() + 1
    out = dict(pred=pred.numpy(), tgt=tgt.numpy(), grad=grad.numpy())
    for rec, p in (("mse", 2.0), ("mse", 1.0), ("mse", 2.4), ("fisher_diag", 2.0), ("fisher_full", 2.0)):
        fn = LossFunction(None, round_loss="none", rec_loss=rec, max_count=10, p=p)
        out[f"mse/{p:g}" if rec == "mse" else rec] = np.float64(float(fn(pred, tgt, grad)))
    np.savez_compressed(os.path.join(HERE, "unit_rec.npz"), **out)
    print({k: float(v) for k, v in out.items() if np.ndim(v) == 0})


if __name__ == "__main__":
    main()

"""QAT baselines to the bit stream without a GPU: the symbols and the restore restated in numpy against
tests/qat_ref.py, the two C entries' declarations and refusals, and the header field a QAT file adds."""
import ctypes
import os

import numpy as np
import pytest

import qat_ref as R
from conftest import ROOT

SHAPES = [(1, 3, 1), (5, 3, 3), (65, 8, 3), (130, 7, 5), (16, 16, 1)]
f32 = np.float32


@pytest.mark.parametrize("bits", [2, 3, 5, 8])
def test_symbols_and_restore_restated(bits):
    """symbol and restore of include/nq_hip.h (above nq_qat_levels) give qat_ref's quantised weights, value for value"""
    rng = np.random.default_rng(11)
    for cout, cin, k in SHAPES:
        w = (0.5 * rng.standard_normal((cout, cin * k * k))).astype(f32)
        w[-1, 1], w[:, 2] = -np.abs(w[:, 1]).max(), 0
        n, t = 2 ** (bits - 1) - 1, np.tanh(w)
        sym = (np.sign(t) * np.floor(np.abs(t) * f32(n))).astype(np.int64) + n
        assert sym.min() >= 0 and sym.max() <= 2 * n
        assert np.array_equal((sym - n).astype(f32) / f32(n), R.ffnerv(w, bits, f32)[0])
        y, s, _, q = R.hinerv(w, bits, None, f32)
        sym = q.astype(np.int64) + 2 ** (bits - 1)
        assert sym.min() >= 0 and sym.max() < 2 ** bits
        assert np.array_equal((sym - 2 ** (bits - 1)).astype(f32) * s, y)


def test_entries_are_declared_exported_and_refuse_before_the_device():
    from neuroquant_amd import _lib
    header = open(os.path.join(ROOT, "include", "nq_hip.h")).read()
    lib = _lib.lib()
    for name in ("nq_qat_levels", "nq_qat_restore"):
        assert f" {name}(" in header and name in _lib.EXPORTS and getattr(lib, name).argtypes
    assert lib.nq_abi_version() == 7 == _lib.ABI_VERSION
    p = 64

    def call(entry, mode=1, form=0, n=1, ws=p, **kw):
        f = dict(w=p, stored=p, scale=p, Cout=4, K=9, bits=6)
        f.update(kw)
        seg = (_lib.QatStreamSeg * 1)(_lib.QatStreamSeg(*[f[k] for k in ("w", "stored", "scale", "Cout", "K", "bits")]))
        args = (seg, n, mode, form) + ((ctypes.c_void_p(ws),) if entry == "nq_qat_levels" else ()) + (None,)
        return getattr(lib, entry)(*args)

    bad = [dict(mode=2), dict(form=2), dict(n=0), dict(w=None), dict(stored=None), dict(scale=None), dict(bits=1), dict(bits=9),
           dict(Cout=0), dict(K=0), dict(Cout=1 << 16, K=1 << 15), dict(w=p + 2), dict(stored=p + 2), dict(scale=p + 2)]
    for entry in ("nq_qat_levels", "nq_qat_restore"):
        assert all(call(entry, **kw) == -1 for kw in bad), entry
    assert call("nq_qat_levels", ws=None) == -1 and call("nq_qat_levels", ws=p + 4) == -1


def test_header_field_of_a_qat_file():
    from neuroquant_amd import bitstream as B
    layers = [dict(shape=[4, 3, 3, 3], c_in_stored=3, n_bits=6), dict(shape=[3, 4, 1, 1], c_in_stored=4, n_bits=5)]
    calibrated = dict(arch="nerv", hadamard=False, bias="soft", layers=layers)
    assert B.qat_entry(calibrated) is None
    assert B.qat_entry(dict(calibrated, weight_quantiser=dict(mode="hinerv", bits=[6, 5]))) == ("hinerv", [6, 5])
    for field, more in ((dict(mode="lsq", bits=[6, 5]), {}), (dict(mode="ffnerv", bits=[6]), {}), (dict(mode="ffnerv", bits=[6, 6]), {}),
                        ("ffnerv", {}), (dict(mode="ffnerv", bits=[6, 5]), dict(hadamard=True)),
                        (dict(mode="ffnerv", bits=[6, 5]), dict(bias="hard"))):
        with pytest.raises(ValueError):
            B.qat_entry(dict(calibrated, weight_quantiser=field, **more))

"""CPU-side checks of the QAT quantisers: what the C entries and QATQuantizer refuse before a device is touched, the trainer's
flags, and that the restatement of 'ffnerv' alone stays under the cap the GPU test allows for floor's discontinuities."""
import ctypes

import numpy as np
import pytest
import torch

import qat_ref as R
from conftest import TINY_HNERV, TINY_NERV


def seg(**kw):
    from neuroquant_amd import _lib
    fields = dict(w=16, g=32, out=48, Cout=5, K=27, bits=4, index=0)
    fields.update(kw)
    return (_lib.QatSeg * 1)(_lib.QatSeg(**fields))


@pytest.mark.parametrize("bad", [dict(w=None), dict(out=None), dict(g=None), dict(w=18), dict(bits=1), dict(bits=9), dict(Cout=0), dict(K=-3),
                                 dict(Cout=1 << 16, K=1 << 15), dict(index=-1), dict(mode=2), dict(ws=None), dict(step=None), dict(nseg=0)], ids=str)
def test_c_entries_refuse_before_the_device(bad):
    from neuroquant_amd import _lib
    lib = _lib.lib()
    call = dict(mode=1, ws=ctypes.c_void_p(64), step=ctypes.c_void_p(128), nseg=1)
    call.update({k: v for k, v in bad.items() if k in call})
    s = seg(**{k: v for k, v in bad.items() if k not in call})
    entries = [lib.nq_qat_backward] if "g" in bad else [lib.nq_qat_forward, lib.nq_qat_backward]
    assert all(f(s, call["nseg"], call["mode"], 1, 903, call["step"], call["ws"], None) == -1 for f in entries)


def test_workspace_query():
    from neuroquant_amd import _lib
    lib = _lib.lib()
    assert lib.nq_qat_ws_floats(seg(), 1, 1) == 4 * 27 and lib.nq_qat_ws_floats(seg(), 1, 0) == 0
    assert lib.nq_qat_ws_floats(seg(bits=9), 1, 1) == -1 and lib.nq_qat_ws_floats(seg(), 1, 2) == -1


def test_qat_quantizer_interface():
    from neuroquant_amd.quantization import QATQuantizer, UniformAffineQuantizer
    w = torch.zeros(4, 3, 3, 3)
    q = QATQuantizer(UniformAffineQuantizer(n_bits=6), w, "hinerv")
    assert (q.n_bits, q.noise, q.round_mode, q.extra_repr()) == (6, True, "hinerv", "bit=6 mode=hinerv")
    with pytest.raises(ValueError, match="Wrong rounding mode"):
        QATQuantizer(UniformAffineQuantizer(n_bits=6), w)(w)          # the constructor's default is no mode, as in the reference
    with pytest.raises(RuntimeError):
        q(w)                                                           # a CPU tensor: no fallback


def test_trainer_flags():
    from neuroquant_amd.methods import regress
    args = regress.parse_args(["--arch", "hnerv"])
    assert (args.qat, args.qat_bits, args.qat_seed) == (None, 8, 0)
    assert regress.build_model(args, TINY_HNERV, "cpu").weight_qat is None      # no quantiser without --qat
    args = regress.parse_args(["--arch", "nerv", "--qat", "hinerv", "--qat_bits", "5", "--qat_seed", "7"])
    model = regress.build_model(args, TINY_NERV, "cpu")
    hook = model.weight_qat
    assert (hook.mode, hook.bits, hook.seed) == ("hinerv", 5, 7) and not any("qat" in k for k in model.state_dict())
    with pytest.raises(SystemExit):
        regress.parse_args(["--arch", "nerv", "--qat", "lsq"])
    with pytest.raises(ValueError):
        regress.build_model(regress.parse_args(["--arch", "nerv", "--qat", "ffnerv", "--qat_bits", "9"]), TINY_NERV, "cpu")
    with pytest.raises(RuntimeError):
        model(torch.zeros(1))                                                   # the hook has no CPU path either


@pytest.mark.parametrize("bits", [2, 4, 8])
def test_ffnerv_restatement_stays_under_the_excuse_cap(bits):
    """float32 numpy against float64 at the GPU test's distribution: the share of elements a discontinuity of floor excuses"""
    w = (0.5 * np.random.default_rng(11).standard_normal((400, 500))).astype(np.float32)
    assert R.ffnerv_excused(R.ffnerv(w, bits, np.float32)[0], w, bits) <= 1e-3

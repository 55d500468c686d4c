"""Unit-wise reconstruction without a GPU: the restatement against the reference's own LossFunction values, and
the argument rules of the new entries and of their ops wrappers, which hold before any device is touched."""
import ctypes

import pytest
import torch

import unit_rec_ref as UR


@pytest.mark.parametrize("key,mode,p", [("mse/2", "lp", 2.0), ("mse/1", "lp", 1.0), ("mse/2.4", "lp", 2.4),
                                        ("fisher_diag", "fisher_diag", 2.0), ("fisher_full", "fisher_full", 2.0)])
def test_restatement_is_the_reference_loss(golden, key, mode, p):
    z = golden("unit_rec.npz")
    pred, tgt, grad = (torch.from_numpy(z[k]) for k in ("pred", "tgt", "grad"))
    assert float(UR.loss(pred, tgt, mode, p, grad)) == pytest.approx(float(z[key]), rel=1e-6)


def _unit(lib, **kw):
    a = dict(pred=64, tgt=64, fisher=64, idx=None, z=None, loss=64, dconv=128, ws=64, B=2, C=3, H=5, W=7, r=2, mode=0, p=2.0)
    a.update(kw)
    return lib.nq_unit_rec_loss(a["pred"], a["tgt"], a["fisher"], a["idx"], a["z"], a["loss"], a["dconv"], a["ws"], a["B"], a["C"],
                                a["H"], a["W"], a["r"], a["mode"], a["p"], None)


@pytest.mark.parametrize("bad", [dict(pred=None), dict(tgt=None), dict(loss=None), dict(dconv=None), dict(ws=None), dict(ws=68),
                                 dict(B=0), dict(H=-1), dict(W=0), dict(r=0), dict(r=6), dict(mode=3), dict(p=0.5),
                                 dict(p=float("nan")), dict(mode=1, fisher=None), dict(mode=2, fisher=None), dict(dconv=64),
                                 dict(B=1 << 16, C=1 << 16, H=1, W=1)])   # the last: 2^32 workgroups, unsupported
def test_unit_rec_entry_refuses(bad):
    from neuroquant_amd import _lib as L
    assert _unit(L.lib(), **bad) == (-2 if "C" in bad else -1)
    assert L.lib().nq_unit_rec_loss_ws_floats(2, 3, 5, 7, 6) == 0 and L.lib().nq_unit_rec_loss_ws_floats(2, 3, 5, 7, 2) > 0


@pytest.mark.parametrize("bad,rc", [(dict(xq=None), -1), (dict(idx=None), -1), (dict(x=None), -1), (dict(B=0), -1), (dict(n=0), -1),
                                    (dict(prob=-0.1), -1), (dict(prob=float("nan")), -1), (dict(xfp=None), -1), (dict(step=None), -1),
                                    (dict(B=65536), -2)])
def test_qdrop_entry_refuses(bad, rc):
    from neuroquant_amd import _lib as L
    a = dict(xq=64, xfp=64, idx=64, x=128, B=2, n=10, prob=0.5, step=64)
    a.update(bad)
    assert L.lib().nq_qdrop_mix(a["xq"], a["xfp"], a["idx"], a["x"], a["B"], a["n"], a["prob"], ctypes.c_uint64(1), a["step"], None) == rc


def test_ops_refuse_before_any_launch():
    from neuroquant_amd import ops
    t = torch.zeros(2, 3, 4, 4)
    for call in (lambda: ops.unit_rec_loss(None, t), lambda: ops.qdrop_mix(t, t, torch.zeros(2, dtype=torch.int64), 0.5),
                 lambda: ops.qdrop_mix(t, t, torch.zeros(2, dtype=torch.int64), -1.0),
                 lambda: ops.qdrop_mix(t, t, torch.zeros(2, dtype=torch.int64), 0.5, seed=-1)):
        with pytest.raises(ValueError):
            call()
    # every value rule is checked before the device rule: a CPU tensor reaches each of them
    idx = torch.zeros(2, dtype=torch.int64)
    for kw, why in ((dict(), "on the GPU"), (dict(mode="l2"), "mode must be"), (dict(p=0.5), "p must be"), (dict(r=3), "r must be"),
                    (dict(r=0), "r must be"), (dict(mode="fisher_diag"), "fisher weights"), (dict(z=t[:1]), "and z"),
                    (dict(idx=idx.int()), "with idx"), (dict(tgt=t[:, :2]), "differ"), (dict(idx=idx), "on the GPU")):
        with pytest.raises(ValueError, match=why):
            ops.unit_rec_loss(t, **{**dict(tgt=t, mode="lp", p=2.0, r=2), **kw})


@pytest.mark.parametrize("name", ["block_reconstruction", "layer_reconstruction"])
def test_reconstruction_signatures_are_the_reference(name):
    import inspect
    from neuroquant_amd import quantization
    sig = inspect.signature(getattr(quantization, name)).parameters
    assert list(sig)[:3] == ["model", name.split("_")[0], "cali_data"]
    assert {k: v.default for k, v in list(sig.items())[3:]} == dict(
        batch_size=8, iters=20000, weight=0.01, opt_mode="mse", asym=False, b_range=(20, 2), warmup=0.0, input_prob=1.0, p=2.0, lr=0.0015)


def test_driver_flags_and_refusals():
    from neuroquant_amd.methods import calibrate_network as cn
    a = cn.parse_args("--granularity block --opt_mode fisher_diag --input_prob 0.5 --asym".split())
    assert (a.granularity, a.opt_mode, a.input_prob, a.asym) == ("block", "fisher_diag", 0.5, True)
    d = cn.parse_args([])
    assert (d.granularity, d.asym) == ("network", False)
    for bad in ("--hadamard", "--rec_loss ssim", "--rec_weights 0.5 0.5", "--rec_ms_weights 0.5 0.5", "--loss_domain yuv420",
                "--rate_lambda 0.1", "--opt_mode fisher_full --norm_p 1", "--opt_mode lp_norm"):
        for gran in ("block", "layer"):
            with pytest.raises(ValueError, match="--granularity " + gran):
                cn.parse_args(f"--granularity {gran} {bad}".split())
        cn.parse_args(bad.split())     # --granularity network takes the flags as it did

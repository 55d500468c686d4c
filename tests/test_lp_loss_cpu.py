"""The absolute-error loss without a GPU: what nq_lp_loss refuses before it touches the device, the checks of
ops.lp_loss_args, and how the 'lp' objective is reached: model_reconstruction(p=), --norm_p, a trainer config's `loss: lp`."""
import ctypes

import pytest

from conftest import TINY_HNERV

NAN, INF = float("nan"), float("inf")
ONE = ctypes.c_void_p(64)                # a non-null pointer: a refused call never reads it
GOOD = dict(pred=ONE, tgt=ONE, cache=None, idx=None, loss3=ONE, grad=ONE, db=None, ws=ONE, B=2, C=3, H=5, W=7, p=1.0, w_abs=1.0,
            w_mse=0.0, scale=1.0, accumulate=0)
REFUSED = [dict(pred=None), dict(loss3=None), dict(ws=None), dict(tgt=None), dict(cache=ONE, idx=ONE), dict(tgt=None, cache=ONE),
           dict(db=ONE, grad=None), dict(db=ONE, grad=None, accumulate=1), dict(B=0), dict(C=-1), dict(H=0), dict(W=0),
           dict(p=0.5), dict(p=NAN), dict(p=INF), dict(w_abs=-1.0), dict(w_mse=-0.5), dict(w_abs=NAN), dict(w_mse=INF),
           dict(w_abs=0.0, w_mse=0.0), dict(scale=INF), dict(scale=NAN), dict(B=2 ** 31 - 1, C=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1)]


@pytest.mark.parametrize("change", REFUSED, ids=lambda c: " ".join(f"{k}={v if not isinstance(v, ctypes.c_void_p) else 'ptr'}" for k, v in c.items()))
def test_c_entry_refuses_before_the_device_is_touched(change):
    from neuroquant_amd import _lib as L
    a = dict(GOOD, **change)
    rc = L.lib().nq_lp_loss(a["pred"], a["tgt"], a["cache"], a["idx"], a["loss3"], a["grad"], a["db"], a["ws"], a["B"], a["C"], a["H"],
                            a["W"], a["p"], a["w_abs"], a["w_mse"], a["scale"], a["accumulate"], None)
    assert rc == -1 and b"invalid" in L.lib().nq_error_string(rc).lower()


def test_workspace_size_and_exports():
    from neuroquant_amd import _lib as L, ops
    K = ops.LP_LOSS_CHUNK
    q = L.lib().nq_lp_loss_ws_floats
    assert (q(1, 1, 1, 1), q(2, 3, 1, K), q(2, 3, 1, K + 1), q(2, 3, 640, 1280), q(0, 3, 4, 4)) == (3, 18, 36, 3 * 1200, 0)
    assert {"nq_lp_loss", "nq_lp_loss_ws_floats"} <= set(L.EXPORTS) and L.lib().nq_abi_version() == 7


@pytest.mark.parametrize("bad", [dict(p=0.99), dict(p=NAN), dict(p=INF), dict(p=None), dict(w_abs=-1.0), dict(w_abs=0.0, w_mse=0.0),
                                 dict(w_mse=NAN), dict(pred_shape=(2, 3, 4)), dict(pred_shape=(2, 0, 4, 4)), dict(tgt_shape=(2, 3, 4, 5))],
                         ids=str)
def test_args_and_objective_refuse_with_value_error(bad):
    from neuroquant_amd import objective, ops
    a = dict(dict(pred_shape=(2, 3, 4, 4), tgt_shape=(2, 3, 4, 4), p=1.0, w_abs=1.0, w_mse=0.0), **bad)
    with pytest.raises(ValueError, match="here"):
        ops.lp_loss_args("here", *a.values())
    if not {"pred_shape", "tgt_shape"} & set(bad):
        with pytest.raises(ValueError):
            objective.resolve("lp", bad)
    assert ops.lp_loss_args("here", (1, 1, 1, 1), (1, 1, 1, 1), 1, 1, 0) == (1.0, 1.0, 0.0)


def test_how_the_lp_objective_is_reached():
    from neuroquant_amd import objective, ops
    from neuroquant_amd.methods import calibrate_network as cn
    from neuroquant_amd.methods import regress
    from neuroquant_amd.quantization import model_reconstruction
    base = ["--arch", "hnerv", "--synthetic", "4"]
    before = ops.lp_loss_launches
    lp = lambda p, w_abs=1.0, w_mse=0.0: dict(p=p, w_abs=w_abs, w_mse=w_mse)
    # the engine's p= and the driver's --norm_p: 2 is the squared error as before, any other p >= 1 is 'lp' with (p, 1, 0)
    assert objective.from_kwargs().name == objective.from_kwargs(p=2.0).name == cn.objective_of(cn.parse_args(base)).name == "l2"
    for p in (1.0, 1.5, 3.5):
        for obj in (objective.from_kwargs(p=p), cn.objective_of(cn.parse_args(base + ["--norm_p", str(p)]))):
            assert (obj.name, obj.params) == ("lp", lp(p)) and obj.entry["lp_mul"](3) == 3 and obj.entry["step_div"] is None
            assert obj.engine_kwargs() == dict(loss_domain="rgb", yuv=None, ssim=None, msssim=None)     # p travels as p=
        assert objective.of_params(lp(p)).name == "lp"
    with pytest.raises(ValueError, match="singular"):
        model_reconstruction(None, cali_data=None, gt=[], p=0.5)
    with pytest.raises(AttributeError):                              # past its checks: it stops at the model it was not given
        model_reconstruction(None, cali_data=None, gt=[], p=1.0)
    for kw in (dict(ssim=dict(w_mse=0.7, w_ssim=0.3)), dict(msssim=dict(w_mse=0.7, w_ms=0.3)), dict(loss_domain="yuv420")):
        assert objective.from_kwargs(p=2.0, **kw).name != "lp"       # the old keyword forms resolve as before
        with pytest.raises(ValueError, match="combine"):
            model_reconstruction(None, cali_data=None, gt=[], p=1.0, **kw)
    for flags in (["--rec_loss", "Fusion5"], ["--rec_weights", "1", "1"], ["--rec_ms_weights", "1", "1"], ["--loss_domain", "yuv420"]):
        with pytest.raises(ValueError, match="combine"):
            cn.objective_of(cn.parse_args(base + ["--norm_p", "1"] + flags))
    with pytest.raises(ValueError, match="singular"):
        cn.objective_of(cn.parse_args(base + ["--norm_p", "0.5"]))
    # the trainer: `loss: lp` with the reference's weights of l1, Fusion7 and Fusion8 (utils.py:117-136)
    rargs = regress.parse_args(base)
    for cfg, want in ((dict(), lp(1.0)), (dict(loss_weights=[0.3, 0.7]), lp(1.0, 0.3, 0.7)), (dict(loss_weights=[0.5, 0.5]), lp(1.0, 0.5, 0.5)),
                      (dict(loss_p=1.5), lp(1.5))):
        params = regress.loss_params(rargs, dict(TINY_HNERV, loss="lp", **cfg))
        assert params == want and objective.of_params(params).name == "lp"
    for cfg in (dict(loss_p=0.5), dict(loss_weights=[1.0]), dict(loss_weights=[0.0, 0.0])):
        with pytest.raises(ValueError):
            regress.loss_params(rargs, dict(TINY_HNERV, loss="lp", **cfg))
    assert ops.lp_loss_launches == before

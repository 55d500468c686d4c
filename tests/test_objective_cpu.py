"""The one table of reconstruction objectives (neuroquant_amd/objective.py) without a GPU: the engine's keywords,
the calibration driver's flags and a trainer config resolve to the same objective; every combination that is refused is refused
with ValueError before anything is launched; every objective combines with the rate term; the two scale factors of the table."""
import argparse

import pytest
import torch

from conftest import TINY_HNERV

BASE = ["--arch", "hnerv", "--synthetic", "4"]
YUV_FLAGS = ["--yuv_matrix", "bt601", "--yuv_range", "full", "--yuv_weights", "4", "1", "1"]
YUV = dict(matrix="bt601", full_range=True, weights=(4.0, 1.0, 1.0))
# name, parameters, model_reconstruction keywords, calibrate_network flags, regress flags, trainer config
CASES = [
    ("l2", {}, {}, [], [], dict(loss="l2")),
    ("yuv420", dict(matrix="bt709", full_range=False, weights=(6.0, 1.0, 1.0)), dict(loss_domain="yuv420"), ["--loss_domain", "yuv420"],
     [], dict(loss="yuv420")),
    ("yuv420", YUV, dict(loss_domain="yuv420", yuv=dict(YUV, weights=[4, 1, 1])), ["--loss_domain", "yuv420"] + YUV_FLAGS, YUV_FLAGS,
     dict(loss="yuv420")),
    ("yuv420", dict(YUV, matrix="bt709"), dict(loss_domain="yuv420", yuv=dict(full_range=True, weights=(4, 1, 1))),
     ["--loss_domain", "yuv420"] + YUV_FLAGS[2:], YUV_FLAGS[2:], dict(loss="yuv420")),
    ("ssim", dict(w_mse=0.0, w_ssim=1.0), dict(ssim=dict(w_mse=0, w_ssim=1)), ["--rec_loss", "ssim"], [], dict(loss="ssim")),
    ("ssim", dict(w_mse=0.7, w_ssim=0.3), dict(ssim=dict(w_mse=0.7, w_ssim=0.3)), ["--rec_loss", "Fusion5"], [], dict(loss="Fusion5")),
    ("ssim", dict(w_mse=0.3, w_ssim=0.7), dict(ssim=dict(w_ssim=0.7, w_mse=0.3)), ["--rec_weights", "0.3", "0.7"], [], dict(loss="Fusion1")),
    ("msssim", dict(w_mse=0.0, w_ms=1.0), dict(msssim=dict(w_mse=0.0, w_ms=1.0)), ["--rec_loss", "msssim"], [], dict(loss="msssim")),
    ("msssim", dict(w_mse=0.5, w_ms=0.25), dict(msssim=dict(w_mse=0.5, w_ms=0.25)), ["--rec_ms_weights", "0.5", "0.25"], [],
     dict(loss="msssim", loss_weights=[0.5, 0.25])),
]
IDS = [f"{c[0]}-{i}" for i, c in enumerate(CASES)]


@pytest.mark.parametrize("name,params,kwargs,flags,rflags,cfg", CASES, ids=IDS)
def test_three_ways_to_one_objective(name, params, kwargs, flags, rflags, cfg):
    from neuroquant_amd import objective
    from neuroquant_amd.methods import calibrate_network as cn
    from neuroquant_amd.methods import regress
    engine = objective.from_kwargs(**kwargs)
    driver = cn.objective_of(cn.parse_args(BASE + flags))
    rargs = regress.parse_args(BASE + rflags)
    trainer = objective.of_params(regress.loss_params(rargs, dict(TINY_HNERV, **cfg)))
    for obj in (engine, driver, trainer):
        assert isinstance(obj, objective.Objective) and obj.name == name and obj.params == params, (obj.name, obj.params)
        assert all(type(v) is float for k, v in obj.params.items() if k.startswith("w_"))
    assert objective.of_params(trainer) is trainer                                # a resolved objective passes through
    assert getattr(rargs, "loss_domain", "rgb") == ("yuv420" if name == "yuv420" else "rgb")
    # the driver hands the engine the keywords that resolve to the same objective again
    kw = driver.engine_kwargs()
    assert set(kw) == {"loss_domain", "yuv", "ssim", "msssim"} and sum(v is not None for v in kw.values()) == 1 + (name != "l2")
    back = objective.from_kwargs(**kw)
    assert (back.name, back.params) == (name, params)
    # and the views of the resolver the tests and tools read
    assert cn.rec_loss_params(cn.parse_args(BASE + flags)) == (params if name == "ssim" else None)
    assert cn.rec_msssim_params(cn.parse_args(BASE + flags)) == (params if name == "msssim" else None)


@pytest.mark.parametrize("name,params,kwargs,flags,rflags,cfg", CASES, ids=IDS)
def test_every_objective_takes_the_rate_term(name, params, kwargs, flags, rflags, cfg):
    from neuroquant_amd import objective
    from neuroquant_amd.methods import calibrate_network as cn
    from neuroquant_amd.quantization import model_reconstruction
    rate = dict(weight=2, pixels=8 * 320 * 640)
    assert objective.from_kwargs(**kwargs).name == name
    assert objective.rate_kwarg(rate) == dict(weight=2.0, pixels=8 * 320 * 640) and objective.rate_kwarg(None) is None
    args = cn.parse_args(BASE + flags + ["--rate_lambda", "2"])
    assert cn.objective_of(args).name == name and cn.rate_params(args, 8 * 320 * 640) == rate
    # the engine accepts the pair: it gets past its checks and stops at the model it was not given
    with pytest.raises(AttributeError):
        model_reconstruction(None, cali_data=None, gt=[], rate=rate, **kwargs)


SSIM, MS = dict(w_mse=0.7, w_ssim=0.3), dict(w_mse=0.7, w_ms=0.3)
NAN, INF = float("nan"), float("inf")
BAD_ENGINE = [
    # what does not combine
    dict(loss_domain="yuv420", ssim=SSIM), dict(loss_domain="yuv420", msssim=MS), dict(ssim=SSIM, msssim=MS),
    dict(loss_domain="yuv420", ssim=SSIM, msssim=MS), dict(loss_domain="yuv444"), dict(loss_domain=None),
    # bad keys, for each of the four dicts
    dict(yuv=dict(colour="bt709")), dict(loss_domain="yuv420", yuv=dict(matrix="bt709", w_mse=1.0)),
    dict(ssim=dict(w_mse=0.7)), dict(ssim=dict(SSIM, w_l1=1.0)), dict(ssim=MS), dict(ssim=(0.7, 0.3)), dict(ssim={}),
    dict(msssim=dict(w_ms=0.3)), dict(msssim=dict(MS, w_l1=1.0)), dict(msssim=SSIM), dict(msssim=(0.7, 0.3)), dict(msssim={}),
    dict(rate=dict(weight=1.0)), dict(rate=dict(pixels=100)), dict(rate=dict(weight=1.0, pixels=100, extra=1)), dict(rate=(1.0, 100)),
    dict(rate=1.0),
    # bad weights (and the other bad values), for each of the four dicts
    dict(loss_domain="yuv420", yuv=dict(weights=(1, 1))), dict(loss_domain="yuv420", yuv=dict(weights=(-1, 1, 1))),
    dict(loss_domain="yuv420", yuv=dict(weights=(0, 0, 0))), dict(loss_domain="yuv420", yuv=dict(weights=(NAN, 1, 1))),
    dict(loss_domain="yuv420", yuv=dict(weights=(1, 1, INF))), dict(loss_domain="yuv420", yuv=dict(weights=None)),
    dict(loss_domain="yuv420", yuv=dict(matrix="bt2020")),
    dict(ssim=dict(w_mse=-1.0, w_ssim=1.0)), dict(ssim=dict(w_mse=0.0, w_ssim=0.0)), dict(ssim=dict(w_mse=NAN, w_ssim=1.0)),
    dict(ssim=dict(w_mse=1.0, w_ssim=INF)), dict(ssim=dict(w_mse=None, w_ssim=1.0)),
    dict(msssim=dict(w_mse=-1.0, w_ms=1.0)), dict(msssim=dict(w_mse=0.0, w_ms=0.0)), dict(msssim=dict(w_mse=NAN, w_ms=1.0)),
    dict(msssim=dict(w_mse=1.0, w_ms=INF)), dict(msssim=dict(w_mse=None, w_ms=1.0)),
    dict(rate=dict(weight=-1.0, pixels=100)), dict(rate=dict(weight=NAN, pixels=100)), dict(rate=dict(weight=INF, pixels=100)),
    dict(rate=dict(weight=None, pixels=100)), dict(rate=dict(weight=1.0, pixels=0)), dict(rate=dict(weight=1.0, pixels=-3)),
    dict(rate=dict(weight=1.0, pixels=1.5)), dict(rate=dict(weight=1.0, pixels=True)),
]


@pytest.mark.parametrize("kwargs", BAD_ENGINE, ids=lambda kw: " ".join(f"{k}={v}" for k, v in kw.items())[:70])
def test_engine_refuses_before_anything_is_launched(kwargs):
    """model=None: a call that got past its checks would fail with AttributeError, not ValueError"""
    from neuroquant_amd import objective, ops
    from neuroquant_amd.quantization import model_reconstruction
    before = (ops.yuv420_loss_launches, ops.ssim_loss_head_launches, ops.msssim_loss_head_launches, ops.level_rate_launches)
    with pytest.raises(ValueError):
        model_reconstruction(None, cali_data=None, gt=[], **kwargs)
    with pytest.raises(ValueError):
        kw = dict(kwargs)
        rate = kw.pop("rate", None)
        objective.from_kwargs(**kw)
        objective.rate_kwarg(rate)
        raise AssertionError("neither the objective nor the rate term was refused")
    assert before == (ops.yuv420_loss_launches, ops.ssim_loss_head_launches, ops.msssim_loss_head_launches, ops.level_rate_launches)


def _flags(**kw):
    """the attributes parse_args leaves, set by hand: argparse itself refuses the flag pairs below with SystemExit"""
    return argparse.Namespace(**dict(dict(rec_loss="l2", rec_weights=None, rec_ms_weights=None, loss_domain="rgb", synthetic=4), **kw))


BAD_DRIVER = [
    # --rec_loss x --rec_weights x --rec_ms_weights, pairwise (and all three)
    dict(rec_loss="Fusion5", rec_weights=[0.7, 0.3]), dict(rec_loss="msssim", rec_weights=[0.7, 0.3]),
    dict(rec_loss="Fusion5", rec_ms_weights=[0.7, 0.3]), dict(rec_loss="msssim", rec_ms_weights=[0.7, 0.3]),
    dict(rec_weights=[1.0, 1.0], rec_ms_weights=[1.0, 1.0]), dict(rec_loss="ssim", rec_weights=[1.0, 1.0], rec_ms_weights=[1.0, 1.0]),
    # the objectives defined on RGB frames x --loss_domain yuv420
    dict(rec_loss="ssim", loss_domain="yuv420"), dict(rec_loss="Fusion1", loss_domain="yuv420"), dict(rec_weights=[0.5, 0.5], loss_domain="yuv420"),
    dict(rec_loss="msssim", loss_domain="yuv420"), dict(rec_ms_weights=[0.5, 0.5], loss_domain="yuv420"),
    # unknown names, bad weights
    dict(rec_loss="l1"), dict(rec_loss="Fusion6"), dict(rec_weights=[0.5]), dict(rec_weights=[0.5, 0.5, 0.5]), dict(rec_ms_weights=[0.5]),
    dict(rec_weights=[-1.0, 1.0]), dict(rec_weights=[0.0, 0.0]), dict(rec_weights=[NAN, 1.0]), dict(rec_weights=[1.0, INF]),
    dict(rec_ms_weights=[-1.0, 1.0]), dict(rec_ms_weights=[0.0, 0.0]), dict(rec_ms_weights=[NAN, 1.0]), dict(rec_ms_weights=[1.0, INF]),
    dict(loss_domain="yuv420", yuv_weights=[0.0, 0.0, 0.0]), dict(loss_domain="yuv420", yuv_weights=[-1.0, 1.0, 1.0]),
    dict(loss_domain="yuv420", yuv_matrix="bt2020"), dict(loss_domain="yuv420", yuv_range="studio"),
]


@pytest.mark.parametrize("kw", BAD_DRIVER, ids=lambda kw: " ".join(f"{k}={v}" for k, v in kw.items())[:70])
def test_driver_refuses_before_anything_is_launched(kw):
    from neuroquant_amd.methods import calibrate_network as cn
    with pytest.raises(ValueError):
        cn.objective_of(_flags(**kw))
    for view in (cn.rec_loss_params, cn.rec_msssim_params):                       # thin views: the resolver's refusals
        with pytest.raises(ValueError):
            view(_flags(**kw))


def test_driver_and_trainer_refusals_that_are_not_value_errors():
    from neuroquant_amd import objective
    from neuroquant_amd.methods import calibrate_network as cn
    from neuroquant_amd.methods import regress
    for pair in (["--rec_loss", "Fusion5", "--rec_weights", "0.7", "0.3"], ["--rec_loss", "msssim", "--rec_ms_weights", "0.7", "0.3"],
                 ["--rec_weights", "1", "1", "--rec_ms_weights", "1", "1"], ["--rec_loss", "l1"]):
        with pytest.raises(SystemExit):
            cn.parse_args(BASE + pair)
    with pytest.raises(ValueError):
        cn.parse_args(BASE + ["--rate_lambda", "-1"])
    rargs = regress.parse_args(BASE)
    for name in ("l1", "Fusion6", "nonsense"):
        with pytest.raises(NotImplementedError):
            regress.loss_params(rargs, dict(TINY_HNERV, loss=name))
    for bad in ([0.5], [0.0, 0.0], [-1.0, 1.0], "0.5 0.5", [NAN, 1.0]):
        with pytest.raises(ValueError):
            regress.loss_params(rargs, dict(TINY_HNERV, loss="msssim", loss_weights=bad))
    for bad in (dict(w_mse=1.0), dict(w_mse=1.0, w_ssim=1.0, w_ms=1.0), dict(weight=1.0, pixels=4), {}):
        with pytest.raises(ValueError):
            objective.of_params(bad)
    with pytest.raises(ValueError):
        objective.resolve("l1")
    with pytest.raises(ValueError):
        objective.resolve("l2", dict(w_mse=1.0))


# the two scale factors that exist (C = channels of the image): `lp` multiplies the ops loss in LossFunction (the scale of
# lp_loss), `step` divides it in regress.step_loss (the trainer's per-channel mean); None = the ops loss as it is
SCALES = {"l2": dict(lp=None, step="C"), "yuv420": dict(lp=None, step=3), "ssim": dict(lp="C", step=None), "msssim": dict(lp="C", step=None)}


@pytest.mark.parametrize("name", list(SCALES))
@pytest.mark.parametrize("C", [1, 3, 5])
def test_scale_factors(monkeypatch, name, C):
    from neuroquant_amd import objective
    from neuroquant_amd.methods import regress
    from neuroquant_amd.quantization.calib_model import LossFunction
    assert set(objective.TABLE) == set(SCALES)
    value = {"C": C, 3: 3, None: None}
    e = objective.TABLE[name]
    for key, want in (("lp_mul", SCALES[name]["lp"]), ("step_div", SCALES[name]["step"])):
        assert (None if e[key] is None else e[key](C)) == value[want], key
    # and through the three callers, on a stand-in for the ops loss (no kernel runs here)
    calls = []

    def fake(pred, tgt, **params):
        calls.append(params)
        return torch.tensor(6.0, dtype=torch.float64)

    monkeypatch.setitem(e, "loss", fake)
    obj = objective.resolve(name)
    x = torch.zeros(2, C, 4, 4)
    lp, step = (1 if v is None else value[v] for v in (SCALES[name]["lp"], SCALES[name]["step"]))
    assert float(obj.lp_loss(x, x)) == 6.0 * lp and float(obj.step_loss(x, x)) == 6.0 / step
    assert float(regress.step_loss(x, x, obj.params or None)) == 6.0 / step and float(regress.step_loss(x, x, obj)) == 6.0 / step
    assert calls == [obj.params] * 4
    if name != "l2":                                                              # LossFunction's 'mse' stays lp_loss(p)
        lf = LossFunction(None, round_loss="none", rec_loss=name)
        assert lf.obj.name == name and float(lf(x, x)) == 6.0 * lp
    with pytest.raises(NotImplementedError):
        LossFunction(None, round_loss="none", rec_loss="fisher_diag")(x, x)
    assert float(LossFunction(None, round_loss="none", rec_loss="mse", p=1.0)(torch.ones(2, C, 4, 4), x)) == float(C)


def test_what_only_l2_and_the_extra_figures_say():
    from neuroquant_amd import objective
    fused = {name: e["fused_head"] for name, e in objective.TABLE.items()}
    assert fused == dict(l2=True, yuv420=False, ssim=False, msssim=False)
    assert {name: e["excludes"] for name, e in objective.TABLE.items()} == dict(l2=(), yuv420=(), ssim=("yuv420",), msssim=("ssim", "yuv420"))
    assert objective.resolve("l2").log_line() is None and objective.resolve("l2").eval_report(None, torch.tensor(0.9)) == ({}, None)
    assert objective.resolve("yuv420").log_line() == ("reconstruction loss: YUV 4:2:0 plane MSEs, "
                                                      "{'matrix': 'bt709', 'full_range': False, 'weights': (6.0, 1.0, 1.0)}")
    assert objective.resolve("ssim", SSIM).log_line() == ("reconstruction loss: C * (w_mse * MSE + w_ssim * (1 - SSIM)), "
                                                          "{'w_mse': 0.7, 'w_ssim': 0.3}")
    assert objective.resolve("msssim", MS).log_line() == ("reconstruction loss: C * (w_mse * MSE + w_ms * (1 - MS-SSIM)), "
                                                          "{'w_mse': 0.7, 'w_ms': 0.3}")
    more, line = objective.resolve("ssim", SSIM).eval_report(torch.tensor([0.5, 1.0]))
    assert list(more) == [objective.SSIM_METRIC_NAME] and float(more[objective.SSIM_METRIC_NAME]) == 0.75
    assert line == "ssim objective {'w_mse': 0.7, 'w_ssim': 0.3}: SSIM 0.75"
    more, line = objective.resolve("yuv420").eval_report(torch.tensor([[40.0, 44.0, 48.0], [42.0, 46.0, 50.0]], dtype=torch.float64))
    assert list(more) == objective.YUV_METRIC_NAMES and [float(v) for v in more.values()] == [41.0, 45.0, 49.0, 42.5]
    assert line == "yuv420: PSNR-Y 41.0 U 45.0 V 49.0 | 6:1:1 42.5"
    ms = objective.resolve("msssim", MS)
    assert ms.eval_report(None, None) == ({}, None)                               # frames too small for five scales: no line
    assert ms.eval_report(None, torch.tensor(0.98766)) == ({}, "msssim objective (0.7, 0.3): MS-SSIM 0.9877")

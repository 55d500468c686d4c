"""CPU-side checks of the rate term: the restated gradient against float64 autograd, R_hard against the
histogram entropy, the C entries (whose argument checks run before the device is touched), ops, the engine's keyword and the
driver's flag."""
import ctypes
import os

import pytest
import torch

import rate_ref as R
from conftest import ROOT

CASES = [(1, 1, 4, 0), (3, 5, 4, 1), (1, 257, 256, 0), (7, 1100, 256, 1), (7, 1100, 16, 1), (5, 300, 64, 0)]


def test_restated_gradient_equals_float64_autograd():
    for i, (rows, rl, K, per_row) in enumerate(CASES):
        t = R.make_tensor(rows, rl, K, per_row, seed=10 + i)
        du, dl = R.margins(t)
        assert du >= 0.04 and dl >= 1e-4
        for scale in (1.0, 0.37):
            ref = R.rate(t["x"], t["alpha"], t["delta"], t["zp"], K, scale=scale)
            r, g = R.rate_autograd(t["x"], t["alpha"], t["delta"], t["zp"], K, scale=scale)
            assert abs(float(r - ref["r_soft"])) <= 1e-12 * max(1.0, abs(float(r)))
            assert float((g - ref["grad"]).abs().max()) <= 1e-12
        if rows * rl > 100:
            assert float(ref["grad"].abs().max()) > 1e-3               # and there is a gradient to compare


def test_soft_rate_equals_hard_rate_at_hard_targets():
    t = R.make_tensor(7, 1100, 16, 1, seed=3, kind="alpha_30")
    ref = R.rate(t["x"], t["alpha"], t["delta"], t["zp"], 16)
    assert abs(float(ref["r_soft"] - ref["r_hard"])) <= 1e-9 * float(ref["r_hard"])
    assert float(ref["grad"].abs().max()) == 0.0


def test_hard_rate_is_at_least_the_histogram_entropy():
    from neuroquant_amd.export import _entropy_bits
    for i, (rows, rl, K, per_row) in enumerate(CASES):
        for kind in ("generic", "one_level", "clamped"):
            t = R.make_tensor(rows, rl, K, per_row, seed=20 + i, kind=kind)
            lv = R.hard_levels(t["x"], t["alpha"], t["delta"], t["zp"], K)
            ref = R.rate(t["x"], t["alpha"], t["delta"], t["zp"], K)
            assert int(ref["counts"].sum()) == rows * rl
            ent = _entropy_bits(lv.to(torch.uint8), K)
            assert abs(ent - R.entropy_bits(lv, K)) <= 1e-9 * max(1.0, ent)
            assert float(ref["r_hard"]) >= ent - 1e-9                   # a code for another distribution is never shorter


def test_entries_are_declared_exported_and_bound():
    from neuroquant_amd import _lib
    header = open(os.path.join(ROOT, "include", "nq_hip.h")).read()
    lib = _lib.lib()
    for name in ("nq_level_rate_ws_words", "nq_level_rate"):
        assert f" {name}(" in header and name in _lib.EXPORTS
        assert getattr(lib, name).argtypes                            # bound with a signature
    assert "nq_rate_seg" in header and ctypes.sizeof(_lib.RateSeg) == 8 * 8 + 2 * 8 + 2 * 4
    assert lib.nq_abi_version() == 7 == _lib.ABI_VERSION


def _ws_formula(n, K):
    """the header's workspace formula"""
    return -(-n // 4096) * (K + 1)


def test_workspace_query_is_its_formula():
    from neuroquant_amd import _lib
    lib = _lib.lib()
    for n, K in [(1, 4), (15, 4), (257, 256), (4096, 16), (4097, 16), (7700, 256), (848 * 64 * 25, 16), (2 ** 40 + 1, 256), (2 ** 63 - 1, 256)]:
        assert lib.nq_level_rate_ws_words(n, K) == _ws_formula(n, K), (n, K)
    for n, K in [(0, 16), (-5, 16), (100, 3), (100, 257), (100, 0), (100, -4)]:
        assert lib.nq_level_rate_ws_words(n, K) == 0, (n, K)


def test_c_entry_rejects_bad_arguments_without_a_gpu():
    from neuroquant_amd import _lib
    lib = _lib.lib()
    p, n = 16, None
    INVALID = -1

    def seg(**kw):
        f = dict(x=p, alpha=p, delta=p, zp=p, dalpha=p, counts=p, cost=p, rate=p, rows=3, row_len=5, per_row=1, n_levels=16)
        f.update(kw)
        s = _lib.RateSeg()
        for k, v in f.items():
            setattr(s, k, v)
        return s

    def call(segs=None, nseg=None, scale=1.0, total=ctypes.c_void_p(p), ws=ctypes.c_void_p(p), words=1 << 20):
        segs = [seg()] if segs is None else segs
        arr = (_lib.RateSeg * max(len(segs), 1))(*segs)
        return lib.nq_level_rate(arr, len(segs) if nseg is None else nseg, scale, n, total, ws, words, n)

    assert lib.nq_level_rate(None, 1, 1.0, n, ctypes.c_void_p(p), ctypes.c_void_p(p), 100, n) == INVALID
    for kw in (dict(nseg=0), dict(nseg=-2), dict(total=n), dict(ws=n), dict(words=0), dict(words=16)):   # 3 x 5 at K = 16 needs 17 words
        assert call(**kw) == INVALID, kw
    nan, inf = float("nan"), float("inf")
    for scale in (-1.0, -1e-30, nan, inf, -inf):
        assert call(scale=scale) == INVALID, scale
    for name in ("x", "alpha", "delta", "zp", "counts", "cost", "rate"):
        assert call(segs=[seg(**{name: None})]) == INVALID, name
    for kw in (dict(rows=0), dict(rows=-1), dict(row_len=0), dict(row_len=-7), dict(row_len=2 ** 31), dict(n_levels=3), dict(n_levels=257),
               dict(n_levels=0), dict(n_levels=2), dict(rows=2 ** 62, row_len=4), dict(rows=2 ** 40, row_len=2 ** 30)):
        assert call(segs=[seg(**kw)]) == INVALID, kw
    # the 17th tensor of a list is checked before the first launch too (a table holds 16)
    assert call(segs=[seg()] * 16 + [seg(n_levels=3)]) == INVALID
    assert call(segs=[seg()] * 16 + [seg(alpha=None)]) == INVALID
    # a workspace that fits one tensor but not two
    assert call(segs=[seg(), seg()], words=17) == INVALID
    # tensors whose workspaces do not fit int64 together
    big = seg(rows=2 ** 31, row_len=2 ** 31 - 1, n_levels=256)
    assert call(segs=[big] * 16, words=2 ** 62) == INVALID


def test_ops_check_arguments_before_any_launch():
    from neuroquant_amd import ops
    x, a, d, z = torch.zeros(3, 5), torch.zeros(3, 5), torch.ones(3), torch.zeros(3)
    before = ops.level_rate_launches
    for scale in (-1.0, float("nan"), float("inf"), None, "x"):
        with pytest.raises(ValueError):
            ops.level_rate_raw([(x, a, d, z, 16)], scale)
    for K in (3, 257, 0, 16.0, None):
        with pytest.raises(ValueError):
            ops.level_rate_raw([(x, a, d, z, K)], 1.0)
    with pytest.raises(ValueError):
        ops.level_rate_raw([], 1.0)
    with pytest.raises(ValueError):
        ops.level_rate_raw([(x, a, d, z)], 1.0)
    with pytest.raises(ValueError):
        ops.level_rate_raw([(x, a, d, z, 16)], 1.0, dalphas=[])
    for w, px in ((-1.0, 100), (float("nan"), 100), (1.0, 0), (1.0, -5), (1.0, 2.5), (1.0, None)):
        with pytest.raises(ValueError):
            ops.level_rate([(x, a, d, z, 16)], w, px)
    with pytest.raises(RuntimeError):
        ops.level_rate_raw([(x, a, d, z, 16)], 1.0)                    # CPU tensors: no fallback
    with pytest.raises(RuntimeError):
        ops.level_rate([(x, a, d, z, 16)], 1.0, 100, dalphas=[torch.zeros(3, 5)])
    assert ops.level_rate_launches == before
    assert ops.LEVEL_RATE_LAUNCHES == 4


def test_engine_keyword_is_checked_before_the_first_iteration():
    from neuroquant_amd.quantization import model_reconstruction
    for bad in (dict(weight=1.0), dict(pixels=100), dict(weight=1.0, pixels=100, extra=1), dict(weight=-1.0, pixels=100),
                dict(weight=float("nan"), pixels=100), dict(weight=float("inf"), pixels=100), dict(weight=None, pixels=100),
                dict(weight=1.0, pixels=0), dict(weight=1.0, pixels=-3), dict(weight=1.0, pixels=1.5), dict(weight=1.0, pixels=True),
                (1.0, 100), 1.0):
        with pytest.raises(ValueError):
            model_reconstruction(None, cali_data=None, gt=[], rate=bad)


def test_driver_flag():
    from neuroquant_amd.methods import calibrate_network as cn
    base = ["--arch", "hnerv"]
    dflt = cn.parse_args(base)
    assert dflt.rate_lambda == 0.0 and cn.rate_params(dflt, 1000) is None
    args = cn.parse_args(base + ["--rate_lambda", "2.5", "--rec_loss", "msssim", "--hadamard", "--embed_bits", "6"])
    assert cn.rate_params(args, 8 * 320 * 640) == dict(weight=2.5, pixels=8 * 320 * 640)
    args = cn.parse_args(base + ["--rate_lambda", "1e3", "--loss_domain", "yuv420"])
    assert cn.rate_params(args, 10) == dict(weight=1000.0, pixels=10)
    with pytest.raises(ValueError):
        cn.parse_args(base + ["--rate_lambda", "-1"])
    for bad in ("-0.5", "nan", "inf", "-inf"):
        with pytest.raises(ValueError):
            cn.parse_args(base + ["--rate_lambda=" + bad])

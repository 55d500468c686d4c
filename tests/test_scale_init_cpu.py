"""CPU-side checks of scale init by search: the numpy restatement of the definition (tests/scale_init_ref.py)
against what the real reference returned (tests/golden/scale_init.npz, written by tests/golden/make_scale_init.py), the three
C entries' argument checks (which run before the device is touched), the binding and the dispatcher's refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

import scale_init_ref as S
from conftest import ROOT

def test_restatement_equals_the_reference(golden):
    z = golden("scale_init.npz")
    assert 0 < float(z["gaussian_delta_rel"]) < 4 * 2.0 ** -24         # the fp32 moments of the reference, not a loose bound
    S.check_against_fixture(z, S.scale_init)


def test_search_clips_at_low_widths_and_keeps_the_range_at_eight_bits(golden):
    """The reason for the feature: on weight rows the search leaves the full range at 2-4 bits."""
    z = golden("scale_init.npz")
    x2, _ = S.rows_of(z["w144"], True)
    for method in ("mse", "l1"):
        assert (S.search(x2, 16, S.P[method])[0] > 0).mean() > 0.5
        assert (S.search(x2, 256, S.P[method])[0] == 0).all()


def test_rows_without_a_winner_and_known_answers():
    x = S.make_rows(4, 30, seed=1)
    x[1, 7], x[2, 3] = np.nan, np.inf
    choice, d, zp, s = S.search(x, 16, 3.5)
    assert choice[1] == -1 and choice[2] == -1 and choice[0] >= 0 and choice[3] >= 0
    assert np.isnan(d[1]) and np.isnan(zp[2]) and np.isfinite(d[[0, 3]]).all()
    rows = S.constructed_rows(65, seed=2)
    choice, d, zp, s = S.search(rows, 16, 1.0)
    assert s[0].max() == 0.0 and choice[0] == 0 and d[0] == np.float32(1e-8) and zp[0] == 0   # zeros: all score 0, the first wins
    assert choice[1] == 0 and d[1] == np.float32(1e-8)     # a constant row: an empty range, the floor of delta
    gd, gz, st, _ = S.gaussian(rows, 16)
    assert st[1, 1] == 0.0 and st[1, 0] == np.float32(0.37) and gd[1] == np.float32(np.float32(0.37) / np.float32(15))
    assert np.isnan(S.gaussian(np.ones((1, 1), np.float32), 16)[0][0])      # one element: no variance, as the reference


def test_an_outlier_a_hundred_times_the_rest_makes_the_search_leave_candidate_0():
    """The constructed outlier row at 4 levels: the restatement leaves the full range at the lengths scale_init_ref lists (its
    comment says why the full range misses the outlier), for both p, and keeps it at the four short lengths."""
    for n in S.OUTLIER_CLIPS_AT_4_LEVELS + S.OUTLIER_STAYS_AT_4_LEVELS:
        row = S.constructed_rows(n, seed=n)[S.OUTLIER]
        if n > 1:
            rest = np.delete(np.abs(row), n // 2).mean()
            assert 90 * rest < row[n // 2] < 110 * rest                 # a hundred times the rest
        for p in (3.5, 1.0):
            win, d, zp, s, cands = S.search_row(row, 4, p)
            assert (win > 0) == (n in S.OUTLIER_CLIPS_AT_4_LEVELS), (n, p, win)
            if win > 0:
                assert s[win] < s[0] and d == cands[win][0] and d < cands[0][0]     # a strictly better, shorter range


def test_entries_are_declared_exported_and_bound():
    from neuroquant_amd import _lib
    header = open(os.path.join(ROOT, "include", "nq_hip.h")).read()
    lib = _lib.lib()
    for name in ("nq_scale_init_search", "nq_scale_init_gaussian", "nq_scale_init_ws_bytes"):
        assert f" {name}(" in header and name in _lib.EXPORTS
        assert getattr(lib, name).argtypes
    assert lib.nq_abi_version() == 7 == _lib.ABI_VERSION


def test_workspace_query_is_its_formula():
    from neuroquant_amd import _lib
    lib = _lib.lib()
    for rows, rl in [(1, 1), (300, 27), (5, 512), (5, 513), (2, 8192), (10 ** 6, 8192)]:
        assert lib.nq_scale_init_ws_bytes(rows, rl) == 16, (rows, rl)             # a token: rows that are not cut
    for rows, rl in [(2, 8193), (1, 70001), (1, 848 * 64 * 25), (7, 3 * 8192)]:
        assert lib.nq_scale_init_ws_bytes(rows, rl) == rows * -(-rl // 8192) * 88, (rows, rl)
    for rows, rl in [(0, 5), (-1, 5), (5, 0), (5, -3), (2 ** 62, 4), (2 ** 40, 2 ** 30), (2 ** 26 + 1, 27), (2 ** 24, 600), (1, 2 ** 40)]:
        assert lib.nq_scale_init_ws_bytes(rows, rl) == -1, (rows, rl)


def test_c_entries_reject_bad_arguments_without_a_gpu():
    from neuroquant_amd import _lib
    lib = _lib.lib()
    p, n = ctypes.c_void_p(16), None
    INVALID = -1

    def search(x=p, rows=3, row_len=5, K=16, pw=3.5, delta=p, zp=p, choice=p, scores=p, ws=p):
        return lib.nq_scale_init_search(x, rows, row_len, K, pw, delta, zp, choice, scores, ws, n)

    def gauss(x=p, rows=3, row_len=5, K=16, delta=p, zp=p, stats=p, ws=p):
        return lib.nq_scale_init_gaussian(x, rows, row_len, K, delta, zp, stats, ws, n)

    for name in ("x", "delta", "zp", "choice", "ws"):
        assert search(**{name: n}) == INVALID, name
    for name in ("x", "delta", "zp", "ws"):
        assert gauss(**{name: n}) == INVALID, name
    sizes = (dict(rows=0), dict(rows=-1), dict(row_len=0), dict(row_len=-7), dict(K=1), dict(K=0), dict(K=-4), dict(K=65537),
             dict(rows=2 ** 62, row_len=4), dict(rows=2 ** 40, row_len=2 ** 30), dict(rows=2 ** 27, row_len=27),
             dict(rows=1, row_len=2 ** 40))
    for kw in sizes:
        assert search(**kw) == INVALID, kw
        assert gauss(**kw) == INVALID, kw
    for pw in (0.0, -1.0, float("nan"), float("inf")):
        assert search(pw=pw) == INVALID, pw


def test_ops_refuse_before_any_launch():
    from neuroquant_amd import ops
    from neuroquant_amd.quantization import UniformAffineQuantizer
    x = torch.zeros(4, 3, 3, 3)
    for method in ("l2", "lp", "", None, 3):
        with pytest.raises(NotImplementedError):
            ops.scale_init(x, 16, True, method)
    with pytest.raises(NotImplementedError):
        UniformAffineQuantizer(n_bits=4, channel_wise=True, scale_method="l2")(x)
    with pytest.raises(NotImplementedError):
        UniformAffineQuantizer(n_bits=4, symmetric=True, channel_wise=True, scale_method="mse")(x)
    for method in ("mse", "l1", "gaussian", "max"):
        with pytest.raises(RuntimeError):
            ops.scale_init(x, 16, True, method)                         # CPU tensors: no fallback
    for bad in (1, 0, 65537, 16.0, None, True):
        with pytest.raises(ValueError):
            ops.scale_init_search_raw(torch.zeros(3, 5), bad, 3.5)
        with pytest.raises(ValueError):
            ops.scale_init_gaussian_raw(torch.zeros(3, 5), bad)
    for bad in (0, -1.0, float("nan"), float("inf"), None, "2"):
        with pytest.raises(ValueError):
            ops.scale_init_search_raw(torch.zeros(3, 5), 16, bad)
    with pytest.raises(ValueError):
        ops.scale_init_search_raw(torch.zeros(15), 16, 3.5)
    assert ops.SCALE_SEARCH_P == S.P and ops.SCALE_CANDIDATES == S.NC

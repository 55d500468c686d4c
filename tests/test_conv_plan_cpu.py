"""Host-only checks behind tests/test_conv_variants.py: the tables of tests/conv_cases.py name every build of the exact-fp32
convolution family, the launch plans (nq_conv_forward_plan / nq_conv_wgrad_plan) really send each row to its build, every row and
the tables as a whole meet the conditions the GPU file relies on, the workspace and split-word queries follow from the same plans,
and plain float32 on the CPU lands well inside the bound on every row (a row on which it did not would say nothing about a kernel)."""
import ctypes
import os

import pytest

import conv_cases as C
from conv_cases import EXTRA_FWD_CASES, FWD_CASES, WGRAD_CASES, case_id

HEAD_ENV = ("NQ_HEAD_FWD", "NQ_HEAD_RD", "NQ_HEAD_DGRAD", "NQ_HEAD_DG_R")
ALL_FWD = FWD_CASES + EXTRA_FWD_CASES


@pytest.fixture(scope="module", autouse=True)
def untuned_environment():
    """the head's routes read these per call: with one of them set from outside, the table describes another library"""
    found = [v for v in HEAD_ENV if v in os.environ]
    assert not found, f"unset {', '.join(found)}: the launch plans read them, and the tables of tests/conv_cases.py set their own"


@pytest.fixture(scope="module")
def lib():
    from neuroquant_amd import _lib
    return _lib.lib()


def fwd_plan(lib, shape, epi, env, monkeypatch, rc_only=False):
    from neuroquant_amd import _lib
    B, cin, H, W, cout, k = shape
    with monkeypatch.context() as m:
        for n, v in env.items():
            m.setenv(n, v)
        q = _lib.ConvPlan()
        rc = lib.nq_conv_forward_plan(B, cin, H, W, cout, k, epi[1], C.EPI_CODE[epi[0]], int(epi[2]), ctypes.byref(q))
        so = lib.nq_conv_split_out(B, cin, H, W, cout, k, epi[1], C.EPI_CODE[epi[0]], int(epi[2]))
    if rc_only:
        return rc
    assert rc == 0, (shape, epi, rc)
    p = {n: getattr(q, n) for n, _ in q._fields_}
    assert so == p["split_out"]
    return p


def wgrad_plan(lib, shape):
    from neuroquant_amd import _lib
    q = _lib.ConvWgradPlan()
    assert lib.nq_conv_wgrad_plan(*shape, ctypes.byref(q)) == 0
    return {n: getattr(q, n) for n, _ in q._fields_}


def test_plans_reject_bad_arguments(lib):
    from neuroquant_amd import _lib
    q, w = _lib.ConvPlan(), _lib.ConvWgradPlan()
    for shape in [(0, 44, 32, 64, 148, 5), (2, 0, 32, 64, 148, 5), (2, 44, 0, 64, 148, 5), (2, 44, 32, 0, 148, 5), (2, 44, 32, 64, 0, 5)]:
        assert lib.nq_conv_forward_plan(*shape, 1, 0, 1, ctypes.byref(q)) == -1, shape
        assert lib.nq_conv_wgrad_plan(*shape, ctypes.byref(w)) == -1, shape
    good = (2, 44, 32, 64, 148, 5)
    assert lib.nq_conv_forward_plan(*good, 1, 0, 1, None) == -1 and lib.nq_conv_wgrad_plan(*good, None) == -1
    assert lib.nq_conv_forward_plan(*good, 1, 5, 1, ctypes.byref(q)) == -1 and lib.nq_conv_forward_plan(*good, 1, -1, 1, ctypes.byref(q)) == -1
    assert lib.nq_conv_forward_plan(*good, 3, 3, 1, ctypes.byref(q)) == -1        # PixelShuffle(3) of 148 channels
    assert lib.nq_conv_forward_plan(*good, 0, 1, 1, ctypes.byref(q)) == -1        # r = 0
    assert lib.nq_conv_forward_plan(*good, 3, 4, 0, ctypes.byref(q)) == -1        # un-shuffle by 3 of 32 x 64
    assert lib.nq_conv_forward_plan(2, 44, 32, 64, 148, 7, 1, 0, 1, ctypes.byref(q)) == -2
    assert lib.nq_conv_wgrad_plan(2, 44, 32, 64, 148, 7, ctypes.byref(w)) == -2
    assert lib.nq_conv_forward_plan(65536, 44, 32, 64, 148, 5, 1, 0, 1, ctypes.byref(q)) == -2


def test_knobs_naming_a_build_that_is_not_compiled_are_refused(lib, monkeypatch):
    head, dg = (2, 7, 8, 8, 3, 3), (2, 3, 8, 8, 7, 3)
    assert fwd_plan(lib, head, ("plain", 1, True), {"NQ_HEAD_RD": "7"}, monkeypatch, rc_only=True) == -2
    assert fwd_plan(lib, dg, ("dgrad", 2, False), {"NQ_HEAD_DG_R": "3"}, monkeypatch, rc_only=True) == -2
    # ... and the knobs are read per call, by the query as by the launch
    assert fwd_plan(lib, head, ("plain", 1, True), {}, monkeypatch)["kernel"] == C.HEAD_FWD
    assert fwd_plan(lib, head, ("plain", 1, True), {"NQ_HEAD_FWD": "1"}, monkeypatch)["kernel"] == C.HEAD_FWD_LDS
    assert fwd_plan(lib, dg, ("dgrad", 2, False), {}, monkeypatch)["split_out"] == 1
    assert fwd_plan(lib, dg, ("dgrad", 2, False), {"NQ_HEAD_DGRAD": "1"}, monkeypatch)["split_out"] == 0


def test_plan_of_the_shipped_layers(lib, monkeypatch):
    """known answers at the benchmark's size: the image head and its data gradient, dec3's data gradient on the fp32 kernels, the
    HNeRV stem and its weight gradient"""
    p = fwd_plan(lib, (2, 37, 640, 1280, 3, 3), ("tanh", 1, True), {}, monkeypatch)
    assert (p["kernel"], p["rows"], p["ws_floats"]) == (C.HEAD_FWD, 4, 0)
    p = fwd_plan(lib, (2, 3, 640, 1280, 37, 3), ("dgrad", 2, False), {}, monkeypatch)
    assert (p["kernel"], p["rows"], p["split_out"]) == (C.HEAD_DGRAD, 4, 1)
    p = fwd_plan(lib, (2, 848, 40, 80, 64, 5), ("dgrad", 2, False), {}, monkeypatch)
    assert (p["kernel"], p["mi"], p["ncg"], p["nsplit"], p["finish"]) == (C.IGEMM, 4, 212, 9, 1)
    assert p["ws_floats"] == 9 * 2 * 64 * 40 * 80
    p = fwd_plan(lib, (2, 1925, 2, 4, 92, 1), ("dgrad", 1, False), {}, monkeypatch)
    assert (p["kernel"], p["ksl"], p["ws_floats"]) == (C.TINY, 64, 0)
    w = wgrad_plan(lib, (2, 37, 640, 1280, 3, 3))
    assert (w["kernel"], w["mi"], w["ni"], w["co_pad"], w["n_pad"], w["nsplit"]) == (C.WG_MFMA, 1, 6, 16, 384, 256)
    assert wgrad_plan(lib, (2, 92, 2, 4, 1925, 1))["kernel"] == C.WG_TINY


def test_tables_are_complete():
    want = {(k, ("igemm", mi)) for k in (1, 3, 5) for mi in C.MIS}
    want |= {(1, ("tiny", ksl)) for ksl in C.KSLS} | {(3, ("head_fwd", R)) for R in C.HEAD_FWD_RS} | {(3, ("head_dgrad", R)) for R in C.HEAD_DGRAD_RS}
    want |= {(k, ("head_fwd_lds", k)) for k in (1, 3, 5)} | {(i[0], ("head_dgrad_lds",) + i) for i in C.HEAD_DGRAD_LDS_INSTS}
    assert len(C.MIS) == 10 and len(C.HEAD_DGRAD_LDS_INSTS) == 16 and len(want) == 30 + 4 + 2 + 2 + 3 + 16
    want -= set(C.UNREACHABLE)
    have = {(shape[5], inst) for shape, inst, _ in FWD_CASES}
    assert have <= want, sorted(have - want)
    assert len(want - have) <= C.ALLOWED_MISSING, sorted(want - have)
    wantw = {(k, ("wgrad",) + i) for k in (1, 3, 5) for i in C.WGRAD_INSTS[k]} | {(1, ("tiny_wgrad", 0)), (1, ("tiny_wgrad", 1))}
    assert len(wantw) == 32
    havew = {(shape[5], inst) for shape, inst, _ in WGRAD_CASES}
    assert havew <= wantw and len(wantw - havew) <= C.ALLOWED_MISSING, sorted(wantw ^ havew)
    for shape, inst, epis in ALL_FWD:
        assert epis and len(set(epis)) == len(epis) and all(C.epi_fits(shape, e) for e in epis), (shape, epis)
        assert C.macs(shape) <= C.MAX_MACS
    for shape, inst, dbs in WGRAD_CASES:
        assert dbs and len(set(dbs)) == len(dbs) and C.macs(shape) <= C.MAX_MACS
    assert len(ALL_FWD) == len({(c[0], c[1]) for c in ALL_FWD}) and len(WGRAD_CASES) == len({c[0] for c in WGRAD_CASES})


def _feats(lib, case, monkeypatch):
    shape, inst, epis = case
    return [C.Feat(shape, fwd_plan(lib, shape, e, C.env_of(shape, inst, e), monkeypatch)) for e in epis]


@pytest.mark.parametrize("case", ALL_FWD, ids=case_id)
def test_forward_row_matches_plan(lib, case, monkeypatch):
    shape, inst, epis = case
    B, cin, H, W, cout, k = shape
    for e, f in zip(epis, _feats(lib, case, monkeypatch)):
        assert f.inst == inst, f"{shape} {e}: planned {f.inst}, recorded {inst}"
        assert C.ROW_OK[inst[0]](f, epis), (shape, e)
        p = f.p
        # one workspace size per shape, whatever the epilogue, and it is what the split of the implicit-GEMM kernel needs
        assert p["ws_floats"] == lib.nq_conv_forward_ws_floats(*shape)
        if inst[0] == "igemm":
            mi = inst[1]
            assert W % 32 != 0 and (H % 4 != 0 or ("dgrad", 4, False) in epis) and macs_ok(shape)
            assert cout % (16 * mi) != 0 or any(x[0] in ("ps", "psgelu") and x[1] == 4 for x in epis)
            assert p["ncg"] == -(-cin // C.CI[k]) and 1 <= p["nsplit"] <= min(32, p["ncg"])
            assert p["ws_floats"] == (p["nsplit"] * B * cout * H * W if p["nsplit"] > 1 else 0)
            assert p["finish"] == (0 if p["nsplit"] == 1 else 8 if B * cout * H * W < 131072 and p["nsplit"] >= 16 else 1)
            assert (p["nsplit"] == 1) == (f.grid // p["nsplit"] >= 384 or p["ncg"] == 1)
            if k == 1:
                assert B * H * W > 256
        else:
            assert p["mi"] == p["nsplit"] == p["finish"] == 0
        if inst[0] == "tiny":
            assert p["ksl"] == (64 if cin > 1024 else 16 if cin > 256 else 4 if cin > 48 else 1) and p["ws_floats"] == 0
        assert p["split_out"] == (1 if inst[0] == "head_dgrad" else 0)


def macs_ok(shape):
    return C.macs(shape) <= C.MAX_MACS


@pytest.mark.parametrize("case", WGRAD_CASES, ids=case_id)
def test_wgrad_row_matches_plan(lib, case):
    shape, inst, dbs = case
    B, cin, H, W, cout, k = shape
    p = wgrad_plan(lib, shape)
    f = C.WFeat(shape, p)
    assert f.inst == inst, f"{shape}: planned {f.inst}, recorded {inst}"
    assert C.WGRAD_ROW_OK[inst[0]](f, dbs)
    assert p["ws_floats"] == lib.nq_conv_wgrad_ws_floats(*shape) > 0
    if inst[0] == "wgrad":
        mi, ni = inst[1:]
        assert (mi, ni) in C.WGRAD_INSTS[k]
        assert p["co_pad"] == -(-cout // (16 * mi)) * 16 * mi and p["n_pad"] == -(-cin * k * k // (64 * ni)) * 64 * ni
        assert p["nseg"] == -(-W // 32) * H * B and 1 <= p["nsplit"] <= min(256, p["nseg"])
        assert p["ws_floats"] == W3_slab(cin, cout, k, mi, ni, p["nsplit"])
        assert W % 32 != 0 and cout % (16 * mi) != 0 and (cin * k * k) % (64 * ni) != 0 and B >= 2
        assert p["nseg"] % p["nsplit"] != 0 or p["nsplit"] in (1, p["nseg"])
    else:
        assert B * H * W <= 256 and k == 1 and p["tiny_px8"] == int(H * W % 8 == 0)


def W3_slab(cin, cout, k, mi, ni, nsplit):
    import wgrad3_cases as W3
    return W3.slab_floats(cin, cout, k, mi, ni, nsplit)       # the same slab layout as the bf16x3 kernels: [co_pad][n_pad] + [co_pad]


def test_tables_meet_the_requirements(lib, monkeypatch):
    for family, k, reqs in C.requirement_groups():
        rows = C.rows_of(FWD_CASES, family, k)
        per_entry = {(c[0], c[1], e): f for c in rows for e, f in zip(c[2], _feats(lib, c, monkeypatch))}
        missing = []
        for label, row_pred, epi_pred, _ in (rq[:4] for rq in reqs):
            if row_pred is not None:
                ok = any(row_pred(per_entry[(s, i, epis[0])]) for s, i, epis in rows)
            else:
                ok = any(epi_pred(per_entry[(s, i, e)], e) for s, i, epis in rows for e in epis)
            if not ok:
                missing.append(label)
        assert not missing, (family, k, missing)
    for family, k, reqs in C.wgrad_requirement_groups():
        rows = C.rows_of(WGRAD_CASES, family, k)
        assert not C.unmet(rows, [C.WFeat(s, wgrad_plan(lib, s)) for s, _, _ in rows], reqs), (family, k)
    # most implicit-GEMM rows hold two or more frames; all but a few rows per kernel size meet the strict row conditions (two
    # column tiles and two rows of tiles; for the weight gradient two segments per row, two rows, three segments in some split)
    ig = C.rows_of(FWD_CASES, "igemm", None)
    assert 3 * sum(1 for c in ig if c[0][0] >= 2) >= 2 * len(ig)
    for k in (1, 3, 5):
        rows = C.rows_of(FWD_CASES, "igemm", k)
        assert sum(1 for c in rows if C.igemm_relaxed(_feats(lib, c, monkeypatch)[0])) <= C.MAX_RELAXED
        rows = C.rows_of(WGRAD_CASES, "wgrad", k)
        assert sum(1 for c in rows if C.wgrad_relaxed(C.WFeat(c[0], wgrad_plan(lib, c[0])))) <= C.MAX_RELAXED


def test_hand_chosen_rows(lib, monkeypatch):
    """<= 4 channels on a side without a head epilogue: the implicit-GEMM kernel with a split K loop, and a workspace for it"""
    for case in EXTRA_FWD_CASES:
        for f in _feats(lib, case, monkeypatch):
            assert f.kernel == C.IGEMM and f.nsplit > 1 and f.p["ws_floats"] == lib.nq_conv_forward_ws_floats(*case[0]) > 0


@pytest.mark.parametrize("case", ALL_FWD, ids=case_id)
def test_float32_alone_is_well_inside_the_bound_forward(case):
    shape, inst, epis = case
    w = C.f32_worst_fwd(shape, epis)
    print(f"{case_id(case)}: float32 on the CPU at {w:.3f} of the bound")
    assert w <= C.F32_MAX


@pytest.mark.parametrize("case", WGRAD_CASES, ids=case_id)
def test_float32_alone_is_well_inside_the_bound_wgrad(case):
    w = C.f32_worst_wgrad(case[0])
    print(f"{case_id(case)}: float32 on the CPU at {w[0]:.3f} (dw) and {w[1]:.3f} (db) of the bound")
    assert max(w) <= C.F32_MAX


"""Host-only checks behind tests/test_conv3_variants.py: the table of tests/conv3_cases.py names every template instantiation
of the bf16x3 forward / data-gradient kernels, the launch plan (nq_conv_forward3_plan) really sends each row to its instantiation,
every row and the table as a whole meet the conditions the GPU file relies on (ragged tiles, every tail chunk kind behind an
even and an odd number of full chunks, uneven splits, both builds of the finish kernel, every epilogue branch), the workspace and
split-word queries follow from the same plan, and the few-pixel plan never offers a launch whose patches do not fit the LDS."""
import ctypes
import math
import os

import pytest
import torch

import conv3_cases as C
from conv3_cases import CASES, FORMERLY_REFUSED, case_id

PLAN_ENV = ("NQ_FLAT3", "NQ_FLAT3_CPW", "NQ_SPLITK_MIN_CHUNKS", "NQ_IG3_OCC3_STEPS")


@pytest.fixture(scope="module", autouse=True)
def untuned_environment():
    """the plans read these once per process: with one of them set, the table describes another library"""
    found = [v for v in PLAN_ENV if v in os.environ]
    assert not found, f"unset {', '.join(found)}: the launch plans read them, and the table of tests/conv3_cases.py is for the defaults"


@pytest.fixture(scope="module")
def lib():
    from neuroquant_amd import _lib
    return _lib.lib()


def plan(lib, shape):
    from neuroquant_amd import _lib
    q = _lib.Conv3Plan()
    assert lib.nq_conv_forward3_plan(*shape, ctypes.byref(q)) == 0
    return {n: getattr(q, n) for n, _ in q._fields_}


def feat(lib, shape):
    return C.Feat(shape, plan(lib, shape))


def test_plan_rejects_bad_arguments(lib):
    from neuroquant_amd import _lib
    q = _lib.Conv3Plan()
    for shape in [(2, 44, 32, 64, 148, 7), (0, 44, 32, 64, 148, 5), (2, 0, 32, 64, 148, 5), (2, 44, 0, 64, 148, 5), (2, 44, 32, 0, 148, 5),
                  (2, 44, 32, 64, 0, 5)]:
        assert lib.nq_conv_forward3_plan(*shape, ctypes.byref(q)) == -1, shape
    assert lib.nq_conv_forward3_plan(2, 44, 32, 64, 148, 5, None) == -1


def test_ps_takes_split_words_without_y(lib):
    """NQ_EPI_PS writes z only, y may be NULL -- also with a split-word bit in `epilogue` (it was compared with the bits still on and
    refused as invalid).  Host-only: k = 7 is refused as unsupported right after the argument check, before any launch."""
    n, p = None, ctypes.c_void_p(16)
    for fmt in (0, C.X_SPLIT, C.Y_SPLIT, C.X_SPLIT | C.Y_SPLIT):
        assert lib.nq_conv_forward3(p, p, n, n, p, n, n, 2, 36, 169, 67, 36, 7, 2, 3 | fmt, n) == -2        # PS: y NULL is fine
        assert lib.nq_conv_forward3(p, p, n, n, p, n, n, 2, 36, 169, 67, 36, 7, 2, 0 | fmt, n) == -1        # plain: y is needed


def test_plan_of_the_shipped_layers(lib):
    """known answers: dec5 at the benchmark's size, HNeRV dec2 forward (few-pixel, two channel blocks) and dec3 data gradient"""
    p = plan(lib, (2, 44, 320, 640, 148, 5))
    assert (p["kernel"], p["mi"], p["waves"], p["nsplit"], p["tail"], p["supported"]) == (C.TILED, 5, 2, 1, 3, 1)
    p = plan(lib, (2, 77, 10, 20, 1024, 3))
    assert (p["kernel"], p["flat_nw"], p["flat_mi"], p["flat_nb"], p["nsplit"], p["supported"]) == (C.FLAT, 8, 2, 5, 1, 1)
    assert p["lds_bytes"] == 8 * 4 * 176 * 16       # 8 patches of 8 rows x 22 pixels, [plane][octet]
    p = plan(lib, (2, 848, 40, 80, 64, 5))
    assert (p["kernel"], p["mi"], p["waves"], p["nsplit"], p["per_split"]) == (C.TILED, 4, 2, 14, 4)


def test_table_is_complete():
    want = {(k, ("tiled", mi, w)) for k in (3, 5) for mi, w in C.TILED_INSTS}
    want |= {(k, ("flat",) + i) for k in (3, 5) for i in C.FLAT_INSTS[k]}
    assert len(C.TILED_INSTS) == 8 and len(C.TILED_XS_INSTS) == 6 and len(C.FLAT_INSTS[3]) == 7 and len(C.FLAT_INSTS[5]) == 4
    assert len(want) == 2 * 8 + 11            # + 2 x 6 split-word-input builds, run on the rows with mi >= 2: 50 in all
    want -= set(C.UNREACHABLE)
    have = {(shape[5], inst) for shape, inst, _ in CASES}
    assert have <= want, sorted(have - want)
    missing = sorted(want - have)
    assert len(missing) <= C.ALLOWED_MISSING, missing
    for shape, inst, epis in CASES:
        assert epis and len(set(epis)) == len(epis), shape
        assert all(C.epi_fits(shape, e) for e in epis), (shape, epis)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_table_matches_plan(lib, case):
    shape, inst, epis = case
    B, cin, H, W, cout, k = shape
    p = plan(lib, shape)
    f = C.Feat(shape, p)
    assert f.inst == inst, f"{shape}: planned {f.inst}, recorded {inst}"
    # the decoder would really take it
    assert lib.nq_conv3_supported(*shape) == 1 == p["supported"]
    # the conditions on every row, spelled out (conv3_cases.tiled_row_ok / flat_row_ok are what the generator asks)
    if inst[0] == "tiled":
        assert C.tiled_row_ok(f)
        mi = inst[1]
        assert W % 32 != 0 and W >= 67 and H % 8 != 0 and H >= 17 and cout % (16 * mi) != 0 and cin > 4
        last = (cin - 1) % 16 + 1                 # channels of the last chunk
        assert p["tail"] == (1 if last <= 4 else 2 if last <= 8 else 3 if last <= 12 else 0)
        assert p["lds_bytes_dgrad"] == (max(p["lds_bytes"], 1024 * 16 * mi) if p["nsplit"] == 1 and mi <= 4 else p["lds_bytes"])
        want_io = (C.X_SPLIT if mi >= 2 else 0) | (C.Y_SPLIT if p["nsplit"] == 1 else 0)
    else:
        assert C.flat_row_ok(f)
        nw, mi, nb = inst[1:]
        P = B * H * W
        assert P % (16 * nb) != 0 and cout % 16 != 0 and P <= 512 and W <= 32
        if nb == 5:
            assert B >= 2 and C.straddles_frame(B, H, W, nb)
        if mi == 2:
            assert 1 <= cout % 32 <= 16
        assert p["lds_bytes"] <= 160 * 1024
        want_io = C.Y_SPLIT if p["nsplit"] == 1 else 0
    # the split {hi | lo} word rule of include/nq_hip.h
    assert lib.nq_conv3_split_io(*shape) == want_io == p["split_io"]
    # the slabs of a split K loop: nsplit copies of the convolution's output
    assert 1 <= p["nsplit"] <= f.nchunk and (p["nsplit"] - 1) * p["per_split"] < f.nchunk <= p["nsplit"] * p["per_split"]
    assert lib.nq_conv_forward3_ws_floats(*shape) == (p["nsplit"] * B * cout * H * W if p["nsplit"] > 1 else 0)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bound_is_within_reach_of_the_arithmetic(case):
    """hi*hi + hi*lo + lo*hi of the bf16 halves, summed exactly, stays within IDEAL_MAX of the GPU file's bound on the row's own
    inputs: what a row then shows beyond that is the kernel's"""
    shape, _, epis = case
    worst = C.ideal_worst(shape, epis)
    assert worst <= C.IDEAL_MAX, f"{shape}: the exact arithmetic is at {worst:.3f} x the bound"


def test_arithmetic_misses_the_bound_at_a_short_contraction():
    """the data gradient the generator first chose for the 80-channel tile (63 products per output, 1.5 million outputs): the exact
    arithmetic is 12 % over the bound there, so no row asks it of a kernel"""
    shape = (2, 7, 169, 67, 68, 3)
    assert 1.0 < C.ideal_worst(shape, [("dgrad", 1, False)]) < 1.2
    assert all(e[0] != "dgrad" for s, _, epis in CASES if s == shape for e in epis)


@pytest.mark.parametrize("k", (3, 5))
@pytest.mark.parametrize("family", ("tiled", "flat"))
def test_table_meets_every_requirement(lib, k, family):
    rows = [c for c in CASES if c[0][5] == k and c[1][0] == family]
    feats = [feat(lib, shape) for shape, _, _ in rows]
    reqs = C.tiled_requirements() if family == "tiled" else C.flat_requirements(k)
    assert len(reqs) == (8 + 2 * 8 + 2 + 22 if family == "tiled" else len(C.FLAT_INSTS[k]) + 4 + 1 + 7)
    missing = C.unmet(rows, feats, reqs)
    assert not missing, missing
    if family == "tiled":
        assert 3 * sum(1 for shape, _, _ in rows if shape[0] >= 2) >= len(rows)
        # every split-word-input build has a row: the X bit is offered on all rows with mi >= 2
        for mi, w in C.TILED_XS_INSTS:
            assert any(f.inst == ("tiled", mi, w) and f.p["split_io"] & C.X_SPLIT for f in feats), (mi, w)


def test_requirements_tell_rows_apart(lib):
    """the predicates are not vacuous: on one unsplit tiled row the requirement list accepts what that row runs and nothing else"""
    shape = (2, 44, 137, 70, 148, 5)          # mi 5, 3 chunks (tail kind 3 behind 2 full ones), W % 4 != 0
    f = feat(lib, shape)
    assert C.tiled_row_ok(f) and f.inst == ("tiled", 5, 2) and f.tail_pair == (3, 0) and f.nsplit == 1
    rows = [(shape, f.inst, [("psgelu", 2, True), ("dgrad", 1, False)])]
    met = {label for label, *_ in C.tiled_requirements()} - set(C.unmet(rows, [f], C.tiled_requirements()))
    assert met == {"instantiation mi 5 waves 2", "dma: tail kind 3, full chunks in front of it even", "PS_GELU r 2, even W (DPP path)",
                   "dgrad narrow through mi 5"}


def _naive_conv(x, w, pad):
    B, cin, H, W = x.shape
    cout, _, k, _ = w.shape
    y = torch.zeros(B, cout, H, W, dtype=torch.float64)
    for b in range(B):
        for co in range(cout):
            for yy in range(H):
                for xx in range(W):
                    s = 0.0
                    for ci in range(cin):
                        for ky in range(k):
                            for kx in range(k):
                                iy, ix = yy + ky - pad, xx + kx - pad
                                if 0 <= iy < H and 0 <= ix < W:
                                    s += float(x[b, ci, iy, ix]) * float(w[co, ci, ky, kx])
                    y[b, co, yy, xx] = s
    return y


def _gelu(v):
    return 0.5 * v * (1.0 + math.erf(v / math.sqrt(2.0)))


def _dgelu(v):
    return 0.5 * (1.0 + math.erf(v / math.sqrt(2.0))) + v * math.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


@pytest.mark.parametrize("k", (3, 5))
def test_reference_is_anchored(k):
    """the float64 reference of the GPU file == plain loops at one tiny shape per epilogue"""
    r = 2
    shape = (2, 3, 4, 6, 8, k)
    B, cin, H, W, cout, _ = shape
    x, w, b = C.forward_inputs(shape)
    conv = C.forward_conv(x, w, k)
    naive = _naive_conv(x.double(), w.double(), k // 2)
    torch.testing.assert_close(conv, naive, rtol=1e-12, atol=1e-12)
    nb = naive + b.double().view(1, -1, 1, 1)
    y, z = C.forward_reference(conv, b, ("plain", 1, True))
    assert z is None
    torch.testing.assert_close(y, nb, rtol=1e-12, atol=1e-12)
    y, z = C.forward_reference(conv, b, ("plain", 1, False))
    torch.testing.assert_close(y, naive, rtol=0, atol=0)
    y, z = C.forward_reference(conv, b, ("tanh", 1, True))
    torch.testing.assert_close(y, nb.clone().apply_(lambda v: math.tanh(v) * 0.5 + 0.5), rtol=1e-12, atol=1e-12)
    shuf = torch.zeros(B, cout // (r * r), H * r, W * r, dtype=torch.float64)
    for bb in range(B):
        for co in range(cout):
            for yy in range(H):
                for xx in range(W):
                    c, rem = divmod(co, r * r)
                    shuf[bb, c, yy * r + rem // r, xx * r + rem % r] = nb[bb, co, yy, xx]
    y, z = C.forward_reference(conv, b, ("ps", r, True))
    assert y is None
    torch.testing.assert_close(z, shuf, rtol=0, atol=0)
    y, z = C.forward_reference(conv, b, ("psgelu", r, True))
    torch.testing.assert_close(y, shuf.clone().apply_(_gelu), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(z, shuf.clone().apply_(_dgelu), rtol=1e-12, atol=1e-12)
    # data gradient of the stored convolution wst (cin -> cout channels): the convolution with the taps reversed and the
    # channel roles exchanged, times gelu', un-shuffled
    xg, wst, zprev = C.dgrad_inputs(shape)
    assert wst.shape == (cin, cout, k, k) and zprev.shape == (B, cout, H, W)
    flipped = wst.double().flip(2, 3).permute(1, 0, 2, 3).contiguous()
    dconv = C.dgrad_conv(xg, wst, shape)
    torch.testing.assert_close(dconv, _naive_conv(xg.double(), flipped, k // 2), rtol=1e-12, atol=1e-12)
    pre_like = torch.linspace(-3, 3, 7, dtype=torch.float64).requires_grad_(True)      # gelu' as dgrad_inputs forms zprev
    torch.testing.assert_close(torch.autograd.grad(torch.nn.functional.gelu(pre_like).sum(), pre_like)[0],
                               pre_like.detach().clone().apply_(_dgelu), rtol=1e-12, atol=1e-12)
    prod = dconv * zprev.double()
    un = torch.zeros(B, cout * r * r, H // r, W // r, dtype=torch.float64)
    for bb in range(B):
        for co in range(cout):
            for yy in range(H):
                for xx in range(W):
                    un[bb, co * r * r + (yy % r) * r + xx % r, yy // r, xx // r] = prod[bb, co, yy, xx]
    torch.testing.assert_close(C.dgrad_reference(dconv, zprev, r), un, rtol=0, atol=0)
    torch.testing.assert_close(C.dgrad_reference(dconv, zprev, 1), prod, rtol=0, atol=0)


def test_few_pixel_plan_fits_the_lds(lib):
    """Every few-pixel shape of the sweep that the plan gives to the few-pixel kernel reports at most 160 KiB of LDS -- the
    launch refuses more -- and the reported size is that of the launch: NW wave-private patches of 4 x ppix 16-byte units, or
    the cross-wave reduction's NW x MI x NB x 1 KiB where that is larger."""
    given = refused = 0
    for k in (3, 5):
        for B in (1, 2, 3, 4, 8, 16):
            for H in range(1, 33):
                for W in range(1, 33):
                    if B * H * W > 512:
                        continue
                    for cin in (64, 65, 80, 129, 145):
                        shape = (B, cin, H, W, 64, k)
                        p = plan(lib, shape)
                        if p["kernel"] == C.FLAT:
                            given += 1
                            assert 0 < p["lds_bytes"] <= 160 * 1024, (shape, p["lds_bytes"])
                            assert p["lds_bytes"] % (p["flat_nw"] * 64) == 0
                            assert p["lds_bytes"] >= p["flat_nw"] * p["flat_mi"] * p["flat_nb"] * 1024
                        else:
                            refused += 1
                            assert p["kernel"] == C.TILED and p["flat_nw"] == 0
    assert given > 10000 and refused > 2000, (given, refused)


@pytest.mark.parametrize("shape", FORMERLY_REFUSED)
def test_unlaunchable_few_pixel_shapes_are_not_offered(lib, shape):
    """their patches need 202752 / 190464 / 172032 B of LDS: nq_conv3_supported said 1 and the launch refused.  Now the tiled
    kernel's plan answers, its grid is too small, and the decoder keeps them on the fp32 kernels."""
    B, cin, H, W, cout, k = shape
    pad, nw = k // 2, 8
    P, HW, VH, PW = B * H * W, H * W, H + 2 * (k // 2), W + 2 * (k // 2)
    rows = max(((min(p0 + 80, P) - 1) // HW * VH + (min(p0 + 80, P) - 1) % HW // W) - (p0 // HW * VH + p0 % HW // W) + 1 + 2 * pad
               for p0 in range(0, P, 80))
    need = nw * 4 * (-(-rows * PW // 4) * 4) * 16
    assert need == {(2, 80, 2, 32, 40, 5): 202752, (2, 80, 3, 27, 64, 5): 190464, (4, 80, 10, 2, 64, 5): 172032}[shape] > 160 * 1024
    p = plan(lib, shape)
    assert p["kernel"] == C.TILED and p["nsplit"] == 5
    assert lib.nq_conv3_supported(*shape) == 0 == p["supported"] and lib.nq_conv3_split_io(*shape) == 0
    assert lib.nq_conv_forward3_ws_floats(*shape) == 5 * B * cout * H * W

"""The half-precision levels forward (nq_conv_forward3_levels_f16: integer weights n = level - zero_point as IEEE halves, the
activations rounded once to half, ONE F16 MFMA per product) on every build of the tiled kernel.

Rows, restated from the table alone as tests/test_levels_conv_gpu.py states them: every row of tests/conv3_cases.CASES that is a
tiled row with a forward epilogue -- where its plan is the unsplit tiled kernel the entry serves it (all 16 (k, mi, waves) builds,
tail kinds 1..3 of both weight-staging families, every forward epilogue branch), where the plan splits it over K the entry must
refuse it -- and four full-last-chunk shapes (tail kind 0) per kernel size.

1. exactness: small-integer activations, 8-bit levels with both extreme levels and zero points, power-of-two steps, biases that
   are multiples of the step: every product and sum is exact in fp32 and the output must equal float64 bit for bit.  This is the
   check of the f16 A/B lane map, the operand image, scale, bias and every epilogue's stores.
2. against the arithmetic itself, delta * conv64(x.half(), n) + bias, at conv3_cases.bound: only fp32 accumulation separates them.
3. against the true convolution conv64(x, n * delta) at the derived bound
       conv3_cases.bound(ref) + L * (2^-11 * conv64(|x|, |n| * delta) + conv64(s, |n| * delta)),
   s = |x| where 0 < |x| < 2^-14 (a half subnormal: flushed to zero at worst), 0 elsewhere.  The middle term is the a-priori error
   of one round-to-nearest-even to 11 significant bits under the sum.  L carries it through the epilogue's function by its largest
   slope: 1 for plain and the shuffles, 0.5 for tanh * 0.5 + 0.5, 1.13 for GELU (max gelu' = 1.129), 1 for the saved gelu'
   (max |gelu''| = 2 * phi(0) = 0.798).
4. subnormals: which way the matrix pipe treats a half subnormal -- either is right, the test prints which.
5. saturation: a finite |x| > 65504 is clamped and raises the flag word; 6e4 does not; NaN passes into its receptive field only.
6. run-to-run identity.  7. a row the plan splits over K is refused with -2."""
import ctypes
import math
import time

import pytest
import torch

import conv3_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
CODE = {"plain": 0, "psgelu": 1, "tanh": 2, "ps": 3}      # NQ_EPI_* (include/nq_hip.h)
F16_MAX = 65504.0
U = 2.0 ** -11                                            # unit roundoff of IEEE half
SLOPE = {"plain": (1.0, None), "tanh": (0.5, None), "ps": (None, 1.0), "psgelu": (1.13, 1.0)}   # (y, z): largest slope, see above


def _plan(shape):
    from neuroquant_amd import _lib
    q = _lib.Conv3Plan()
    assert _lib.lib().nq_conv_forward3_plan(*shape, ctypes.byref(q)) == 0
    return {n: getattr(q, n) for n, _ in q._fields_}


def _unsplit_tiled(p):
    return p["kernel"] == C.TILED and p["supported"] == 1 and p["nsplit"] == 1


# full last chunk (tail kind 0): (shape without k, mi, waves per SIMD); plain with bias, the 36-channel rows PS_GELU r 2 as well
_EXTRA = [((2, 16, 169, 67, 5), 1, 3), ((2, 48, 169, 67, 17), 2, 3), ((2, 30, 169, 67, 36), 3, 3), ((2, 32, 169, 67, 68), 5, 2)]
EXTRA = [(s + (k,), ("tiled", mi, w), [("plain", 1, True)] + ([("psgelu", 2, True)] if s[4] % 4 == 0 else []))
         for k in (3, 5) for s, mi, w in _EXTRA]
CANDIDATES = [(shape, inst, [e for e in epis if e[0] != "dgrad"]) for shape, inst, epis in C.CASES
              if inst[0] == "tiled" and any(e[0] != "dgrad" for e in epis)]
ROWS = CANDIDATES + EXTRA
IDS = [C.case_id(r) for r in ROWS]


@pytest.fixture(scope="module")
def ops():
    from neuroquant_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def _flag():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def _check_plan(ops, row):
    shape, inst, _ = row
    p = _plan(shape)
    assert _unsplit_tiled(p) and C.inst_of(p) == inst, "the plan no longer sends this shape to the build it is listed for"
    assert ops.conv3_levels_supported(*shape)
    return p


def _refused(ops, row):
    """a row the plan splits over K (or gives to another kernel): not offered, and the launch says unsupported"""
    from neuroquant_amd import _lib
    shape = row[0]
    B, cin, H, W, cout, k = shape
    assert not ops.conv3_levels_supported(*shape)
    x, n, scale = torch.zeros(B, cin, H, W, device=DEV), torch.zeros(cout, cin, k, k, device=DEV), torch.ones(cout, device=DEV)
    y, flag = torch.empty(B, cout, H, W, device=DEV), _flag()
    wt = ops.levels_operand(n, dtype="f16")
    rc = _lib.lib().nq_conv_forward3_levels_f16(x.data_ptr(), wt.data_ptr(), scale.data_ptr(), None, y.data_ptr(), None,
                                                flag.data_ptr(), B, cin, H, W, cout, k, 1, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == -2
    with pytest.raises(_lib.NQLibraryError):
        ops.conv3_forward_levels_f16_raw(x, wt, scale, None, cout, k, 0, 1, flag)
    assert int(flag.item()) == 0


def test_rows_cover_every_build_tail_and_epilogue():
    """what the parametrised tests below rely on: a tuning change of the plan shows up here, not as a thinner test"""
    served = [r for r in ROWS if _unsplit_tiled(_plan(r[0]))]
    assert len(served) - len(EXTRA) == 34 and len(EXTRA) == 8 and served[-len(EXTRA):] == EXTRA
    assert len(CANDIDATES) > 34                      # ... and some split-K rows, for the refusal
    feats = [(r, C.Feat(r[0], _plan(r[0]))) for r in served]
    for k in (3, 5):
        fk = [(r, f) for r, f in feats if r[0][5] == k]
        assert {f.inst[1:] for _, f in fk} == set(C.TILED_INSTS)
        for fam in ("reg", "dma"):
            assert {f.tail for _, f in fk if f.family == fam} == {0, 1, 2, 3}, (k, fam)
        epis = {(e[0], e[1], e[2], r[0][3] % 2) for r, _ in fk for e in r[2]}
        names = {(e[0], e[1], e[2]) for e in epis}
        assert {("plain", 1, True), ("plain", 1, False), ("tanh", 1, True), ("ps", 3, True), ("psgelu", 3, True), ("ps", 4, True),
                ("psgelu", 4, True)} <= names
        for name in ("ps", "psgelu"):
            assert (name, 2, True, 0) in epis and (name, 2, True, 1) in epis     # r 2: even W (DPP stores) and odd W
    for (shape, inst, _), f in feats[-len(EXTRA):]:
        assert f.tail == 0 and f.inst == inst


def _levels_inputs(shape, n_bits):
    """(x, n, delta, b) on the CPU: Gaussian activations, integer weights n = level - zero_point with both extreme levels in every
    output channel and both extreme zero points, steps that give the weights the scale of conv3_cases.forward_inputs"""
    B, cin, H, W, cout, k = shape
    g = C._gen(shape, 5)
    x = torch.randn(B, cin, H, W, generator=g)
    L = 2 ** n_bits
    lv = torch.randint(0, L, (cout, cin, k, k), generator=g)
    lv.view(cout, -1)[:, 0] = 0
    lv.view(cout, -1)[:, 1] = L - 1
    zp = torch.randint(0, L, (cout,), generator=g)
    zp[0], zp[-1] = 0, L - 1
    delta = (0.5 + torch.rand(cout, generator=g)) * math.sqrt(3) / (L * math.sqrt(cin * k * k))
    b = torch.randn(cout, generator=g) * 0.1
    n = (lv - zp.view(-1, 1, 1, 1)).float()
    return x, n, delta, b


def _run(ops, xg, wt, scale, bias, shape, epi, flag):
    name, r, has_bias = epi
    return ops.conv3_forward_levels_f16_raw(xg, wt, scale, bias if has_bias else None, shape[4], shape[5], CODE[name], r, flag)


def _ratio(got, ref, bound):
    return 0.0 if ref is None else float(((got.detach().cpu().double() - ref).abs() / bound).max())


def _shuffled(t, epi):
    return t if epi[0] in ("plain", "tanh") else torch.nn.functional.pixel_shuffle(t, epi[1])


def _true_bounds(extra, ry, rz, epi):
    """the derived bound of (3) for the outputs (y, z) of an epilogue; extra = the pre-activation term, bias-free layout"""
    e = _shuffled(extra, epi)
    ly, lz = SLOPE[epi[0]]
    return (None if ry is None else C.bound(ry) + ly * e), (None if rz is None else C.bound(rz) + lz * e)


def _rounding_term(x, n, delta, k):
    """2^-11 * conv64(|x|, |n| * delta) + conv64(s, |n| * delta): the convolution is linear in its first argument"""
    ax = x.double().abs()
    s = torch.where((ax > 0) & (ax < 2.0 ** -14), ax, torch.zeros_like(ax))
    return C.forward_conv(U * ax + s, n.double().abs() * delta.double().view(-1, 1, 1, 1), k)


_SERVED_BEFORE = {}


def _n_bits(idx):
    """2 .. 8, cycling over the rows that are served"""
    if not _SERVED_BEFORE:
        c = 0
        for i, r in enumerate(ROWS):
            _SERVED_BEFORE[i] = c
            c += int(_unsplit_tiled(_plan(r[0])))
    return 2 + _SERVED_BEFORE[idx] % 7


def _exact_epis(epis):
    """plain (with / without bias) and ps: a shuffle is a permutation; a PS_GELU entry contributes its shuffle"""
    out = []
    for name, r, bias in epis:
        e = (name, r, bias) if name in ("plain", "ps") else ("ps", r, bias) if name == "psgelu" else None
        if e is not None and e not in out:
            out.append(e)
    return out


@pytest.mark.parametrize("idx", [i for i in range(len(ROWS)) if _exact_epis(ROWS[i][2])],
                         ids=[IDS[i] for i in range(len(ROWS)) if _exact_epis(ROWS[i][2])])
def test_exact_on_integer_inputs(ops, idx):
    row = ROWS[idx]
    shape, inst, epis = row
    B, cin, H, W, cout, k = shape
    if not _unsplit_tiled(_plan(shape)):
        return _refused(ops, row)
    _check_plan(ops, row)
    K = cin * k * k
    assert K <= (1179 if k == 3 else 1275) and 4 * 255 * K + 8 < 2 ** 24     # every partial sum is an integer fp32 holds
    g = C._gen(shape, 6)
    x = torch.randint(-4, 5, (B, cin, H, W), generator=g).float()
    lv = torch.randint(0, 256, (cout, cin, k, k), generator=g)
    lv.view(cout, -1)[:, 0] = 0
    lv.view(cout, -1)[:, 1] = 255
    zp = torch.randint(0, 256, (cout,), generator=g)
    zp[0], zp[-1] = 0, 255
    n = (lv - zp.view(-1, 1, 1, 1)).float()
    assert float(n.max()) == 255 and float(n.min()) == -255
    assert torch.equal(n.half().float(), n) and torch.equal(x.half().float(), x)
    delta = torch.tensor([2.0 ** -(co % 7) for co in range(cout)])
    b = torch.randint(-8, 9, (cout,), generator=g).float() * delta
    conv = C.forward_conv(x, n, k) * delta.double().view(1, -1, 1, 1)        # integers times a power of two: exact
    assert float(conv.abs().max()) < 2 ** 24
    xg, scale, bg, flag = x.to(DEV), delta.to(DEV), b.to(DEV), _flag()
    wt = ops.levels_operand(n.to(DEV), dtype="f16")
    for epi in _exact_epis(epis):
        ry, rz = C.forward_reference(conv, b, epi)
        y, z = _run(ops, xg, wt, scale, bg, shape, epi, flag)
        for got, ref in ((y, ry), (z, rz)):
            assert (got is None) == (ref is None)
            if ref is not None:
                want = ref.float()
                assert torch.equal(want.double(), ref), "the reference itself is not exact in fp32"
                assert torch.equal(got.cpu(), want), f"{epi}: {int((got.cpu() != want).sum())} of {want.numel()} outputs differ"
    assert int(flag.item()) == 0


@pytest.mark.parametrize("idx", range(len(ROWS)), ids=IDS)
def test_against_the_arithmetic_and_the_true_convolution(ops, idx):
    """checks (2) and (3) on one set of inputs, references and launches per row"""
    row = ROWS[idx]
    shape, inst, epis = row
    B, cin, H, W, cout, k = shape
    t0 = time.time()
    if not _unsplit_tiled(_plan(shape)):
        return _refused(ops, row)
    p = _check_plan(ops, row)
    n_bits = _n_bits(idx)
    x, n, delta, b = _levels_inputs(shape, n_bits)
    assert float(n.abs().max()) == 2 ** n_bits - 1
    dcol = delta.double().view(1, -1, 1, 1)
    true = C.forward_conv(x, n.double() * delta.double().view(-1, 1, 1, 1), k)           # float64 throughout
    arith = C.forward_conv(x.half().double(), n.double(), k) * dcol                       # the half arithmetic, exactly
    extra = _rounding_term(x, n, delta, k)
    used = float(((arith - true).abs() / extra).max())                                     # share of the a-priori term the exact arithmetic uses
    xg, scale, bg, flag = x.to(DEV), delta.to(DEV), b.to(DEV), _flag()
    wt = ops.levels_operand(n.to(DEV), dtype="f16")
    for epi in epis:
        ty, tz = C.forward_reference(true, b, epi)
        ay, az = C.forward_reference(arith, b, epi)
        by, bz = _true_bounds(extra, ty, tz, epi)
        y, z = _run(ops, xg, wt, scale, bg, shape, epi, flag)
        assert (y is None) == (ty is None) and (z is None) == (tz is None)
        a_y, a_z = _ratio(y, ay, None if ay is None else C.bound(ay)), _ratio(z, az, None if az is None else C.bound(az))
        t_y, t_z = _ratio(y, ty, by), _ratio(z, tz, bz)
        over = max(_ratio(y, ty, None if ty is None else C.bound(ty)), _ratio(z, tz, None if tz is None else C.bound(tz)))
        print(f"half {IDS[idx]} {n_bits} bits {epi[0]} r {epi[1]} bias {int(epi[2])} tail {p['tail']}: against the arithmetic "
              f"y {a_y:.4f} z {a_z:.4f} of the bf16x3 bound; against the true convolution y {t_y:.4f} z {t_z:.4f} of the derived bound "
              f"({over:.1f} x the bf16x3 bound; the exact arithmetic uses {used:.3f} of the rounding term)")
        assert a_y <= 1.0 and a_z <= 1.0, f"{epi}: {max(a_y, a_z):.3f} x the bound against delta * conv64(x.half(), n) + bias"
        assert t_y <= 1.0 and t_z <= 1.0, f"{epi}: {max(t_y, t_z):.3f} x the derived bound against the true convolution"
    assert int(flag.item()) == 0
    print(f"half {IDS[idx]}: {time.time() - t0:.2f} s")


SMALL = (2, 7, 169, 67, 17, 3)      # register-staged tile, two frames, several tiles


def test_subnormal_activation(ops):
    """one activation of 2^-20 (a half subnormal) against a weight of 1, step 1: 2^-20 when the conversion and the matrix pipe keep
    half subnormals, 0 when either flushes them"""
    B, cin, H, W, cout, k = SMALL
    assert _unsplit_tiled(_plan(SMALL))
    x, n = torch.zeros(B, cin, H, W), torch.zeros(cout, cin, k, k)
    x[1, 3, 50, 40] = 2.0 ** -20
    n[2, 3, k // 2, k // 2] = 1.0
    y, _ = ops.conv3_forward_levels_f16_raw(x.to(DEV), ops.levels_operand(n.to(DEV), dtype="f16"), torch.ones(cout, device=DEV), None,
                                            cout, k, 0, 1, _flag())
    y = y.cpu()
    got = float(y[1, 2, 50, 40])
    print(f"half subnormal 2^-20 times 1: {got!r} -> half subnormals are {'KEPT' if got != 0.0 else 'FLUSHED to zero'}")
    assert got in (2.0 ** -20, 0.0)
    y[1, 2, 50, 40] = 0.0
    assert not bool(y.any())


def _with_activation(x, value):
    x = x.clone()
    x[1, 3, 50, 40] = value
    return x


def test_saturation_flag_and_clamp(ops):
    B, cin, H, W, cout, k = SMALL
    assert _unsplit_tiled(_plan(SMALL))
    x0, n, delta, b = _levels_inputs(SMALL, 5)
    scale, bg = delta.to(DEV), b.to(DEV)
    wt = ops.levels_operand(n.to(DEV), dtype="f16")
    epi = ("plain", 1, True)
    w64 = n.double() * delta.double().view(-1, 1, 1, 1)

    def check(x_in, x_ref, want_flag):
        flag = _flag()
        y, _ = _run(ops, x_in.to(DEV), wt, scale, bg, SMALL, epi, flag)
        ref, _ = C.forward_reference(C.forward_conv(x_ref, w64, k), b, epi)
        bound, _ = _true_bounds(_rounding_term(x_ref, n, delta, k), ref, None, epi)
        e = _ratio(y, ref, bound)
        print(f"saturation: activation {float(x_in[1, 3, 50, 40]):g}: flag {int(flag.item())}, error / derived bound {e:.4f}")
        assert int(flag.item()) == want_flag and e <= 1.0
        return flag

    for sign in (1.0, -1.0):
        check(_with_activation(x0, sign * 1e5), _with_activation(x0, sign * F16_MAX), 1)
        check(_with_activation(x0, sign * 6e4), _with_activation(x0, sign * 6e4), 0)
    # the word is sticky: a clean launch on a raised flag leaves it raised
    flag = check(_with_activation(x0, 1e5), _with_activation(x0, F16_MAX), 1)
    _run(ops, x0.to(DEV), wt, scale, bg, SMALL, epi, flag)
    assert int(flag.item()) == 1


def test_nan_stays_in_its_receptive_field(ops):
    B, cin, H, W, cout, k = SMALL
    x0, n, delta, b = _levels_inputs(SMALL, 5)
    flag = _flag()
    wt = ops.levels_operand(n.to(DEV), dtype="f16")
    clean, _ = _run(ops, x0.to(DEV), wt, delta.to(DEV), b.to(DEV), SMALL, ("plain", 1, True), flag)
    y, _ = _run(ops, _with_activation(x0, float("nan")).to(DEV), wt, delta.to(DEV), b.to(DEV), SMALL, ("plain", 1, True), flag)
    field = torch.zeros(B, cout, H, W, dtype=torch.bool)
    field[1, :, 50 - k // 2:50 + k // 2 + 1, 40 - k // 2:40 + k // 2 + 1] = True
    y, clean = y.cpu(), clean.cpu()
    assert torch.equal(torch.isnan(y), field)
    assert torch.equal(y[~field], clean[~field])
    assert int(flag.item()) == 0                     # a NaN is not a saturation


@pytest.mark.parametrize("shape,epi", [((2, 7, 169, 67, 17, 3), ("plain", 1, True)), ((2, 7, 169, 67, 36, 5), ("ps", 2, True)),
                                       ((2, 7, 81, 67, 99, 3), ("psgelu", 3, True))])
def test_two_calls_agree_bit_for_bit(ops, shape, epi):
    """one register-staged tile (mi 2) and two LDS-DMA tiles (mi 3, mi 4)"""
    p = _plan(shape)
    assert _unsplit_tiled(p) and (p["mi"] <= 2) == (shape[4] == 17)
    x, n, delta, b = _levels_inputs(shape, 5)
    xg, scale, bg, flag = x.to(DEV), delta.to(DEV), b.to(DEV), _flag()
    first = _run(ops, xg, ops.levels_operand(n.to(DEV), dtype="f16"), scale, bg, shape, epi, flag)
    again = _run(ops, xg, ops.levels_operand(n.to(DEV), dtype="f16"), scale, bg, shape, epi, flag)
    for a, c in zip(first, again):
        assert (a is None and c is None) or torch.equal(a.view(torch.int32), c.view(torch.int32))


def test_split_k_row_is_refused(ops):
    rows = [r for r in CANDIDATES if not _unsplit_tiled(_plan(r[0]))]
    assert rows and _plan(rows[0][0])["nsplit"] > 1
    _refused(ops, rows[0])


def test_operand_is_the_layout_image_in_half(ops):
    """same size and slots as weight_layout3; where bf16 and half agree bit-wise after widening (the integers), the hi planes hold
    the same VALUES and the lo planes are zero"""
    n = torch.zeros(17, 7, 3, 3, device=DEV)
    n[0, 0, 0, 0], n[16, 6, 2, 2], n[5, 3, 1, 1] = 256.0, -255.0, 3.0
    a, h = ops.levels_operand(n), ops.levels_operand(n, dtype="f16")
    assert a.shape == h.shape and a.dtype == h.dtype == torch.uint8
    av, hv = a.view(torch.bfloat16).float(), h.view(torch.float16).float()
    assert torch.equal(av, hv) and sorted(hv[hv != 0].tolist()) == [-255.0, 3.0, 256.0]
    with pytest.raises(ValueError):
        ops.levels_operand(n, dtype="fp8")
    m = n.clone()
    m[3, 4, 1, 2] = 0.5
    with pytest.raises(ValueError):
        ops.levels_operand(m, dtype="f16")

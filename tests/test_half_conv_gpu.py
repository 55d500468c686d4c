"""The half-precision levels forward (nq_conv_forward3_levels_f16: integer weights n = level - zero_point as IEEE halves, the
activations rounded once to half, ONE F16 MFMA per product) on every build of the tiled kernel.

Rows: the table of tests/levels_cases.py, as tests/test_levels_conv_gpu.py uses it: every row of tests/conv3_cases.CASES that is a
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
import time

import pytest
import torch

import conv3_cases as C
import levels_cases as L
from levels_cases import DEV, IDS, ROWS

pytestmark = pytest.mark.gpu

SEED, EXACT_SEED = 5, 6     # of the Gaussian and of the exact-integer inputs
F16_MAX = 65504.0
U = 2.0 ** -11                                            # unit roundoff of IEEE half
SLOPE = {"plain": (1.0, None), "tanh": (0.5, None), "ps": (None, 1.0), "psgelu": (1.13, 1.0)}   # (y, z): largest slope, see above


@pytest.fixture(scope="module")
def ops():
    from neuroquant_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def test_rows_cover_every_build_tail_and_epilogue():
    L.check_rows_cover_every_build_tail_and_epilogue()


def _run(ops, xg, wt, scale, bias, shape, epi, flag):
    return L.run(ops, "f16", xg, wt, scale, bias, shape, epi, flag)


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


@pytest.mark.parametrize("idx", L.EXACT_IDX, ids=[IDS[i] for i in L.EXACT_IDX])
def test_exact_on_integer_inputs(ops, idx):
    L.check_exact_on_integer_inputs(ops, idx, "f16", EXACT_SEED)


@pytest.mark.parametrize("idx", range(len(ROWS)), ids=IDS)
def test_against_the_arithmetic_and_the_true_convolution(ops, idx):
    """checks (2) and (3) on one set of inputs, references and launches per row"""
    row = ROWS[idx]
    shape, inst, epis = row
    B, cin, H, W, cout, k = shape
    t0 = time.time()
    if not L.unsplit_tiled(L.plan(shape)):
        return L.refused(ops, row, "f16")
    p = L.check_plan(ops, row)
    n_bits = L.n_bits(idx)
    x, n, delta, b = L.levels_inputs(shape, n_bits, SEED)
    assert float(n.abs().max()) == 2 ** n_bits - 1
    dcol = delta.double().view(1, -1, 1, 1)
    true = C.forward_conv(x, n.double() * delta.double().view(-1, 1, 1, 1), k)           # float64 throughout
    arith = C.forward_conv(x.half().double(), n.double(), k) * dcol                       # the half arithmetic, exactly
    extra = _rounding_term(x, n, delta, k)
    used = float(((arith - true).abs() / extra).max())                                     # share of the a-priori term the exact arithmetic uses
    xg, scale, bg, flag = x.to(DEV), delta.to(DEV), b.to(DEV), L.new_flag()
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
    assert L.unsplit_tiled(L.plan(SMALL))
    x, n = torch.zeros(B, cin, H, W), torch.zeros(cout, cin, k, k)
    x[1, 3, 50, 40] = 2.0 ** -20
    n[2, 3, k // 2, k // 2] = 1.0
    y, _ = ops.conv3_forward_levels_raw(x.to(DEV), ops.levels_operand(n.to(DEV), dtype="f16"), torch.ones(cout, device=DEV), None,
                                        cout, k, 0, 1, "f16", L.new_flag())
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
    assert L.unsplit_tiled(L.plan(SMALL))
    x0, n, delta, b = L.levels_inputs(SMALL, 5, SEED)
    scale, bg = delta.to(DEV), b.to(DEV)
    wt = ops.levels_operand(n.to(DEV), dtype="f16")
    epi = ("plain", 1, True)
    w64 = n.double() * delta.double().view(-1, 1, 1, 1)

    def check(x_in, x_ref, want_flag):
        flag = L.new_flag()
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
    x0, n, delta, b = L.levels_inputs(SMALL, 5, SEED)
    flag = L.new_flag()
    wt = ops.levels_operand(n.to(DEV), dtype="f16")
    clean, _ = _run(ops, x0.to(DEV), wt, delta.to(DEV), b.to(DEV), SMALL, ("plain", 1, True), flag)
    y, _ = _run(ops, _with_activation(x0, float("nan")).to(DEV), wt, delta.to(DEV), b.to(DEV), SMALL, ("plain", 1, True), flag)
    field = torch.zeros(B, cout, H, W, dtype=torch.bool)
    field[1, :, 50 - k // 2:50 + k // 2 + 1, 40 - k // 2:40 + k // 2 + 1] = True
    y, clean = y.cpu(), clean.cpu()
    assert torch.equal(torch.isnan(y), field)
    assert torch.equal(y[~field], clean[~field])
    assert int(flag.item()) == 0                     # a NaN is not a saturation


@pytest.mark.parametrize("shape,epi", L.TWO_CALLS)
def test_two_calls_agree_bit_for_bit(ops, shape, epi):
    L.check_two_calls_agree_bit_for_bit(ops, shape, epi, "f16", SEED)


def test_split_k_row_is_refused(ops):
    rows = [r for r in L.CANDIDATES if not L.unsplit_tiled(L.plan(r[0]))]
    assert rows and L.plan(rows[0][0])["nsplit"] > 1
    L.refused(ops, rows[0], "f16")


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

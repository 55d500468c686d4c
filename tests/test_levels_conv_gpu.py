"""The levels forward (nq_conv_forward3_levels: integer weights n = level - zero_point, two BF16 MFMAs per product, the quantiser
step applied per output channel in the epilogue) on every build of the tiled kernel.

Rows (tests/levels_cases.py): every row of tests/conv3_cases.CASES whose plan is the unsplit tiled kernel, with its forward
epilogues -- all 16 (k, mi, waves) builds, tail kinds 1..3 of both weight-staging families, every forward epilogue branch -- and,
for the full last chunk (tail kind 0) no such row has, four shapes per kernel size beside them.  The parametrisation is every tiled
row with a forward epilogue, read from the table alone; a row the plan splits over K is checked for being refused instead.

1. parity: against the float64 convolution of x with (level - zero_point) * delta at the project's bf16x3 bounds
   (conv3_cases.bound), after the arithmetic itself, evaluated exactly on the CPU, has been held to IDEAL_MAX of that bound on
   the very inputs -- a row that fails that gate FAILS, none drops out;
2. exactness: small-integer inputs and power-of-two steps make every product, sum, scale and bias add exact in fp32, so the output
   must equal the float64 computation bit for bit -- pins the indexing of weights, scale, bias and every epilogue's stores;
3. run-to-run identity;  4. what ops.levels_operand refuses."""
import time

import pytest
import torch

import conv3_cases as C
import levels_cases as L
from levels_cases import DEV, IDS, ROWS

pytestmark = pytest.mark.gpu

SEED, EXACT_SEED = 3, 4     # of the Gaussian and of the exact-integer inputs


@pytest.fixture(scope="module")
def ops():
    from neuroquant_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def test_rows_cover_every_build_tail_and_epilogue():
    L.check_rows_cover_every_build_tail_and_epilogue()


def _ratio(got, ref):
    return 0.0 if ref is None else float(((got.detach().cpu().double() - ref).abs() / C.bound(ref)).max())


@pytest.mark.parametrize("idx", range(len(ROWS)), ids=IDS)
def test_parity_to_float64(ops, idx):
    row = ROWS[idx]
    shape, inst, epis = row
    B, cin, H, W, cout, k = shape
    t0 = time.time()
    if not L.unsplit_tiled(L.plan(shape)):
        return L.refused(ops, row, "bf16")
    p = L.check_plan(ops, row)
    n_bits = L.n_bits(idx)
    x, n, delta, b = L.levels_inputs(shape, n_bits, SEED)
    assert float(n.abs().max()) == 2 ** n_bits - 1
    dcol = delta.double().view(1, -1, 1, 1)
    conv = C.forward_conv(x, n.double() * delta.double().view(-1, 1, 1, 1), k)          # the reference: float64 throughout
    xh, xl = C._split_bf16(x)
    ideal = C.forward_conv(xh + xl, n.double(), k) * dcol                                # the levels arithmetic, exactly
    xg, scale, bg = x.to(DEV), delta.to(DEV), b.to(DEV)
    wt = ops.levels_operand(n.to(DEV))
    for epi in epis:
        ry, rz = C.forward_reference(conv, b, epi)
        iy, iz = C.forward_reference(ideal, b, epi)
        gate = max(0.0 if ry is None else float(((iy - ry).abs() / C.bound(ry)).max()),
                   0.0 if rz is None else float(((iz - rz).abs() / C.bound(rz)).max()))
        y, z = L.run(ops, "bf16", xg, wt, scale, bg, shape, epi)
        assert (y is None) == (ry is None) and (z is None) == (rz is None)
        e_y, e_z = _ratio(y, ry), _ratio(z, rz)
        print(f"levels {IDS[idx]} {n_bits} bits {epi[0]} r {epi[1]} bias {int(epi[2])} tail {p['tail']}: exact arithmetic / bound "
              f"{gate:.4f}, y error / bound {e_y:.4f}, z error / bound {e_z:.4f}")
        assert gate <= C.IDEAL_MAX, f"{epi}: the exact levels arithmetic takes {gate:.3f} of the bound on this row"
        assert e_y <= 1.0, f"{epi}: y off by {e_y:.3f} x the bound"
        assert e_z <= 1.0, f"{epi}: z off by {e_z:.3f} x the bound"
    torch.cuda.synchronize()
    print(f"levels {IDS[idx]}: {time.time() - t0:.2f} s")


@pytest.mark.parametrize("idx", L.EXACT_IDX, ids=[IDS[i] for i in L.EXACT_IDX])
def test_exact_on_integer_inputs(ops, idx):
    L.check_exact_on_integer_inputs(ops, idx, "bf16", EXACT_SEED)


@pytest.mark.parametrize("shape,epi", L.TWO_CALLS)
def test_two_calls_agree_bit_for_bit(ops, shape, epi):
    L.check_two_calls_agree_bit_for_bit(ops, shape, epi, "bf16", SEED)


def test_levels_operand_refuses_inexact_weights(ops):
    n = torch.zeros(8, 8, 3, 3, device=DEV)
    n[0, 0, 0, 0], n[1, 2, 1, 1], n[7, 7, 2, 2] = 256.0, -256.0, 255.0
    assert ops.levels_operand(n).dtype == torch.uint8
    for bad in (0.5, 257.0, -300.0, float("nan")):
        m = n.clone()
        m[3, 4, 1, 2] = bad
        with pytest.raises(ValueError):
            ops.levels_operand(m)
    with pytest.raises(ValueError):
        ops.levels_operand(torch.zeros(8, 8, 7, 7, device=DEV))

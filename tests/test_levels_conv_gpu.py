"""The levels forward (nq_conv_forward3_levels: integer weights n = level - zero_point, two BF16 MFMAs per product, the quantiser
step applied per output channel in the epilogue) on every build of the tiled kernel.

Rows: every row of tests/conv3_cases.CASES whose plan is the unsplit tiled kernel, with its forward epilogues -- all 16
(k, mi, waves) builds, tail kinds 1..3 of both weight-staging families, every forward epilogue branch -- and, for the full last
chunk (tail kind 0) no such row has, four shapes per kernel size beside them.  The parametrisation is every tiled row with a
forward epilogue, read from the table alone; a row the plan splits over K is checked for being refused instead.

1. parity: against the float64 convolution of x with (level - zero_point) * delta at the project's bf16x3 bounds
   (conv3_cases.bound), after the arithmetic itself, evaluated exactly on the CPU, has been held to IDEAL_MAX of that bound on
   the very inputs -- a row that fails that gate FAILS, none drops out;
2. exactness: small-integer inputs and power-of-two steps make every product, sum, scale and bias add exact in fp32, so the output
   must equal the float64 computation bit for bit -- pins the indexing of weights, scale, bias and every epilogue's stores;
3. run-to-run identity;  4. what ops.levels_operand refuses."""
import ctypes
import math
import time

import pytest
import torch

import conv3_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
CODE = {"plain": 0, "psgelu": 1, "tanh": 2, "ps": 3}      # NQ_EPI_* (include/nq_hip.h)


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
# Every tiled row of the table that has a forward epilogue, taken from the table alone (nothing is asked of the library while
# the module is collected, and the test ids do not move with the plan).  The rows whose plan is the UNSPLIT tiled kernel are the
# ones the levels entry serves -- 34 today, counted below; on a split-K row the tests check that it is refused.
CANDIDATES = [(shape, inst, [e for e in epis if e[0] != "dgrad"]) for shape, inst, epis in C.CASES
              if inst[0] == "tiled" and any(e[0] != "dgrad" for e in epis)]
ROWS = CANDIDATES + EXTRA
IDS = [C.case_id(r) for r in ROWS]


@pytest.fixture(scope="module")
def ops():
    from neuroquant_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


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
    y = torch.empty(B, cout, H, W, device=DEV)
    rc = _lib.lib().nq_conv_forward3_levels(x.data_ptr(), ops.levels_operand(n).data_ptr(), scale.data_ptr(), None, y.data_ptr(),
                                            None, B, cin, H, W, cout, k, 1, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == -2
    with pytest.raises(_lib.NQLibraryError):
        ops.conv3_forward_levels_raw(x, ops.levels_operand(n), scale, None, cout, k, 0, 1)


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
    """(x, n, delta, b) on the CPU: activations, integer weights n = level - zero_point with both extreme levels in every
    output channel and both extreme zero points, steps that give the weights the scale of conv3_cases.forward_inputs"""
    B, cin, H, W, cout, k = shape
    g = C._gen(shape, 3)
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


def _run(ops, xg, wt, scale, bias, shape, epi):
    name, r, has_bias = epi
    return ops.conv3_forward_levels_raw(xg, wt, scale, bias if has_bias else None, shape[4], shape[5], CODE[name], r)


def _ratio(got, ref):
    return 0.0 if ref is None else float(((got.detach().cpu().double() - ref).abs() / C.bound(ref)).max())


@pytest.mark.parametrize("idx", range(len(ROWS)), ids=IDS)
def test_parity_to_float64(ops, idx):
    row = ROWS[idx]
    shape, inst, epis = row
    B, cin, H, W, cout, k = shape
    t0 = time.time()
    if not _unsplit_tiled(_plan(shape)):
        return _refused(ops, row)
    p = _check_plan(ops, row)
    n_bits = 2 + sum(_unsplit_tiled(_plan(r[0])) for r in ROWS[:idx]) % 7      # 2 .. 8, cycling over the rows that are served
    x, n, delta, b = _levels_inputs(shape, n_bits)
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
        y, z = _run(ops, xg, wt, scale, bg, shape, epi)
        assert (y is None) == (ry is None) and (z is None) == (rz is None)
        e_y, e_z = _ratio(y, ry), _ratio(z, rz)
        print(f"levels {IDS[idx]} {n_bits} bits {epi[0]} r {epi[1]} bias {int(epi[2])} tail {p['tail']}: exact arithmetic / bound "
              f"{gate:.4f}, y error / bound {e_y:.4f}, z error / bound {e_z:.4f}")
        assert gate <= C.IDEAL_MAX, f"{epi}: the exact levels arithmetic takes {gate:.3f} of the bound on this row"
        assert e_y <= 1.0, f"{epi}: y off by {e_y:.3f} x the bound"
        assert e_z <= 1.0, f"{epi}: z off by {e_z:.3f} x the bound"
    torch.cuda.synchronize()
    print(f"levels {IDS[idx]}: {time.time() - t0:.2f} s")


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
    g = C._gen(shape, 4)
    x = torch.randint(-4, 5, (B, cin, H, W), generator=g).float()
    lv = torch.randint(0, 256, (cout, cin, k, k), generator=g)
    lv.view(cout, -1)[:, 0] = 0
    lv.view(cout, -1)[:, 1] = 255
    zp = torch.randint(0, 256, (cout,), generator=g)
    zp[0], zp[-1] = 0, 255
    n = (lv - zp.view(-1, 1, 1, 1)).float()
    assert float(n.max()) == 255 and float(n.min()) == -255
    delta = torch.tensor([2.0 ** -(co % 7) for co in range(cout)])
    b = torch.randint(-8, 9, (cout,), generator=g).float() * delta
    conv = C.forward_conv(x, n, k) * delta.double().view(1, -1, 1, 1)        # integers times a power of two: exact
    assert float(conv.abs().max()) < 2 ** 24
    xg, scale, bg = x.to(DEV), delta.to(DEV), b.to(DEV)
    wt = ops.levels_operand(n.to(DEV))
    for epi in _exact_epis(epis):
        ry, rz = C.forward_reference(conv, b, epi)
        y, z = _run(ops, xg, wt, scale, bg, shape, epi)
        for got, ref in ((y, ry), (z, rz)):
            assert (got is None) == (ref is None)
            if ref is not None:
                want = ref.float()
                assert torch.equal(want.double(), ref), "the reference itself is not exact in fp32"
                assert torch.equal(got.cpu(), want), f"{epi}: {int((got.cpu() != want).sum())} of {want.numel()} outputs differ"


@pytest.mark.parametrize("shape,epi", [((2, 7, 169, 67, 17, 3), ("plain", 1, True)), ((2, 7, 169, 67, 36, 5), ("ps", 2, True)),
                                       ((2, 7, 81, 67, 99, 3), ("psgelu", 3, True))])
def test_two_calls_agree_bit_for_bit(ops, shape, epi):
    """one register-staged tile (mi 2) and two LDS-DMA tiles (mi 3, mi 4)"""
    p = _plan(shape)
    assert _unsplit_tiled(p) and (p["mi"] <= 2) == (shape[4] == 17)
    x, n, delta, b = _levels_inputs(shape, 5)
    xg, scale, bg = x.to(DEV), delta.to(DEV), b.to(DEV)
    wt = ops.levels_operand(n.to(DEV))
    first = _run(ops, xg, wt, scale, bg, shape, epi)
    again = _run(ops, xg, ops.levels_operand(n.to(DEV)), scale, bg, shape, epi)
    for a, c in zip(first, again):
        assert (a is None and c is None) or torch.equal(a.view(torch.int32), c.view(torch.int32))


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

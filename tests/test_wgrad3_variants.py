"""Every template instantiation of the bf16x3 weight-gradient kernels (conv_wgrad3_impl.h: 47 per kernel size) against a
float64 reference, on the shape tests/wgrad3_cases.py records for it: ragged W, Cout and Cin*k*k, frame boundaries inside a
split, several tiles, uneven splits (tests/test_wgrad3_plan_cpu.py asserts those properties of the table, host-only).
Per case: accuracy at the project's bounds (those of test_hip_parity.py::test_wgrad_bf16x3), run-to-run identity, split-word
operands, the deferred reduction, and for the narrow problems the role-swapped entry point that reaches them in the decoder."""
import ctypes

import pytest
import torch

from wgrad3_cases import ALL_PCS, CASES, EXTRA_CASES, case_id, db_bound, dw_bound, inputs, reference, swapped_reference

pytestmark = pytest.mark.gpu

DEV = "cuda"
# one case per pc also runs without a bias gradient: the first of the table
NO_DB = {next(i for i, (_, inst) in enumerate(CASES) if inst[2] == pc) for pc in ALL_PCS}
RUN = CASES + EXTRA_CASES


@pytest.fixture(scope="module")
def ops():
    from neuroquant_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def _plan(B, cin, H, W, cout, k):
    from neuroquant_amd import _lib
    v = [ctypes.c_int() for _ in range(4)]
    assert _lib.lib().nq_conv_wgrad3_plan(B, cin, H, W, cout, k, *[ctypes.byref(t) for t in v]) == 0
    return tuple(t.value for t in v)      # (mi, ni, nsplit, pc)


def _worst(got, ref, bound):
    """largest error as a fraction of its bound (<= 1 passes)"""
    return float(((got.detach().cpu().double() - ref).abs() / bound).max())


@pytest.mark.parametrize("idx", range(len(RUN)), ids=[case_id(c) + ("" if i < len(CASES) else f"-w{c[0][3]}") for i, c in enumerate(RUN)])
def test_variant(ops, idx):
    shape, (mi, ni, pc) = RUN[idx]
    B, cin, H, W, cout, k = shape
    pmi, pni, nsplit, ppc = _plan(*shape)
    assert (pmi, pni, ppc) == (mi, ni, pc), "the plan no longer sends this shape to the instantiation it is listed for"
    x, dy = inputs(shape)
    ref_dw, ref_db = reference(x, dy, k)
    xg, dyg = x.to(DEV), dy.to(DEV)

    # accuracy
    dw, db = ops.conv_wgrad3_raw(xg, dyg, cout, k, True)
    e_dw, e_db = _worst(dw, ref_dw, dw_bound(ref_dw)), _worst(db, ref_db, db_bound(ref_db))
    print(f"wgrad3 {case_id(RUN[idx])} {shape} nsplit {nsplit}: dw error / bound {e_dw:.4f}, db error / bound {e_db:.4f}")
    assert e_dw <= 1.0, f"dw off by {e_dw:.3f} x the bound"
    assert e_db <= 1.0, f"db off by {e_db:.3f} x the bound"

    # run-to-run identity
    dw2, db2 = ops.conv_wgrad3_raw(xg, dyg, cout, k, True)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)

    # split {hi | lo} word operands: the same bits
    io = ops.conv_wgrad3_split_io(*shape)
    assert io == (3 if pc in (1, 12, 14) else 0)
    if io == 3:
        xs, ds = ops.split_words(xg), ops.split_words(dyg)
        for fmt, xa, da in ((1, xs, dyg), (2, xg, ds), (3, xs, ds)):
            dwf, dbf = ops.conv_wgrad3_raw(xa, da, cout, k, True, fmt=fmt)
            assert torch.equal(dw, dwf), f"fmt {fmt}"
            if fmt == 1:
                assert torch.equal(db, dbf)

    # deferred reduction: the split kernel now, one multi-tensor reduction at flush()
    pend = ops.PendingReductions()
    dwd, dbd = ops.conv_wgrad3_raw(xg, dyg, cout, k, True, defer=pend)
    pend.flush()
    assert torch.equal(dw, dwd) and torch.equal(db, dbd)

    # no bias gradient
    if idx in NO_DB:
        dwn, dbn = ops.conv_wgrad3_raw(xg, dyg, cout, k, False)
        assert dbn is None and torch.equal(dw, dwn)
        pend = ops.PendingReductions()
        dwn, dbn = ops.conv_wgrad3_raw(xg, dyg, cout, k, False, defer=pend)
        pend.flush()
        assert dbn is None and torch.equal(dw, dwn)

    # The narrow problems are reached through the role-swapped entry: this case is the exchanged problem of the convolution
    # dy (cout channels) -> x (cin <= 4 channels), whose weight gradient is the tap-reversed transpose of ref_dw (anchored
    # in the CPU file); the reduction writes it in that order.
    if cin * k * k <= 64 and cin <= 4:
        assert ops.conv_wgrad_swapped3_supported(B, cout, H, W, cin, k)
        ref_sw = swapped_reference(ref_dw)
        dws, _ = ops.conv_wgrad_swapped3(dyg, xg, cin, k, False)
        e_sw = _worst(dws, ref_sw, dw_bound(ref_sw))
        print(f"wgrad3 {case_id(RUN[idx])} swapped: dw error / bound {e_sw:.4f}")
        assert e_sw <= 1.0, f"swapped dw off by {e_sw:.3f} x the bound"
        pend = ops.PendingReductions()
        dwsd, _ = ops.conv_wgrad_swapped3(dyg, xg, cin, k, False, defer=pend)
        pend.flush()
        assert torch.equal(dws, dwsd)


@pytest.mark.parametrize("pc", (1, 12, 14))
def test_split_word_operands_direct_and_deferred(ops, pc):
    """fmt = 3 of nq_conv_wgrad3, with and without a pending reduction, on the smallest table row of each row-segment
    producer/consumer kernel: dw has the bits of the float call, db (summed from hi + lo of dy) stays within the table's bound"""
    shape, _ = min((c for c in CASES if c[1][2] == pc), key=lambda c: c[0][0] * (c[0][1] + c[0][4]) * c[0][2] * c[0][3])
    B, cin, H, W, cout, k = shape
    assert _plan(*shape)[3] == pc and ops.conv_wgrad3_split_io(*shape) == 3
    x, dy = inputs(shape)
    ref_db = dy.double().sum((0, 2, 3))       # reference()'s db (anchored in the CPU file), without its dw
    xg, dyg = x.to(DEV), dy.to(DEV)
    xs, ds = ops.split_words(xg), ops.split_words(dyg)
    dw, db = ops.conv_wgrad3_raw(xg, dyg, cout, k, True)
    dwf, dbf = ops.conv_wgrad3_raw(xs, ds, cout, k, True, fmt=3)
    pend = ops.PendingReductions()
    dwd, dbd = ops.conv_wgrad3_raw(xs, ds, cout, k, True, defer=pend, fmt=3)
    pend.flush()
    assert torch.equal(dw, dwf) and torch.equal(dw, dwd)
    assert torch.equal(dbf, dbd)
    e_db, d_db = _worst(dbf, ref_db, db_bound(ref_db)), _worst(dbf, db.cpu().double(), db_bound(ref_db))
    print(f"wgrad3 fmt 3 pc {pc} {shape}: db error / bound {e_db:.4f}, db against the float call / bound {d_db:.4f}")
    assert e_db <= 1.0 and d_db <= 1.0


@pytest.mark.parametrize("shape", [(1, 2500, 8, 8, 3, 3), (2, 2432, 8, 16, 3, 3), (2, 2700, 8, 16, 1, 5)])
def test_swapped_entries_refuse_few_pixel_shapes(ops, shape):
    """(B, cin, H, W, cout, k) of heads whose exchanged problem belongs to the few-pixel kernel: the library sizes a 4-float
    token for it, and the role-swapped C entry refuses, direct and deferred, before anything is launched.  The workspace handed over here holds
    the slabs the launch used to write, so that a regression fails this test instead of writing out of bounds."""
    from neuroquant_amd import _lib
    B, cin, H, W, cout, k = shape
    lib = _lib.lib()
    assert lib.nq_conv_wgrad3_ws_floats(B, cout, H, W, cin, k) == 4
    assert not ops.conv_wgrad_swapped3_supported(*shape)
    mi, ni, nsplit, pc = _plan(B, cout, H, W, cin, k)
    ct, nt = -(-cin // (16 * mi)), -(-cout * k * k // (64 * ni))
    x, dy = inputs(shape)
    xg, dyg = x.to(DEV), dy.to(DEV)
    ws = torch.zeros(nsplit * ct * 16 * mi * (nt * 64 * ni + 1), device=DEV)
    dw = torch.full((cout, cin, k, k), 7.0, device=DEV)

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    assert lib.nq_conv_wgrad3_swapped(p(xg), p(dyg), p(dw), p(ws), B, cin, H, W, cout, k, None, None) == -2
    seg = _lib.WgrSeg()
    assert lib.nq_conv_wgrad3_swapped(p(xg), p(dyg), p(dw), p(ws), B, cin, H, W, cout, k, ctypes.byref(seg), None) == -2
    torch.cuda.synchronize()
    assert float(ws.abs().max()) == 0.0 and bool((dw == 7.0).all())
    # the layer still gets its gradient: the fp32 kernel, where ops._wgrad_plain now sends it
    ref_dw, _ = reference(x, dy, k)
    got = ops._wgrad_plain(xg, dyg, k)
    assert _worst(got, ref_dw, dw_bound(ref_dw)) <= 1.0

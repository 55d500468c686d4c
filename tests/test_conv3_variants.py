"""Every template instantiation of the bf16x3 forward / data-gradient kernels (conv_igemm3_impl.h: 14 per kernel size with the
split-word-input builds; conv_flat3.hip: 7 + 4) against a float64 reference, on the shapes tests/conv3_cases.py records for them:
ragged tiles on every side, every tail chunk kind behind an even and an odd number of full chunks, uneven splits, both builds of
nq_conv_splitk_finish, every epilogue branch (tests/test_conv3_plan_cpu.py asserts those properties of the table, host-only).
Per row and epilogue: accuracy at the bounds of test_hip_parity.py::test_conv_bf16x3, run-to-run identity, split-word input and
output where the shape offers them, refusal where it does not."""
import ctypes
import time

import pytest
import torch

import conv3_cases as C
from conv3_cases import CASES, FORMERLY_REFUSED, case_id

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from neuroquant_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def _plan(shape):
    from neuroquant_amd import _lib
    q = _lib.Conv3Plan()
    assert _lib.lib().nq_conv_forward3_plan(*shape, ctypes.byref(q)) == 0
    return {n: getattr(q, n) for n, _ in q._fields_}


def _worst(got, ref):
    """largest error as a fraction of its bound (<= 1 passes)"""
    return float(((got.detach().cpu().double() - ref).abs() / C.bound(ref)).max())


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_variant(ops, idx):
    shape, inst, epis = CASES[idx]
    B, cin, H, W, cout, k = shape
    t0 = time.time()
    p = _plan(shape)
    assert C.inst_of(p) == inst, "the plan no longer sends this shape to the instantiation it is listed for"
    io = ops.conv3_split_io(*shape)
    assert io == p["split_io"]
    code = {"plain": ops.EPI_PLAIN, "tanh": ops.EPI_TANH, "psgelu": ops.EPI_PS_GELU, "ps": ops.EPI_PS, "dgrad": ops.EPI_DGRAD_GELU}
    fwd = dg = None
    for epi in epis:
        name, r, bias = epi
        if name == "dgrad":
            if dg is None:
                x, wst, zprev = C.dgrad_inputs(shape)
                dg = (x.to(DEV), ops.weight_layout3(wst.to(DEV), transposed=True), zprev.to(DEV), C.dgrad_conv(x, wst, shape), zprev)
            xg, wt3, zp, conv, zprev = dg
            ref_y, ref_z, bg = C.dgrad_reference(conv, zprev, r), None, None
        else:
            if fwd is None:
                x, w, b = C.forward_inputs(shape)
                fwd = (x.to(DEV), ops.weight_layout3(w.to(DEV)), b.to(DEV), C.forward_conv(x, w, k), b)
            xg, wt3, bdev, conv, b = fwd
            ref_y, ref_z = C.forward_reference(conv, b, epi)
            zp, bg = None, (bdev if bias else None)

        def run(xin, fmt=0):
            return ops.conv3_forward_raw(xin, wt3, bg, cout, k, code[name], r, zprev=zp, fmt=fmt)

        # accuracy
        y, z = run(xg)
        assert (y is None) == (ref_y is None) and (z is None) == (ref_z is None)
        e_y = _worst(y, ref_y) if y is not None else 0.0
        e_z = _worst(z, ref_z) if z is not None else 0.0
        print(f"conv3 {case_id(CASES[idx])} {name} r {r} bias {int(bias)} nsplit {p['nsplit']} tail {p['tail']}: "
              f"y error / bound {e_y:.4f}, z error / bound {e_z:.4f}")
        assert e_y <= 1.0, f"{epi}: y off by {e_y:.3f} x the bound"
        assert e_z <= 1.0, f"{epi}: z off by {e_z:.3f} x the bound"

        def same(a, b_):
            return (a is None and b_ is None) or torch.equal(_bits(a), _bits(b_))

        # run-to-run identity
        y2, z2 = run(xg)
        assert same(y, y2) and same(z, z2), f"{epi}: a second call differs"

        # split {hi | lo} word input: the same bits
        if io & C.X_SPLIT:
            xs = ops.split_words(xg)
            y1, z1 = run(xs, C.X_SPLIT)
            assert same(y, y1) and same(z, z1), f"{epi}: split-word input changes the result"
        else:
            with pytest.raises(Exception):
                run(xg, C.X_SPLIT)
        # split-word output: the split of the float output, z untouched
        if io & C.Y_SPLIT:
            ys, zs = run(xg, C.Y_SPLIT)
            assert same(z, zs), f"{epi}: split-word output changes z"
            if y is not None:
                assert torch.equal(_bits(ops.split_words(y)), _bits(ys)), f"{epi}: split-word output is not the split of y"
            if io & C.X_SPLIT:
                ys2, zs2 = run(ops.split_words(xg), C.X_SPLIT | C.Y_SPLIT)
                assert same(ys, ys2) and same(zs, zs2), f"{epi}: split words on both sides"
        else:
            with pytest.raises(Exception):
                run(xg, C.Y_SPLIT)
    torch.cuda.synchronize()
    print(f"conv3 {case_id(CASES[idx])}: {time.time() - t0:.2f} s")


@pytest.mark.parametrize("shape", FORMERLY_REFUSED)
def test_formerly_refused_shapes_are_computed(ops, shape):
    """few-pixel shapes nq_conv3_supported offered although their launch could not fit the LDS: ops routed them to the bf16x3
    path and raised.  They are no longer offered, and the routed convolution and data gradient (the fp32 kernels) hold the same bounds."""
    B, cin, H, W, cout, k = shape
    assert not ops.conv3_supported(*shape)
    x, w, _ = C.forward_inputs(shape)
    got = ops._conv_plain(x.to(DEV), w.to(DEV))
    e = _worst(got, C.forward_conv(x, w, k))
    xd, wst, _ = C.dgrad_inputs(shape)
    gd = ops._dgrad_plain(xd.to(DEV), wst.to(DEV))
    ed = _worst(gd, C.dgrad_conv(xd, wst, shape))
    print(f"conv3 formerly refused {shape}: forward error / bound {e:.4f}, data gradient error / bound {ed:.4f}")
    assert e <= 1.0 and ed <= 1.0

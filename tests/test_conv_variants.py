"""Every build of the exact-fp32 convolution family -- conv_igemm<MI> (10 per kernel size 1 / 3 / 5) on its own epilogues and
behind both builds of the finish kernel, tiny_pw_fwd<KSL>, the streaming and the LDS-staged head forward and data gradient (all 16
head_dgrad_kernel builds), conv_wgrad<MI, NI> (10 per kernel size) and tiny_pw_wgrad -- against a float64 reference, on the
shapes tests/conv_cases.py records for them (tests/test_conv_plan_cpu.py asserts the properties of the tables, host-only).
Per row and entry: the plan is the recorded one; accuracy at the bounds of the bf16x3 tables (tests/conv3_cases.py,
tests/wgrad3_cases.py: "error at the fp32 level"); a second call, with outputs and workspace supplied by the test, is bit-identical,
leaves the output the epilogue does not own untouched and writes nothing behind the workspace the size query asked for;
split-word output where the plan offers it, refusal where it does not; the deferred weight-gradient reduction has the bits of the
immediate one."""
import ctypes
import time

import pytest
import torch

import conv3_cases as C3
import conv_cases as C
import wgrad3_cases as W3
from conv_cases import EXTRA_FWD_CASES, FWD_CASES, WGRAD_CASES, case_id

pytestmark = pytest.mark.gpu

DEV = "cuda"
ALL_FWD = FWD_CASES + EXTRA_FWD_CASES
SENTINEL = 12345.678
GUARD = 4096        # floats kept behind the workspace


@pytest.fixture(scope="module")
def ops():
    from neuroquant_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def _fwd_plan(shape, epi):
    from neuroquant_amd import _lib
    B, cin, H, W, cout, k = shape
    q = _lib.ConvPlan()
    assert _lib.lib().nq_conv_forward_plan(B, cin, H, W, cout, k, epi[1], C.EPI_CODE[epi[0]], int(epi[2]), ctypes.byref(q)) == 0
    return {n: getattr(q, n) for n, _ in q._fields_}


def _wgrad_plan(shape):
    from neuroquant_amd import _lib
    q = _lib.ConvWgradPlan()
    assert _lib.lib().nq_conv_wgrad_plan(*shape, ctypes.byref(q)) == 0
    return {n: getattr(q, n) for n, _ in q._fields_}


def _worst(got, ref, bound):
    """largest error as a fraction of its bound (<= 1 passes)"""
    return float(((got.detach().cpu().double() - ref).abs() / bound).max())


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(_bits(a), _bits(b)))


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _sentinel(shape_or_n):
    return torch.full(shape_or_n if isinstance(shape_or_n, tuple) else (shape_or_n,), SENTINEL, device=DEV)


def _untouched(t):
    return bool((t == SENTINEL).all())


def _direct_forward(x, wt, dims, bias, shape, code, r, zprev, like_y, like_z, nws):
    """nq_conv_forward on buffers of the test: (y, z, other, guard ok?) -- y / z sentinel-filled before the launch, `other` the
    output this epilogue must not write (handed over all the same), the workspace followed by a guard band"""
    from neuroquant_amd import _lib
    B, cin, H, W, cout, k = shape
    y = _sentinel(tuple(like_y.shape)) if like_y is not None else None
    z = _sentinel(tuple(like_z.shape)) if like_z is not None else None
    other = _sentinel((B, cout, H, W))
    ws = _sentinel(nws + GUARD)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib().nq_conv_forward(_p(x), _p(wt), _p(bias), _p(y if y is not None else other), _p(z if z is not None else other),
                                    _p(ws), B, cin, H, W, cout, k, dims[0], dims[1], r, code, _p(zprev), stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return y, z, other, _untouched(ws[nws:])


@pytest.mark.parametrize("idx", range(len(ALL_FWD)), ids=[case_id(c) for c in ALL_FWD])
def test_forward_variant(ops, idx, monkeypatch):
    shape, inst, epis = ALL_FWD[idx]
    B, cin, H, W, cout, k = shape
    t0 = time.time()
    fwd = dg = None
    for epi in epis:
        name, r, bias = epi
        code = C.EPI_CODE[name]
        with monkeypatch.context() as m:
            for n, v in C.env_of(shape, inst, epi).items():
                m.setenv(n, v)
            p = _fwd_plan(shape, epi)
            assert C.inst_of(p) == inst, f"{epi}: the plan no longer sends this call to the build it is listed for"
            if name == "dgrad":
                if dg is None:
                    x, wst, zprev = C3.dgrad_inputs(shape)
                    _, _, wb, db_ = ops.weight_layouts(wst.to(DEV), True)
                    dg = (x.to(DEV), wb, db_, zprev.to(DEV), C3.dgrad_conv(x, wst, shape), zprev)
                xg, wt, dims, zp, conv, zprev = dg
                ref_y, ref_z, bg = C3.dgrad_reference(conv, zprev, r), None, None
            else:
                if fwd is None:
                    x, w, b = C3.forward_inputs(shape)
                    wf, df, _, _ = ops.weight_layouts(w.to(DEV), False)
                    fwd = (x.to(DEV), wf, df, b.to(DEV), C3.forward_conv(x, w, k), b)
                xg, wt, dims, bdev, conv, b = fwd
                ref_y, ref_z = C3.forward_reference(conv, b, epi)
                zp, bg = None, (bdev if bias else None)

            # accuracy
            y, z = ops.conv_forward_raw(xg, wt, dims, bg, cout, k, code, r, zprev=zp)
            assert (y is None) == (ref_y is None) and (z is None) == (ref_z is None)
            e_y = _worst(y, ref_y, C3.bound(ref_y)) if y is not None else 0.0
            e_z = _worst(z, ref_z, C3.bound(ref_z)) if z is not None else 0.0
            print(f"conv {case_id(ALL_FWD[idx])} {name} r {r} bias {int(bias)} nsplit {p['nsplit']} finish {p['finish']}: "
                  f"y error / bound {e_y:.4f}, z error / bound {e_z:.4f}")
            assert e_y <= 1.0, f"{epi}: y off by {e_y:.3f} x the bound"
            assert e_z <= 1.0, f"{epi}: z off by {e_z:.3f} x the bound"

            # a second call on the test's own buffers: the same bits, nothing written that the epilogue does not own
            assert p["ws_floats"] == ops._q("nq_conv_forward_ws_floats", *shape)
            y2, z2, other, guard_ok = _direct_forward(xg, wt, dims, bg, shape, code, r, zp, y, z, p["ws_floats"])
            assert _same(y, y2) and _same(z, z2), f"{epi}: a second call differs"
            assert _untouched(other), f"{epi}: an output this epilogue does not own was written"
            assert guard_ok, f"{epi}: the launch wrote behind the {p['ws_floats']} floats of workspace it asked for"

            # split-word output: the split of the float output where the plan offers it, refused where not
            assert ops.conv_split_out(B, cin, H, W, cout, k, r, code, bias) == bool(p["split_out"])
            if p["split_out"]:
                ys, _ = ops.conv_forward_raw(xg, wt, dims, bg, cout, k, code, r, zprev=zp, fmt=C.Y_SPLIT)
                assert torch.equal(_bits(ops.split_words(y)), _bits(ys)), f"{epi}: split-word output is not the split of y"
            else:
                with pytest.raises(Exception):
                    ops.conv_forward_raw(xg, wt, dims, bg, cout, k, code, r, zprev=zp, fmt=C.Y_SPLIT)
    torch.cuda.synchronize()
    print(f"conv {case_id(ALL_FWD[idx])}: {time.time() - t0:.2f} s")


@pytest.mark.parametrize("idx", range(len(WGRAD_CASES)), ids=[case_id(c) for c in WGRAD_CASES])
def test_wgrad_variant(ops, idx):
    from neuroquant_amd import _lib
    shape, inst, dbs = WGRAD_CASES[idx]
    B, cin, H, W, cout, k = shape
    t0 = time.time()
    p = _wgrad_plan(shape)
    assert C.wgrad_inst_of(p) == inst, "the plan no longer sends this shape to the build it is listed for"
    x, dy = W3.inputs(shape)
    ref_dw, ref_db = W3.reference(x, dy, k)
    xg, dyg = x.to(DEV), dy.to(DEV)

    # accuracy
    dw, db = ops.conv_wgrad_raw(xg, dyg, cout, k, True)
    e_dw, e_db = _worst(dw, ref_dw, W3.dw_bound(ref_dw)), _worst(db, ref_db, W3.db_bound(ref_db))
    print(f"conv wgrad {case_id(WGRAD_CASES[idx])} nsplit {p['nsplit']} of {p['nseg']} segments: dw error / bound {e_dw:.4f}, "
          f"db error / bound {e_db:.4f}")
    assert e_dw <= 1.0, f"dw off by {e_dw:.3f} x the bound"
    assert e_db <= 1.0, f"db off by {e_db:.3f} x the bound"

    # a second call on the test's own buffers: the same bits, nothing behind the workspace
    nws = p["ws_floats"]
    assert nws == ops._q("nq_conv_wgrad_ws_floats", *shape)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for want_db in (True, False) if False in dbs else (True,):
        ws, dw2, db2 = _sentinel(nws + GUARD), _sentinel(tuple(dw.shape)), _sentinel(cout)
        rc = _lib.lib().nq_conv_wgrad(_p(xg), _p(dyg), _p(dw2), _p(db2) if want_db else None, _p(ws), B, cin, H, W, cout, k, None, stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert _same(dw, dw2), f"db {want_db}: a second call differs"
        assert _same(db, db2) if want_db else _untouched(db2)
        assert _untouched(ws[nws:]), f"the launch wrote behind the {nws} floats of workspace it asked for"

    # deferred reduction: the split kernel now, one multi-tensor reduction at flush()
    for want_db in dbs:
        pend = ops.PendingReductions()
        dwd, dbd = ops.conv_wgrad_raw(xg, dyg, cout, k, want_db, defer=pend)
        pend.flush()
        assert _same(dw, dwd) and (_same(db, dbd) if want_db else dbd is None), f"db {want_db}: the deferred reduction differs"
    torch.cuda.synchronize()
    print(f"conv wgrad {case_id(WGRAD_CASES[idx])}: {time.time() - t0:.2f} s")

"""GPU tests of the parameter-side kernels at their edge shapes: the quantisers, the rounding regulariser, Adam, the Hadamard
transform and the launches fused with it, the step prologue and the small reductions around the loss -- every HIP result
against the oracle (oracle/nq_oracle.py) or the restatements of tests/param_ref.py, never against another HIP kernel.

Tolerances (param_ref.py holds the figures, taken from tests/test_hip_parity.py):
  - integer-grid / clamp / round / gather / copy arithmetic, the transform in the oracle's butterfly order: bit-exact;
  - soft forward, d(alpha), alpha0, regulariser gradient: the figures of test_adaround_kernels / test_round_regulariser_kernels,
    applied term by term (a relative figure on a sum of two terms is wrong where they cancel);
  - Adam: the figures of test_adam_kernel on the parameters; the moments by the gradient's bound carried through the recursion;
  - sums: SUM_RTOL = 1e-5 of sum |term|, computed in float64 from the oracle's fp32 terms (the project's bar is 1e-4).
Nothing is masked: the inputs come from param_ref's generators, which keep every element off the discontinuities;
tests/test_param_ref_cpu.py asserts that with an exclusion count of zero.  Each check prints its worst error / bound ratio.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import param_ref as R
from oracle import nq_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from neuroquant_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


@pytest.fixture(scope="module")
def lib():
    from neuroquant_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def multi():
    return R.multi_case()


@pytest.fixture(scope="module")
def fused():
    cache = {}

    def get(per_row):
        if per_row not in cache:
            cache[per_row] = R.fused_case(per_row)
        return cache[per_row]

    return get


def G(t):
    return t.to(DEV)


def exact(got, want, what=""):
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    np.testing.assert_array_equal(got.detach().cpu().numpy(), want.detach().cpu().numpy(), err_msg=what)


def within(got, want, bound, what=""):
    """|got - want| <= bound for EVERY element (bound: tensor or number); prints the worst error / bound ratio first"""
    got = got.detach().cpu().double().reshape(-1)
    want = torch.as_tensor(want).detach().cpu().double().reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bound = torch.as_tensor(bound, dtype=torch.float64).detach().cpu().reshape(-1).expand_as(want)
    assert torch.isfinite(got).all() and torch.isfinite(want).all(), what
    err = (got - want).abs()
    ratio = err / bound.clamp_min(1e-300)
    ratio[(err == 0)] = 0
    worst = int(ratio.argmax()) if ratio.numel() else 0
    print(f"{what}: worst error / bound {float(ratio.max()):.3g} (error {float(err[worst]):.3g}, value {float(want[worst]):.6g})")
    assert bool((err <= bound).all()), (what, worst, float(got[worst]), float(want[worst]), float(bound[worst]))


def sum_close(got, want64, abs_sum, what=""):
    within(got, want64, R.SUM_RTOL * torch.as_tensor(abs_sum, dtype=torch.float64) + 1e-30, what)


class Arena:
    """One flat, densely packed GPU buffer (the gradient arena of data-parallel runs): tensors cut from it start 1, 2 or 3
    floats past a 16-byte boundary, so the multi-tensor kernels take their scalar (`vec == 0`) branch, tail included."""

    def __init__(self, numel, count):
        self.buf = torch.zeros(numel + 8 * count + 8, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.pos = 0

    def put(self, t, off):
        start = (self.pos + 3) // 4 * 4 + off
        v = self.buf[start:start + t.numel()].view(t.shape)
        v.copy_(t)
        self.pos = start + t.numel()
        assert v.data_ptr() % 16 == 4 * off and v.is_contiguous()
        return v


def placed(tensors, mode, which):
    """tensors: list (one per segment) of dicts of GPU tensors.  mode 'own': as they are (each its own allocation); else the
    entries named in `which[mode]` become views of one arena at float offsets 1, 2, 3 in turn."""
    if mode == "own":
        return tensors
    names = which[mode]
    arena = Arena(sum(t[n].numel() for t in tensors for n in names), len(tensors) * len(names))
    out = []
    for k, t in enumerate(tensors):
        t = dict(t)
        for n in names:
            t[n] = arena.put(t[n], 1 + k % 3)
        out.append(t)
    return out


# ================================================================================================ single-tensor quantisers
@pytest.fixture(scope="module")
def single():
    cache = {}

    def get(shape, per_row, nb):
        key = (shape, per_row, nb)
        if key not in cache:
            cache[key] = R.single_case(*shape, per_row, nb)
        return cache[key]

    return get


@pytest.mark.parametrize("nb", R.SINGLE_BITS)
@pytest.mark.parametrize("per_row", (True, False), ids=("per_row", "scalar"))
@pytest.mark.parametrize("shape", R.SINGLE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_single_tensor_quantisers(ops, single, shape, per_row, nb):
    """every tensor in its own allocation (the cases and ids this test has always had; the checks: _single_tensor_quantisers)"""
    _single_tensor_quantisers(ops, single, shape, per_row, nb, "own")


@pytest.mark.parametrize("place", (1, 2, 3), ids=lambda p: f"at{p}")
@pytest.mark.parametrize("nb", R.SINGLE_BITS)
@pytest.mark.parametrize("per_row", (True, False), ids=("per_row", "scalar"))
@pytest.mark.parametrize("shape", R.SINGLE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_single_tensor_quantisers_in_an_arena(ops, single, shape, per_row, nb, place):
    """the placement parameter of test_single_tensor_quantisers: 1, 2, 3 floats past a 16-byte boundary"""
    _single_tensor_quantisers(ops, single, shape, per_row, nb, place)


def _single_tensor_quantisers(ops, single, shape, per_row, nb, place):
    """scale_init / uaq_fwd / uaq_bwd / adaround_alpha_init / adaround_fwd / adaround_bwd of quant.hip at row lengths on both
    sides of one reduction pass (256) and of one block of 1024 elements, per-row and scalar scale.  The single-tensor entries
    are one-segment launches of the multi-tensor kernels: `place` puts x, gy, alpha and the outputs passed through out= each in
    its own allocation (16-byte accesses, the row lookup across a thread's four elements) or 1, 2, 3 floats past a 16-byte
    boundary of one arena (the element-by-element branch); want_dx / want_xq run the two instantiations only they launch."""
    c = single(shape, per_row, nb)
    nl, tag = c["nl"], f"{shape} per_row={per_row} bits={nb} place={place}"
    x, gy, alpha = G(c["x"]), G(c["gy"]), G(c["alpha"])
    outs = [None] * 4
    if place != "own":
        arena = Arena(7 * x.numel(), 7)
        x, gy, alpha = (arena.put(t, place) for t in (x, gy, alpha))
        outs = [arena.put(torch.full_like(x, -77.0), place) for _ in range(4)]
    # ---- UAQ
    d0, z0 = ops.scale_init_max(x, nl, per_row)
    exact(d0, c["d0"], "scale_init delta " + tag)
    exact(z0, c["z0"], "scale_init zp " + tag)
    d0, z0 = G(c["d0"]), G(c["z0"])
    exact(ops.uaq_forward(x, d0, z0, nl, out=outs[0]), O.uaq_fake_quant(c["x"], c["d0"], c["z0"], nl), "uaq_forward " + tag)
    dd, dx = ops.uaq_backward(x, gy, d0, z0, nl, want_dx=True)
    t = R.uaq_ddelta_terms(c["x"], c["gy"], c["d0"], c["z0"], nl).double()
    dims = (1, 2, 3) if per_row else (0, 1, 2, 3)
    assert dd.shape == d0.shape
    sum_close(dd, t.sum(dims), t.abs().sum(dims), "uaq_backward d(delta) " + tag)
    exact(dx, R.uaq_dx(c["x"], c["gy"], c["d0"], c["z0"], nl), "uaq_backward dx " + tag)
    exact(ops.uaq_backward(x, gy, d0, z0, nl), dd, "uaq_backward without dx " + tag)      # the other instantiation: same sums
    # ---- AdaRound init
    d, z, a0 = ops.adaround_init(x, d0, z0)
    exact(d, c["d"], "adaround_init delta " + tag)
    exact(z, c["z"], "adaround_init zp " + tag)
    within(a0, c["a0"], R.ALPHA0_RTOL * c["a0"].abs() + R.ALPHA0_ATOL, "alpha0 " + tag)
    # ---- AdaRound forward / backward
    d, z = G(c["d"]), G(c["z"])
    yh, xqh = ops.adaround_forward(x, alpha, d, z, nl, False, want_xq=True, out=outs[1])
    rh, rxh = O.adaround_fake_quant(c["x"], c["alpha"], c["d"], c["z"], nl, False)
    exact(yh, rh, "hard forward " + tag)
    exact(xqh, rxh, "hard x_quant " + tag)
    ys, xqs = ops.adaround_forward(x, alpha, d, z, nl, True, want_xq=True, out=outs[2])
    rs, rxs = O.adaround_fake_quant(c["x"], c["alpha"], c["d"], c["z"], nl, True)
    within(ys, rs, R.soft_bound(rs, c["d"]), "soft forward " + tag)
    within(xqs, rxs, 4e-6 * nl, "soft x_quant " + tag)
    exact(ops.adaround_forward(x, alpha, d, z, nl, True), ys, "soft forward without x_quant " + tag)
    t1, _, bound = R.dalpha_terms(c["x"], c["gy"], c["alpha"], c["d"], c["z"], nl)
    within(ops.adaround_backward(x, gy, alpha, d, z, nl, out=outs[3]), t1, bound, "d(alpha) " + tag)
    rw, rb = R.SINGLE_REG
    t1, t2, bound = R.dalpha_terms(c["x"], c["gy"], c["alpha"], c["d"], c["z"], nl, rw, rb)
    within(ops.adaround_backward(x, gy, alpha, d, z, nl, reg_weight=rw, reg_b=rb, out=outs[3]), t1 + t2, bound,
           "d(alpha) + regulariser " + tag)
    if place != "own":      # the inputs are untouched and nothing was written between the arena's tensors
        exact(x, c["x"], "x " + tag), exact(gy, c["gy"], "gy " + tag), exact(alpha, c["alpha"], "alpha " + tag)
        used = torch.zeros_like(arena.buf, dtype=torch.bool)
        for v in [x, gy, alpha] + outs:
            off = (v.data_ptr() - arena.buf.data_ptr()) // 4
            used[off:off + v.numel()] = True
        assert not bool(arena.buf[~used].any()), "a write outside the tensors " + tag


def test_uaq_backward_whole_tensor_as_one_row(ops):
    """scalar-scale uaq_backward over 1 048 577 elements: ONE workgroup sums them all (4097 passes of its loop)"""
    n, nl = 1048577, 16
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, generator=g)
    x[::1000] *= 6.0                                   # a tail beyond the clamp range of most elements' scale
    gy = torch.randn(n, generator=g)
    d, z = O.scale_init_max(x, nl, True)               # 1-D: one scalar pair
    d = d * 0.5                                        # half the elements clamp: both sides of the `inside` mask are populated
    t = R.uaq_ddelta_terms(x, gy, d, z, nl).double()
    dd, dx = ops.uaq_backward(G(x), G(gy), G(d), G(z), nl, want_dx=True)
    assert dd.shape == d.shape
    sum_close(dd, t.sum(), t.abs().sum(), "uaq_backward 1048577")
    exact(dx, R.uaq_dx(x, gy, d, z, nl), "uaq_backward dx 1048577")


# ================================================================================================ multi-tensor launches
def _seg_tensors(multi, grad_step=0):
    return [dict(x=G(c["x"]), gy=G(c["gys"][grad_step]), alpha=G(c["alpha"]), d=G(c["d"]), z=G(c["z"]), d0=G(c["d0"]), z0=G(c["z0"]))
            for c in multi]


WHICH = {"x": ("x",), "gy": ("gy",), "alpha": ("alpha",), "all": ("x", "gy", "alpha")}


@pytest.mark.parametrize("mode", ("own", "x", "alpha", "all"))
def test_adaround_forward_multi_against_oracle(ops, multi, mode):
    ts = placed(_seg_tensors(multi), mode, WHICH)
    outs = ops.adaround_forward_multi([(t["x"], t["alpha"], t["d"], t["z"], c["nl"], c["soft"]) for t, c in zip(ts, multi)])
    for k, (c, y) in enumerate(zip(multi, outs)):
        ref, _ = O.adaround_fake_quant(c["x"], c["alpha"], c["d"], c["z"], c["nl"], c["soft"])
        if c["soft"]:
            within(y, ref, R.soft_bound(ref, c["d"]), f"forward_multi[{mode}] segment {k} {R.MULTI_SEGS[k]}")
        else:
            exact(y, ref, f"forward_multi[{mode}] segment {k} {R.MULTI_SEGS[k]}")
        # the single-tensor kernel in addition (not the reference): the same bits
        assert torch.equal(y, ops.adaround_forward(G(c["x"]), G(c["alpha"]), G(c["d"]), G(c["z"]), c["nl"], c["soft"])), k


@pytest.mark.parametrize("variant", ("host", "dyn_gate1", "dyn_gate0"))
@pytest.mark.parametrize("mode", ("own", "x", "gy", "alpha", "all"))
def test_adaround_backward_multi_against_oracle(ops, multi, mode, variant):
    ts = placed(_seg_tensors(multi), mode, WHICH)
    rb = R.MULTI_REG_BS[0]
    gate = 0.0 if variant == "dyn_gate0" else 1.0
    items = [(t["x"], t["gy"], t["alpha"], t["d"], t["z"], c["nl"], c["rw"]) for t, c in zip(ts, multi)]
    if variant == "host":
        outs = ops.adaround_backward_multi(items, rb)
    else:
        dyn = torch.tensor([rb, gate, 123.0, 456.0], dtype=torch.float32, device=DEV)
        outs = ops.adaround_backward_multi(items, reg_b=-1.0, dyn=dyn)     # the host reg_b must be ignored
    for k, (c, da) in enumerate(zip(multi, outs)):
        t1, t2, bound = R.dalpha_terms(c["x"], c["gys"][0], c["alpha"], c["d"], c["z"], c["nl"], c["rw"] * gate, rb)
        within(da, t1 + t2, bound, f"backward_multi[{mode},{variant}] segment {k} {R.MULTI_SEGS[k]}")
        assert tuple(da.shape) == tuple(c["alpha"].shape)


def _check_ada_adam(refs, params, opt, step, what):
    for k, (ref, p) in enumerate(zip(refs, params)):
        within(p, ref.alpha, R.ADAM_RTOL * ref.alpha.abs() + R.ADAM_ATOL, f"{what} step {step} alpha segment {k}")
        within(opt.m[k], ref.m, ref.bm, f"{what} step {step} m segment {k}")
        within(opt.v[k], ref.v, ref.bv, f"{what} step {step} v segment {k}")


@pytest.mark.parametrize("variant", ("host", "dyn_gate1", "dyn_gate0"))
@pytest.mark.parametrize("mode", ("own", "x", "gy", "alpha", "all"))
def test_adaround_adam_multi_against_oracle(ops, multi, mode, variant):
    """d(alpha) + regulariser gradient + Adam in one launch, two steps (m and v are non-zero in the second)"""
    gate = 0.0 if variant == "dyn_gate0" else 1.0
    ts0, ts1 = _seg_tensors(multi, 0), _seg_tensors(multi, 1)
    for t0, t1 in zip(ts0, ts1):
        t0["gy1"] = t1["gy"]
    ts = placed(ts0, mode, {k: v + (("gy1",) if "gy" in v else ()) for k, v in WHICH.items()})
    params = [t["alpha"] for t in ts]
    opt = ops.FusedAdam(params, lr=R.MULTI_LR)
    refs = [R.AdaAdamRef(c["x"], c["alpha"], c["d"], c["z"], c["nl"], R.MULTI_LR) for c in multi]
    for step in range(2):
        rb = R.MULTI_REG_BS[step]
        items = [(t["x"], t["gy" if step == 0 else "gy1"], t["alpha"], t["d"], t["z"], c["nl"], c["rw"]) for t, c in zip(ts, multi)]
        if variant == "host":
            ops.adaround_adam_multi(items, opt, rb)
        else:
            dyn = torch.tensor([rb, gate, *R.adam_scalars(R.MULTI_LR, step + 1)], dtype=torch.float32, device=DEV)
            ops.adaround_adam_multi(items, opt, reg_b=-1.0, dyn=dyn)
        assert opt.t == step + 1
        for ref, c in zip(refs, multi):
            ref.step(c["gys"][step], c["rw"] * gate, rb)
        _check_ada_adam(refs, params, opt, step + 1, f"adaround_adam_multi[{mode},{variant}]")
    for t, c in zip(ts, multi):       # nothing but alpha / m / v was written
        assert torch.equal(t["x"], G(c["x"])) and torch.equal(t["gy"], G(c["gys"][0])) and torch.equal(t["gy1"], G(c["gys"][1]))


def _check_adam_step_single(ops, n, place):
    """ops.adam_step: the one-segment launch of the multi-tensor Adam kernel, three steps, p / g / m / v each in its own
    allocation or 1, 2, 3 floats past a 16-byte boundary"""
    g = torch.Generator().manual_seed(70 + n)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (10.0 if k == 1 else 0.1) for k in range(3)]
    ts = dict(p=G(p0), m=torch.zeros(n, device=DEV), v=torch.zeros(n, device=DEV), g0=G(grads[0]), g1=G(grads[1]), g2=G(grads[2]))
    if place != "own":
        arena = Arena(6 * n, 6)
        ts = {k: arena.put(t, place) for k, t in ts.items()}
    rp, rm, rv = p0.clone(), torch.zeros(n), torch.zeros(n)
    for step in range(3):
        ops.adam_step(ts["p"], ts[f"g{step}"], ts["m"], ts["v"], R.MULTI_LR, step + 1)
        R.adam_step(rp, grads[step], rm, rv, R.MULTI_LR, step + 1)
    what = f"adam_step n={n} place={place}"
    within(ts["p"], rp, R.ADAM_RTOL * rp.abs() + R.ADAM_ATOL, what + " p")
    within(ts["m"], rm, 2e-6 * (rm.abs() + 0.1 * sum(g_.abs() for g_ in grads)), what + " m")
    within(ts["v"], rv, R.BETA2_DEV * rv + 1e-30, what + " v")
    for k in range(3):
        exact(ts[f"g{k}"], grads[k], what + " gradient untouched")


@pytest.mark.parametrize("use_dyn", (False, True), ids=("host", "dyn"))
@pytest.mark.parametrize("mode", ("own", "p", "g", "all"))
def test_fused_adam_step_against_torch_restatement(ops, mode, use_dyn):
    ps, grads = R.adam_case()
    ts = [dict(p=G(p), g0=G(grads[0][i]), g1=G(grads[1][i]), g2=G(grads[2][i])) for i, p in enumerate(ps)]
    gs = ("g0", "g1", "g2")
    ts = placed(ts, mode, {"p": ("p",), "g": gs, "all": ("p",) + gs})
    params = [t["p"] for t in ts]
    opt = ops.FusedAdam(params, lr=R.MULTI_LR)
    rp = [p.clone() for p in ps]
    rm, rv = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    for step in range(3):
        dyn = None
        if use_dyn:
            dyn = torch.tensor([0.0, 0.0, *R.adam_scalars(R.MULTI_LR, step + 1)], dtype=torch.float32, device=DEV)
        opt.step([t[gs[step]] for t in ts], dyn=dyn)
        for i in range(len(ps)):
            R.adam_step(rp[i], grads[step][i], rm[i], rv[i], R.MULTI_LR, step + 1)
    what = f"FusedAdam[{mode},{'dyn' if use_dyn else 'host'}]"
    for i in range(len(ps)):
        # 3 steps against the figures of 25 (test_adam_kernel); m / v: fp32 rounding of a 3-term recursion, plus 1 - beta formed
        # from the fp32 beta the C ABI carries (param_ref.AdaAdamRef.step)
        within(params[i], rp[i], R.ADAM_RTOL * rp[i].abs() + R.ADAM_ATOL, f"{what} p segment {i}")
        within(opt.m[i], rm[i], 2e-6 * (rm[i].abs() + 0.1 * sum(g[i].abs() for g in grads)), f"{what} m segment {i}")
        within(opt.v[i], rv[i], R.BETA2_DEV * rv[i] + 1e-30, f"{what} v segment {i}")
    if not use_dyn:      # the single-tensor entry (no device scalars): aligned with "own", else 1, 2 or 3 floats off
        for n in (1, 3, 1023, 1025):
            _check_adam_step_single(ops, n, {"own": "own", "p": 1, "g": 2, "all": 3}[mode])


@pytest.mark.parametrize("mode", ("own", "x", "gy", "all"))
def test_uaq_multi_against_oracle(ops, multi, mode):
    ts = placed(_seg_tensors(multi), mode, WHICH)
    ys = ops.uaq_forward_multi([(t["x"], t["d0"], t["z0"], c["nl"]) for t, c in zip(ts, multi)])
    dds = ops.uaq_backward_multi([(t["x"], t["gy"], t["d0"], t["z0"], c["nl"]) for t, c in zip(ts, multi)])
    for k, (c, y, dd) in enumerate(zip(multi, ys, dds)):
        exact(y, O.uaq_fake_quant(c["x"], c["d0"], c["z0"], c["nl"]), f"uaq_forward_multi[{mode}] segment {k}")
        t = R.uaq_ddelta_terms(c["x"], c["gys"][0], c["d0"], c["z0"], c["nl"]).double()
        dims = (1, 2, 3) if c["x"].dim() == 4 else (0,)
        assert dd.shape == c["d0"].shape
        sum_close(dd, t.sum(dims), t.abs().sum(dims), f"uaq_backward_multi[{mode}] segment {k} {R.MULTI_SEGS[k]}")


# ================================================================================================ Hadamard transform
FWHT_NK = [(n, inner) for n in (1, 2, 4, 8, 512, 1024) for inner in (1, 9, 25) if n * inner <= 8192]
FWHT_LIMIT = [(256, 25), (512, 25)]       # n * inner = 6400 (tile kernel) and 12800 (column-gather kernel)


def _fwht_cases(n, inner):
    """(outer, n_in, n_out) of one (n, inner): outer on both sides of the rows per workgroup (OPB + 1 = one full workgroup and
    a one-row one) and 37; n_in / n_out from one channel to all"""
    opb = R.fwht_opb(n, inner) if n * inner <= 8192 else 1
    cs = sorted({1, n // 2 + 1, n} & set(range(1, n + 1)))
    return [(o, a, b) for o in sorted({1, opb - 1, opb + 1, 37} - {0}) for a in cs for b in cs]


@pytest.mark.parametrize("n,inner", FWHT_NK + FWHT_LIMIT, ids=lambda v: str(v))
def test_fwht_edges(ops, n, inner):
    """fwht_channels against the oracle, bit for bit (same butterfly order; tests/test_hip_parity.py::test_fwht)"""
    k = math.isqrt(inner)
    g = torch.Generator().manual_seed(100 * n + inner)
    refs = {}
    for outer, n_in, n_out in _fwht_cases(n, inner):
        if (outer, n_in) not in refs:
            w = torch.randn(outer, n_in, k, k, generator=g)
            refs[(outer, n_in)] = (w, R.fwht_pad(w, n))
        w, ref = refs[(outer, n_in)]
        got = ops.fwht_channels(G(w), n, n_out)
        exact(got, ref[:, :n_out], f"fwht n={n} inner={inner} outer={outer} n_in={n_in} n_out={n_out}")


def test_fwht_multi_against_oracle(ops):
    """17 tensors in one fwht_channels_multi call (16 per launch; the long-row tensor goes to the column-gather kernel)"""
    g = torch.Generator().manual_seed(9)
    picks = []
    for n, inner in FWHT_NK + FWHT_LIMIT:
        cases = _fwht_cases(n, inner)
        picks.append((n, inner) + cases[(7 * len(picks) + 3) % len(cases)])
    picks = picks[:17]
    assert len(picks) == 17 and any(n * inner > 8192 for n, inner, *_ in picks)
    ws = [torch.randn(outer, n_in, math.isqrt(inner), math.isqrt(inner), generator=g) for n, inner, outer, n_in, n_out in picks]
    outs = ops.fwht_channels_multi([(G(w), p[0], p[4]) for w, p in zip(ws, picks)])
    for w, p, y in zip(ws, picks, outs):
        exact(y, R.fwht_pad(w, p[0])[:, :p[4]], f"fwht_multi {p}")


@pytest.mark.parametrize("per_row", (True, False), ids=("per_row", "scalar"))
def test_adaround_fwht_multi_against_chain(ops, fused, per_row):
    """the fused forward H(Q(x))[:, :c_in], weights and biases interleaved, against fake-quant then transform of the oracle"""
    case = fused(per_row)
    for n, inner in R.FUSED_NK:
        assert ops.fq_fwht_fusable(n, inner)
    assert not ops.fq_fwht_fusable(512, 25) and not ops.fq_fwht_fusable(2048, 1)
    outs = ops.adaround_fwht_multi([(G(c["x"]), G(c["alpha"]), G(c["d"]), G(c["z"]), c["nl"], c["soft"], c["n"], c["c_in"])
                                    for c in case])
    for k, (c, y) in enumerate(zip(case, outs)):
        what = f"adaround_fwht_multi[{per_row}] segment {k} n={c['n']} c_in={c['c_in']} shape={tuple(c['x'].shape)}"
        if c["n"]:
            ref, bound = R.fq_fwht_forward(c["x"], c["alpha"], c["d"], c["z"], c["nl"], c["soft"], c["c_in"])
            if c["soft"]:
                within(y, ref, bound, what)
            else:
                exact(y, ref, what)
        else:
            ref, _ = O.adaround_fake_quant(c["x"], c["alpha"], c["d"], c["z"], c["nl"], True)
            within(y, ref, R.soft_bound(ref, c["d"]), what)


@pytest.mark.parametrize("variant", ("host", "dyn_gate1", "dyn_gate0"))
@pytest.mark.parametrize("gy_mode", ("own", "gy"))
@pytest.mark.parametrize("per_row", (True, False), ids=("per_row", "scalar"))
def test_fwht_adaround_adam_multi_against_chain(ops, fused, per_row, gy_mode, variant):
    """the fused backward: H(pad(gy)), d(alpha) + regulariser gradient, Adam -- two steps against the oracle pieces + param_ref"""
    case = fused(per_row)
    gate = 0.0 if variant == "dyn_gate0" else 1.0
    ts = [dict(x=G(c["x"]), alpha=G(c["alpha"]), d=G(c["d"]), z=G(c["z"]), gy=G(c["gys"][0]), gy1=G(c["gys"][1])) for c in case]
    ts = placed(ts, gy_mode, {"gy": ("gy", "gy1")})
    params = [t["alpha"] for t in ts]
    opt = ops.FusedAdam(params, lr=R.MULTI_LR)
    refs = [R.AdaAdamRef(c["x"], c["alpha"], c["d"], c["z"], c["nl"], R.MULTI_LR) for c in case]
    for step in range(2):
        rb = R.MULTI_REG_BS[step]
        items = [(t["x"], t["gy" if step == 0 else "gy1"], t["alpha"], t["d"], t["z"], c["nl"], c["rw"], c["n"], c["c_in"])
                 for t, c in zip(ts, case)]
        if variant == "host":
            ops.fwht_adaround_adam_multi(items, opt, rb)
        else:
            dyn = torch.tensor([rb, gate, *R.adam_scalars(R.MULTI_LR, step + 1)], dtype=torch.float32, device=DEV)
            ops.fwht_adaround_adam_multi(items, opt, reg_b=-1.0, dyn=dyn)
        for ref, c in zip(refs, case):
            ref.step(c["gts"][step], c["rw"] * gate, rb)
        _check_ada_adam(refs, params, opt, step + 1, f"fwht_adaround_adam_multi[{per_row},{gy_mode},{variant}]")


# ================================================================================================ step prologue
def _prologue_tables(B, nscal, steps, rows, seed):
    g = torch.Generator().manual_seed(seed)
    order = torch.randint(0, rows, (steps, B), generator=g)
    for s in range(steps):                     # one out-of-range index on each side (they alternate where B = 1)
        order[s, (3 * s) % B] = -3 - s if (s % 2 == 0 or B > 1) else rows + 2
        if B > 1:
            order[s, (3 * s + 1) % B] = rows + s
    scal = torch.randn(steps, nscal, generator=g)
    return order, scal


# Not the full 3 x 3 grid of B in {1, 2, 256} and nscal in {1, 4, 256}: the kernels copy the nscal floats and the B indices in two
# statements that do not see each other (`t < B`, `t < nscal`), so every B and every nscal is reached once, with the two extremes crossed (five pairs here, the three
# diagonal ones for the gather).
@pytest.mark.parametrize("B,nscal", ((1, 1), (2, 4), (256, 256), (1, 256), (256, 1)))
def test_step_prologue(ops, B, nscal):
    steps = 5
    order, scal = _prologue_tables(B, nscal, steps, 11, 7 * B + nscal)
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    cur_idx = torch.full((B,), -77, dtype=torch.int64, device=DEV)
    cur_scal = torch.full((nscal,), -77.0, device=DEV)
    order_g, scal_g = G(order), G(scal)
    for s in range(steps):
        ops.step_prologue(order_g, scal_g, ctr, cur_idx, cur_scal)
        ri, rs = R.step_prologue(order, scal, s)
        exact(cur_idx, ri, f"cur_idx step {s}")
        exact(cur_scal, rs, f"cur_scal step {s}")
        assert ctr.tolist() == [s + 1]
    exact(order_g, order), exact(scal_g, scal)


# B * row_len on both sides of one gather block of 4096 elements, and past the cap of 64 blocks with a ragged last block.
# B = 1 meets 1, 4095, 4096, 4097 and 64 * 4096 + 5 exactly.  The odd ones are no multiple of 2 or 256, so B = 2 and B = 256
# take the nearest row lengths on either side: 4094 / 4096 / 4098 and 32 * 8192 + 6; 3840 / 4096 / 4352 and 64 * 4100.
GATHER_ROW_LENS = {1: (1, 4095, 4096, 4097, 64 * 4096 + 5), 2: (1, 2047, 2048, 2049, 32 * 4096 + 3),
                   256: (1, 15, 16, 17, 1025)}


@pytest.mark.parametrize("B,nscal", ((1, 1), (2, 4), (256, 256)))
def test_step_prologue_gather(ops, B, nscal):
    """the prologue with the batch gather: 2 .. 65 workgroups, the last to finish advances the counter and re-arms the ticket"""
    steps, rows = 5, 7
    order, scal = _prologue_tables(B, nscal, steps, rows, 13 * B + nscal)
    order_g, scal_g = G(order), G(scal)
    for row_len in GATHER_ROW_LENS[B]:
        g = torch.Generator().manual_seed(row_len)
        table = torch.randn(rows, row_len, generator=g)
        table_g = G(table)
        ctr = torch.zeros(2, dtype=torch.int32, device=DEV)
        cur_idx = torch.full((B,), -77, dtype=torch.int64, device=DEV)
        cur_scal = torch.full((nscal,), -77.0, device=DEV)
        out = torch.full((B, row_len), -77.0, device=DEV)
        for s in range(steps):
            ops.step_prologue_gather(order_g, scal_g, ctr, cur_idx, cur_scal, table_g, out)
            ri, rs = R.step_prologue(order, scal, s)
            what = f"B={B} row_len={row_len} step {s}"
            exact(cur_idx, ri, "cur_idx " + what)
            exact(cur_scal, rs, "cur_scal " + what)
            exact(out, R.step_gather(order, s, table), "gathered rows " + what)
            assert ctr.tolist() == [s + 1, 0], what          # counter = launches so far, ticket word back at 0
        exact(table_g, table, "table untouched")


# ================================================================================================ reductions and small kernels
RED_N = (1, 4095, 4097, 256 * 4096 + 1)     # one stage-1 chunk, two, and 257 partial sums: stage 2 loops twice


@pytest.mark.parametrize("n", RED_N)
def test_round_loss_sizes(ops, n):
    g = torch.Generator().manual_seed(n)
    alpha = torch.randn(n, generator=g) * 3
    ag = G(alpha)
    for b in (20.0, 2.0):
        t = R.round_loss_terms(alpha, b).double()
        want, asum = 0.01 * t.sum(), 0.01 * t.abs().sum()
        sum_close(ops.round_loss(ag, b, 0.01), want, asum, f"round_loss n={n} b={b}")
        acc = torch.full((), 0.5, device=DEV)
        ops.round_loss(ag, b, 0.01, out=acc, accumulate=True)
        ops.round_loss(ag, b, 0.01, out=acc, accumulate=True)
        within(acc, 0.5 + 2 * want, 2 * R.SUM_RTOL * asum + 2e-7 * (0.5 + 2 * float(want)), f"round_loss accumulate n={n} b={b}")


@pytest.mark.parametrize("n", RED_N)
def test_l2_loss_sizes(ops, n):
    g = torch.Generator().manual_seed(n + 1)
    for C in (1, 3):
        if n % C:
            continue
        shape = (1, C, n // C, 1)
        pred, tgt = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
        want, grad = R.l2_loss64(pred, tgt)
        loss, dpred = ops.l2_loss_and_grad(G(pred), G(tgt))
        mean_count = n // C
        asum = ((pred - tgt) ** 2).double().sum() / mean_count
        within(loss, want, R.SUM_RTOL * asum + 1e-7 * float(want), f"l2_loss n={n} C={C}")
        exact(dpred, grad, f"l2_loss gradient n={n} C={C}")
        pg = G(pred).requires_grad_(True)               # the autograd wrapper: same kernel, gradient times the upstream 1
        ops.l2_loss(pg, G(tgt)).backward()
        exact(pg.grad, grad, f"l2_loss autograd gradient n={n} C={C}")


@pytest.mark.parametrize("frames", (1, 3))
@pytest.mark.parametrize("flen", (1, 1023, 1025, 3 * 17 * 23))
def test_frame_psnr_sizes(ops, flen, frames):
    g = torch.Generator().manual_seed(flen + frames)
    shape = (frames, 3, 17, 23) if flen == 3 * 17 * 23 else (frames, flen)
    out, gt = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    sse = R.frame_sse64(out, gt)
    want = -10 * torch.log10(sse / flen + 1e-9)
    # d(dB) = 10 / ln 10 * d(mse) / mse, d(mse) / mse <= SUM_RTOL (all terms are positive) plus the fp32 log10 and division
    within(ops.frame_psnr(G(out), G(gt)), want, 10 / math.log(10) * (R.SUM_RTOL + 3e-7) + 2e-7 * want.abs(), f"frame_psnr {shape}")


@pytest.mark.parametrize("shape", ((1, 1, 1), (2, 3, 511), (2, 3, 513), (3, 37, 17 * 23), (1, 5, 512 * 256 + 7)))
def test_channel_sum_sizes(ops, shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g)
    x[:, 0] += 3.0                     # a channel whose sum is large, next to channels whose sums nearly cancel
    s, sa = R.channel_sum64(x)
    sum_close(ops.channel_sum(G(x)), s, sa, f"channel_sum {shape}")


def test_bias_add(ops, lib):
    g = torch.Generator().manual_seed(4)
    B, C, HW = 2, 5, 7
    x, bias = torch.randn(B, C, HW, generator=g), torch.randn(C, generator=g)
    for xin in (x, None):
        y = torch.full((B, C, HW), -77.0, device=DEV)
        xg, bg = (None if xin is None else G(xin)), G(bias)
        lib.check(lib.lib().nq_bias_add(ops._p(xg), ops._p(bg), ops._p(y), B, C, HW, ops._stream()), "bias_add")
        exact(y, (x if xin is not None else torch.zeros_like(x)) + bias[None, :, None], f"bias_add x={'yes' if xin is not None else 'no'}")
    # and through the autograd Functions that own the kernel
    xg, bg = G(x.view(B, C, HW, 1)).requires_grad_(True), G(bias).requires_grad_(True)
    y = ops._BiasAddDD.apply(xg, bg)
    exact(y, (x + bias[None, :, None]).view(B, C, HW, 1), "bias_add Function")


@pytest.mark.parametrize("n", (1, 3, 4, 5, 1027))
def test_tanh_out_backward_sizes(ops, lib, n):
    g = torch.Generator().manual_seed(n)
    dimg, img = torch.randn(n, generator=g), torch.rand(n, generator=g)
    out = torch.full((n + 4,), -77.0, device=DEV)
    dg, ig = G(dimg), G(img)
    lib.check(lib.lib().nq_tanh_out_backward(ops._p(dg), ops._p(ig), ops._p(out), n, ops._stream()), "tanh_backward")
    t = 2.0 * img - 1.0
    exact(out[:n], dimg * 0.5 * (1.0 - t * t), f"tanh_out_backward n={n}")      # fp32, the kernel's op order
    assert out[n:].tolist() == [-77.0] * 4                                      # nothing past the end


@pytest.mark.parametrize("r", (1, 2, 3, 4, 5))
def test_ps_gelu_backward_strides(ops, lib, r):
    """PixelShuffle + GELU backward on a ragged (2, 3, 5, 7) grid; r = 3 takes the runtime-r instantiation"""
    B, C, H, W = 2, 3, 5, 7
    g = torch.Generator().manual_seed(r)
    da, z = torch.randn(B, C, H * r, W * r, generator=g), torch.randn(B, C, H * r, W * r, generator=g)
    out = torch.full((B, C * r * r, H, W), -77.0, device=DEV)
    dag, zg = G(da), G(z)
    lib.check(lib.lib().nq_ps_gelu_backward(ops._p(dag), ops._p(zg), ops._p(out), B, C, H, W, r, ops._stream()), "ps_gelu_backward")
    exact(out, F.pixel_unshuffle(da * z, r), f"ps_gelu_backward r={r}")


@pytest.mark.parametrize("flen", (297, 1024 + 3))
def test_gather_frames_u8_sizes(ops, flen):
    g = torch.Generator().manual_seed(flen)
    frames = torch.randint(0, 256, (6, flen), generator=g, dtype=torch.uint8)
    for idx in ([5, 4, 3, 2, 1, 0], [2, 2, 2], [4, 0, 4, 1], [3]):
        got = ops.gather_frames_u8(G(frames), torch.tensor(idx))
        exact(got, frames[idx].float() / 255.0, f"gather_frames_u8 flen={flen} idx={idx}")

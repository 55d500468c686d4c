"""Anchors of tests/param_ref.py (CPU only): each restatement the GPU file tests/test_param_side_edges.py compares a HIP kernel
with is tied here to torch, to the oracle or to the reference's recorded outputs, and every input generator of that file is
shown to satisfy the stability conditions of param_ref's docstring -- with an exclusion count of zero, because the GPU
tests mask nothing."""
import numpy as np
import pytest
import torch

import param_ref as R
from conftest import T
from oracle import nq_oracle as O


def eq(a, b, rtol=0.0, atol=0.0):
    a = a.detach().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol)


# ------------------------------------------------------------------------------------------ restatements
def test_adam_is_torch_optim_adam():
    """25 steps with gradients of two magnitudes (the inputs of test_adam_kernel): p, and the moments through torch's state."""
    g = torch.Generator().manual_seed(0)
    p0 = torch.randn(1000, generator=g)
    pc = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pc], lr=0.003)
    p, m, v = p0.clone(), torch.zeros(1000), torch.zeros(1000)
    for step in range(25):
        grad = torch.randn(1000, generator=g) * (0.1 if step % 3 else 10.0)
        pc.grad = grad.clone()
        opt.step()
        R.adam_step(p, grad, m, v, 0.003, step + 1)
    eq(p, pc, rtol=1e-7, atol=1e-7)
    eq(m, opt.state[pc]["exp_avg"], rtol=1e-6, atol=1e-9)
    eq(v, opt.state[pc]["exp_avg_sq"], rtol=1e-6, atol=1e-12)
    s1, s2 = R.adam_scalars(0.003, 7)
    assert s1 == 0.003 / (1 - 0.9 ** 7) and s2 == (1 - 0.999 ** 7) ** 0.5


def test_regulariser_gradient_and_terms_match_the_recorded_reference(golden):
    z = golden("roundloss.npz")
    alpha = T(z["alpha"])
    for b in (20, 7.3, 2):
        tag = str(b).replace(".", "p")
        eq(R.reg_dalpha(alpha, b, 0.01), z[f"dalpha_b{tag}"], rtol=2e-5, atol=1e-9)
        eq(0.01 * R.round_loss_terms(alpha, b).double().sum(), z[f"loss_b{tag}"], rtol=1e-5)
        ap = alpha.clone().requires_grad_(True)                     # and the oracle's own autograd
        O.round_regulariser([ap], b, 0.01).backward()
        eq(R.reg_dalpha(alpha, b, 0.01), ap.grad, rtol=2e-5, atol=1e-9)


@pytest.mark.parametrize("per_row", (True, False))
def test_dalpha_terms_and_uaq_terms_are_the_oracles(per_row):
    c = R.single_case(3, 257, per_row, 4)
    x, gy, alpha, d, z, nl = c["x"], c["gy"], c["alpha"], c["d"], c["z"], c["nl"]
    t1, t2, bound = R.dalpha_terms(x, gy, alpha, d, z, nl, 0.01, 7.3)
    assert torch.equal(t1, O.adaround_dalpha(x, gy, alpha, d, z, nl)) and (bound > 0).all()
    ap = alpha.clone().requires_grad_(True)                         # data + regulariser = autograd through the oracle
    y, _ = O.adaround_fake_quant(x, ap, d, z, nl, True)
    ((y * gy).sum() + O.round_regulariser([ap], 7.3, 0.01)).backward()
    eq(t1 + t2, ap.grad, rtol=2e-5, atol=1e-7)
    assert torch.equal(R.dalpha_terms(x, gy, alpha, d, z, nl)[1], torch.zeros_like(x))
    # UAQ: the summands add up to the oracle's closed form, which autograd confirms; dx is the clamp mask times (gy*d)/d
    t = R.uaq_ddelta_terms(x, gy, c["d0"], c["z0"], nl)
    want = O.uaq_ddelta(x, gy, c["d0"], c["z0"], nl)
    got = t.double().sum((1, 2, 3), keepdim=True) if per_row else t.double().sum()
    eq(got, want, rtol=1e-5, atol=1e-5 * float(t.abs().sum()))
    dx = R.uaq_dx(x, gy, c["d0"], c["z0"], nl)
    xi = (x / c["d0"]).round() + c["z0"]
    inside = (xi >= 0) & (xi <= nl - 1)
    assert torch.equal(dx, torch.where(inside, (gy * c["d0"]) / c["d0"], torch.zeros_like(gy)))


def test_fused_chain_is_fake_quant_then_hadamard():
    for per_row in (True, False):
        case = R.fused_case(per_row)
        for c in case[::5]:
            if not c["n"]:
                continue
            out, bound = R.fq_fwht_forward(c["x"], c["alpha"], c["d"], c["z"], c["nl"], c["soft"], c["c_in"])
            y, _ = O.adaround_fake_quant(c["x"], c["alpha"], c["d"], c["z"], c["nl"], c["soft"])
            assert torch.equal(out, O.hadamard_along_cin(y)[:, :c["c_in"]])
            assert bound.shape == out.shape and ((bound > 0).all() if c["soft"] else (bound == 0).all())
            # the backward's transform is the adjoint of `transform, then keep c_in channels`
            gy, gt = c["gys"][0], c["gts"][0]
            eq((gt.double() * y.double()).sum(), (gy.double() * out.double()).sum(), rtol=1e-5,
               atol=1e-5 * float((gt.abs() * y.abs()).sum()))


def test_step_prologue_reference_clamps_only_the_gather():
    order = torch.tensor([[0, 3], [-2, 9], [1, 1]])
    scal = torch.arange(12.0).view(3, 4)
    table = torch.arange(12.0).view(4, 3)
    idx, sc = R.step_prologue(order, scal, 1)
    assert idx.tolist() == [-2, 9] and sc.tolist() == [4.0, 5.0, 6.0, 7.0]
    assert torch.equal(R.step_gather(order, 1, table), table[[0, 3]])
    assert torch.equal(R.step_gather(order, 0, table), table[[0, 3]]) and torch.equal(R.step_gather(order, 2, table), table[[1, 1]])


def test_reduction_references():
    g = torch.Generator().manual_seed(3)
    pred, tgt = torch.rand(3, 3, 17, 23, generator=g), torch.rand(3, 3, 17, 23, generator=g)
    pc = pred.clone().requires_grad_(True)
    O.lp_loss(pc, tgt).backward()
    loss, grad = R.l2_loss64(pred, tgt)
    eq(loss, O.lp_loss(pred, tgt), rtol=1e-6)
    eq(grad, pc.grad, rtol=1e-6, atol=1e-12)
    eq(-10 * torch.log10(R.frame_sse64(pred, tgt) / pred[0].numel() + 1e-9), O.psnr_per_frame(pred, tgt), rtol=1e-6)
    s, sa = R.channel_sum64(pred)
    eq(s, pred.sum((0, 2, 3)), rtol=1e-5)
    eq(sa, s)


# ------------------------------------------------------------------------------------------ stability of the generators
def f32(v):
    """the Python number rounded to fp32"""
    return float(torch.tensor(v, dtype=torch.float32))


def _long_weight_cases():
    """(rows, row_len, x) of every per-row weight the GPU file quantises: the single-tensor shapes and the multi-tensor segments"""
    for rows, row_len in R.SINGLE_SHAPES:
        for nb in R.SINGLE_BITS:
            yield rows, row_len, R.single_case(rows, row_len, True, nb)["x"], 2 ** nb
    for seg, c in zip(R.MULTI_SEGS, R.multi_case()):
        if len(seg) == 2:
            yield seg[0], seg[1], c["x"], c["nl"]


def test_edge_rows_keep_their_kind_over_the_whole_row():
    """Every kind holds for the WHOLE row, sentinels included, and shows in the oracle's scales: zp == 0 for a positive row,
    zp == qmax for a negative one, delta == 0.37 / qmax for a constant one, a delta of the row's own size for x20 / x1e-3.
    Every kind occurs past one reduction pass (row_len > 256) and past one block per row (row_len > 1024)."""
    seen = {}
    for rows, row_len, x, nl in _long_weight_cases():
        w, kinds = x.view(rows, row_len), R.row_kinds(rows, row_len)
        d, z = O.scale_init_max(x, nl, True)
        d, z = d.view(-1), z.view(-1)
        for r, kind in enumerate(kinds):
            seen.setdefault(kind, set()).add(row_len)
            what = (rows, row_len, r, kind)
            row = w[r]
            if kind == "positive":
                assert (row > 0).all() and float(z[r]) == 0, what
            elif kind == "negative":
                assert (row < 0).all() and float(z[r]) == nl - 1, what
            elif kind == "constant":
                assert (row == R.CONSTANT).all() and float(z[r]) == 0, what
                assert float(d[r]) == f32(f32(R.CONSTANT) / (nl - 1)), what
            else:
                scale = R.ROW_SCALE[kind]
                assert float(row.abs().max()) <= f32(scale * (R.SENTINEL_FIRST + 0.125 * rows)), what
                if row_len > 64:                     # own elements on both sides of zero, a zero point inside the grid
                    assert (row[1:-1] > 0).any() and (row[1:-1] < 0).any() and 0 < float(z[r]) < nl - 1, what
            # the sentinels: the row's extremum, in the row's own sign and scale; none in a constant row
            if kind != "constant":
                scale = R.ROW_SCALE[kind]
                if r < rows - 1 and (row_len > 1 or r == 0):
                    assert float(row[-1]) == f32((-1.0 if kind == "negative" else 1.0) * scale * (R.SENTINEL_LAST + 0.125 * r)), what
                    if row_len > 2:
                        assert float(row[-1].abs()) > float(row[1:-1].abs().max()), what
                if r > 0:
                    assert float(row[0]) == f32((1.0 if kind == "positive" else -1.0) * scale * (R.SENTINEL_FIRST + 0.125 * r)), what
                    if row_len > 2:
                        assert float(row[0].abs()) > float(row[1:-1].abs().max()), what
    for kind in R.ROW_KINDS:
        assert any(256 < n <= 1024 for n in seen[kind]) and any(n > 1024 for n in seen[kind]), (kind, sorted(seen[kind]))


@pytest.mark.parametrize("per_row", (True, False))
@pytest.mark.parametrize("shape", R.SINGLE_SHAPES)
def test_single_tensor_inputs_are_stable(shape, per_row):
    for nb in R.SINGLE_BITS:
        c = R.single_case(*shape, per_row, nb)
        assert torch.isfinite(c["a0"]).all() and torch.isfinite(c["alpha"]).all() and float(c["d"].min()) > 0
        assert int(R.unstable(c["x"], c["alpha"], c["d"], c["z"], c["nl"]).sum()) == 0
        lin = R.lin_of(c["alpha"])
        assert float(torch.minimum(lin.abs(), (lin - 1).abs()).min()) >= R.LIN_MARGIN
        # the soft forward on soft targets H_ULPS either way stays inside the forward's own tolerance: no rounding tie of xi
        ref, _ = O.adaround_fake_quant(c["x"], c["alpha"], c["d"], c["z"], c["nl"], True)
        fl, h = torch.floor(c["x"] / c["d"]), torch.clamp(lin, 0, 1)
        for dh in (-R.H_ULPS, R.H_ULPS):
            hh = torch.where((h > 0) & (h < 1), torch.clamp(h + dh, 0, 1), h)
            y = (torch.clamp((fl + hh) + c["z"], 0, c["nl"] - 1) - c["z"]) * c["d"]
            assert int(((y - ref).abs() > R.soft_bound(ref, c["d"])).sum()) == 0
        if shape[1] >= 255:      # the whole range of alpha is there: saturated both ways and the open interval
            assert (lin < 0).any() and (lin > 1).any() and ((lin > 0) & (lin < 1)).any()


def _trajectory_is_stable(c):
    """both trajectories the GPU file runs: regulariser on, and gated off"""
    for rw in sorted({c["rw"], 0.0}):
        ref = R.AdaAdamRef(c["x"], c["alpha"], c["d"], c["z"], c["nl"], R.MULTI_LR)
        for g_t, rb in zip(c["gts"] if "gts" in c else c["gys"], R.MULTI_REG_BS):
            assert int(R.unstable(c["x"], ref.alpha, c["d"], c["z"], c["nl"]).sum()) == 0
            t1, t2, _ = R.dalpha_terms(c["x"], g_t, ref.alpha, c["d"], c["z"], c["nl"], rw, rb)
            assert int(R.cancelling(t1, t2).sum()) == 0
            ref.step(g_t, rw, rb)
        assert int(ref.bad.sum()) == 0
    assert float((ref.alpha - c["alpha"]).abs().max()) > 1e-4 or not (ref.v > 0).any()     # the parameters did move


def test_multi_tensor_inputs_are_stable():
    case = R.multi_case()
    assert len(case) == 19 and [tuple(c["x"].shape[:2]) if c["x"].dim() == 4 else tuple(c["x"].shape) for c in case] == R.MULTI_SEGS
    for c in case:
        _trajectory_is_stable(c)


@pytest.mark.parametrize("per_row", (True, False))
def test_fused_launch_inputs_are_stable(per_row):
    case = R.fused_case(per_row)
    assert len(case) == 2 * len(R.fused_shapes()) and len(case) > 32
    for n, inner in R.FUSED_NK:
        assert n * inner <= 8192 and n <= 1024       # ops.fq_fwht_fusable, restated (no GPU library on this side)
    for c in case:
        _trajectory_is_stable(c)
        if c["n"]:
            assert tuple(c["d"].shape) == ((c["x"].shape[0], 1, 1, 1) if per_row else ())

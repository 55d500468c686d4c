"""The table of tests/decoder_cases.py against ops.plan_decoder, and ops.plan_decoder against the library's own capability queries
-- on the table's rows and on a seeded sweep of the generator's sampler.  Needs the built library, no GPU: every plan and every
query is a pure host function of the shapes.

The invariants are stated without plan_decoder's rules: for every launch of a plan they ask nq_conv3_supported,
nq_conv3_split_io, nq_conv_wgrad3_supported, nq_conv_wgrad3_split_io, nq_conv_split_out and the swapped entries' queries for that
launch's exact shape (the data gradient is the convolution cout -> cin on the same pixels)."""
import random

import pytest

import decoder_cases as D

SWEEP_SEED, SWEEP, SWEEP_DEEP = 11, 2500, 500
IDS = [D.case_id(r) for r in D.CASES]


def _lib():
    from neuroquant_amd import _lib
    return _lib.lib()


def check_invariants(row, plan, precision="bf16x3"):
    from neuroquant_amd import ops
    lib = _lib()
    B, _, fc, layers, wshapes = row[:5]
    n = len(plan)
    sizes, _ = D.geometry(row)
    for l, p in enumerate(plan):
        assert (p.H, p.W) == sizes[l] and (p.k, p.r, p.act) == tuple(layers[l]) and (p.cout, p.cin) == tuple(wshapes[l])
        fwd_shape, bwd_shape = (B, p.cin, p.H, p.W, p.cout, p.k), (B, p.cout, p.H, p.W, p.cin, p.k)
        # routes: only where the library offers them
        assert p.fwd in ("bf16x3", "fp32") and p.dgrad in ("bf16x3", "fp32", None) and p.wgrad in ("bf16x3", "fp32", "swapped3")
        if precision == "fp32":
            assert p.fwd == p.wgrad == "fp32" and p.dgrad in ("fp32", None)
        if p.fwd == "bf16x3":
            assert lib.nq_conv3_supported(*fwd_shape) == 1
        if p.dgrad == "bf16x3":
            assert lib.nq_conv3_supported(*bwd_shape) == 1
        if p.wgrad == "bf16x3":
            assert lib.nq_conv_wgrad3_supported(*fwd_shape) == 1
        if p.wgrad == "swapped3":
            assert lib.nq_conv_wgrad3_swapped_supported(*fwd_shape) == 1 and lib.nq_conv_wgrad3_swapped_ws_floats(*fwd_shape) > 0
        # an X_SPLIT / Y_SPLIT bit only on a launch whose kernel reports that capability for that exact shape
        assert not (p.fwd_fmt | p.dgrad_fmt) & ~(D.X_SPLIT | D.Y_SPLIT) and not p.wgrad_fmt & ~3
        if p.fwd_fmt:
            assert p.fwd == "bf16x3" and not p.fwd_fmt & ~lib.nq_conv3_split_io(*fwd_shape), (l, hex(p.fwd_fmt))
        if p.dgrad_fmt & D.X_SPLIT:
            assert p.dgrad == "bf16x3"
        if p.dgrad_fmt:
            if p.dgrad == "bf16x3":
                assert not p.dgrad_fmt & ~lib.nq_conv3_split_io(*bwd_shape), (l, hex(p.dgrad_fmt))
            else:
                assert p.dgrad == "fp32" and p.dgrad_fmt == D.Y_SPLIT and p.dgrad_epi == ops.EPI_DGRAD_GELU
                assert lib.nq_conv_split_out(*bwd_shape, p.dgrad_r, ops.EPI_DGRAD_GELU, 0) == 1
        if p.wgrad_fmt:
            assert p.wgrad == "bf16x3" and not p.wgrad_fmt & ~lib.nq_conv_wgrad3_split_io(*fwd_shape), (l, p.wgrad_fmt)
        # a tensor's writer and all its readers agree on its form: x_l (epilogue of layer l - 1 -> forward and weight gradient
        # of layer l), g_l (data gradient of layer l + 1 -> data gradient and weight gradient of layer l)
        assert bool(p.fwd_fmt & D.X_SPLIT) == p.x_split == bool(p.wgrad_fmt & 1)
        assert bool(p.dgrad_fmt & D.X_SPLIT) == p.g_split == bool(p.wgrad_fmt & 2)
        assert bool(p.fwd_fmt & D.Y_SPLIT) == (l + 1 < n and plan[l + 1].x_split)
        assert bool(p.dgrad_fmt & D.Y_SPLIT) == (l > 0 and plan[l - 1].g_split)
        if l == 0:
            assert not p.x_split and not p.g_split and p.dgrad_fmt == 0     # the embedding and layer 0's data gradient: floats
        if l == n - 1:
            assert not p.g_split                                            # the gradient at the head's output comes from the loss
        if p.x_split:
            assert p.fwd == p.wgrad == "bf16x3" and plan[l - 1].fwd == "bf16x3" and plan[l - 1].act
        if p.g_split:
            assert p.dgrad == p.wgrad == "bf16x3" and plan[l - 1].act
            assert not (l == 1 and fc != (1, 1))      # the channel -> space reshape of floats sits between g_1's writer and reader
        # the data gradient's epilogue un-shuffles by the factor of the layer below
        assert (p.dgrad_epi, p.dgrad_r) == ((ops.EPI_DGRAD_GELU, layers[l - 1][1]) if l and layers[l - 1][2] else (ops.EPI_PLAIN, 1))


@pytest.mark.parametrize("row", D.CASES, ids=IDS)
def test_plan_matches_the_literal(row):
    from neuroquant_amd import ops
    plan = D.make_plan(row, "bf16x3")
    assert D.notation(plan) == row[5]
    assert D.notation(D.make_plan(row, "fp32")) == " ".join(["f-f"] + ["fff"] * (len(row[3]) - 1))
    n = len(plan)
    assert [p.epi for p in plan] == [ops.EPI_PLAIN] + [ops.EPI_PS_GELU] * (n - 2) + [ops.EPI_TANH] and all(p.has_bias for p in plan)


def test_table_covers_the_requirements():
    assert 0 < len(D.CASES) <= D.MAX_ROWS and len(D.ARENA_SPLIT) == len(D.CASES)
    assert all(1 <= split <= len(row[3]) - 1 for row, split in zip(D.CASES, D.ARENA_SPLIT))
    for row in D.CASES:
        assert D.consistent(row) and D.macs(row) <= D.MAX_MACS, D.case_id(row)
    missing = D.unmet(D.CASES)
    assert not missing, f"no row of tests/decoder_cases.py carries: {missing} (python tools/gen_decoder_cases.py --write)"


def test_hessian_rows_have_a_layer_on_bf16x3_in_all_three_letters():
    rows = D.hessian_rows()
    assert len(rows) == 2 and all(any(w[:3] == "333" for w in r[5].split()) for r in rows)


@pytest.mark.parametrize("row", D.CASES, ids=IDS)
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_embedding_gradient_changes_layer0_data_gradient_only(row, precision):
    from neuroquant_amd import ops
    off, on = D.make_plan(row, precision), D.make_plan(row, precision, want_emb_grad=True)
    assert off[0].dgrad is None and on[0].dgrad == "fp32"
    for l, (p, q) in enumerate(zip(off, on)):
        for field in ops.LayerPlan.__slots__:
            if (l, field) != (0, "dgrad"):
                assert getattr(p, field) == getattr(q, field), (l, field)


def _swept_rows():
    rng, deep = random.Random(SWEEP_SEED), random.Random(SWEEP_SEED + 1)
    return [D.sample(rng) for _ in range(SWEEP)] + [D.sample_deep(deep) for _ in range(SWEEP_DEEP)]


def test_plan_invariants_on_the_table_and_a_sweep(monkeypatch):
    rows = [r[:5] for r in D.CASES] + _swept_rows()
    assert len(rows) >= 2000 + len(D.CASES)
    words = set()
    for row in rows:
        assert D.consistent(row)
        for emb_grad in (False, True):
            plan = D.make_plan(row, "bf16x3", emb_grad)
            check_invariants(row, plan)
            check_invariants(row, D.make_plan(row, "fp32", emb_grad), "fp32")
        words |= set(D.notation(D.make_plan(row, "bf16x3")).split())
    # the sweep is not vacuous: it reaches split flags, every route letter, the few-pixel layer 0 and split words that start
    # two layers below the head
    assert {"333xg", "ffs", "f-f"} <= words and any(w.endswith("x") for w in words) and any(w.startswith("3-") for w in words)
    assert any(p.x_split for row in rows for p in D.make_plan(row)[:-2])
    # NQ_SPLIT_IO=0 clears every flag and keeps every route
    plans = [D.make_plan(row, "bf16x3") for row in rows]
    monkeypatch.setenv("NQ_SPLIT_IO", "0")
    for row, on in zip(rows, plans):
        off = D.make_plan(row, "bf16x3")
        assert D.notation(off) == D.notation(off, splits=False) == D.notation(on, splits=False)
        assert not any(p.x_split or p.g_split or p.fwd_fmt or p.dgrad_fmt or p.wgrad_fmt for p in off)
        check_invariants(row, off)

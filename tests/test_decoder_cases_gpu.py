"""The fused decoder node (ops.decoder_stack and its schedule variants) and the twice-differentiable decoder
(ops.decoder_stack_dd) against float64 on the stacks of tests/decoder_cases.py: plans that ops.plan_decoder composes at shapes
outside the four shipped decoders.  The references, the two reference-error runs and the tolerance rule are described in
tests/decoder_cases.py; every check prints its worst error / bound ratio and the cases collect their misses, so one run shows
every figure."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import decoder_cases as D

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = [D.case_id(r) for r in D.CASES]


@pytest.fixture(scope="module")
def ops():
    from neuroquant_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


@pytest.fixture(scope="module")
def refs():
    """row -> first_order_reference / second_order_reference, computed once per row on the CPU and never modified"""
    cache = {}

    def get(row, order=1, u8=False):
        key = (D.case_id(row), order, u8)
        if key not in cache:
            cache[key] = D.first_order_reference(row, u8) if order == 1 else D.second_order_reference(row)
        return cache[key]
    return get


def _names(n):
    return [f"d{t}{l}" for l in range(n) for t in ("W", "b")]


def _arena_split(row):
    """the layer at which the two-phase schedule cuts the arena (ops.set_grad_arena_hook): a literal per row, written beside
    the table by tools/gen_decoder_cases.py"""
    return D.ARENA_SPLIT[D.CASES.index(row)]


def run(ops, row, prec, mode, monkeypatch):
    """one forward + backward of the row under a schedule -> {tensor name: tensor}"""
    _, _, fc, layers, wshapes = row[:5]
    n = len(layers)
    emb, ws, frames, idx, tgt = D.inputs(row)
    emb = emb.to(DEV).requires_grad_(mode != "manual")
    ws = [(w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)) for w, b in ws]
    frames, idx, tgt = frames.to(DEV), idx.to(DEV), tgt.to(DEV)
    if mode == "base_u8":      # the plain schedule on the second target: the frames of the uint8 cache as floats
        tgt = ops.gather_frames_u8(frames, idx)
    spec = ops.DecoderSpec(layers, fc, True, precision=prec)
    spec.overlap_wgrad = mode == "stream"
    sizes = [s for (cout, cin), (k, _, _) in zip(wshapes, layers) for s in (cout * cin * k * k, cout)]
    with monkeypatch.context() as m:
        m.delenv("NQ_FUSED_HEAD_LOSS", raising=False)
        m.delenv("NQ_FUSED_LOSS", raising=False)
        m.setenv("NQ_DEFER_REDUCE", "0" if mode == "nodefer" else "1")
        m.setenv("NQ_SPLIT_IO", "0" if mode == "nosplit" else "1")
        if mode == "manual":
            img, node = ops.decoder_forward_manual(emb, spec, ws)
            assert notation_of(node) == D.notation(D.make_plan(row, prec, False))
            loss, dpred = ops.l2_loss_and_grad(img, tgt)
            steps, parts = ops.decoder_backward_steps(node, dpred), []
            while True:
                try:
                    part, last = next(steps)
                    parts.append((part.clone(), last))
                except StopIteration as done:
                    grads = done.value
                    break
            assert grads[0] is None and grads[1] is None and [last for _, last in parts] == [False, True]
            assert [p.numel() for p, _ in parts] == [sum(sizes[:2 * _arena_split(row)]), sum(sizes[2 * _arena_split(row):])]
            out = {"img": img, "loss": loss, **dict(zip(_names(n), grads[2:]))}
            assert torch.equal(torch.cat([p for p, _ in parts]), torch.cat([out[name].reshape(-1) for name in _names(n)]))
            return out
        seen = []
        if mode == "arena1":
            hook = ops.grad_arena_hook(lambda part: seen.append((part.clone(), None)))
        elif mode == "arena2":
            hook = ops.grad_arena_hook(lambda part, last: seen.append((part.clone(), last)), two_phase=True)
        else:
            hook = contextlib.nullcontext()
        fused = {"fused": dict(tgt=tgt), "fused_u8": dict(cache_u8=frames, idx=idx)}.get(mode)
        with hook, (ops.fused_head_loss(**fused) if fused else contextlib.nullcontext()):
            img = ops.decoder_stack(emb, spec, ws)
            assert notation_of(img.grad_fn) == D.notation(D.make_plan(row, prec, True))
            if fused:
                assert img.grad_fn.nq_head.loss is not None, "the fused loss tail did not run behind the head"
                loss, g = ops.l2_loss_head_grad(img, **fused)
                img.backward(g)
            else:
                from neuroquant_amd.quantization.quantizer import lp_loss
                loss = lp_loss(img, tgt)
                loss.backward()
        out = {"img": img.detach(), "loss": loss.detach(), "d_emb": emb.grad}
        for l, (w, b) in enumerate(ws):
            out[f"dW{l}"], out[f"db{l}"] = w.grad, b.grad
        if mode in ("arena1", "arena2"):
            assert ops.arena_reduced(img)
            want = [(sum(sizes), None)] if mode == "arena1" else \
                [(sum(sizes[:2 * _arena_split(row)]), False), (sum(sizes[2 * _arena_split(row):]), True)]
            assert [(p.numel(), last) for p, last in seen] == want
            assert torch.equal(torch.cat([p for p, _ in seen]), torch.cat([out[name].reshape(-1) for name in _names(n)]))
        return out


def notation_of(node):
    return D.notation(node.plan)


def head_qualifies(ops, row, prec):
    """the fused loss tail behind the head (nq_head_forward_loss): a 3 x 3 head on the fp32 kernel, frame and operand rows of
    whole float4s"""
    (k, _, _), (_, cin), W = row[3][-1], row[4][-1], D.geometry(row)[1][1]
    return k == 3 and W % 4 == 0 and ops.conv_operand_dims(cin, 3, 3)[1] % 4 == 0 and D.make_plan(row, prec)[-1].fwd == "fp32"


def check(tag, got, ref, prec, bad, absent=()):
    """every tensor of the reference but `absent` must be there, and inside its bound"""
    names = [name for name in ref["f64"] if name not in absent]
    missing = [name for name in names if got.get(name) is None]
    assert not missing and not [name for name in absent if got.get(name) is not None], (tag, missing)
    ratios = {name: D.ratio(name, got[name], ref, prec) for name in names}
    worst = max(ratios, key=ratios.get)
    print(f"{tag}: worst error / bound {ratios[worst]:.3f} ({worst}); " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    bad += [(tag, name, round(v, 3)) for name, v in ratios.items() if not v <= 1.0]
    return ratios


@pytest.mark.parametrize("prec", ("bf16x3", "fp32"))
@pytest.mark.parametrize("row", D.CASES, ids=IDS)
def test_decoder_node_matches_float64_under_every_schedule(ops, refs, row, prec, monkeypatch):
    """image, loss, every dW and db and d(embedding) of ops.decoder_stack against float64: the plain schedule (twice: identical
    bits), then every other schedule -- against float64, and bit for bit against the plain one where that is documented"""
    ref = refs(row)
    tag = f"{D.case_id(row)} [{row[5] if prec == 'bf16x3' else 'fp32'}]"
    n, bad = len(row[3]), []
    base = run(ops, row, prec, "base", monkeypatch)
    assert tuple(base["img"].shape) == (row[0], 3) + D.geometry(row)[1]
    check(f"{tag} decoder_stack", base, ref, prec, bad)
    again = run(ops, row, prec, "base", monkeypatch)
    assert all(torch.equal(base[name], again[name]) for name in base), "two calls differ"
    grads = _names(n)
    # the schedules that run the same kernels on the same operands as the plain backward are documented bit-identical to it
    # (ops._decoder_backward_steps, ops.PendingReductions); NQ_SPLIT_IO=0 but for the bias gradients (ops.plan_decoder: a weight
    # gradient sums db from hi + lo of a split g); the fused loss tail but for the loss and the head's bias gradient, which it
    # sums in another order (include/nq_hip.h: nq_head_forward_loss)
    same = {"stream": grads + ["img", "loss", "d_emb"], "arena1": grads + ["img", "loss", "d_emb"],
            "arena2": grads + ["img", "loss", "d_emb"], "nodefer": grads + ["img", "loss", "d_emb"], "manual": grads + ["img", "loss"],
            "nosplit": [g for g in grads if g[1] == "W"] + ["img", "loss", "d_emb"],
            "fused": [g for g in grads if g != f"db{n - 1}"] + ["img", "d_emb"],
            "fused_u8": [g for g in grads if g != f"db{n - 1}"] + ["img", "d_emb"]}
    modes = ["stream", "arena1", "arena2", "nodefer", "manual", "nosplit"]
    if head_qualifies(ops, row, prec):
        modes += ["fused", "base_u8", "fused_u8"]
    for mode in modes:
        got = run(ops, row, prec, mode, monkeypatch)
        # the manual node is built without the embedding's gradient (ops.decoder_forward_manual): the one tensor a schedule lacks
        check(f"{tag} {mode}", got, refs(row, u8=True) if mode.endswith("_u8") else ref, prec, bad,
              absent=("d_emb",) if mode == "manual" else ())
        if mode == "base_u8":       # what the fused tail on the uint8 cache is compared with, bit for bit
            base_u8 = got
            continue
        differ = [name for name in same[mode] if not torch.equal(got[name], (base_u8 if mode == "fused_u8" else base)[name])]
        if differ:
            bad.append((tag, mode, "bits differ from the plain schedule", differ))
    assert not bad, bad


@pytest.mark.parametrize("prec", ("bf16x3", "fp32"))
@pytest.mark.parametrize("which", (0, 1))
def test_decoder_stack_dd_hessian_vector_product_matches_float64(ops, refs, which, prec):
    """values, first gradients and one Hessian-vector product (the recipe of methods/bit_assign.py) at shapes where
    ops._conv_plain / _dgrad_plain / _wgrad_plain take the bf16x3 kernels"""
    row = D.hessian_rows()[which]
    ref = refs(row, order=2)
    B, _, fc, layers, wshapes = row[:5]
    if prec == "bf16x3":    # the shapes do reach the bf16x3 kernels: some layer has all three
        assert any(ops.conv3_supported(B, cin, H, W, cout, k) and ops.conv3_supported(B, cout, H, W, cin, k)
                   and ops.conv_wgrad3_supported(B, cin, H, W, cout, k)
                   for (k, _, _), (cout, cin), (H, W) in zip(layers, wshapes, D.geometry(row)[0]) if k in (3, 5))
    emb, ws, _, _, tgt = D.inputs(row)
    params = [w.to(DEV).requires_grad_(True) for w, _ in ws]
    ops.set_conv_precision(prec)
    try:
        spec = ops.DecoderSpec(layers, fc, True, precision=prec)
        img = ops.decoder_stack_dd(emb.to(DEV), spec, [(w, b.to(DEV)) for w, (_, b) in zip(params, ws)])
        loss = F.mse_loss(img, tgt.to(DEV))
        grad_f = torch.autograd.grad(loss, params, create_graph=True)
        sum((g * v.to(DEV)).sum() for g, v in zip(grad_f, ref["v"])).backward()
    finally:
        ops.set_conv_precision(None)
    got = {"img": img.detach(), "loss": loss.detach()}
    for l, (g, w) in enumerate(zip(grad_f, params)):
        got[f"dW{l}"], got[f"Hv{l}"] = g.detach(), w.grad
    bad = []
    check(f"{D.case_id(row)} [{prec}] decoder_stack_dd", got, ref, prec, bad)
    assert not bad, bad

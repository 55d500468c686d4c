"""ops.plan_decoder -- the one place where the fused decoder node's launches are routed -- against a table of literals.  The
table was produced by restating, over shapes only, the rules plan_decoder replaced (the forward pre-pass of the decoder node
and the support queries its backward made per weight gradient), so it pins the routing independently of plan_decoder.  Needs
the built library, no GPU: the plan is a pure function of the shapes.

Notation per layer: forward / data-gradient / weight-gradient route, 3 = bf16x3, f = fp32, s = swapped3, - = no launch; a
trailing x / g marks x_split / g_split."""
import pytest

from conftest import HNERV_3M, NERV_3M, TINY_HNERV, TINY_NERV

# config -> (architecture, model config, embedding H x W)
CONFIGS = {"tiny_hnerv": ("hnerv", TINY_HNERV, (1, 2)), "tiny_nerv": ("nerv", TINY_NERV, (1, 1)),
           "hnerv_3m": ("hnerv", HNERV_3M, (2, 4)), "nerv_3m": ("nerv", NERV_3M, (1, 1))}
BF16X3 = {
    ("tiny_hnerv", 1): "f-f fff fff fff ff3 333 ffs",
    ("tiny_hnerv", 2): "f-f fff fff fff ff3 333 ffs",
    ("tiny_nerv", 1): "f-f fff fff fff ff3 333 ffs",
    ("tiny_nerv", 2): "f-f fff fff fff ff3 333 ffs",
    ("hnerv_3m", 2): "f-f fff 333 333xg 333xg 333xg ffs",
    ("hnerv_3m", 1): "f-f fff 333 33f 333xg 333xg ffs",
    ("nerv_3m", 2): "f-f 333 333 333xg 333xg 333xg ffs",
    ("nerv_3m", 1): "f-f 333 333 f3f 333g 333xg ffs",
}
FP32 = "f-f fff fff fff fff fff fff"
LETTER = {"bf16x3": "3", "fp32": "f", "swapped3": "s", None: "-"}


@pytest.fixture(scope="module")
def stacks():
    """config -> (DecoderSpec, [(cout, cin)], [has_bias]) of the shipped decoders, built as plain CPU modules"""
    from neuroquant_amd.models import HNeRV, NeRV, _decode
    out = {}
    for name, (arch, cfg, _) in CONFIGS.items():
        spec, provs = _decode._fused_stack((HNeRV if arch == "hnerv" else NeRV)(cfg))
        wb = [p() for p in provs]
        out[name] = (spec, [tuple(W.shape[:2]) for W, _ in wb], [b is not None for _, b in wb])
    return out


def make_plan(stacks, name, precision, B, want_emb_grad=False):
    from neuroquant_amd import ops
    spec, wshapes, has_bias = stacks[name]
    spec.precision = precision            # read when the plan is made, not when the spec was
    return ops.plan_decoder(spec, wshapes, has_bias, B, *CONFIGS[name][2], want_emb_grad)


def notation(plan, splits=True):
    return " ".join(LETTER[p.fwd] + LETTER[p.dgrad] + LETTER[p.wgrad]
                    + ("x" if splits and p.x_split else "") + ("g" if splits and p.g_split else "") for p in plan)


@pytest.mark.parametrize("name,B", sorted(BF16X3))
def test_plan_matches_the_routing_table(stacks, name, B):
    from neuroquant_amd import ops
    plan = make_plan(stacks, name, "bf16x3", B)
    assert notation(plan) == BF16X3[name, B]
    assert notation(make_plan(stacks, name, "fp32", B)) == FP32
    # the shapes the routes were decided for: the head sees the full frame, every block ends in PixelShuffle + GELU
    spec, wshapes, has_bias = stacks[name]
    cfg = CONFIGS[name][1]
    assert (plan[-1].H, plan[-1].W) == (cfg["crop_h"], cfg["crop_w"]) and (plan[0].H, plan[0].W) == CONFIGS[name][2]
    assert [(p.k, p.r, p.act) for p in plan] == spec.layers
    assert [(p.cout, p.cin) for p in plan] == wshapes and [p.has_bias for p in plan] == has_bias
    assert [p.epi for p in plan] == [ops.EPI_PLAIN] + [ops.EPI_PS_GELU] * 5 + [ops.EPI_TANH]
    # the split flags are the fmt words: a tensor's writer and its readers agree on its form
    for l, p in enumerate(plan):
        assert bool(p.fwd_fmt & ops.EPI_X_SPLIT) == p.x_split == bool(p.wgrad_fmt & 1)
        assert bool(p.dgrad_fmt & ops.EPI_X_SPLIT) == p.g_split == bool(p.wgrad_fmt & 2)
        if l:
            assert bool(plan[l - 1].fwd_fmt & ops.EPI_Y_SPLIT) == p.x_split
            assert bool(p.dgrad_fmt & ops.EPI_Y_SPLIT) == plan[l - 1].g_split


@pytest.mark.parametrize("name,B", sorted(BF16X3))
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_embedding_gradient_changes_layer0_data_gradient_only(stacks, name, B, precision):
    from neuroquant_amd import ops
    off, on = make_plan(stacks, name, precision, B), make_plan(stacks, name, precision, B, want_emb_grad=True)
    assert off[0].dgrad is None and on[0].dgrad == "fp32"
    for l, (p, q) in enumerate(zip(off, on)):
        for field in ops.LayerPlan.__slots__:
            if (l, field) != (0, "dgrad"):
                assert getattr(p, field) == getattr(q, field), (l, field)


@pytest.mark.parametrize("name,B", sorted(BF16X3))
def test_split_io_switch_clears_the_flags_and_keeps_the_routes(stacks, name, B, monkeypatch):
    monkeypatch.setenv("NQ_SPLIT_IO", "0")
    plan = make_plan(stacks, name, "bf16x3", B)
    assert notation(plan) == notation(plan, splits=False) == " ".join(w.rstrip("xg") for w in BF16X3[name, B].split())
    assert not any(p.x_split or p.g_split or p.fwd_fmt or p.dgrad_fmt or p.wgrad_fmt for p in plan)


def test_reshape_between_layers_0_and_1_keeps_layer1_gradient_in_floats():
    """The `l == 1 and fc_hw != (1, 1)` exclusion, which no shipped configuration reaches (their layer 0 has no GELU): the tail
    of HNeRV-3M as a four-layer stack whose layer 0 ends in GELU.  Layer 1 sees the same 160 x 320 input either way and takes
    g_split -- unless the channel -> space reshape sits between its data gradient and layer 0 (rows from the same restatement
    of the replaced rules as the table above)."""
    from neuroquant_amd import ops
    layers = [(5, 4, True), (5, 2, True), (5, 2, True), (3, 1, False)]
    rows = {}
    for fc_hw, w0, H in (((1, 1), (848, 64), 40), ((2, 1), (1696, 64), 20)):
        spec = ops.DecoderSpec(layers, fc_hw, True, precision="bf16x3")
        plan = ops.plan_decoder(spec, [w0, (176, 53), (148, 44), (3, 37)], [True] * 4, 2, H, 80, False)
        assert (plan[1].H, plan[1].W) == (160, 320)
        rows[fc_hw] = notation(plan)
    assert rows[1, 1] == "3-3 333g 333xg ffs"
    assert rows[2, 1] == "3-f 333 333xg ffs"

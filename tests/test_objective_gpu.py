"""The resolved objective (neuroquant_amd/objective.py) on the GPU: `head_grad` returns the bits of the direct
ops.*_head_grad call it stands for -- `rec`, `dimg` and, with a hand-over slot, the head's bias gradient -- for a float target and
for a (cache_u8, idx) target, and `head_request` asks for the fused head loss for l2 only.  torch.equal, no tolerance: both
sides launch the same kernel with the same arguments, and these kernels are bit-identical from call to call."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

PARAMS = {"l2": {}, "yuv420": dict(matrix="bt601", full_range=True, weights=(4.0, 1.0, 2.0)), "ssim": dict(w_mse=0.7, w_ssim=0.3),
          "msssim": dict(w_mse=0.3, w_ms=0.7)}
CASES = [("l2", (2, 3, 64, 64)),        # H * W = 4096: the fused tanh-head kernel applies
         ("l2", (2, 3, 12, 20)),        # it does not: l2_loss_head_grad returns None, the fallback is l2_loss_and_grad
         ("yuv420", (2, 3, 4, 6)),
         ("ssim", (2, 3, 11, 11)),      # the 11 x 11 minimum, a single window position
         ("ssim", (1, 3, 17, 119)),     # one past ops.SSIM_LOSS_TILE in both directions
         ("msssim", (1, 3, 161, 162))]  # the smallest legal size, with unequal sides


def _inputs(shape):
    g = torch.Generator().manual_seed(shape[2] * 1000 + shape[3])
    pred = 0.5 * torch.tanh(torch.randn(shape, generator=g)) + 0.5
    cache = torch.randint(0, 256, (4,) + shape[1:], generator=g, dtype=torch.uint8)
    idx = torch.tensor([2, 0, 3][:shape[0]], dtype=torch.int64)
    return pred.to(DEV), torch.rand(shape, generator=g).to(DEV), cache.to(DEV), idx.to(DEV)


def _node():
    """a stand-in for the decoder node that owns a hand-over slot"""
    from neuroquant_amd import ops

    class Node:
        nq_head = ops._HeadHandoff()
    return Node


@pytest.mark.parametrize("slot", [False, True], ids=["no_slot", "slot"])
@pytest.mark.parametrize("cached", [False, True], ids=["float", "cache"])
@pytest.mark.parametrize("name,shape", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_head_grad_is_the_direct_call(name, shape, cached, slot):
    from neuroquant_amd import objective, ops
    assert ops.SSIM_LOSS_TILE == (8, 118)
    pred, tgt, cache, idx = _inputs(shape)
    obj = objective.resolve(name, PARAMS[name])
    direct_fn = {"l2": ops.l2_loss_head_grad, "yuv420": ops.yuv420_loss_head_grad, "ssim": ops.ssim_loss_head_grad,
                 "msssim": ops.msssim_loss_head_grad}[name]
    kw = dict(cache_u8=cache, idx=idx) if cached else dict(tgt=tgt)
    want_node, got_node = (_node(), _node()) if slot else (None, None)
    want = direct_fn(pred, node=want_node, **kw, **PARAMS[name])
    if name == "l2":
        fused = slot and (shape[2] * shape[3]) % 4096 == 0
        assert (want is not None) == fused                             # the case exercises the path it is there for
        if want is None:
            want = ops.l2_loss_and_grad(pred, ops.gather_frames_u8(cache, idx) if cached else tgt)
        want_rec = want[0]
    else:
        want_rec = want[0][0]
    rec, dimg = obj.head_grad(pred, (cache, idx) if cached else tgt, got_node)
    assert rec.shape == () and torch.equal(rec, want_rec) and bool(torch.isfinite(rec)) and float(rec) > 0.0
    assert dimg.shape == pred.shape and torch.equal(dimg, want[1]) and float(dimg.abs().max()) > 0.0
    if slot and not (name == "l2" and not fused):
        head, ref = got_node.nq_head, want_node.nq_head
        assert dimg is head.dconv and head.version == dimg._version and head.loss is None
        assert head.db.shape == (shape[1],) and torch.equal(head.db, ref.db)
    elif slot:                                                         # the fallback leaves the slot alone
        assert got_node.nq_head.dconv is None and got_node.nq_head.db is None


@pytest.mark.parametrize("cached", [False, True], ids=["float", "cache"])
def test_head_request_is_set_for_l2(monkeypatch, cached):
    from neuroquant_amd import objective, ops
    monkeypatch.delenv("NQ_FUSED_HEAD_LOSS", raising=False)
    pred, tgt, cache, idx = _inputs((2, 3, 12, 20))
    assert getattr(ops._LOSS_TLS, "req", None) is None
    with objective.resolve("l2").head_request((cache, idx) if cached else tgt):
        req = ops._LOSS_TLS.req
        assert len(req) == 3 and (req[0] is None and req[1] is cache and req[2] is idx if cached
                                  else req[0] is tgt and req[1] is None and req[2] is None)
    assert ops._LOSS_TLS.req is None


@pytest.mark.parametrize("name", ["yuv420", "ssim", "msssim"])
def test_head_request_is_absent_for_the_other_objectives(monkeypatch, name):
    from neuroquant_amd import objective, ops
    monkeypatch.delenv("NQ_FUSED_HEAD_LOSS", raising=False)
    pred, tgt, cache, idx = _inputs((2, 3, 12, 20))
    for target in (tgt, (cache, idx)):
        with objective.resolve(name, PARAMS[name]).head_request(target):
            assert getattr(ops._LOSS_TLS, "req", None) is None
        assert getattr(ops._LOSS_TLS, "req", None) is None

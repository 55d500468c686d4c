"""The HIP ConvNeXt block (ops.convnext_block, csrc/convnext.hip) against its float64 restatement (tests/convnext_ref.py)."""
import copy

import pytest
import torch

import convnext_ref as R
from conftest import TINY_HNERV

pytestmark = pytest.mark.gpu

NAMES = ["out", "dx"] + ["d_" + k for k in R.SHAPES]
SHAPES = [(2, 8, 1, 2),       # the tiny config's last stage: the window is larger than the image
          (2, 16, 2, 4),      # the 3M model's last stage
          (2, 16, 5, 9),      # smaller than the halo, odd sizes
          (1, 64, 17, 33),    # one past the tile boundaries in both directions
          (1, 64, 40, 72),    # several workgroups: the partial sums and the finishing launch
          (1, 24, 7, 7)]      # a width that is neither 16 nor 64


def hip_out_and_grads(tensors, dy):
    from neuroquant_amd import ops
    leaves = [t.cuda().requires_grad_(True) for t in tensors]
    out = ops.convnext_block(*leaves)
    return [out.detach()] + list(torch.autograd.grad(out, leaves, dy.cuda()))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_block_matches_float64_and_repeats(shape):
    x, params, dy = R.inputs(shape, seed=sum(shape))
    ref64, ref32 = R.out_and_grads([x] + params, dy, torch.float64), R.out_and_grads([x] + params, dy, torch.float32)
    got, again = hip_out_and_grads([x] + params, dy), hip_out_and_grads([x] + params, dy)
    ok = [R.within_bound(f"{shape} {n}", g, r64, r32) for n, g, r64, r32 in zip(NAMES, got, ref64, ref32)]
    assert all(ok), [n for n, o in zip(NAMES, ok) if not o]
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_block_at_the_module_init():
    """gamma = 1e-6, weights of std 0.02: what a fresh encoder runs; out and dx"""
    shape = (1, 16, 9, 12)
    x, params, dy = R.inputs(shape, seed=5, init=True)
    ref64, ref32 = R.out_and_grads([x] + params, dy, torch.float64), R.out_and_grads([x] + params, dy, torch.float32)
    got = hip_out_and_grads([x] + params, dy)
    assert all([R.within_bound(f"init {n}", g, r64, r32) for n, g, r64, r32 in list(zip(NAMES, got, ref64, ref32))[:2]])


def test_second_derivative_is_refused():
    x, params, dy = R.inputs((1, 8, 3, 4), seed=2)
    from neuroquant_amd import ops
    leaves = [t.cuda().requires_grad_(True) for t in [x] + params]
    with pytest.raises(NotImplementedError):
        torch.autograd.grad(ops.convnext_block(*leaves), leaves, dy.cuda(), create_graph=True)


def test_hnerv_encoder_on_hip_blocks():
    from neuroquant_amd.models import HNeRV
    from neuroquant_amd.models._layers import Block
    with pytest.raises(ValueError):
        Block(12, kernels='hip')
    torch.manual_seed(3)
    m_torch, m_hip = HNeRV(TINY_HNERV), HNeRV(dict(TINY_HNERV, enc_kernels='hip'))
    with torch.no_grad():
        for name, p in m_torch.encoder.named_parameters():
            if name.endswith("gamma"):
                p.fill_(0.5)      # at 1e-6 the blocks would hide under their residuals
    assert m_hip.state_dict().keys() == m_torch.state_dict().keys()
    m_hip.load_state_dict(m_torch.state_dict())
    img = torch.rand(2, 3, TINY_HNERV["crop_h"], TINY_HNERV["crop_w"])

    def run(model, dtype, device):
        enc = copy.deepcopy(model).to(device=device, dtype=dtype).encoder
        y = enc(img.to(device=device, dtype=dtype))
        dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(4)).to(device=device, dtype=dtype)
        y.backward(dy)
        return {"out": y.detach().cpu(), **{k: p.grad.cpu() for k, p in enc.named_parameters()}}

    ref64, ref32, got = run(m_torch, torch.float64, "cpu"), run(m_torch, torch.float32, "cpu"), run(m_hip, torch.float32, "cuda")
    ok = {k: R.within_bound("encoder " + k, got[k], ref64[k], ref32[k]) for k in ref64}
    assert all(ok.values()), [k for k, o in ok.items() if not o]

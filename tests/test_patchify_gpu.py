"""The HIP encoder stages (ops.patchify_ln, csrc/patchify.hip) against their float64 restatement (tests/patchify_ref.py) under the
project's bound (convnext_ref.within_bound)."""
import copy

import pytest
import torch

import patchify_ref as R
from conftest import TINY_HNERV
from convnext_ref import within_bound

pytestmark = pytest.mark.gpu

CASES = [(2, 3, 10, 20, 16, 5, "post"),      # K = 75 with a padded tail, 8 output pixels: fewer than one tile
         (1, 3, 23, 87, 64, 5, "post"),      # ignored remainder rows and columns, 4 x 17 pixels (one past a tile), four M tiles
         (1, 3, 80, 400, 64, 5, "post"),     # 80 tiles: partials over many workgroups and the finishing launch
         (2, 16, 2, 4, 8, 2, "pre"),         # the tiny config's last stage: 1 x 2 output pixels, C_out = 8 (half an M tile)
         (2, 64, 4, 8, 16, 2, "pre"),        # the 3M model's last stage: 8-byte loads, C_out != C_in
         (1, 64, 12, 132, 64, 4, "pre"),     # the 16-byte path, K = 1024 (the K split), 3 x 33 output pixels
         (2, 32, 64, 96, 64, 4, "pre"),      # 48 tiles over both frames, C_in = 32
         (1, 24, 7, 11, 40, 3, "pre")]       # s = 3, widths that are neither 16 nor 64, remainders in both directions


def hip_out_and_grads(tensors, dy, order, x_grad=True):
    from neuroquant_amd import ops
    leaves = [t.cuda().requires_grad_(True) for t in tensors]
    leaves[0].requires_grad_(x_grad)
    out = ops.patchify_ln(*leaves, order)
    grads = list(torch.autograd.grad(out, leaves if x_grad else leaves[1:], dy.cuda()))
    return [out.detach()] + ([] if x_grad else [None]) + grads


@pytest.mark.parametrize("case", CASES, ids=str)
def test_stage_matches_float64_and_repeats(case):
    *shape, order = case
    x, params, dy = R.inputs(shape, order, seed=sum(shape))
    ref64, ref32 = (R.out_and_grads([x] + params, dy, order, dt) for dt in (torch.float64, torch.float32))
    got, again = hip_out_and_grads([x] + params, dy, order), hip_out_and_grads([x] + params, dy, order)
    ok = [within_bound(f"{case} {n}", g, r64, r32) for n, g, r64, r32 in zip(R.NAMES, got, ref64, ref32)]
    assert all(ok), [n for n, o in zip(R.NAMES, ok) if not o]
    H, W, s = shape[2], shape[3], shape[5]
    assert not got[1][:, :, H // s * s:, :].any() and not got[1][:, :, :, W // s * s:].any()
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_post_without_input_gradient():
    x, params, dy = R.inputs((1, 3, 23, 87, 64, 5), "post", seed=7)
    full, nodx = hip_out_and_grads([x] + params, dy, "post"), hip_out_and_grads([x] + params, dy, "post", x_grad=False)
    assert nodx[1] is None and full[1] is not None
    assert all(torch.equal(a, b) for a, b in zip(full[2:], nodx[2:]))


def test_second_derivative_is_refused():
    from neuroquant_amd import ops
    x, params, dy = R.inputs((1, 8, 4, 6, 8, 2), "pre", seed=2)
    leaves = [t.cuda().requires_grad_(True) for t in [x] + params]
    with pytest.raises(NotImplementedError):
        torch.autograd.grad(ops.patchify_ln(*leaves, "pre"), leaves, dy.cuda(), create_graph=True)


def test_hnerv_encoder_on_hip_blocks_and_stages():
    from neuroquant_amd.models import HNeRV
    torch.manual_seed(3)
    m_torch, m_hip = HNeRV(TINY_HNERV), HNeRV(dict(TINY_HNERV, enc_kernels='hip_all'))
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
    ok = {k: within_bound("encoder " + k, got[k], ref64[k], ref32[k]) for k in ref64}
    assert all(ok.values()), [k for k, o in ok.items() if not o]

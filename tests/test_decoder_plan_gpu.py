"""The decoder node launches what ops.plan_decoder planned: the per-launch profile of one forward + backward holds exactly the
kernels, shapes and counts that the plan predicts (the routing table itself is pinned in test_decoder_plan_cpu.py)."""
import collections

import pytest
import torch

from conftest import TINY_HNERV, TINY_NERV

pytestmark = pytest.mark.gpu

DEV = "cuda"


def predicted_launches(plan, B):
    """profile keys (family, k, cin, cout, H, W, B, epilogue) -> launch count of one forward + backward by this plan"""
    want = collections.Counter()
    for l, p in enumerate(plan):
        want["conv_igemm3" if p.fwd == "bf16x3" else "conv_igemm", p.k, p.cin, p.cout, p.H, p.W, B, p.epi] += 1
        if p.dgrad is not None:   # the data gradient is a convolution cout -> cin on the same pixels
            epi = p.dgrad_epi if l else 0
            want["conv_igemm3" if p.dgrad == "bf16x3" else "conv_igemm", p.k, p.cout, p.cin, p.H, p.W, B, epi] += 1
        if p.wgrad == "swapped3":   # the head's weight gradient runs as the exchanged problem cout -> cin
            want["conv_wgrad3", p.k, p.cout, p.cin, p.H, p.W, B, 0] += 1
        else:
            want["conv_wgrad3" if p.wgrad == "bf16x3" else "conv_wgrad", p.k, p.cin, p.cout, p.H, p.W, B, 0] += 1
    return dict(want)


@pytest.mark.parametrize("prec", ("bf16x3", "fp32"))
@pytest.mark.parametrize("arch", ("hnerv", "nerv"))
def test_decoder_node_launches_its_plan(arch, prec):
    """tiny HNeRV / NeRV at B = 2 and 320 x 640 frames: the smallest shipped shapes at which all three weight-gradient routes
    and both forward routes occur"""
    from neuroquant_amd import ops
    from neuroquant_amd.models import HNeRV, NeRV, _decode
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.manual_seed(3)
    model = (HNeRV(TINY_HNERV) if arch == "hnerv" else NeRV(TINY_NERV)).to(DEV)
    spec, provs = _decode._fused_stack(model)
    spec.precision = prec
    ws = [p() for p in provs]
    B, (H, W) = 2, (1, 2) if arch == "hnerv" else (1, 1)
    emb = torch.randn(B, ws[0][0].shape[1], H, W, device=DEV)
    plan = ops.plan_decoder(spec, [tuple(w.shape[:2]) for w, _ in ws], [b is not None for _, b in ws], B, H, W, False)
    if prec == "bf16x3":
        assert {p.wgrad for p in plan} == {"bf16x3", "swapped3", "fp32"} and {p.fwd for p in plan} == {"bf16x3", "fp32"}
    ops.profile_start()
    try:
        img = ops.decoder_stack(emb, spec, ws)
        img.backward(torch.randn_like(img))
    finally:
        prof = ops.profile_stop()
    assert tuple(img.shape) == (B, 3, 320, 640)
    assert {key: launches for key, (launches, _) in prof.items()} == predicted_launches(plan, B)
    assert all(w.grad is not None and b.grad is not None for w, b in ws)

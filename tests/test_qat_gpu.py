"""The QAT weight quantisers on the GPU (ops.qat_weight, csrc/qat.hip) against their numpy restatement (tests/qat_ref.py): hinerv
forward bit for bit in float32, the gradients against float64 under the project's bound (DESIGN.md §20,
convnext_ref.within_bound), and one `regress --qat` step per mode."""
import copy
import functools

import numpy as np
import pytest
import torch

import qat_ref as R
from conftest import TINY_HNERV
from convnext_ref import within_bound

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 1), (5, 3, 3), (65, 8, 3), (130, 7, 5), (16, 16, 1)]   # a one-row column | K = 27 | rows cross a wave's chunk | three column tiles, one partial | all 16-byte
BITS = [2, 4, 8]
SEED, STEP = 903, 5


@functools.lru_cache(None)
def tensors():
    """[(w, g)] per shape: w ~ 0.5 N(0, 1) with, where there is room, a tie for a column's maximum between its row and the last
    row (column 1) and a column of zeros (column 2)"""
    rng = np.random.default_rng(11)
    out = []
    for cout, cin, k in SHAPES:
        w = (0.5 * rng.standard_normal((cout, cin * k * k))).astype(np.float32)
        w[-1, 1] = -np.abs(w[:, 1]).max()
        w[:, 2] = 0
        g = rng.standard_normal((cout, cin, k, k)).astype(np.float32)
        out.append((torch.from_numpy(w.reshape(g.shape)).cuda(), torch.from_numpy(g).cuda()))
    return out


def masks(noise):
    return [R.mask(w.shape, SEED, STEP, i) if noise else None for i, (w, _) in enumerate(tensors())]


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("bits", BITS)
def test_hinerv_forward_bit_for_bit(bits, noise):
    from neuroquant_amd import ops
    ws = [w for w, _ in tensors()]
    ys, work = ops.qat_weight_raw(ws, bits, "hinerv", noise, SEED, STEP)
    for i, (w, y, (s, a), m) in enumerate(zip(ws, ys, ops.qat_stats(work, ws), masks(noise))):
        ry, rs, ra, _ = R.hinerv(w.cpu().numpy(), bits, m, np.float32)
        assert np.array_equal(s.cpu().numpy(), rs) and np.array_equal(a.cpu().numpy(), ra), SHAPES[i]
        assert np.array_equal(y.cpu().numpy().reshape(ry.shape), ry), SHAPES[i]      # with noise: the mask is the generator's
        alone = ops.qat_weight_raw([w], bits, "hinerv", noise, SEED, STEP, indices=[i])[0][0]
        assert torch.equal(alone, y), SHAPES[i]


def test_noise_mask_rate_on_a_million_elements():
    from neuroquant_amd import ops
    w = torch.randn(1000, 1000, generator=torch.Generator().manual_seed(2)).cuda()
    m = R.mask(w.shape, SEED, STEP, 0)
    assert abs(m.mean() - 0.1) <= 0.0015                       # 5 sigma of a binomial
    y = ops.qat_weight_raw([w], 8, "hinerv", True, SEED, STEP)[0][0].cpu().numpy()
    assert np.array_equal(y, R.hinerv(w.cpu().numpy(), 8, m, np.float32)[0])
    assert abs((y == w.cpu().numpy()).mean() - 0.1) <= 0.0015  # untouched elements: the mask's (and the odd element that is its own level)


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("bits", BITS)
def test_hinerv_backward_matches_float64_and_repeats(bits, noise):
    from neuroquant_amd import ops
    ws, gs = zip(*tensors())
    work = ops.qat_weight_raw(ws, bits, "hinerv", noise, SEED, STEP)[1]
    got, again = (ops.qat_weight_backward_raw(ws, gs, bits, "hinerv", noise, SEED, STEP, ws=work) for _ in range(2))
    for i, (w, g, d, d2, m) in enumerate(zip(ws, gs, got, again, masks(noise))):
        r64, r32 = (torch.from_numpy(R.hinerv_backward(w.cpu().numpy(), g.cpu().numpy(), bits, m, dt)) for dt in (np.float64, np.float32))
        assert within_bound(f"hinerv {SHAPES[i]} b{bits}", d.reshape(r64.shape), r64, r32) and torch.equal(d, d2), SHAPES[i]
        assert noise or not d.reshape(r64.shape)[:, 2].any()                 # the column of zeros: no scale gradient


@pytest.mark.parametrize("bits", BITS)
def test_ffnerv_matches_float64(bits):
    from neuroquant_amd import ops
    ws, gs = zip(*tensors())
    leaves = [w.clone().requires_grad_(True) for w in ws]
    ys = ops.qat_weight(leaves, bits, "ffnerv")
    dws = torch.autograd.grad(ys, leaves, gs)
    off = [R.ffnerv_excused(y.detach().cpu().numpy(), w.cpu().numpy(), bits) * w.numel() for w, y in zip(ws, ys)]
    assert sum(off) / sum(w.numel() for w in ws) <= 1e-3
    for i, (w, g, d) in enumerate(zip(ws, gs, dws)):
        r64, r32 = (torch.from_numpy(R.ffnerv_backward(w.cpu().numpy(), g.cpu().numpy(), dt)) for dt in (np.float64, np.float32))
        assert within_bound(f"ffnerv {SHAPES[i]} b{bits}", d, r64, r32), SHAPES[i]


@pytest.mark.parametrize("mode", ["ffnerv", "hinerv"])
def test_one_regress_step_with_qat(mode):
    """The latent gradients of one trainer step = the decoder's gradients at the quantised weights (the same step with them fed as
    plain leaves) pushed through the restatement's backward; everything else bit for bit; evaluations decode quantised weights."""
    from neuroquant_amd import objective, ops
    from neuroquant_amd.methods import regress
    bits = 6
    args = regress.parse_args(["--arch", "hnerv", "--enc_kernels", "hip_all", "--qat", mode, "--qat_bits", str(bits), "--qat_seed", str(SEED)])
    torch.manual_seed(1)
    model = regress.build_model(args, TINY_HNERV, "cuda")
    plain = copy.deepcopy(model)
    plain.weight_qat = None
    sample = {"img": torch.rand(2, 3, 320, 640, generator=torch.Generator().manual_seed(3)).cuda()}
    obj = objective.of_params(None)
    names = [n for n, p in model.named_parameters() if not n.startswith("encoder") and p.dim() == 4]
    latent = {n: p.detach().clone() for n, p in model.named_parameters()}
    regress.train_step(model, torch.optim.SGD(model.parameters(), lr=0.0), sample, args, obj)
    step = int(model.weight_qat.step) if mode == "hinerv" else 0
    quantised = ops.qat_weight_raw([latent[n] for n in names], bits, mode, True, SEED, step)[0]
    assert len(names) == 7 and all(torch.equal(a, b) for a, b in zip(quantised, model.weight_qat.last))
    with torch.no_grad():
        for n, q in zip(names, quantised):
            plain.get_parameter(n).copy_(q)
    regress.train_step(plain, torch.optim.SGD(plain.parameters(), lr=0.0), sample, args, obj)
    got, G = {n: p.grad for n, p in model.named_parameters()}, {n: p.grad for n, p in plain.named_parameters()}
    assert all(torch.equal(got[n], G[n]) for n in got if n not in names)          # the encoder and the biases
    for i, n in enumerate(names):
        w, g = latent[n].cpu().numpy(), G[n].cpu().numpy()
        m = R.mask(w.shape, SEED, step, i)
        r64, r32 = (torch.from_numpy(R.hinerv_backward(w, g, bits, m, dt) if mode == "hinerv" else R.ffnerv_backward(w, g, dt))
                    for dt in (np.float64, np.float32))
        assert within_bound(f"{mode} {n}", got[n].reshape(r64.shape), r64, r32), n
    model.eval()
    with torch.no_grad():
        model(sample["img"])
    full = ops.qat_weight_raw([latent[n] for n in names], bits, mode, False)[0]
    assert all(torch.equal(a, b) for a, b in zip(full, model.weight_qat.last)) and not torch.equal(full[3], latent[names[3]])
    assert set(model.state_dict()) == set(plain.state_dict())

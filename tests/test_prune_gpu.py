"""Magnitude pruning on the GPU (csrc/prune.hip through ops) against the numpy restatement (tests/prune_ref.py): threshold, tie
count, mask words and pruned weights are integers and zeros, so everything is compared exactly."""
import functools

import numpy as np
import pytest
import torch

import prune_ref as R
from conftest import TINY_HNERV

pytestmark = pytest.mark.gpu


@functools.lru_cache(None)
def run():
    from neuroquant_amd import _lib
    return _lib.lib().nq_prune_run()


# unaligned heads and tails | a segment inside one wave | a run that spans a segment boundary | several workgroups
LENGTHS = {"one": lambda: [1], "small": lambda: [63, 1, 130], "span": lambda: [run() - 1, 2, run() + 5], "runs": lambda: [3 * run() + 5]}
RECIPES = ["normal", "bytes", "zeros", "two"]
KS = ["0", "1", "N-1", "N", "tie", "0.4N"]


@functools.lru_cache(None)
def patterns(lengths, recipe):
    """the list's values as one flat float32 array"""
    n = sum(LENGTHS[lengths]())
    rng = np.random.default_rng(5)
    sign = rng.integers(0, 2, n).astype(np.uint32) << 31
    if recipe == "normal":
        return rng.standard_normal(n).astype(np.float32)
    if recipe == "bytes":        # differ in the lowest byte only, or in the highest only: the last / the first pass decides
        lo = np.uint32(0x3f000000) | rng.integers(0, 256, n).astype(np.uint32)
        hi = (rng.integers(0, 0x7f, n).astype(np.uint32) << 24) | np.uint32(0x00345678)
        return (np.where(rng.integers(0, 2, n) == 0, lo, hi) | sign).view(np.float32)
    if recipe == "zeros":        # half +-0, a quarter subnormals, a quarter normals
        kind = rng.integers(0, 4, n)
        sub = rng.integers(1, 0x800000, n).astype(np.uint32)
        nrm = rng.standard_normal(n).astype(np.float32).view(np.uint32) & np.uint32(0x7fffffff)
        return (np.where(kind < 2, np.uint32(0), np.where(kind == 2, sub, nrm)) | sign).view(np.float32)
    return rng.choice(np.array([0.25, -0.25, 1.5, -1.5], np.float32), n)   # ties across every boundary


def resolve_k(k, m):
    n = m.size
    if k == "tie":               # the middle of the run of ties around the median magnitude
        v = np.sort(m)[n // 2]
        return int((m < v).sum() + (m == v).sum() // 2)
    return {"0": 0, "1": 1, "N-1": n - 1, "N": n, "0.4N": int(np.floor(0.4 * n))}[k]


def on_device(flat, lens):
    """the segments as contiguous views of ONE buffer behind a one-element offset: every alignment occurs"""
    buf = torch.zeros(flat.size + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(flat).cuda()
    return list(buf[1:].split(lens))


def bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("lengths", list(LENGTHS))
def test_select_mask_apply_equal_the_reference(lengths, recipe, k):
    from neuroquant_amd import ops
    lens, flat = LENGTHS[lengths](), patterns(lengths, recipe)
    k = resolve_k(k, flat.view(np.uint32) & np.uint32(0x7fffffff))
    ws = on_device(flat, lens)
    ref = [w.copy() for w in np.split(flat, np.cumsum(lens)[:-1])]
    T, r, below, keep = R.prune_ref(ref, k)
    sel = ops.magnitude_select(ws, k)
    print(lengths, recipe, k, sel.tolist(), (T, r, below))
    assert sel.tolist() == [T, r, below, k]
    mask = ops.prune_mask(ws, sel)
    assert np.array_equal(mask.cpu().numpy().view(np.uint64), R.mask_words(keep))
    ops.prune_apply_(ws, mask)
    for w, w0, b in zip(ws, ref, keep):
        w0[~b] = 0.0
        assert np.array_equal(bits(w), w0.view(np.uint32))          # +0 exactly where pruned, every other bit untouched


def test_repeats_bit_for_bit_and_k_from_the_device():
    from neuroquant_amd import ops
    ws = on_device(patterns("span", "two"), LENGTHS["span"]())
    n = sum(w.numel() for w in ws)
    k_dev = torch.tensor([n // 3], dtype=torch.int64, device="cuda")
    a, b = ops.magnitude_select(ws, k_dev), ops.magnitude_select(ws, n // 3)
    assert torch.equal(a, b) and torch.equal(ops.prune_mask(ws, a), ops.prune_mask(ws, b))
    copy = [w.clone() for w in ws]
    (m1, s1), (m2, s2) = ops.magnitude_prune_(ws, 1 / 3), ops.magnitude_prune_(copy, 1 / 3)
    assert torch.equal(m1, m2) and torch.equal(s1, s2) and all(torch.equal(x, y) for x, y in zip(ws, copy))


def test_apply_masks_all_three_companions():
    from neuroquant_amd import ops
    lens, flat = LENGTHS["span"](), patterns("span", "normal")
    ws = on_device(flat, lens)
    comp = [on_device(np.random.default_rng(s).standard_normal(flat.size).astype(np.float32) + 3.0, lens) for s in (1, 2, 3)]
    before = [[c.clone() for c in cs] for cs in comp]
    keep = R.prune_ref(np.split(flat, np.cumsum(lens)[:-1]), flat.size // 2)[3]
    mask = ops.prune_mask(ws, ops.magnitude_select(ws, flat.size // 2))
    ops.prune_apply_(ws, mask, comp[0], [comp[1][0], None, comp[1][2]], comp[2])
    for j, (cs, bs) in enumerate(zip(comp, before)):
        for i, (c, c0, b) in enumerate(zip(cs, bs, keep)):
            want = c0.cpu().numpy()
            if not (j == 1 and i == 1):                                  # the companion that was not given stays whole
                want[~b] = 0.0
            assert np.array_equal(bits(c), want.view(np.uint32)), (j, i)


def test_three_trainer_steps_hold_the_mask():
    from neuroquant_amd import objective
    from neuroquant_amd.methods import regress
    args = regress.parse_args(["--arch", "hnerv", "--prune_ratio", "0.5"])
    torch.manual_seed(1)
    model = regress.build_model(args, TINY_HNERV, "cuda")
    names = [n for n, p in model.named_parameters() if not n.startswith("encoder") and p.dim() == 4]
    dense = {n: p.detach().cpu().numpy().copy() for n, p in model.named_parameters()}
    keys = set(model.state_dict())
    pruner = regress.prune_model(model, args)
    assert all(np.array_equal(p.detach().cpu().numpy(), dense[n]) for n, p in model.named_parameters() if n not in names)
    n_all = sum(dense[n].size for n in names)
    keep = R.prune_ref([dense[n] for n in names], n_all // 2)[3]
    assert len(names) == 7 and list(pruner.names) == names
    assert np.array_equal(pruner.mask.cpu().numpy().view(np.uint64), R.mask_words(keep))
    sp = pruner.sparsity()
    assert sp["total"] == (n_all // 2) / n_all and all(sp[n] == float((~b).sum()) / b.size for n, b in zip(names, keep))
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=0.)
    sample = {"img": torch.rand(2, 3, 320, 640, generator=torch.Generator().manual_seed(3)).cuda()}
    for _ in range(3):
        regress.train_step(model, optimizer, sample, args, objective.of_params(None), pruner)
        for n, b in zip(names, keep):
            p = model.get_parameter(n)
            w = p.detach().cpu().numpy().reshape(-1)
            assert not w[~b].view(np.uint32).any() and not np.array_equal(w[b], dense[n].reshape(-1)[b]), n
            assert not optimizer.state[p]["exp_avg"].cpu().numpy().reshape(-1)[~b].any(), n
    assert set(model.state_dict()) == keys                                   # the checkpoint keeps its keys

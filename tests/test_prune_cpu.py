"""Magnitude pruning without a GPU: the argument rules of ops and of the C entries, the trainer's refusal, and the numpy
restatement (tests/prune_ref.py) on a case worked by hand."""
import ctypes

import numpy as np
import pytest
import torch

import prune_ref as R


def test_reference_on_a_hand_worked_case():
    # magnitudes 2 0 1 | 1 0 3: the order is (0: a1) (-0: b1) (1: a2) (-1: b0) (2: a0) (3: b2)
    ws = [np.array([2.0, 0.0, 1.0], np.float32), np.array([-1.0, -0.0, 3.0], np.float32)]
    one = int(np.float32(1.0).view(np.uint32))
    T, r, below, keep = R.prune_ref(ws, 3)
    assert (T, r, below) == (one, 1, 2)                             # the first of the two ties at 1 goes: a2, not b0
    assert [b.tolist() for b in keep] == [[True, False, False], [True, False, True]]
    assert R.mask_words(keep).tolist() == [0b001, 0b101]
    assert R.prune_ref(ws, 0)[:3] == (0, 0, 0) and all(b.all() for b in R.prune_ref(ws, 0)[3])
    T, r, below, keep = R.prune_ref(ws, 6)
    assert (T, r, below) == (int(np.float32(3.0).view(np.uint32)), 1, 5) and not any(b.any() for b in keep)


@pytest.mark.parametrize("bad", [[], [torch.zeros(4, 4).t()], [torch.zeros(3, dtype=torch.float64)], [torch.zeros(0)],
                                 [torch.zeros(1)] * 17])
def test_ops_refuse_bad_lists_before_the_device(bad):
    from neuroquant_amd import ops
    for call in (lambda: ops.magnitude_select(bad, 1), lambda: ops.magnitude_prune_(bad, 0.5),
                 lambda: ops.prune_mask(bad, torch.zeros(4, dtype=torch.int64)),
                 lambda: ops.prune_apply_(bad, torch.zeros(1, dtype=torch.int64))):
        with pytest.raises(ValueError):
            call()


def test_ops_refuse_bad_ratio_k_mask_and_companions():
    from neuroquant_amd import ops
    w = [torch.zeros(70)]
    for ratio in (-0.1, 1.5, float("nan"), "0.4", True):
        with pytest.raises(ValueError):
            ops.magnitude_prune_(w, ratio)
    with pytest.raises(ValueError):
        ops.magnitude_select(w, 0.5)
    with pytest.raises(ValueError):
        ops.prune_apply_(w, torch.zeros(1, dtype=torch.int64))              # 70 elements are two words
    with pytest.raises(ValueError):
        ops.prune_apply_(w, torch.zeros(2, dtype=torch.int64), grads=[torch.zeros(71)])
    with pytest.raises(RuntimeError):
        ops.magnitude_select(w, 1)                                          # a valid list that is not on the GPU: no fallback


def test_c_entries_check_arguments_without_a_gpu():
    from neuroquant_amd import _lib
    lib, p = _lib.lib(), ctypes.c_void_p(64)
    segs = (_lib.PruneSeg * 2)()
    segs[0].w, segs[0].n, segs[1].w, segs[1].n = 64, 1, 1024, lib.nq_prune_run() + 1
    assert lib.nq_prune_ws_bytes(segs, 2) == 2 * 1028                       # the second segment starts a second run
    assert lib.nq_prune_ws_bytes(segs, 0) == 0 and lib.nq_prune_ws_bytes(None, 2) == 0
    assert lib.nq_magnitude_select(segs, 2, None, p, p, None) == -1 and lib.nq_prune_mask(segs, 2, p, ctypes.c_void_p(68), p, None) == -1
    assert lib.nq_prune_apply(segs, 2, None, None) == -1
    segs[1].n = 0
    assert lib.nq_magnitude_select(segs, 2, p, p, p, None) == -1 and lib.nq_prune_ws_bytes(segs, 2) == 0
    segs[1].n, segs[1].w = 5, 1026                                          # not 4-byte aligned
    assert lib.nq_prune_apply(segs, 2, p, None) == -1
    assert lib.nq_prune_apply((_lib.PruneSeg * 17)(), 17, p, None) == -2


def test_trainer_refuses_prune_with_qat_and_a_ratio_out_of_range():
    from neuroquant_amd.methods import regress
    for flags in (["--prune_ratio", "0.4", "--qat", "ffnerv"], ["--prune_ratio", "1.2"]):
        with pytest.raises(ValueError):
            regress.train(regress.parse_args(["--arch", "hnerv"] + flags), {})
    assert regress.parse_args(["--arch", "hnerv"]).prune_ratio is None

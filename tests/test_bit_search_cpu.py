"""Bit allocation under a size budget, host side: the restatement against hand-computed cases, the quadratic-form
identity behind the Omega table, the argument checks of the two new C entries, the refusal of CPU tensors, the new driver
flags and the sharding of the table's columns over ranks.  No GPU."""
import ctypes
import itertools
import json
import math

import numpy as np
import pytest
import torch

import bit_search_ref as R


# ------------------------------------------------------------------------------------------ restatement, by hand
def test_restatement_single_layer_is_the_smallest_feasible_diagonal_entry():
    G = np.diag([5.0, 3.0, 1.0])
    sizes = [[10, 20, 30]]
    assert R.search(G, sizes, 30) == (1.0, 2, 3)
    assert R.search(G, sizes, 29) == (3.0, 1, 2)          # the 30-bit choice no longer fits
    assert R.search(G, sizes, 10) == (5.0, 0, 1)
    assert R.search(G, sizes, 9) == (math.inf, None, 0)   # nothing fits


def test_restatement_two_layers_with_a_negative_cross_term():
    # rows / columns: (layer 0, choice 0), (0, 1), (1, 0), (1, 1)
    G = np.array([[4.0, 0.0, -1.0, 0.5],
                  [0.0, 1.0, 2.0, -3.0],
                  [-1.0, 2.0, 3.0, 0.0],
                  [0.5, -3.0, 0.0, 2.0]])
    sizes = [[1, 2], [1, 2]]
    omega, size = R.enumerate_all(G, sizes)
    # index = c_0 + 2 c_1;  Omega = G[a,a] + G[a,b] + G[b,a] + G[b,b] with a = c_0, b = 2 + c_1
    #   index 0 (c = 0,0): 4 + (-1) + (-1) + 3 = 5         size 2
    #   index 1 (c = 1,0): 1 +   2  +   2  + 3 = 8         size 3
    #   index 2 (c = 0,1): 4 + 0.5  + 0.5  + 2 = 7         size 3
    #   index 3 (c = 1,1): 1 + (-3) + (-3) + 2 = -3        size 4
    assert omega.tolist() == [5.0, 8.0, 7.0, -3.0]
    assert size.tolist() == [2, 3, 3, 4]
    assert [R.omega_of(G, R.index_to_digits(i, 2, 2), 2) for i in range(4)] == [5.0, 8.0, 7.0, -3.0]
    assert R.search(G, sizes, 4) == (-3.0, 3, 4)
    assert R.search(G, sizes, 3) == (5.0, 0, 3)
    assert R.search(G, sizes, 1) == (math.inf, None, 0)
    # ties go to the lowest index; a NaN is never selected
    assert R.search(np.zeros((4, 4)), sizes, 3) == (0.0, 0, 3)
    Gn = G.copy()
    Gn[1, 1] = np.nan                                      # poisons indices 1 and 3
    assert R.search(Gn, sizes, 4) == (5.0, 0, 4)
    assert R.bits_to_index([8, 2, 5], [2, 5, 8]) == 2 + 0 * 3 + 1 * 9
    assert R.index_to_bits(11, 3, [2, 5, 8]) == [8, 2, 5]


# ------------------------------------------------------------------------------------------ the identity
def _random_problem(seed=3, dims=(13, 9, 18), K=3):
    rng = np.random.default_rng(seed)
    n = sum(dims)
    A = rng.standard_normal((n, n))
    H = A + A.T
    off = np.concatenate([[0], np.cumsum(dims)])
    v = [[rng.standard_normal(d) for _ in range(K)] for d in dims]
    return H, off, v


def _gram(H, off, v):
    """G[(l,c),(m,d)] = <e_{l,c}, H e_{m,d}> with e_{l,c} = v_l(c) on block l and zero elsewhere."""
    L, K = len(v), len(v[0])
    E = np.zeros((L * K, H.shape[0]))
    for l in range(L):
        for c in range(K):
            E[l * K + c, off[l]:off[l + 1]] = v[l][c]
    return E @ H @ E.T


def test_table_omega_equals_the_quadratic_form_for_every_allocation():
    from neuroquant_amd.methods.bit_assign import omega_from_table
    H, off, v = _random_problem()
    G = _gram(H, off, v)
    choices = [3, 5, 8]
    for digits in itertools.product(range(3), repeat=3):
        full = np.concatenate([v[l][d] for l, d in enumerate(digits)])
        direct = float(full @ H @ full)
        bits = [choices[d] for d in digits]
        got = omega_from_table(G, bits, choices)
        parts = sum(abs(G[l * 3 + digits[l], m * 3 + digits[m]]) for l in range(3) for m in range(3))
        assert abs(got - direct) <= 1e-12 * max(abs(direct), parts), (digits, got, direct)
        assert got == R.omega_of(G, digits, 3)                       # the package's helper and the restatement: same order
        assert got == omega_from_table(torch.from_numpy(G), bits, choices)


def test_fisher_diag_table_is_additive_and_a_loose_budget_gives_the_per_layer_argmin():
    rng = np.random.default_rng(5)
    L, K = 4, 3
    d = rng.random(L * K) + 0.1
    G = np.diag(d)
    sizes = rng.integers(1, 100, size=(L, K))
    omega, _ = R.enumerate_all(G, sizes)
    for idx in range(K ** L):
        digits = R.index_to_digits(idx, L, K)
        want = 0.0
        for l in range(L):                                           # zeros off the diagonal add nothing, in any order
            want = want + d[l * K + digits[l]]
        assert abs(omega[idx] - want) <= 1e-15 * want
    best, index, n_fit = R.search(G, sizes, int(sizes.max()) * L)
    assert n_fit == K ** L
    assert R.index_to_digits(index, L, K) == [int(np.argmin(d[l * K:(l + 1) * K])) for l in range(L)]


# ------------------------------------------------------------------------------------------ C entries without a device
def test_new_entries_reject_bad_arguments_without_a_gpu():
    from neuroquant_amd import _lib
    lib = _lib.lib()
    n, p = None, ctypes.c_void_p(64)
    for args in [(n, p, p, p), (p, n, p, p), (p, p, n, p), (p, p, p, n)]:
        V, g, out, ws = args
        assert lib.nq_rows_dot(V, g, out, 7, 100, ws, n) == -1
    assert lib.nq_rows_dot(p, p, p, 0, 100, p, n) == -1
    assert lib.nq_rows_dot(p, p, p, 9, 100, p, n) == -1
    assert lib.nq_rows_dot(p, p, p, 7, 0, p, n) == -1
    for args in [(n, p, p, p, p), (p, n, p, p, p), (p, p, n, p, p), (p, p, p, n, p), (p, p, p, p, n)]:
        G, sizes, om, ix, ws = args
        assert lib.nq_bit_search(G, sizes, 7, 7, 1000, om, ix, ws, n) == -1
    assert lib.nq_bit_search(p, p, 0, 7, 1000, p, p, p, n) == -1
    assert lib.nq_bit_search(p, p, 7, 0, 1000, p, p, p, n) == -1
    assert lib.nq_bit_search(p, p, 7, 9, 1000, p, p, p, n) == -1
    assert lib.nq_bit_search(p, p, 13, 2, 1000, p, p, p, n) == -2       # more than 12 layers
    assert lib.nq_bit_search(p, p, 12, 7, 1000, p, p, p, n) == -2       # 7^12 >= 2^32 candidates
    assert lib.nq_rows_dot_ws_bytes(7, 100003) > 0 and lib.nq_rows_dot_ws_bytes(7, 100003) % 8 == 0
    assert lib.nq_bit_search_ws_bytes(7, 7) > 0 and lib.nq_bit_search_ws_bytes(7, 7) % 16 == 0
    assert lib.nq_rows_dot_ws_bytes(9, 100) == 0 and lib.nq_rows_dot_ws_bytes(7, 0) == 0
    assert lib.nq_bit_search_ws_bytes(12, 7) == 0 and lib.nq_bit_search_ws_bytes(13, 2) == 0


def test_ops_refuse_cpu_tensors():
    from neuroquant_amd import ops
    with pytest.raises(RuntimeError):
        ops.rows_dot(torch.zeros(3, 10), torch.zeros(10))
    with pytest.raises(RuntimeError):
        ops.bit_search(torch.zeros(4, 4, dtype=torch.float64), torch.ones(2, 2, dtype=torch.int64), 10)


# ------------------------------------------------------------------------------------------ flags
BASE = ["--arch", "hnerv", "--config", "cfg.yaml", "--synthetic", "8"]


def test_bit_assign_budget_flags(capsys):
    from neuroquant_amd.methods import bit_assign
    a = bit_assign.parse_args(BASE)
    assert a.budget_bytes is None and a.budget_avg_bits is None and a.candidates is None      # as before: candidate scoring
    assert a.bit_choices == [2, 3, 4, 5, 6, 7, 8] and a.size_model == "nominal" and a.frontier is None and a.out is None
    a = bit_assign.parse_args(BASE + ["--budget_bytes", "1400000", "--size_model", "entropy", "--bit_choices", "3", "4", "6",
                                      "--frontier", "1000000", "2000000", "--out", "bits.json"])
    assert (a.budget_bytes, a.size_model, a.bit_choices, a.frontier, a.out) == (1400000, "entropy", [3, 4, 6], [1e6, 2e6], "bits.json")
    assert bit_assign.parse_args(BASE + ["--budget_avg_bits", "4.79"]).budget_avg_bits == 4.79
    for bad in (["--budget_bytes", "10", "--budget_avg_bits", "5"], ["--budget_avg_bits", "5", "--bit_choices", "4", "3"],
                ["--budget_avg_bits", "5", "--bit_choices", "2", "9"], ["--size_model", "exact"]):
        with pytest.raises(SystemExit):
            bit_assign.parse_args(BASE + bad)
    capsys.readouterr()


def test_budget_in_bits_follows_the_functions_that_define_it():
    from neuroquant_amd.methods.bit_assign import average_bits, budget_to_bits, size_tables
    numels = [(1200, 12), (900, 10), (77, 3)]
    assert budget_to_bits(numels, budget_bytes=500) == 4000                      # ceil(s / 8) <= 500  <=>  s <= 4000
    num = sum(a + b for a, b in numels)
    for x in (2.0, 4.79, 5.0, 6.123456, 8.0):
        s = budget_to_bits(numels, budget_avg_bits=x)
        assert s / float(num) <= x < (s + 1) / float(num)
    t = size_tables(numels, [2, 5], [[10.2, 99.0], [3.0, 7.5], [0.0, 1.01]])
    assert t["nominal"] == [[2424, 6060], [1820, 4550], [160, 400]]
    assert t["entropy"] == [[11, 99], [3, 8], [0, 2]]
    assert average_bits([2, 5, 5], numels) == (2 * 1212 + 5 * 910 + 5 * 80) / num


def test_precision_file_round_trip_and_errors(tmp_path, capsys):
    from neuroquant_amd.methods import calibrate_network as cn
    assert cn.parse_args(BASE).precision == [8] * 7                               # as before
    assert cn.parse_args(BASE + ["--precision", "6", "5", "4", "5", "5", "6", "6"]).precision == [6, 5, 4, 5, 5, 6, 6]
    path = tmp_path / "bits.json"
    result = dict(bits=[6, 5, 4, 5, 5, 6, 6], omega=1.25e-3, size_bits=123456, avg_bits=4.79, mode="omega",
                  bit_choices=[2, 3, 4, 5, 6, 7, 8], budget=dict(bits=130000, bytes=None, avg_bits=5.0, size_model="nominal"))
    path.write_text(json.dumps(result))
    assert json.loads(path.read_text()) == result
    a = cn.parse_args(BASE + ["--precision_file", str(path)])
    assert a.precision == [6, 5, 4, 5, 5, 6, 6] and a.precision_file == str(path)
    assert cn.read_precision_file(str(path), 7) == [6, 5, 4, 5, 5, 6, 6]
    with pytest.raises(SystemExit):
        cn.parse_args(BASE + ["--precision_file", str(path), "--precision", "8", "8", "8", "8", "8", "8", "8"])
    with pytest.raises(ValueError, match="6 quantised layers"):
        cn.read_precision_file(str(path), 6)
    short = tmp_path / "short.json"
    short.write_text(json.dumps(dict(bits=[6, 5, 4])))
    with pytest.raises(ValueError, match="lists 3 bit-widths"):
        cn.read_precision_file(str(short), 7)
    for bad in ({"bits": [6, 9]}, {"bits": []}, {"bits": "6 5"}, {}):
        short.write_text(json.dumps(bad))
        with pytest.raises(ValueError):
            cn.read_precision_file(str(short))
    capsys.readouterr()


# ------------------------------------------------------------------------------------------ columns over ranks
@pytest.mark.parametrize("world", (1, 2, 3))
def test_direction_sharding_is_a_partition_and_rebuilds_the_table(world):
    from neuroquant_amd.methods.bit_assign import direction_names, gather_scores, owned_candidates
    L, K = 7, 7
    names = direction_names(L, K)
    assert len(names) == 49 == len(set(names)) and names[0] == "0:0" and names[K] == "1:0" and names[-1] == "6:6"
    owned = [owned_candidates(names, r, world) for r in range(world)]
    assert sorted(n for o in owned for n in o) == sorted(names)                   # covers every column ...
    assert sum(len(o) for o in owned) == len(names)                               # ... exactly once
    assert max(len(o) for o in owned) - min(len(o) for o in owned) <= 1
    assert [owned_candidates(list(range(49)), r, world) for r in range(world)] == [list(range(r, 49, world)) for r in range(world)]
    G = torch.from_numpy(np.random.default_rng(world).standard_normal((49, 49)))
    per_rank = [{n: G[:, names.index(n)].clone() for n in o} for o in owned]
    assert list(gather_scores(per_rank[0], 1)) == owned[0]                        # one rank: its own dict
    merged = {k: v for d in per_rank for k, v in d.items()}                       # gather_scores' union over the ranks' dicts
    assert torch.equal(torch.stack([merged[n] for n in names], dim=1), G)

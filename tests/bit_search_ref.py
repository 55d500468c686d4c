"""Host restatement of the bit-allocation search in numpy float64: what nq_bit_search and nq_rows_dot are
tested against.  Nothing here imports the package.

A candidate is the mixed-radix index sum_l c_l K^l (layer 0 = least significant digit) of its per-layer choices c_l; row /
column (l, c) of the table G sits at l K + c.  Omega of a candidate is summed from 0.0 with l ascending in the outer loop and
m ascending in the inner loop by plain float64 additions -- the kernel's order, so results compare with ==.  The winner is the
lexicographic minimum of (Omega, index) over the candidates whose sizes sum to at most the budget; a NaN Omega is never
selected."""
import math

import numpy as np


def bits_to_index(bits, bit_choices):
    choices = [int(c) for c in bit_choices]
    K = len(choices)
    return sum(choices.index(int(b)) * K ** l for l, b in enumerate(bits))


def index_to_digits(index, L, K):
    return [(int(index) // K ** l) % K for l in range(L)]


def index_to_bits(index, L, bit_choices):
    return [int(bit_choices[d]) for d in index_to_digits(index, L, len(bit_choices))]


def omega_of(G, digits, K):
    """Scalar loop: Omega of one candidate in the specified order."""
    cols = [l * K + d for l, d in enumerate(digits)]
    acc = 0.0
    for i in cols:
        for j in cols:
            acc = acc + float(G[i, j])
    return acc


def enumerate_all(G, size_bits, chunk=1 << 16):
    """-> (omega, size) of all K^L candidates in index order.  Chunked: within a chunk every candidate's sum runs in the
    specified order (one vector addition per (l, m) pair, elementwise)."""
    G = np.asarray(G, dtype=np.float64)
    sizes = np.asarray(size_bits, dtype=np.int64)
    L, K = sizes.shape
    assert G.shape == (L * K, L * K)
    assert int(sizes.min()) >= 0 and int(sizes.max()) < 2 ** 58        # L <= 12 of them sum without wrapping
    total = K ** L
    omega = np.empty(total, dtype=np.float64)
    size = np.empty(total, dtype=np.int64)
    for lo in range(0, total, chunk):
        idx = np.arange(lo, min(lo + chunk, total), dtype=np.int64)
        cols = [l * K + (idx // K ** l) % K for l in range(L)]
        acc = np.zeros(idx.shape, dtype=np.float64)
        sz = np.zeros(idx.shape, dtype=np.int64)
        for l in range(L):
            sz = sz + sizes.reshape(-1)[cols[l]]
            for m in range(L):
                acc = acc + G[cols[l], cols[m]]
        omega[lo:lo + idx.size] = acc
        size[lo:lo + idx.size] = sz
    return omega, size


def select(omega, size, budget):
    """-> (best omega, best index | None, number of candidates that fit) from enumerate_all's arrays."""
    fit = size <= budget
    n_fit = int(fit.sum())
    ok = fit & (omega < np.inf)                      # false for NaN: never selected
    if not ok.any():
        return math.inf, None, n_fit
    best = omega[ok].min()
    return float(best), int(np.flatnonzero(ok & (omega == best))[0]), n_fit


def search(G, size_bits, budget, chunk=1 << 16):
    omega, size = enumerate_all(G, size_bits, chunk)
    return select(omega, size, budget)


def rows_dot(V, g):
    """out[r] = sum_i V[r, i] g[i]: exact float64 products, correctly rounded sum (math.fsum)."""
    V = np.asarray(V, dtype=np.float32).reshape(len(V), -1).astype(np.float64)
    g = np.asarray(g, dtype=np.float32).reshape(-1).astype(np.float64)
    return np.array([math.fsum(row * g) for row in V], dtype=np.float64)


def rows_dot_bound(V, g):
    """|err| <= n 2^-52 sum_i |V_i g_i| for any order of n float64 additions of exact products (each addition errs by at most
    2^-53 of its partial sum, itself at most (1 + n 2^-53) sum |.|)."""
    V = np.asarray(V, dtype=np.float32).reshape(len(V), -1).astype(np.float64)
    g = np.asarray(g, dtype=np.float32).reshape(-1).astype(np.float64)
    return np.array([g.size * 2.0 ** -52 * math.fsum(np.abs(row * g)) for row in V], dtype=np.float64)

"""Global magnitude pruning restated in numpy (the definition: include/nq_hip.h above nq_magnitude_select)."""
import numpy as np


def prune_ref(ws, k):
    """ws: float32 arrays, k: elements to prune -> (T, r, below, keep): keep one bool array per tensor"""
    m = np.concatenate([w.reshape(-1).view(np.uint32) & np.uint32(0x7fffffff) for w in ws])
    k = min(max(int(k), 0), m.size)
    order = np.argsort(m, kind="stable")                  # concatenation order is (segment, index): stable = the rank
    T = int(m[order[min(k, m.size - 1)]])
    below = int((m < T).sum())
    keep = np.ones(m.size, bool)
    keep[order[:k]] = False
    return T, k - below, below, np.split(keep, np.cumsum([w.size for w in ws])[:-1])


def mask_words(keep):
    """the keep bits as the kernels lay them out: every tensor from a fresh 64-bit word, padding bits 0"""
    return np.concatenate([np.packbits(np.pad(b, (0, -b.size % 64)), bitorder="little").view(np.uint64) for b in keep])

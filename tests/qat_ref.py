"""Plain numpy restatement of the QAT weight quantisers (include/nq_hip.h above nq_qat_forward): the reference's
QATQuantizer 'ffnerv' / 'hinerv' as autograd differentiates them, in the reference's operation order.  dt = np.float32 for the
bit-exact checks, np.float64 for the bounds.  A weight (Cout, Cin, k, k) is taken as (Cout, K)."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 (Salmon et al., SC'11) on uint64 arrays holding 32-bit words -> the four output words"""
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def mask(shape, seed, step, index):
    """m of every element: counter {e >> 2, 0, index, step}, key {seed low, seed high}, word e & 3; 1 iff its top 24 bits / 2^24 > 0.9"""
    e = np.arange(int(np.prod(shape)), dtype=np.uint64)
    z = np.zeros_like(e)
    words = philox4x32_10(e >> np.uint64(2), z, z + np.uint64(index), z + np.uint64(step), np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))
    word = np.choose((e & np.uint64(3)).astype(np.int64), words)
    return ((word >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24) > np.float32(0.9)).reshape(shape[0], -1)


def hinerv(w, bits, m, dt):
    """-> y, s_c, a(c), q;  m: the mask (Cout, K) or None for noise off"""
    w = w.reshape(w.shape[0], -1).astype(dt)
    a = np.abs(w)
    s = dt(2) * a.max(0) / dt(2 ** bits - 1) + dt(1e-6)
    q = np.clip(np.rint(w / s), -2 ** (bits - 1), 2 ** (bits - 1) - 1).astype(dt)
    wq = q * s
    return (wq if m is None else w * m.astype(dt) + wq * (dt(1) - m.astype(dt))), s, a.argmax(0), q


def hinerv_backward(w, g, bits, m, dt):
    """dL/dw = g m + [i = a(c)] sign(w) (2 / R) sum_j g (1 - m) q"""
    _, _, arg, q = hinerv(w, bits, m, dt)
    w, g = w.reshape(q.shape).astype(dt), g.reshape(q.shape).astype(dt)
    m = np.zeros(q.shape, dt) if m is None else m.astype(dt)
    dw, cols = g * m, np.arange(q.shape[1])
    dw[arg, cols] += np.sign(w[arg, cols]) * (dt(2) / dt(2 ** bits - 1)) * (g * (dt(1) - m) * q).sum(0)
    return dw


def ffnerv(w, bits, dt):
    """-> y, |t| n (what floor sees)"""
    t, n = np.tanh(w.astype(dt)), dt(2 ** (bits - 1) - 1)
    return np.floor(np.abs(t) * n) / n * np.sign(t), np.abs(t) * n


def ffnerv_backward(w, g, dt):
    t = np.tanh(w.astype(dt))
    return g.astype(dt) * (dt(1) - t * t)


def ffnerv_excused(y, w, bits):
    """Share of the elements of a float32 result y that differ from the float64 restatement by more than 2 ulps; each of them
    must sit where floor is discontinuous (the reference's |t| n within 8 * 2^-24 * n of an integer) on the neighbouring level,
    else AssertionError."""
    n = 2 ** (bits - 1) - 1
    y64, tn = ffnerv(w, bits, np.float64)
    diff = np.abs(y.astype(np.float64) - y64)
    off = diff > 2 * np.spacing(np.abs(y64).astype(np.float32)).astype(np.float64)
    near = np.abs(tn - np.rint(tn)) <= 8 * 2.0 ** -24 * n
    assert np.all(near[off]) and np.all(np.abs(diff[off] * n - 1) < 1e-3), "an element is off a level away from a discontinuity"
    return off.mean()

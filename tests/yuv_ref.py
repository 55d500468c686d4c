"""numpy restatement of the 8-bit YUV 4:2:0 conversions of include/nq_hip.h.

`rgb_to_yuv420` and `yuv420_to_rgb` are float32 throughout, in the operation order of the header, with every constant formed
in float64 and rounded once to float32: the kernels (built with contraction off) must match them bit for bit.
`rgb_to_yuv420_f64` states the forward conversion in float64 with unrounded constants and returns the values BEFORE rounding
and clamping: the yardstick the float32 statement itself is held to."""
import numpy as np

F = np.float32
MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def constants(matrix, dtype=F):
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    c = dict(kr=kr, kg=kg, kb=kb, icb=1.0 / (2.0 * (1.0 - kb)), icr=1.0 / (2.0 * (1.0 - kr)), c_r=2.0 * (1.0 - kr),
             c_b=2.0 * (1.0 - kb), c_gb=kb * (2.0 * (1.0 - kb)) / kg, c_gr=kr * (2.0 * (1.0 - kr)) / kg,
             i219=1.0 / 219.0, i224=1.0 / 224.0, i255=1.0 / 255.0)
    return {k: dtype(v) for k, v in c.items()}


def frame_bytes(H, W):
    return H * W * 3 // 2


def _clamp01(x):
    c = np.where(x > 0, x, x.dtype.type(0))      # NaN fails the comparison -> 0
    return np.where(c < 1, c, x.dtype.type(1))


def _block_mean(c):
    """((c00 + c01) + (c10 + c11)) * 0.25 over 2 x 2 blocks of (n, H, W)"""
    t = c.dtype.type
    return ((c[:, 0::2, 0::2] + c[:, 0::2, 1::2]) + (c[:, 1::2, 0::2] + c[:, 1::2, 1::2])) * t(0.25)


def _forward(x, matrix, full_range, dtype):
    k = constants(matrix, dtype)
    t = dtype
    x = _clamp01(np.asarray(x, dtype=np.float32)).astype(dtype)
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    y = (k["kr"] * r + k["kg"] * g) + k["kb"] * b
    cb = _block_mean((b - y) * k["icb"])
    cr = _block_mean((r - y) * k["icr"])
    if full_range:
        return t(255) * y, t(128) + t(255) * cb, t(128) + t(255) * cr
    return t(16) + t(219) * y, t(128) + t(224) * cb, t(128) + t(224) * cr


def _codes(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)   # rint: round half to even


def _i420(Y, U, V):
    n = Y.shape[0]
    return np.concatenate([Y.reshape(n, -1), U.reshape(n, -1), V.reshape(n, -1)], axis=1)


def rgb_to_yuv420(x, matrix="bt709", full_range=False):
    """(n, 3, H, W) float32 -> (n, H * W * 3 / 2) uint8, float32 arithmetic"""
    with np.errstate(invalid="ignore"):
        return _i420(*(_codes(p) for p in _forward(x, matrix, full_range, np.float32)))


def rgb_to_yuv420_f64(x, matrix="bt709", full_range=False):
    """(n, 3, H, W) float32 -> (n, H * W * 3 / 2) float64: the values before rounding and clamping"""
    with np.errstate(invalid="ignore"):
        return _i420(*_forward(x, matrix, full_range, np.float64))


def yuv420_to_rgb(buf, H, W, matrix="bt709", full_range=False):
    """(n, H * W * 3 / 2) uint8 -> (n, 3, H, W) uint8, float32 arithmetic; each chroma sample serves its 2 x 2 block"""
    k = constants(matrix)
    buf = np.asarray(buf, dtype=np.uint8).reshape(-1, frame_bytes(H, W))
    n, HW = buf.shape[0], H * W
    Y = buf[:, :HW].reshape(n, H, W).astype(F)
    up = lambda p: p.reshape(n, H // 2, W // 2).astype(F).repeat(2, axis=1).repeat(2, axis=2)
    U, V = up(buf[:, HW:HW + HW // 4]), up(buf[:, HW + HW // 4:])
    if full_range:
        y, cb, cr = (Y - F(0)) * k["i255"], (U - F(128)) * k["i255"], (V - F(128)) * k["i255"]
    else:
        y, cb, cr = (Y - F(16)) * k["i219"], (U - F(128)) * k["i224"], (V - F(128)) * k["i224"]
    r = y + k["c_r"] * cr
    b = y + k["c_b"] * cb
    g = (y - k["c_gb"] * cb) - k["c_gr"] * cr
    return np.stack([np.rint(_clamp01(p) * F(255)).astype(np.uint8) for p in (r, g, b)], axis=1)


def plane_sse(a, b, H, W):
    """(n, FB) uint8 x 2 -> int64 (n, 3): sums of squared differences of the Y, U and V planes"""
    d = (np.asarray(a, dtype=np.int64) - np.asarray(b, dtype=np.int64)) ** 2
    HW = H * W
    return np.stack([d[:, :HW].sum(1), d[:, HW:HW + HW // 4].sum(1), d[:, HW + HW // 4:].sum(1)], axis=1)


def edge_frames(n, H, W, seed):
    """random frames in [-0.1, 1.1] with values below 0 and above 1, NaN, infinities and exact 0, 1 and 0.5 among them"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.1, 1.1, size=(n, 3, H, W)).astype(np.float32)
    special = np.array([0.0, 1.0, np.nan, -0.25, 1.75, 0.5, np.inf, -np.inf, 1.0, 0.0, np.nan, 1.0], dtype=np.float32)
    flat = x.reshape(-1)
    k = min(flat.size, special.size)
    flat[rng.permutation(flat.size)[:k]] = special[:k]
    return x

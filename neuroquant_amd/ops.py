"""Torch-facing wrappers of the libnqhip C ABI (include/nq_hip.h).

PyTorch is plumbing here: device memory, the current HIP stream and the autograd tape.  All arithmetic on
the hot path runs in the hand-written gfx950 kernels; there is NO CPU / eager fallback -- every op raises if
its tensors are not fp32 HIP tensors or if libnqhip.so is missing.
"""
import collections
import contextlib
import ctypes
import functools
import math
import os
import threading

import torch
from torch.autograd import Function

from . import _lib as L

_QCACHE = {}


def _q(name, *args):
    """Pure shape queries of the library (supported / workspace size / operand size), memoised: ~40 ctypes round trips
    per iteration otherwise.  The two environment switches that change a plan are part of the key (tools/bench_kernels.py
    flips them between launches of one process)."""
    key = (name, args, os.environ.get("NQ_WGRAD3_PC"), os.environ.get("NQ_WGRAD3_SS"))
    v = _QCACHE.get(key)
    if v is None:
        v = _QCACHE[key] = getattr(L.lib(), name)(*args)
    return v

EPI_PLAIN, EPI_PS_GELU, EPI_TANH, EPI_PS, EPI_DGRAD_GELU = (L.EPI_PLAIN, L.EPI_PS_GELU, L.EPI_TANH, L.EPI_PS,
                                                                L.EPI_DGRAD_GELU)
# split {hi | lo} word interchange between the bf16x3 kernels (include/nq_hip.h: NQ_EPI_X_SPLIT / NQ_EPI_Y_SPLIT)
EPI_X_SPLIT, EPI_Y_SPLIT = 0x100, 0x200


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- optional per-launch timing with HIP events on the launch stream (bench.py's roofline object) ----
_PROF = None
_PROF_ON = True


def profile_start():
    global _PROF, _PROF_ON
    _PROF, _PROF_ON = {}, True


def profile_sample(on: bool):
    """Pause / resume recording while a profile is open (bench.py times every N-th step only: each event record is a
    marker packet in the queue, 50 of them per step cost ~4 % throughput)."""
    global _PROF_ON
    _PROF_ON = bool(on)


def profile_stop():
    """-> {key: (launches, total_ms)}; synchronises."""
    global _PROF
    prof, _PROF = _PROF, None
    torch.cuda.synchronize()
    return {k: (len(v), sum(s.elapsed_time(e) for s, e in v)) for k, v in (prof or {}).items()}


def profiling_active():
    """True while per-launch HIP events are being recorded (such steps are launched eagerly, never replayed from a graph)."""
    return _PROF is not None and _PROF_ON


def _timed(key, fn):
    if _PROF is None or not _PROF_ON:
        return fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    _PROF.setdefault(key, []).append((s, e))
    return out


def _dev(t: torch.Tensor, name="tensor") -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"neuroquant_amd: {name} must live on the GPU (no CPU fallback exists)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"neuroquant_amd: {name} must be float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _rows(x: torch.Tensor, scale: torch.Tensor):
    """(rows, row_len, per_row) of the quantiser kernels for tensor x and its delta/zp tensor."""
    if scale.numel() > 1:
        rows = x.shape[0]
        if scale.numel() != rows:
            raise RuntimeError("delta/zero_point must hold one value per output channel or a single value")
        return rows, x.numel() // rows, 1
    return 1, x.numel(), 0


# ------------------------------------------------------------------------------------------ quantisers
def _scale_rows(x: torch.Tensor, channel_wise: bool):
    """(rows, result shape) of a scale init: a row is an output channel of a channel-wise 4-D weight, else the whole tensor
    (reference quantizer.py:127-152)."""
    if channel_wise:
        if x.dim() == 4:
            return x.shape[0], (-1, 1, 1, 1)
        if x.dim() == 1:
            return 1, (-1,)
        raise ValueError
    return 1, ()


def scale_init_max(x: torch.Tensor, n_levels: int, channel_wise: bool):
    """UniformAffineQuantizer.init_quantization_scale 'max' (reference quantizer.py:127-168)."""
    x = _dev(x.detach(), "x")
    rows, shape = _scale_rows(x, channel_wise)
    delta = torch.empty(rows, device=x.device, dtype=torch.float32)
    zp = torch.empty_like(delta)
    L.check(L.lib().nq_scale_init_max(_p(x), rows, x.numel() // rows, n_levels, _p(delta), _p(zp), _stream()), "scale_init")
    return delta.view(shape), zp.view(shape)


SCALE_SEARCH_P = {"mse": 3.5, "l1": 1.0}   # the reference's lp_loss exponent / F.l1_loss (quantizer.py:181, 215)
SCALE_CANDIDATES = 10


def _scale_init_args(what, x, n_levels):
    if isinstance(n_levels, bool) or not isinstance(n_levels, int) or not 2 <= n_levels <= 65536:
        raise ValueError(f"{what}: n_levels must be an int in [2, 65536], got {n_levels!r}")
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.numel() == 0:
        raise ValueError(f"{what}: x is a non-empty (rows, row_len) tensor")
    x = _dev(x.detach(), "x")
    rows, row_len = x.shape
    nbytes = _q("nq_scale_init_ws_bytes", rows, row_len)
    if nbytes <= 0:
        raise ValueError(f"{what}: {rows} rows of {row_len} elements are more than one launch holds")
    return x, rows, row_len, torch.empty((nbytes + 7) // 8, device=x.device, dtype=torch.float64)


def _scale_init_out(what, out, specs, device):
    """out= of the raw scale inits: every buffer is on x's device, contiguous, of the entry's dtype and exact size (the C entry
    writes them unchecked); a None is allowed only where the entry takes NULL."""
    if len(out) != len(specs):
        raise ValueError(f"{what}: out holds {len(specs)} buffers")
    for t, (name, dtype, numel, optional) in zip(out, specs):
        if t is None and optional:
            continue
        if (not isinstance(t, torch.Tensor) or t.device != device or t.dtype != dtype or t.numel() != numel
                or not t.is_contiguous()):
            raise ValueError(f"{what}: out buffer {name} must be a contiguous {dtype} tensor of {numel} elements on {device}")
    return out


def scale_init_search_raw(x, n_levels, p, want_scores=True, out=None):
    """x (rows, row_len) -> delta, zp [float (rows,)], choice [int32 (rows,), -1: no candidate scored below 1e10], scores
    [float64 (rows, 10) or None]: the ten-candidate range search of include/nq_hip.h (nq_scale_init_search), on the device,
    nothing read by the host.  out: (delta, zp, choice, scores) buffers to write instead of fresh ones (checked: device,
    dtype, size, contiguity; scores may be None)."""
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not math.isfinite(p) or p <= 0:
        raise ValueError(f"scale_init_search: p must be a finite positive number, got {p!r}")
    x, rows, row_len, ws = _scale_init_args("scale_init_search", x, n_levels)
    if out is None:
        delta = torch.empty(rows, device=x.device, dtype=torch.float32)
        zp = torch.empty_like(delta)
        choice = torch.empty(rows, device=x.device, dtype=torch.int32)
        scores = torch.empty((rows, SCALE_CANDIDATES), device=x.device, dtype=torch.float64) if want_scores else None
    else:
        delta, zp, choice, scores = _scale_init_out("scale_init_search", out, (
            ("delta", torch.float32, rows, False), ("zp", torch.float32, rows, False), ("choice", torch.int32, rows, False),
            ("scores", torch.float64, rows * SCALE_CANDIDATES, True)), x.device)
    L.check(L.lib().nq_scale_init_search(_p(x), rows, row_len, n_levels, float(p), _p(delta), _p(zp), _p(choice), _p(scores),
                                         _p(ws), _stream()), "scale_init_search")
    return delta, zp, choice, scores


def scale_init_gaussian_raw(x, n_levels, want_stats=True, out=None):
    """x (rows, row_len) -> delta, zp [float (rows,)], stats [float (rows, 2) = {mean, unbiased variance} or None]
    (nq_scale_init_gaussian).  out: (delta, zp, stats) buffers to write instead of fresh ones (checked likewise; stats may be None)."""
    x, rows, row_len, ws = _scale_init_args("scale_init_gaussian", x, n_levels)
    if out is None:
        delta = torch.empty(rows, device=x.device, dtype=torch.float32)
        zp = torch.empty_like(delta)
        stats = torch.empty((rows, 2), device=x.device, dtype=torch.float32) if want_stats else None
    else:
        delta, zp, stats = _scale_init_out("scale_init_gaussian", out, (
            ("delta", torch.float32, rows, False), ("zp", torch.float32, rows, False), ("stats", torch.float32, 2 * rows, True)), x.device)
    L.check(L.lib().nq_scale_init_gaussian(_p(x), rows, row_len, n_levels, _p(delta), _p(zp), _p(stats), _p(ws), _stream()),
            "scale_init_gaussian")
    return delta, zp, stats


def scale_init(x: torch.Tensor, n_levels: int, channel_wise: bool, method: str = "max"):
    """UniformAffineQuantizer.init_quantization_scale for every scale_method the reference implements (quantizer.py:127-225):
    'max' (any name holding it, as the reference tests) is scale_init_max, unchanged; 'mse' / 'l1' search ten clipped ranges
    per row, 'gaussian' takes mean -+ 6 * variance (include/nq_hip.h).  Result shapes as for 'max'.  One host read per call of
    a searched or gaussian init: a row without a finite result (a NaN or Inf in it) is a ValueError that names the row."""
    if not isinstance(method, str):
        raise NotImplementedError(f"scale_method {method!r}")
    if "max" in method:
        return scale_init_max(x, n_levels, channel_wise)
    if method not in SCALE_SEARCH_P and method != "gaussian":
        raise NotImplementedError(f"scale_method {method!r}: the reference implements max, mse, gaussian and l1")
    rows, shape = _scale_rows(x, channel_wise)
    x2 = _dev(x.detach(), "x").view(rows, -1)
    if method == "gaussian":
        delta, zp, _ = scale_init_gaussian_raw(x2, n_levels, want_stats=False)
        bad = ~torch.isfinite(delta)
        if bool(bad.any()):
            raise ValueError(f"scale init 'gaussian': row {int(bad.nonzero()[0])} of {rows} has no finite mean and variance "
                             "(a NaN or Inf in it, or a single element)")
    else:
        delta, zp, choice, _ = scale_init_search_raw(x2, n_levels, SCALE_SEARCH_P[method], want_scores=False)
        if int(choice.min()) < 0:
            raise ValueError(f"scale init {method!r}: row {int((choice < 0).nonzero()[0])} of {rows} has no candidate with a "
                             "score below 1e10 (a NaN or Inf in it)")
    return delta.view(shape), zp.view(shape)


def uaq_forward(x, delta, zp, n_levels, out=None):
    x, delta, zp = _dev(x), _dev(delta), _dev(zp)
    rows, rl, per_row = _rows(x, delta)
    y = torch.empty_like(x) if out is None else out
    L.check(L.lib().nq_uaq_forward(_p(x), _p(delta), _p(zp), _p(y), rows, rl, per_row, n_levels, _stream()), "uaq_forward")
    return y


def uaq_backward(x, gy, delta, zp, n_levels, want_dx=False):
    """d(delta) of the UAQ fake-quant; want_dx -> (d(delta), dx) with dx the straight-through gradient w.r.t. x."""
    x, gy, delta, zp = _dev(x), _dev(gy), _dev(delta), _dev(zp)
    rows, rl, per_row = _rows(x, delta)
    dd = torch.empty_like(delta)
    dx = torch.empty_like(x) if want_dx else None
    L.check(L.lib().nq_uaq_backward(_p(x), _p(gy), _p(delta), _p(zp), _p(dd), _p(dx), rows, rl, per_row, n_levels, _stream()),
            "uaq_backward")
    return (dd, dx) if want_dx else dd


def adaround_init(x, delta_uaq, zp_uaq):
    """-> (delta, zp) after the fp16 round trip, alpha  (reference quantizer.py:264-265, 305-314)."""
    x, d0, z0 = _dev(x.detach()), _dev(delta_uaq.detach()), _dev(zp_uaq.detach())
    rows, rl, per_row = _rows(x, d0)
    d, z, a = torch.empty_like(d0), torch.empty_like(z0), torch.empty_like(x)
    L.check(L.lib().nq_adaround_init(_p(x), _p(d0), _p(z0), _p(d), _p(z), _p(a), rows, rl, per_row, _stream()),
            "adaround_init")
    return d, z, a


def adaround_forward(x, alpha, delta, zp, n_levels, soft, want_xq=False, out=None):
    x, alpha, delta, zp = _dev(x), _dev(alpha), _dev(delta), _dev(zp)
    rows, rl, per_row = _rows(x, delta)
    y = torch.empty_like(x) if out is None else out
    xq = torch.empty_like(x) if want_xq else None
    L.check(L.lib().nq_adaround_forward(_p(x), _p(alpha), _p(delta), _p(zp), _p(y), _p(xq), rows, rl, per_row, n_levels,
                                        1 if soft else 0, _stream()), "adaround_forward")
    return (y, xq) if want_xq else y


def adaround_backward(x, gy, alpha, delta, zp, n_levels, reg_weight=0.0, reg_b=0.0, out=None):
    x, gy, alpha, delta, zp = _dev(x), _dev(gy), _dev(alpha), _dev(delta), _dev(zp)
    rows, rl, per_row = _rows(x, delta)
    da = torch.empty_like(alpha) if out is None else out
    L.check(L.lib().nq_adaround_backward(_p(x), _p(gy), _p(alpha), _p(delta), _p(zp), _p(da), rows, rl, per_row, n_levels,
                                         float(reg_weight), float(reg_b), _stream()), "adaround_backward")
    return da


def round_loss(alpha, b, weight, out=None, accumulate=False):
    alpha = _dev(alpha)
    n = alpha.numel()
    ws = torch.empty(_q("nq_reduce_ws_floats", n), device=alpha.device, dtype=torch.float32)
    if out is None:
        out = torch.zeros((), device=alpha.device, dtype=torch.float32)
    L.check(L.lib().nq_round_loss(_p(alpha), n, float(b), float(weight), _p(ws), _p(out), 1 if accumulate else 0, _stream()),
            "round_loss")
    return out


def adam_step(p, g, m, v, lr, step, beta1=0.9, beta2=0.999, eps=1e-8):
    """One torch.optim.Adam update of tensor p in place (step counts from 1)."""
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    L.check(L.lib().nq_adam_step(_p(p), _p(_dev(g)), _p(m), _p(v), p.numel(), lr / bc1, beta1, beta2, eps, bc2 ** 0.5,
                                 _stream()), "adam_step")


def _ada_segs(items, out_like=None, opt=None, absent=()):
    """items: [(x, gy, alpha, delta, zp, n_levels, reg_weight, soft)] -> (segments, outputs, temporaries).  An AdaSeg array whose
    outputs are freshly allocated in the shape of the input named by out_like ("x" | "alpha" | "delta"); or, given opt, an
    AdaAdamSeg array over opt's moments (updated in place: no outputs, soft is implied).  absent names the inputs the launch
    does not read ("gy", "alpha"): they become null pointers; every other input must be a device tensor.  The temporaries are
    the contiguous device tensors the segments point to: the wrapper's local keeps them alive past its launch call."""
    segs = ((L.AdaSeg if opt is None else L.AdaAdamSeg) * len(items))()
    outs, keep = [], []
    for i, (sg, (x, gy, alpha, delta, zp, n_levels, reg_weight, soft)) in enumerate(zip(segs, items)):
        t = {"x": x, "gy": gy, "alpha": alpha, "delta": delta, "zp": zp}
        t = {name: None if name in absent else _dev(a, name) for name, a in t.items()}
        for name, a in t.items():
            setattr(sg, name, _p(a))
        sg.rows, sg.row_len, sg.per_row = _rows(t["x"], t["delta"])
        sg.n_levels, sg.reg_weight = n_levels, float(reg_weight)
        if opt is None:
            outs.append(torch.empty_like(t[out_like]))
            sg.out, sg.soft = _p(outs[-1]), int(bool(soft))
        else:
            sg.m, sg.v = _p(opt.m[i]), _p(opt.v[i])
        keep.append(t)
    return segs, outs, keep


def adaround_forward_multi(items):
    """items: [(x, alpha, delta, zp, n_levels, soft)] -> [fake-quantised tensors], ONE launch for all of them
    (same arithmetic as adaround_forward, bit for bit)."""
    segs, outs, keep = _ada_segs([(x, None, alpha, delta, zp, n_levels, 0.0, soft)
                                  for x, alpha, delta, zp, n_levels, soft in items], "x", absent=("gy",))
    L.check(L.lib().nq_adaround_forward_multi(segs, len(items), _stream()), "adaround_forward_multi")
    return outs


def uaq_forward_multi(items):
    """items: [(x, delta, zp, n_levels)] -> [UAQ fake-quantised tensors], ONE launch (same arithmetic as uaq_forward)."""
    segs, outs, keep = _ada_segs([(x, None, None, delta, zp, n_levels, 0.0, 0) for x, delta, zp, n_levels in items], "x",
                                 absent=("gy", "alpha"))
    L.check(L.lib().nq_uaq_forward_multi(segs, len(items), _stream()), "uaq_forward_multi")
    return outs


def uaq_backward_multi(items):
    """items: [(x, gy, delta, zp, n_levels)] -> [d(delta)], ONE launch (same arithmetic and summation order as uaq_backward)."""
    segs, outs, keep = _ada_segs([(x, gy, None, delta, zp, n_levels, 0.0, 0) for x, gy, delta, zp, n_levels in items], "delta",
                                 absent=("alpha",))
    L.check(L.lib().nq_uaq_backward_multi(segs, len(items), _stream()), "uaq_backward_multi")
    return outs


def step_prologue(order_tab, scal_tab, step_ctr, cur_idx, cur_scal):
    """nq_step_prologue: cur_idx <- order_tab[*step], cur_scal <- scal_tab[*step], *step += 1 (captured iterations)."""
    L.check(L.lib().nq_step_prologue(_p(order_tab), _p(scal_tab), _p(step_ctr), _p(cur_idx), _p(cur_scal), cur_idx.numel(),
                                     cur_scal.numel(), _stream()), "step_prologue")


def step_prologue_gather(order_tab, scal_tab, step_ctr, cur_idx, cur_scal, table, out):
    """nq_step_prologue_gather: step_prologue + out <- table[order_tab[*step]] in ONE launch (step_ctr: two int32 {counter,
    ticket}, both zero at the start of an epoch)."""
    table = _dev(table)
    if step_ctr.numel() < 2 or out.shape[0] != cur_idx.numel() or out[0].numel() != table[0].numel() or not out.is_contiguous():
        raise RuntimeError("step_prologue_gather: step_ctr needs two ints, out must be (B,) + table.shape[1:], contiguous")
    L.check(L.lib().nq_step_prologue_gather(_p(order_tab), _p(scal_tab), _p(step_ctr), _p(cur_idx), _p(cur_scal), cur_idx.numel(),
                                            cur_scal.numel(), _p(table), table.shape[0], table[0].numel(), _p(out), _stream()),
            "step_prologue_gather")


def adaround_backward_multi(items, reg_b=0.0, dyn=None):
    """items: [(x, gy, alpha, delta, zp, n_levels, reg_weight)] -> [d(alpha)] (+ regulariser gradient where
    reg_weight != 0), ONE launch.  dyn (device floats {reg_b, gate, ...} of the current step) replaces the host reg_b and
    gates reg_weight (captured iterations; same arithmetic)."""
    segs, outs, keep = _ada_segs([tuple(it) + (1,) for it in items], "alpha")
    if dyn is not None:
        L.check(L.lib().nq_adaround_backward_multi_dyn(segs, len(items), _p(dyn), _stream()), "adaround_backward_multi_dyn")
    else:
        L.check(L.lib().nq_adaround_backward_multi(segs, len(items), float(reg_b), _stream()), "adaround_backward_multi")
    return outs


def adaround_adam_multi(items, opt, reg_b=0.0, dyn=None, beta1=0.9, beta2=0.999, eps=1e-8):
    """items: [(x, gy, alpha, delta, zp, n_levels, reg_weight)] in the order of opt.params (= the alphas): d(alpha) (+ the
    regulariser gradient) and opt's Adam step in ONE launch; advances opt.t.  Bit-identical to adaround_backward_multi
    followed by opt.step (tested); d(alpha) itself is not materialised."""
    assert len(items) == len(opt.params)
    opt.t += 1
    segs, _, keep = _ada_segs([tuple(it) + (1,) for it in items], opt=opt)
    if any(t["alpha"].data_ptr() != p.data_ptr() for t, p in zip(keep, opt.params)):
        raise RuntimeError("adaround_adam_multi: items must be in the optimiser's parameter order")
    step_size, bc2_sqrt = opt.scalars(opt.t, beta1, beta2)
    L.check(L.lib().nq_adaround_adam_multi(segs, len(items), float(reg_b), step_size, beta1, beta2, eps, bc2_sqrt, _p(dyn),
                                           _stream()), "adaround_adam_multi")


class FusedAdam:
    """torch.optim.Adam(params, lr) with default betas/eps; all tensors updated by ONE nq_adam_step_multi launch."""

    def __init__(self, params, lr):
        self.params = [p for p in params]
        self.lr = lr
        self.t = 0
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    def scalars(self, t, beta1=0.9, beta2=0.999):
        """(lr/(1-beta1^t), sqrt(1-beta2^t)) of step t, as the eager path passes them (host doubles -> fp32)."""
        return self.lr / (1 - beta1 ** t), (1 - beta2 ** t) ** 0.5

    def step(self, grads=None, beta1=0.9, beta2=0.999, eps=1e-8, dyn=None):
        """dyn: device floats whose [2], [3] hold scalars(t) of this step (captured iterations)."""
        self.t += 1
        todo = [(p, (p.grad if grads is None else grads[i]), self.m[i], self.v[i]) for i, p in enumerate(self.params)]
        todo = [t for t in todo if t[1] is not None]
        if not todo:
            return
        segs = (L.AdamSeg * len(todo))()
        keep = []
        for sg, (p, g, m, v) in zip(segs, todo):
            g = _dev(g).contiguous()
            keep.append(g)
            sg.p, sg.g, sg.m, sg.v, sg.n = _p(p.data), _p(g), _p(m), _p(v), p.numel()
        if dyn is not None:
            L.check(L.lib().nq_adam_step_multi_dyn(segs, len(todo), _p(dyn), beta1, beta2, eps, _stream()), "adam_step_multi_dyn")
            return
        bc1, bc2 = 1 - beta1 ** self.t, 1 - beta2 ** self.t
        L.check(L.lib().nq_adam_step_multi(segs, len(todo), self.lr / bc1, beta1, beta2, eps, bc2 ** 0.5, _stream()),
                "adam_step_multi")


# ---- rate-aware calibration: the entropy cost of the stored levels (include/nq_hip.h: nq_level_rate) ----
LEVEL_RATE_LAUNCHES = 4        # kernel launches of one nq_level_rate call per 16 tensors: histogram, finish, rate pass, sum
level_rate_launches = 0        # ops.level_rate_raw calls issued (or captured) by this process: the default paths issue none
LevelRate = collections.namedtuple("LevelRate", "counts cost rate total")


def level_rate_args(what, scale, n_levels=()):
    """ValueError unless scale is a finite number >= 0 and every n_levels lies in 4 .. 256 -> float(scale)."""
    try:
        s = float(scale)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: scale must be a number, got {scale!r}")
    if not math.isfinite(s) or s < 0.0:
        raise ValueError(f"{what}: scale must be finite and >= 0, got {scale!r}")
    for k in n_levels:
        if not isinstance(k, int) or not 4 <= k <= 256:
            raise ValueError(f"{what}: n_levels must be an int in 4 .. 256, got {k!r}")
    return s


def level_rate_raw(items, scale, dyn=None, dalphas=None):
    """items: [(x, alpha, delta, zp, n_levels)], the weight tensors of a decoder with their rounding variables -> LevelRate(counts
    [int32 (n_levels,)], cost [float (n_levels,)], rate (tensors, 2) = {R_soft, R_hard} bits per tensor, total (2,) = their sums
    in list order), all on the device, nothing read by the host (nq_level_rate; the definition is in include/nq_hip.h).  dalphas
    (a list of contiguous float tensors shaped like the alphas, entries may be None) receive += gate * scale * (cost[hi] -
    cost[lo]) * h' in place; dyn (the device slots of the current step) supplies the gate, else 1.  Four launches per 16
    tensors.  ValueError for a bad scale, level count or list before any launch; RuntimeError for CPU tensors."""
    global level_rate_launches
    items = list(items)
    if not items:
        raise ValueError("level_rate: no tensors")
    if any(len(it) != 5 for it in items):
        raise ValueError("level_rate: items are (x, alpha, delta, zp, n_levels)")
    scale = level_rate_args("level_rate", scale, [it[4] for it in items])
    if dalphas is not None and len(dalphas) != len(items):
        raise ValueError(f"level_rate: {len(dalphas)} d(alpha) tensors for {len(items)} items")
    segs = (L.RateSeg * len(items))()
    keep, words, ks = [], 0, []
    for i, (sg, (x, alpha, delta, zp, n_levels)) in enumerate(zip(segs, items)):
        x, alpha, delta, zp = _dev(x, "x"), _dev(alpha, "alpha"), _dev(delta, "delta"), _dev(zp, "zp")
        if alpha.numel() != x.numel():
            raise ValueError("level_rate: alpha must have the shape of x")
        da = None if dalphas is None else dalphas[i]
        if da is not None:
            _dev(da, "d(alpha)")
            if not da.is_contiguous() or da.numel() != x.numel():
                raise ValueError("level_rate: d(alpha) must be contiguous and shaped like alpha (it is updated in place)")
        sg.rows, sg.row_len, sg.per_row = _rows(x, delta)
        sg.n_levels = n_levels
        if zp.numel() != delta.numel():
            raise ValueError("level_rate: delta and zero_point must have the same size")
        keep.append((x, alpha, delta, zp, da))
        ks.append(n_levels)
        words += _q("nq_level_rate_ws_words", x.numel(), n_levels)
    dev = keep[0][0].device
    if dyn is not None:
        dyn = _dev(dyn, "dyn")
        if dyn.numel() < 2:
            raise ValueError("level_rate: dyn holds {reg_b, gate, ...}")
    counts = torch.empty(sum(ks), device=dev, dtype=torch.int32)
    cost = torch.empty(sum(ks), device=dev, dtype=torch.float32)
    rate = torch.empty((len(items), 2), device=dev, dtype=torch.float32)
    total = torch.empty(2, device=dev, dtype=torch.float32)
    ws = torch.empty(words, device=dev, dtype=torch.int32)
    counts_l, cost_l = list(counts.split(ks)), list(cost.split(ks))
    for i, (sg, (x, alpha, delta, zp, da)) in enumerate(zip(segs, keep)):
        sg.x, sg.alpha, sg.delta, sg.zp, sg.dalpha = _p(x), _p(alpha), _p(delta), _p(zp), _p(da)
        sg.counts, sg.cost, sg.rate = _p(counts_l[i]), _p(cost_l[i]), _p(rate[i])
    level_rate_launches += 1
    _timed("level_rate", lambda: L.check(L.lib().nq_level_rate(segs, len(items), scale, _p(dyn), _p(total), _p(ws), words, _stream()),
                                         "level_rate"))
    return LevelRate(counts_l, cost_l, rate, total)


def level_rate(items, weight, pixels, dyn=None, dalphas=None):
    """The rate term of a calibration iteration: level_rate_raw with scale = weight / pixels (lambda * bits per pixel of the
    clip: pixels = frames * H * W), the gradient added to dalphas in place."""
    if not isinstance(pixels, int) or pixels <= 0:
        raise ValueError(f"level_rate: pixels must be a positive int, got {pixels!r}")
    weight = level_rate_args("level_rate", weight)
    return level_rate_raw(items, weight / pixels, dyn=dyn, dalphas=dalphas)


class _UAQFn(Function):
    @staticmethod
    def forward(ctx, x, delta, zp, n_levels):
        ctx.save_for_backward(x, delta, zp)
        ctx.n_levels = n_levels
        return uaq_forward(x, delta, zp, n_levels)

    @staticmethod
    def backward(ctx, gy):
        x, delta, zp = ctx.saved_tensors
        # round_ste (quantizer.py:53-57): d/dx = gy inside the clamp range.  Only computed when somebody asks for it (a
        # trainable quantiser input); the calibration engine never does -- the FP weight is not optimised
        if ctx.needs_input_grad[0]:
            dd, dx = uaq_backward(x, gy, delta, zp, ctx.n_levels, want_dx=True)
            return dx, dd.view_as(delta), None, None
        return None, uaq_backward(x, gy, delta, zp, ctx.n_levels).view_as(delta), None, None


class _AdaRoundFn(Function):
    @staticmethod
    def forward(ctx, x, alpha, delta, zp, n_levels, soft):
        y, xq = adaround_forward(x, alpha, delta, zp, n_levels, soft, want_xq=True)
        ctx.save_for_backward(x, alpha, delta, zp)
        ctx.n_levels, ctx.soft = n_levels, soft
        ctx.mark_non_differentiable(xq)
        return y, xq

    @staticmethod
    def backward(ctx, gy, _gxq):
        x, alpha, delta, zp = ctx.saved_tensors
        # x enters through floor(x/delta) (quantizer.py:290), whose gradient is zero: None IS the reference's gradient
        # for x.  d(delta) exists in the reference's graph but no optimiser ever steps it in phase 2 (calib_model.py:
        # 186-195 collects alpha only); it is not computed here -- ask loudly rather than return silent zeros
        if ctx.needs_input_grad[2] and os.environ.get("NQ_STRICT_GRADS"):
            raise NotImplementedError("d(delta) of the AdaRound fake-quant is not built (never stepped by the reference)")
        da = adaround_backward(x, gy, alpha, delta, zp, ctx.n_levels) if ctx.soft else None
        return None, da, None, None, None, None


class _RoundLossFn(Function):
    @staticmethod
    def forward(ctx, alpha, b, weight):
        ctx.save_for_backward(alpha)
        ctx.b, ctx.weight = float(b), float(weight)
        return round_loss(alpha, b, weight)

    @staticmethod
    def backward(ctx, g):
        (alpha,) = ctx.saved_tensors
        da = torch.empty_like(alpha)
        L.check(L.lib().nq_round_loss_backward(_p(alpha), alpha.numel(), ctx.b, ctx.weight, _p(_dev(g)), _p(da), 0, _stream()),
                "round_loss_backward")
        return da, None, None


def uaq_fake_quant(x, delta, zp, n_levels):
    return _UAQFn.apply(x, delta, zp, n_levels)


def adaround_fake_quant(x, alpha, delta, zp, n_levels, soft):
    return _AdaRoundFn.apply(x, alpha, delta, zp, n_levels, soft)


def round_regulariser(alpha, b, weight):
    return _RoundLossFn.apply(alpha, b, weight)


# ------------------------------------------------------------------------------------------ Hadamard
def next_pow2(n: int) -> int:
    return 1 if n == 0 else 2 ** math.ceil(math.log2(n))


def fwht_channels(w: torch.Tensor, n: int, n_out: int) -> torch.Tensor:
    """WHT of length n along dim 1 of (C_out, C, KH, KW): input zero-padded from C to n, first n_out kept."""
    w = _dev(w)
    co, c, kh, kw = w.shape
    y = torch.empty((co, n_out, kh, kw), device=w.device, dtype=torch.float32)
    L.check(L.lib().nq_fwht(_p(w), _p(y), co, n, kh * kw, c, n_out, _stream()), "fwht")
    return y


def fwht_channels_multi(items):
    """items: [(w, n, n_out)] -> [fwht_channels(w, n, n_out)], ONE launch for all tensors (bit-identical results)."""
    segs = (L.FwhtSeg * len(items))()
    outs = []
    for sg, (w, n, n_out) in zip(segs, items):
        w = _dev(w)
        co, c, kh, kw = w.shape
        y = torch.empty((co, n_out, kh, kw), device=w.device, dtype=torch.float32)
        sg.x, sg.y, sg.outer, sg.inner, sg.n, sg.n_in, sg.n_out = _p(w), _p(y), co, kh * kw, n, c, n_out
        outs.append(y)
    if items:
        L.check(L.lib().nq_fwht_multi(segs, len(items), _stream()), "fwht_multi")
    return outs


def _fq_fwht_segs(items, bwd):
    """items: [(x, alpha, delta, zp, n_levels, soft, n, c_in, reg_weight, gy, m, v)] -> (FqFwhtSeg array, outputs, keep-alive).
    n == 0: a plain tensor (bias); else x / alpha are (C_out, n, kh, kw) and the spatial side is (C_out, c_in, kh, kw)."""
    segs = (L.FqFwhtSeg * len(items))()
    outs, keep = [], []
    for sg, (x, alpha, delta, zp, n_levels, soft, n, c_in, reg_weight, gy, m, v) in zip(segs, items):
        x, alpha, delta, zp = _dev(x), _dev(alpha), _dev(delta), _dev(zp)
        sg.x, sg.alpha, sg.delta, sg.zp = _p(x), _p(alpha), _p(delta), _p(zp)
        sg.n_levels, sg.soft, sg.reg_weight = n_levels, int(bool(soft)), float(reg_weight)
        if n:
            co, npad, kh, kw = x.shape
            if npad != n or delta.numel() not in (1, co):
                raise RuntimeError("fused fake-quant + FWHT: x must be (C_out, n, kh, kw) with per-channel or scalar delta")
            sg.outer, sg.inner, sg.n, sg.c_in, sg.per_row = co, kh * kw, n, c_in, int(delta.numel() > 1)
            spatial = (co, c_in, kh, kw)
        else:
            if delta.numel() != 1:
                raise RuntimeError("fused fake-quant + FWHT: a plain tensor takes one scalar delta / zero point")
            sg.outer, sg.inner, sg.n, sg.c_in, sg.per_row = x.numel(), 1, 0, 0, 0
            spatial = tuple(x.shape)
        if bwd:
            gy = _dev(gy)
            if tuple(gy.shape) != spatial:
                raise RuntimeError(f"fused FWHT + d(alpha) + Adam: gradient shape {tuple(gy.shape)} != {spatial}")
            sg.gy, sg.m, sg.v = _p(gy), _p(m), _p(v)
            keep.append((x, gy))
        else:
            y = torch.empty(spatial, device=x.device, dtype=torch.float32)
            sg.y = _p(y)
            outs.append(y)
            keep.append(x)
    return segs, outs, keep


def adaround_fwht_multi(items):
    """items: [(x, alpha, delta, zp, n_levels, soft, n, c_in)] -> [H(Q(x))[:, :c_in]] (n == 0: Q(x) of a bias), ONE launch
    (nq_adaround_fwht_multi): bit-identical to adaround_forward_multi followed by fwht_channels_multi."""
    segs, outs, keep = _fq_fwht_segs([it + (0.0, None, None, None) for it in items], bwd=False)
    L.check(L.lib().nq_adaround_fwht_multi(segs, len(items), _stream()), "adaround_fwht_multi")
    return outs


def fwht_adaround_adam_multi(items, opt, reg_b=0.0, dyn=None, beta1=0.9, beta2=0.999, eps=1e-8):
    """items: [(x, gy, alpha, delta, zp, n_levels, reg_weight, n, c_in)] in the order of opt.params (= the alphas); gy is the
    SPATIAL-domain gradient d(loss)/d(W^) (C_out, c_in, kh, kw) (n == 0: the bias gradient).  H on the zero-padded gradient,
    d(alpha) (+ regulariser gradient) and opt's Adam step in ONE launch; advances opt.t.  Bit-identical to
    fwht_channels_multi + adaround_adam_multi."""
    assert len(items) == len(opt.params)
    opt.t += 1
    full = []
    for i, (x, gy, alpha, delta, zp, n_levels, reg_weight, n, c_in) in enumerate(items):
        if alpha.data_ptr() != opt.params[i].data_ptr():
            raise RuntimeError("fwht_adaround_adam_multi: items must be in the optimiser's parameter order")
        full.append((x, alpha, delta, zp, n_levels, True, n, c_in, reg_weight, gy, opt.m[i], opt.v[i]))
    segs, _, keep = _fq_fwht_segs(full, bwd=True)
    step_size, bc2_sqrt = opt.scalars(opt.t, beta1, beta2)
    L.check(L.lib().nq_fwht_adaround_adam_multi(segs, len(items), float(reg_b), step_size, beta1, beta2, eps, bc2_sqrt, _p(dyn),
                                                _stream()), "fwht_adaround_adam_multi")


def fq_fwht_fusable(n, inner):
    """rows short enough for the fused launches' LDS tile (every layer of the shipped models: n <= 256, 3 x 3 kernels)"""
    return n * inner <= 8192 and n <= 1024


class _HadamardFn(Function):
    @staticmethod
    def forward(ctx, w, n, n_out):
        ctx.n, ctx.c_in = n, w.shape[1]
        return fwht_channels(w, n, n_out)

    @staticmethod
    def backward(ctx, g):
        return fwht_channels(g, ctx.n, ctx.c_in), None, None


def hadamard_along_channel_weight(x: torch.Tensor, n_out=None) -> torch.Tensor:
    """reference quant_layer.py:16-22 (differentiable; n_out folds the [:, :C] slice of :71 into the store)."""
    n = next_pow2(x.shape[1])
    if n != x.shape[1] and n_out is None:
        raise ValueError("channel count must be a power of two (pad first, quant_layer.py:45-49)")
    return _HadamardFn.apply(x, n, x.shape[1] if n_out is None else n_out)


def hadamard_weight_of(w: torch.Tensor) -> torch.Tensor:
    """zero-pad C_in to 2^k, then transform (reference quant_layer.py:45-49)."""
    n = next_pow2(w.shape[1])
    return fwht_channels(w.detach(), n, n)


# ------------------------------------------------------------------------------------------ convolution
@functools.lru_cache(maxsize=None)
def conv_operand_dims(cin, cout, k):
    kr, ld = ctypes.c_int(0), ctypes.c_int(0)
    L.check(L.lib().nq_conv_operand_dims(cin, cout, k, ctypes.byref(kr), ctypes.byref(ld)), "conv_operand_dims")
    return kr.value, ld.value


def _wl_segs(items):
    """items: [(w, need_fwd, need_bwd)] -> (WLSeg array, [(wt_fwd | None, dims_fwd, wt_bwd | None, dims_bwd)], temporaries): the
    fp32 GEMM operand buffers of OIHW weights, allocated, and the segments that fill them.  The temporaries (the contiguous
    weights the segments point to) stay alive in the wrapper's local past its launch call."""
    segs = (L.WLSeg * len(items))()
    outs, keep = [], []
    for sg, (w, need_fwd, need_bwd) in zip(segs, items):
        w = _dev(w)
        cout, cin, k, _ = w.shape
        wt = wb = None
        kf = lf = kb = lb = 0
        if need_fwd:
            kf, lf = conv_operand_dims(cin, cout, k)
            wt = torch.empty(kf * lf, device=w.device, dtype=torch.float32)
        if need_bwd:
            kb, lb = conv_operand_dims(cout, cin, k)
            wb = torch.empty(kb * lb, device=w.device, dtype=torch.float32)
        sg.w, sg.wt_fwd, sg.wt_bwd, sg.Cout, sg.Cin, sg.k = _p(w), _p(wt), _p(wb), cout, cin, k
        sg.krows_fwd, sg.ld_fwd, sg.krows_bwd, sg.ld_bwd = kf, lf, kb, lb
        outs.append((wt, (kf, lf), wb, (kb, lb)))
        keep.append(w)
    return segs, outs, keep


def _wl3_segs(items):
    """items: [(w, transposed)] -> (WL3Seg array, [operand buffers], temporaries): as _wl_segs for the pre-split (bf16 hi / lo)
    operands of the bf16x3 kernels; transposed -> operand of the data gradient."""
    segs = (L.WL3Seg * len(items))()
    outs, keep = [], []
    for sg, (w, transposed) in zip(segs, items):
        w = _dev(w)
        cw_out, cw_in, k, _ = w.shape
        cin, cout = (cw_out, cw_in) if transposed else (cw_in, cw_out)
        outs.append(torch.empty(_q("nq_conv3_weight_bytes", cin, cout, k), device=w.device, dtype=torch.uint8))
        sg.w, sg.wt3, sg.Cin, sg.Cout, sg.k, sg.transposed = _p(w), _p(outs[-1]), cin, cout, k, int(bool(transposed))
        keep.append(w)
    return segs, outs, keep


def weight_layouts(w, need_bwd):
    """-> (wt_fwd, dims_fwd, wt_bwd | None, dims_bwd | None) GEMM operands of an OIHW weight."""
    (sg,), (out,), (w,) = _wl_segs([(w, True, need_bwd)])
    L.check(L.lib().nq_weight_layouts(_p(w), _p(out[0]), _p(out[2]), sg.Cout, sg.Cin, sg.k, sg.krows_fwd, sg.ld_fwd, sg.krows_bwd,
                                      sg.ld_bwd, _stream()), "weight_layouts")
    return out


def weight_layouts_multi(items):
    """items: [(w, need_fwd, need_bwd)] -> [(wt_fwd | None, dims_fwd, wt_bwd | None, dims_bwd)] as weight_layouts, ONE launch."""
    segs, outs, keep = _wl_segs(items)
    if items:
        L.check(L.lib().nq_weight_layouts_multi(segs, len(items), _stream()), "weight_layouts_multi")
    return outs


def weight_layouts_all(items3, items_f):
    """weight_layout3_multi(items3) and weight_layouts_multi(items_f) in ONE launch (nq_weight_layouts_all; same bytes)."""
    if not items3 or not items_f or os.environ.get("NQ_LAYOUTS_ALL", "1") == "0":
        return weight_layout3_multi(items3), weight_layouts_multi(items_f)
    segs3, outs3, keep3 = _wl3_segs(items3)
    segsf, outsf, keepf = _wl_segs(items_f)
    L.check(L.lib().nq_weight_layouts_all(segs3, len(items3), segsf, len(items_f), _stream()), "weight_layouts_all")
    return outs3, outsf


def _conv_outputs(x, cout, epilogue, r):
    """(y, z) of a convolution launch on x with this epilogue, allocated: z = shuffled pre-activation of the PixelShuffle
    epilogues (y is None for EPI_PS), y = un-shuffled gradient for EPI_DGRAD_GELU."""
    B, _, H, W = x.shape
    y = z = None
    if epilogue in (EPI_PS_GELU, EPI_PS):
        z = torch.empty((B, cout // (r * r), H * r, W * r), device=x.device, dtype=torch.float32)
        if epilogue == EPI_PS_GELU:
            y = torch.empty_like(z)
    elif epilogue == EPI_DGRAD_GELU:
        y = torch.empty((B, cout * r * r, H // r, W // r), device=x.device, dtype=torch.float32)
    else:
        y = torch.empty((B, cout, H, W), device=x.device, dtype=torch.float32)
    return y, z


def conv_forward_raw(x, wt, dims, bias, cout, k, epilogue, r, zprev=None, fmt=0):
    """One nq_conv_forward launch.  Returns (y, z) as _conv_outputs describes them.  fmt = EPI_Y_SPLIT: y as split {hi | lo}
    words (conv_split_out says where)."""
    B, cin, H, W = x.shape
    y, z = _conv_outputs(x, cout, epilogue, r)
    nws = _q("nq_conv_forward_ws_floats", B, cin, H, W, cout, k)
    ws = torch.empty(nws, device=x.device, dtype=torch.float32) if nws else None
    _timed(("conv_igemm", k, cin, cout, H, W, B, epilogue),
           lambda: L.check(L.lib().nq_conv_forward(_p(x), _p(wt), _p(bias), _p(y), _p(z), _p(ws), B, cin, H, W, cout, k,
                                                   dims[0], dims[1], r, epilogue | fmt, _p(zprev), _stream()), "conv_forward"))
    return y, z


def conv3_supported(B, cin, H, W, cout, k):
    return bool(_q("nq_conv3_supported", B, cin, H, W, cout, k))


def conv3_split_io(B, cin, H, W, cout, k):
    """EPI_X_SPLIT | EPI_Y_SPLIT bits: the sides of conv3_forward_raw that may travel as split {hi | lo} words for this shape"""
    return int(_q("nq_conv3_split_io", B, cin, H, W, cout, k))


def conv_wgrad3_split_io(B, cin, H, W, cout, k):
    """bit 0: x, bit 1: dy of conv_wgrad3_raw may be split words for this shape"""
    return int(_q("nq_conv_wgrad3_split_io", B, cin, H, W, cout, k))


def conv_split_out(B, cin, H, W, cout, k, r, epilogue, has_bias=False):
    """True when conv_forward_raw can write y as split words for this call (the streaming head data gradient)"""
    return bool(_q("nq_conv_split_out", B, cin, H, W, cout, k, r, epilogue, 1 if has_bias else 0))


def split_words(x):
    """float tensor -> the same shape holding split {hi | lo} words (bit patterns in a float32 tensor)"""
    x = _dev(x).contiguous()
    y = torch.empty_like(x)
    L.check(L.lib().nq_split_words(_p(x), _p(y), x.numel(), _stream()), "split_words")
    return y


def weight_layout3(w, transposed=False, dtype="bf16"):
    """pre-split (bf16 hi/lo) operand of the bf16x3 conv kernels; transposed=True -> operand of the data gradient.
    dtype='f16' (forward operand only): the same layout and size, the hi plane as IEEE halves, the lo plane zero."""
    (sg,), (buf,), (w,) = _wl3_segs([(w, transposed)])
    if dtype == "f16":
        if transposed:
            raise ValueError("weight_layout3: dtype='f16' builds forward operands only")
        L.check(L.lib().nq_weight_layout3_f16(_p(w), _p(buf), sg.Cin, sg.Cout, sg.k, _stream()), "weight_layout3_f16")
    else:
        L.check(L.lib().nq_weight_layout3(_p(w), _p(buf), sg.Cin, sg.Cout, sg.k, sg.transposed, _stream()), "weight_layout3")
    return buf


def weight_layout3_multi(items):
    """items: [(w, transposed)] -> [operand buffers], ONE launch (same bytes as weight_layout3 per item)."""
    segs, outs, keep = _wl3_segs(items)
    if items:
        L.check(L.lib().nq_weight_layout3_multi(segs, len(items), _stream()), "weight_layout3_multi")
    return outs


def conv3_forward_raw(x, wt3, bias, cout, k, epilogue, r, zprev=None, fmt=0):
    """bf16x3 counterpart of conv_forward_raw (same outputs).  fmt: EPI_X_SPLIT (x holds split words) | EPI_Y_SPLIT (y is
    written as split words), where conv3_split_io allows."""
    B, cin, H, W = x.shape
    y, z = _conv_outputs(x, cout, epilogue, r)
    nws = _q("nq_conv_forward3_ws_floats", B, cin, H, W, cout, k)
    ws = torch.empty(nws, device=x.device, dtype=torch.float32) if nws else None
    _timed(("conv_igemm3", k, cin, cout, H, W, B, epilogue),
           lambda: L.check(L.lib().nq_conv_forward3(_p(x), _p(wt3), _p(bias), _p(y), _p(z), _p(zprev), _p(ws), B, cin, H, W,
                                                    cout, k, r, epilogue | fmt, _stream()), "conv_forward3"))
    return y, z


def conv3_levels_supported(B, cin, H, W, cout, k):
    """True where conv3_forward_levels_raw serves the shape: the unsplit tiled bf16x3 kernel has it (nq_conv_forward3_plan)."""
    return bool(_q("nq_conv3_levels_supported", B, cin, H, W, cout, k))


def levels_representable(n):
    """True when every entry of the float tensor n is an integer of magnitude <= 256 that bf16 holds exactly
    (n == n.bfloat16().float()): what level - zero_point of a quantiser of up to 8 bits with an integer zero point gives.
    Checked on the device; one synchronisation."""
    n = _dev(n.detach(), "n")
    return bool(((n == n.bfloat16().float()) & (n == n.round()) & (n.abs() <= 256)).all())


def levels_operand(n, checked=False, dtype="bf16"):
    """operand of conv3_forward_levels_raw with the same dtype from the OIHW float tensor n = level - zero_point of a stored
    weight: weight_layout3(n, dtype=dtype), whose lo plane is all zeros and never read.  n must satisfy levels_representable
    (bf16 and half both hold such integers exactly): ValueError otherwise; checked=True: the caller has asked already."""
    n = _dev(n.detach(), "n")
    if dtype not in ("bf16", "f16"):
        raise ValueError(f"levels_operand: dtype must be 'bf16' or 'f16', got {dtype!r}")
    if n.dim() != 4 or n.shape[2] != n.shape[3] or n.shape[2] not in (3, 5):
        raise ValueError(f"levels_operand takes an OIHW float32 tensor with k = 3 or 5, got {tuple(n.shape)}")
    if not checked and not levels_representable(n):
        raise ValueError("levels_operand: every entry must be an integer of magnitude <= 256 that bf16 holds exactly "
                         "(level - zero_point of an integer zero point)")
    return weight_layout3(n.contiguous(), dtype=dtype)


def _levels_scale(scale, cout, who):
    scale = _dev(scale, "scale")
    if scale.numel() != cout or scale.dtype != torch.float32 or not scale.is_contiguous():
        raise ValueError(f"{who}: scale must hold one float32 per output channel ({cout}), got {tuple(scale.shape)}")
    return scale


def conv3_forward_levels_raw(x, wt, scale, bias, cout, k, epilogue, r, dtype="bf16", sat_flag=None):
    """Levels counterpart of conv3_forward_raw: y = scale[co] * conv(x, n) + bias[co] with wt = levels_operand(n, dtype=dtype).
    Forward epilogues only; returns (y, z) as conv3_forward_raw does; serves the shapes of conv3_levels_supported.
    dtype='bf16': two BF16 MFMAs per product (include/nq_hip.h); takes no flag word.
    dtype='f16': conv(f16(x), n), one F16 MFMA per product (an approximation); sat_flag: one int32 on the
    device, the launch stores 1 to it when it clamped a finite |x| > 65504 and never clears it.  No synchronisation here."""
    who = "conv3_forward_levels_raw"
    if dtype not in ("bf16", "f16"):
        raise ValueError(f"{who}: dtype must be 'bf16' or 'f16', got {dtype!r}")
    B, cin, H, W = x.shape
    scale = _levels_scale(scale, cout, who)
    if epilogue == EPI_DGRAD_GELU:
        raise ValueError(f"{who} serves forward epilogues only")
    if dtype == "f16":
        sat_flag = _dev_as(sat_flag, torch.int32, "sat_flag")
        if sat_flag.numel() != 1:
            raise ValueError(f"{who}: sat_flag must be one int32 on the device")
    elif sat_flag is not None:
        raise ValueError(f"{who}: dtype='bf16' takes no sat_flag")
    y, z = _conv_outputs(x, cout, epilogue, r)
    sfx, flag = ("_f16", [_p(sat_flag)]) if dtype == "f16" else ("", [])     # the two entries differ by the flag word alone
    fn = getattr(L.lib(), "nq_conv_forward3_levels" + sfx)
    _timed(("conv_igemm3_levels" + sfx, k, cin, cout, H, W, B, epilogue),
           lambda: L.check(fn(_p(x), _p(wt), _p(scale), _p(bias), _p(y), _p(z), *flag, B, cin, H, W, cout, k, r, epilogue, _stream()),
                           "conv_forward3_levels" + sfx))
    return y, z


def conv3_forward_levels_f16_raw(x, wt, scale, bias, cout, k, epilogue, r, sat_flag):
    """the half launch under its first name, which callers outside this package hold: conv3_forward_levels_raw(dtype='f16')"""
    return conv3_forward_levels_raw(x, wt, scale, bias, cout, k, epilogue, r, "f16", sat_flag)


def conv_wgrad3_supported(B, cin, H, W, cout, k):
    return bool(_q("nq_conv_wgrad3_supported", B, cin, H, W, cout, k))


class PendingReductions:
    """Slab reductions of several weight-gradient launches, performed by ONE nq_wgrad_reduce_multi launch at `flush()`
    (bit-identical to the per-launch reductions; the slabs and outputs stay referenced until then)."""

    def __init__(self):
        self.segs, self.keep = [], []

    def add(self, seg, *tensors):
        self.segs.append(seg)
        self.keep.append(tensors)

    def flush(self):
        if self.segs:
            arr = (L.WgrSeg * len(self.segs))(*self.segs)
            L.check(L.lib().nq_wgrad_reduce_multi(arr, len(self.segs), _stream()), "wgrad_reduce_multi")
        self.segs, self.keep = [], []


def _wgrad_outputs(x, cout, k, want_db, out):
    """(dw, db) of a weight-gradient launch on x: out = (dw, db) pre-allocated contiguous outputs (views of a flat gradient
    arena) or None -> allocated here; db is None unless want_db."""
    dw = torch.empty((cout, x.shape[1], k, k), device=x.device, dtype=torch.float32) if out is None else out[0]
    db = (torch.empty(cout, device=x.device, dtype=torch.float32) if out is None else out[1]) if want_db else None
    return dw, db


def _seg_ref(seg):
    return None if seg is None else ctypes.byref(seg)


def conv_wgrad3_raw(x, dy, cout, k, want_db, out=None, defer=None, fmt=0):
    """bf16x3 counterpart of conv_wgrad_raw (out as _wgrad_outputs takes it).  defer (PendingReductions): only the split
    kernel runs now, dw / db are valid after defer.flush().  fmt bit 0 / 1: x / dy hold split {hi | lo} words
    (conv_wgrad3_split_io)."""
    B, cin, H, W = x.shape
    ws = torch.empty(_q("nq_conv_wgrad3_ws_floats", B, cin, H, W, cout, k), device=x.device, dtype=torch.float32)
    dw, db = _wgrad_outputs(x, cout, k, want_db, out)
    seg = None if defer is None else L.WgrSeg()
    _timed(("conv_wgrad3", k, cin, cout, H, W, B, 0),
           lambda: L.check(L.lib().nq_conv_wgrad3(_p(x), _p(dy), _p(dw), _p(db), _p(ws), B, cin, H, W, cout, k, fmt,
                                                  _seg_ref(seg), _stream()), "conv_wgrad3"))
    if seg is not None:
        defer.add(seg, ws, dw, db)
    return dw, db


def channel_sum(x):
    x = _dev(x)
    B, C = x.shape[0], x.shape[1]
    out = torch.empty(C, device=x.device, dtype=torch.float32)
    ws = torch.empty(512 * C, device=x.device, dtype=torch.float32)
    L.check(L.lib().nq_channel_sum(_p(x), _p(out), _p(ws), B, C, x.numel() // (B * C), _stream()), "channel_sum")
    return out


def conv_wgrad_swapped3_supported(B, cin, H, W, cout, k):
    """True when conv_wgrad_swapped3 serves this (cin -> cout) layer: a head with <= 4 output channels whose exchanged problem
    (cout -> cin) the tiled bf16x3 kernels take (the few-pixel kernel has no exchanged form)."""
    return bool(_q("nq_conv_wgrad3_swapped_supported", B, cin, H, W, cout, k))


def conv_wgrad_swapped3(x, dy, cout, k, want_db, out=None, defer=None):
    """Weight gradient of a conv with very few OUTPUT channels (the 3-channel head) by swapping operand roles:
    R[ci][(co,kh,kw)] = sum_p x[ci][p] * dy[co][p + tap]  is the weight gradient of the conv  dy -> x-channels, and
    dW[co][ci][kh][kw] = R[ci][co][K-1-kh][K-1-kw].  The big tensor (x, 242 MB) is then the un-shifted GEMM operand
    read exactly once, only the 3-channel dy needs halo rows, and the MFMA tile is 37(->48) x 27(->64) instead of
    3(->16) x 333(->384)."""
    B, cin, H, W = x.shape
    ws = torch.empty(_q("nq_conv_wgrad3_swapped_ws_floats", B, cin, H, W, cout, k), device=x.device, dtype=torch.float32)
    dw, _ = _wgrad_outputs(x, cout, k, False, out)
    seg = None if defer is None else L.WgrSeg()
    # the slab reduction writes dW[co][ci][K-1-kh][K-1-kw] directly (no permute / flip / copy passes)
    _timed(("conv_wgrad3", k, cout, cin, H, W, B, 0),
           lambda: L.check(L.lib().nq_conv_wgrad3_swapped(_p(x), _p(dy), _p(dw), _p(ws), B, cin, H, W, cout, k,
                                                          _seg_ref(seg), _stream()), "conv_wgrad3_swapped"))
    if seg is not None:
        defer.add(seg, ws, dw)
    db = None
    if want_db:
        db = channel_sum(dy)
        if out is not None:
            out[1].copy_(db)
            db = out[1]
    return dw, db


def conv_wgrad_raw(x, dy, cout, k, want_db, out=None, defer=None):
    """fp32 weight (and bias) gradient; out / defer as conv_wgrad3_raw."""
    B, cin, H, W = x.shape
    ws = torch.empty(_q("nq_conv_wgrad_ws_floats", B, cin, H, W, cout, k), device=x.device, dtype=torch.float32)
    dw, db = _wgrad_outputs(x, cout, k, want_db, out)
    seg = None if defer is None else L.WgrSeg()
    _timed(("conv_wgrad", k, cin, cout, H, W, B, 0),
           lambda: L.check(L.lib().nq_conv_wgrad(_p(x), _p(dy), _p(dw), _p(db), _p(ws), B, cin, H, W, cout, k,
                                                 _seg_ref(seg), _stream()), "conv_wgrad"))
    if seg is not None:
        defer.add(seg, ws, dw, db)
    return dw, db


class _ConvFn(Function):
    """stride-1 'same' conv (+bias) fused with PixelShuffle+GELU or tanh*0.5+0.5 (reference quant_layer.py:80,
    quant_block.py:31-35, models/_layers.py:10-36)."""

    @staticmethod
    def forward(ctx, x, w, b, epilogue, r):
        x, w = _dev(x, "x"), _dev(w, "weight")
        b = _dev(b, "bias") if b is not None else None
        cout, cin, k, k2 = w.shape
        if k != k2 or x.shape[1] != cin:
            raise ValueError(f"conv shape mismatch: x {tuple(x.shape)} w {tuple(w.shape)}")
        need_dx = ctx.needs_input_grad[0]
        wt, dims, wb, dims_b = weight_layouts(w, need_dx)
        y, z = conv_forward_raw(x, wt, dims, b, cout, k, epilogue, r)
        ctx.save_for_backward(x, wb, z if epilogue == EPI_PS_GELU else (y if epilogue == EPI_TANH else None))
        ctx.meta = (cout, cin, k, epilogue, r, dims_b, b is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, wb, aux = ctx.saved_tensors
        cout, cin, k, epilogue, r, dims_b, has_b = ctx.meta
        B, _, H, W = x.shape
        gy = _dev(gy, "grad")
        if epilogue == EPI_PS_GELU:
            dconv = torch.empty((B, cout, H, W), device=x.device, dtype=torch.float32)
            L.check(L.lib().nq_ps_gelu_backward(_p(gy), _p(aux), _p(dconv), B, cout // (r * r), H, W, r, _stream()),
                    "ps_gelu_backward")
        elif epilogue == EPI_TANH:
            dconv = torch.empty_like(gy)
            L.check(L.lib().nq_tanh_out_backward(_p(gy), _p(aux), _p(dconv), gy.numel(), _stream()), "tanh_backward")
        else:
            dconv = gy
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx, _ = conv_forward_raw(dconv, wb, dims_b, None, cin, k, EPI_PLAIN, 1)
        if ctx.needs_input_grad[1] or (has_b and ctx.needs_input_grad[2]):
            dw, db = conv_wgrad_raw(x, dconv, cout, k, has_b)
        return dx, dw, db, None, None


# ---- twice-differentiable convolution (Hessian-vector products of the Omega bit-allocation criterion) ----
# A stride-1 'same' convolution is bilinear in (x, w), so F = conv(x, w), D = dgrad(gy, w) and Wg = wgrad(x, gy) are
# closed under differentiation:  dF = (D(gy,w), Wg(x,gy));  dD = (F(g,w), Wg(g,gy));  dWg = (D(gy,G), F(x,G)).
# Each is an autograd Function whose backward is built from the other two, so create_graph=True works to any order
# on the same HIP kernels as the calibration loop (bf16x3 where the grid fills the chip, exact fp32 MFMA otherwise).
_PRECISION = None   # set_conv_precision() override; None -> NQ_CONV_PRECISION (default 'bf16x3')


def set_conv_precision(precision):
    """'bf16x3' | 'fp32' | None (= environment NQ_CONV_PRECISION, default 'bf16x3'): which MFMA pipe the large
    convolutions run on from now on.  bench.py / the precision gate switch it between runs of one process."""
    global _PRECISION
    if precision not in (None, "fp32", "bf16x3"):
        raise ValueError(f"unknown conv precision {precision!r}")
    _PRECISION = precision


def get_conv_precision():
    return _PRECISION or os.environ.get("NQ_CONV_PRECISION", "bf16x3")


def _use3(precision):
    return (precision or get_conv_precision()) == "bf16x3"


def _conv_plain(x, w, precision=None):
    cout, cin, k, _ = w.shape
    B, _, H, W = x.shape
    if _use3(precision) and conv3_supported(B, cin, H, W, cout, k):
        return conv3_forward_raw(x, weight_layout3(w), None, cout, k, EPI_PLAIN, 1)[0]
    wt, dims, _, _ = weight_layouts(w, need_bwd=False)
    return conv_forward_raw(x, wt, dims, None, cout, k, EPI_PLAIN, 1)[0]


def _dgrad_plain(gy, w, precision=None):
    cout, cin, k, _ = w.shape
    B, _, H, W = gy.shape
    if _use3(precision) and conv3_supported(B, cout, H, W, cin, k):
        return conv3_forward_raw(gy, weight_layout3(w, transposed=True), None, cin, k, EPI_PLAIN, 1)[0]
    _, _, wb, dims_b = weight_layouts(w, need_bwd=True)
    return conv_forward_raw(gy, wb, dims_b, None, cin, k, EPI_PLAIN, 1)[0]


def _wgrad_plain(x, gy, k, precision=None):
    B, cin, H, W = x.shape
    cout = gy.shape[1]
    if _use3(precision) and conv_wgrad3_supported(B, cin, H, W, cout, k):
        return conv_wgrad3_raw(x, gy, cout, k, False)[0]
    if _use3(precision) and conv_wgrad_swapped3_supported(B, cin, H, W, cout, k):
        return conv_wgrad_swapped3(x, gy, cout, k, False)[0]
    return conv_wgrad_raw(x, gy, cout, k, False)[0]


class _ConvF(Function):
    @staticmethod
    def forward(ctx, x, w):
        x, w = _dev(x, "x").contiguous(), _dev(w, "weight").contiguous()
        ctx.save_for_backward(x, w)
        return _conv_plain(x, w)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = gy.contiguous()
        return (_ConvD.apply(gy, w) if ctx.needs_input_grad[0] else None,
                _ConvWg.apply(x, gy, w.shape[-1]) if ctx.needs_input_grad[1] else None)


class _ConvD(Function):
    @staticmethod
    def forward(ctx, gy, w):
        gy, w = _dev(gy, "gy").contiguous(), _dev(w, "weight").contiguous()
        ctx.save_for_backward(gy, w)
        return _dgrad_plain(gy, w)

    @staticmethod
    def backward(ctx, g):
        gy, w = ctx.saved_tensors
        g = g.contiguous()
        return (_ConvF.apply(g, w) if ctx.needs_input_grad[0] else None,
                _ConvWg.apply(g, gy, w.shape[-1]) if ctx.needs_input_grad[1] else None)


class _ConvWg(Function):
    @staticmethod
    def forward(ctx, x, gy, k):
        x, gy = _dev(x, "x").contiguous(), _dev(gy, "gy").contiguous()
        ctx.save_for_backward(x, gy)
        return _wgrad_plain(x, gy, k)

    @staticmethod
    def backward(ctx, G):
        x, gy = ctx.saved_tensors
        G = G.contiguous()
        return (_ConvD.apply(gy, G) if ctx.needs_input_grad[0] else None,
                _ConvF.apply(x, G) if ctx.needs_input_grad[1] else None, None)


# ---- the elementwise pieces of the decoder, twice differentiable on this repo's own kernels (round 4: they went through
#      ATen before).  Each Function's backward is built from Functions of the same family, so
#      torch.autograd.grad(create_graph=True) followed by .backward() -- the reference's Hessian-vector recipe,
#      methods/bit_assign.py:88-114 -- never leaves libnqhip. ----
_ACT_BASE = {"gelu": 0, "tanh": 3}


def act_dd_raw(x, kind, order, g=None, g2=None):
    """f^(order)(x) * g * g2 (nq_act_dd): kind 'gelu' = exact-erf GELU (nn.GELU(), _layers.py:104-105), 'tanh' = OutImg's
    tanh(x)*0.5+0.5 (_layers.py:10-16); order 0 / 1 / 2 = value, first and second derivative."""
    x = _dev(x, "x")
    g = _dev(g, "g") if g is not None else None
    g2 = _dev(g2, "g2") if g2 is not None else None
    y = torch.empty_like(x)
    L.check(L.lib().nq_act_dd(_p(x), _p(g), _p(g2), _p(y), x.numel(), _ACT_BASE[kind] + order, _stream()), "act_dd")
    return y


class _ActDD(Function):
    """y = f^(order)(x) * g  (g may be None).  d/dx = gy * g * f^(order+1)(x), d/dg = gy * f^(order)(x): the same Function one
    order up / without g, so the graph of a backward pass is itself differentiable (up to the second derivative: the
    Hessian-vector products need no more; a third is refused loudly)."""

    @staticmethod
    def forward(ctx, x, g, kind, order):
        ctx.save_for_backward(x, g)
        ctx.kind, ctx.order = kind, order
        return act_dd_raw(x, kind, order, g)

    @staticmethod
    def backward(ctx, gy):
        x, g = ctx.saved_tensors
        gy = gy.contiguous()
        dx = dg = None
        if ctx.needs_input_grad[0]:
            if ctx.order >= 2:
                raise NotImplementedError("third derivative of the activation is not built (Hessian-vector products need two)")
            dx = _ActDD2.apply(x, gy, g, ctx.kind, ctx.order + 1)
        if g is not None and ctx.needs_input_grad[1]:
            dg = _ActDD.apply(x, gy, ctx.kind, ctx.order)
        return dx, dg, None, None


class _ActDD2(Function):
    """y = f^(order)(x) * g * h (h may be None): the d/dx of _ActDD with its two multipliers kept apart (no elementwise product
    outside the kernel).  Differentiable w.r.t. g and h (what the second backward pass asks for) and, while order < 2, x."""

    @staticmethod
    def forward(ctx, x, g, h, kind, order):
        ctx.save_for_backward(x, g, h)
        ctx.kind, ctx.order = kind, order
        return act_dd_raw(x, kind, order, g, h)

    @staticmethod
    def backward(ctx, gy):
        x, g, h = ctx.saved_tensors
        gy = gy.contiguous()
        dx = dg = dh = None
        if ctx.needs_input_grad[0]:
            if ctx.order >= 2 or h is not None:
                raise NotImplementedError("third derivative of the activation is not built (Hessian-vector products need two)")
            dx = _ActDD2.apply(x, gy, g, ctx.kind, ctx.order + 1)
        if ctx.needs_input_grad[1]:
            dg = _ActDD2.apply(x, gy, h, ctx.kind, ctx.order) if h is not None else _ActDD.apply(x, gy, ctx.kind, ctx.order)
        if h is not None and ctx.needs_input_grad[2]:
            dh = _ActDD2.apply(x, gy, g, ctx.kind, ctx.order)
        return dx, dg, dh, None, None


def gelu_dd(x):
    """exact-erf GELU, twice differentiable (reference nn.GELU(), models/_layers.py:104-105)."""
    return _ActDD.apply(x.contiguous(), None, "gelu", 0)


def tanh_out_dd(x):
    """OutImg: tanh(x) * 0.5 + 0.5, twice differentiable (reference models/_layers.py:10-16)."""
    return _ActDD.apply(x.contiguous(), None, "tanh", 0)


def pixel_shuffle_raw(x, r, inverse=False):
    x = _dev(x, "x")
    B, Cx, Hx, Wx = x.shape
    if inverse:
        if Hx % r or Wx % r:
            raise ValueError("pixel_unshuffle: spatial size not divisible by r")
        C, H, W = Cx, Hx // r, Wx // r
        y = torch.empty((B, C * r * r, H, W), device=x.device, dtype=torch.float32)
    else:
        if Cx % (r * r):
            raise ValueError("pixel_shuffle: channels not divisible by r*r")
        C, H, W = Cx // (r * r), Hx, Wx
        y = torch.empty((B, C, H * r, W * r), device=x.device, dtype=torch.float32)
    L.check(L.lib().nq_pixel_shuffle(_p(x), _p(y), B, C, H, W, r, 1 if inverse else 0, _stream()), "pixel_shuffle")
    return y


class _PixelShuffleDD(Function):
    """PixelShuffle(r) / its inverse: a permutation, so the backward is the inverse permutation of the same family (any order)."""

    @staticmethod
    def forward(ctx, x, r, inverse):
        ctx.r, ctx.inverse = r, inverse
        return pixel_shuffle_raw(x.contiguous(), r, inverse)

    @staticmethod
    def backward(ctx, gy):
        return _PixelShuffleDD.apply(gy.contiguous(), ctx.r, not ctx.inverse), None, None


def pixel_shuffle_dd(x, r):
    """torch.nn.PixelShuffle(r) (reference models/_layers.py:20-36), differentiable to any order."""
    return _PixelShuffleDD.apply(x, r, False)


class _BiasAddDD(Function):
    """y = x + bias[None, :, None, None].  d/dx = gy, d/dbias = channel sums of gy -- a Function whose backward is the
    broadcast again: linear, differentiable to any order."""

    @staticmethod
    def forward(ctx, x, bias):
        x, bias = _dev(x, "x").contiguous(), _dev(bias, "bias").contiguous()
        y = torch.empty_like(x)
        B, C = x.shape[0], x.shape[1]
        L.check(L.lib().nq_bias_add(_p(x), _p(bias), _p(y), B, C, x.numel() // (B * C), _stream()), "bias_add")
        return y

    @staticmethod
    def backward(ctx, gy):
        gy = gy.contiguous()
        return (gy if ctx.needs_input_grad[0] else None), (_ChannelSumDD.apply(gy) if ctx.needs_input_grad[1] else None)


class _ChannelSumDD(Function):
    @staticmethod
    def forward(ctx, x):
        ctx.shape = tuple(x.shape)
        return channel_sum(x.contiguous())

    @staticmethod
    def backward(ctx, g):   # broadcast of g over (B, :, H, W)
        g = _dev(g, "g").contiguous()
        B, C = ctx.shape[0], ctx.shape[1]
        y = torch.empty(ctx.shape, device=g.device, dtype=torch.float32)
        L.check(L.lib().nq_bias_add(None, _p(g), _p(y), B, C, y.numel() // (B * C), _stream()), "bias_add")
        return y


def conv2d_dd(x, w, b=None):
    """stride-1 'same' convolution (+bias), differentiable to any order (reference F.conv2d, quant_layer.py:80, as used
    under torch.autograd.grad(create_graph=True) by methods/bit_assign.py:88-114)."""
    y = _ConvF.apply(x, w)
    return y if b is None else _BiasAddDD.apply(y, b)


def decoder_stack_dd(emb, spec, weights):
    """Decoder forward (reference HNeRV.py:49-71 / NeRV.py:44-65), twice differentiable, every operator on this repo's HIP
    kernels: the bilinear convolution family (_ConvF / _ConvD / _ConvWg), the bias broadcast, PixelShuffle, the exact-erf
    GELU and OutImg's tanh with their first and second derivatives (nq_act_dd).  Only the NeRV channel -> space view of
    layer 0 (NeRV.py:49-51: a reshape / permute, no arithmetic) is a PyTorch tensor view."""
    x = emb
    for l, ((k, r, act), (W, b)) in enumerate(zip(spec.layers, weights)):
        x = conv2d_dd(x, W, b)
        if l == 0 and spec.fc_hw != (1, 1):
            x = _space_from_channels(x, *spec.fc_hw)
        if r > 1:
            x = pixel_shuffle_dd(x, r)
        if act:
            x = gelu_dd(x)
    return tanh_out_dd(x) if spec.tanh_out else x


def conv2d_fused(x, w, b, epilogue=EPI_PLAIN, r=1):
    if not torch.is_grad_enabled() or not (x.requires_grad or w.requires_grad or (b is not None and b.requires_grad)):
        # inference (the per-frame evaluation decodes, calibrate_network.py:82-145): no graph to record, and the big
        # layers can take the bf16x3 kernel like the calibration loop does
        x, w = _dev(x, "x"), _dev(w, "weight")
        b = _dev(b, "bias") if b is not None else None
        cout, cin, k, k2 = w.shape
        if k != k2 or x.shape[1] != cin:
            raise ValueError(f"conv shape mismatch: x {tuple(x.shape)} w {tuple(w.shape)}")
        B, _, H, W = x.shape
        if _use3(None) and conv3_supported(B, cin, H, W, cout, k):
            return conv3_forward_raw(x, weight_layout3(w), b, cout, k, epilogue, r)[0]
        wt, dims, _, _ = weight_layouts(w, False)
        return conv_forward_raw(x, wt, dims, b, cout, k, epilogue, r)[0]
    return _ConvFn.apply(x, w, b, epilogue, r)


class DecoderSpec:
    """Static description of a conv decoder stack for `decoder_stack`: per layer (k, shuffle r, gelu after),
    the (fc_h, fc_w) channel->space reshape after layer 0 and whether OutImg is tanh*0.5+0.5."""

    def __init__(self, layers, fc_hw=(1, 1), tanh_out=True, precision=None):
        self.layers = [tuple(l) for l in layers]
        self.fc_hw = tuple(fc_hw)
        self.tanh_out = tanh_out
        # 'bf16x3': convolutions whose grid fills the chip run on the BF16 matrix pipe with split fp32 operands
        # (hi*hi + hi*lo + lo*hi, fp32 accumulate; see conv_igemm3_impl.h); 'fp32': exact fp32 MFMA everywhere.
        self.precision = precision or get_conv_precision()
        if self.precision not in ("fp32", "bf16x3"):
            raise ValueError(f"unknown conv precision {self.precision!r}")
        # NQ_WGRAD_STREAM=1: weight gradients on a second HIP stream, concurrent with the data-gradient chain (measured
        # +3 % it/s on HNeRV-3M; off by default so that per-kernel durations in profiles stay separable)
        self.overlap_wgrad = os.environ.get("NQ_WGRAD_STREAM", "0") == "1"


def _space_from_channels(x, fh, fw):
    n, c, h, w = x.shape  # reference NeRV.py:49-51
    return x.view(n, -1, fh, fw, h, w).permute(0, 1, 4, 2, 5, 3).reshape(n, -1, fh * h, fw * w)


def _channels_from_space(g, fh, fw):
    n, c, hh, ww = g.shape
    return g.view(n, c, hh // fh, fh, ww // fw, fw).permute(0, 1, 3, 5, 2, 4).reshape(n, c * fh * fw, hh // fh, ww // fw)


# Data-parallel hook: when set, the decoder node writes ALL conv weight/bias gradients into one flat arena
# and calls the hook on it (e.g. an in-place RCCL all-reduce with ReduceOp.AVG): no flatten / un-flatten copies around the
# collective.  The hook is per-thread state that every decoder node CAPTURES in its forward (ctx.nq_arena), so the
# backward -- which PyTorch runs on its own autograd thread -- uses what was installed when the forward ran, two decoders
# in one process do not see each other's hook, and whether the exchange happened is recorded on the node itself
# (`img.grad_fn.nq_arena_reduced`), not in a module global.
_ARENA_TLS = threading.local()


def _arena_state():
    return getattr(_ARENA_TLS, "state", (None, False))


def set_grad_arena_hook(fn, two_phase=False):
    """fn(arena) is called once per backward with the flat gradient arena.  two_phase=True: the node first runs ALL data
    gradients, then the weight gradients of the deep layers (most of the parameters, little work), calls
    fn(arena[:split], False), runs the weight gradients of the last layers (most of the work, few parameters) and calls
    fn(arena[split:], True): an asynchronous collective started by the first call overlaps the expensive kernels.
    Applies to decoder nodes whose FORWARD runs on this thread from now on; prefer the `grad_arena_hook` context manager."""
    _ARENA_TLS.state = (fn, bool(two_phase) and fn is not None)


@contextlib.contextmanager
def grad_arena_hook(fn, two_phase=False):
    """`with ops.grad_arena_hook(fn, two_phase):` installs the hook for the body and restores the previous one on the way
    out, exceptions included."""
    prev = _arena_state()
    set_grad_arena_hook(fn, two_phase)
    try:
        yield
    finally:
        _ARENA_TLS.state = prev


def arena_reduced(img):
    """True when the decoder node behind `img` handed its gradient arena to a hook during backward (the caller then
    skips its own gradient exchange)."""
    return bool(getattr(getattr(img, "grad_fn", None), "nq_arena_reduced", False))


# Fused loss tail (round 4): inside `with ops.fused_head_loss(...)` a tanh-headed decoder node whose head is the 3-channel 3x3
# convolution runs nq_head_forward_loss -- the head AND lp_loss / tanh backward / bias gradient in one pass over the image --
# and leaves the result in its hand-over slot; l2_loss_head_grad then returns it without launching anything.  Per-thread
# state like the arena hook; a decoder that cannot use it simply ignores the request.
_LOSS_TLS = threading.local()


@contextlib.contextmanager
def fused_head_loss(tgt=None, cache_u8=None, idx=None):
    """Request the fused loss tail for decoder forwards in the body: target = float frames `tgt` (B,3,H,W) or frames
    cache_u8[idx] / 255 of the uint8 frame cache."""
    prev = getattr(_LOSS_TLS, "req", None)
    _LOSS_TLS.req = None if os.environ.get("NQ_FUSED_HEAD_LOSS", "1") == "0" else (tgt, cache_u8, idx)
    try:
        yield
    finally:
        _LOSS_TLS.req = prev


def head_forward_loss_raw(x, wt, dims, bias, cout, k, tgt=None, cache_u8=None, idx=None):
    """nq_head_forward_loss: -> (img, loss, dconv, db) or None when the fused kernel does not apply."""
    B, cin, H, W = x.shape
    if cout != 3 or k != 3 or (W & 3) or (dims[1] & 3) or os.environ.get("NQ_HEAD_FWD") == "1":
        return None
    if cache_u8 is not None:
        if not cache_u8.is_cuda or cache_u8.dtype != torch.uint8 or not cache_u8.is_contiguous() \
                or tuple(cache_u8.shape[1:]) != (cout, H, W) or idx is None or idx.numel() != B:
            return None
        idx = idx.to(device=x.device, dtype=torch.int64).contiguous()
        tgt = None
    elif tgt is not None:
        if not tgt.is_cuda or tgt.dtype != torch.float32 or tuple(tgt.shape) != (B, cout, H, W):
            return None
        tgt = tgt.contiguous()
    else:
        return None
    y = torch.empty((B, cout, H, W), device=x.device, dtype=torch.float32)
    dconv = torch.empty_like(y)
    loss = torch.empty((), device=x.device, dtype=torch.float32)
    db = torch.empty(cout, device=x.device, dtype=torch.float32)
    ws = torch.empty(_q("nq_head_forward_loss_ws_floats", B, H, W), device=x.device, dtype=torch.float32)
    rc = _timed(("conv_igemm", k, cin, cout, H, W, B, EPI_TANH),
                lambda: L.lib().nq_head_forward_loss(_p(x), _p(wt), dims[1], _p(bias), _p(y), _p(tgt), _p(cache_u8), _p(idx), _p(loss),
                                                     _p(dconv), _p(db), _p(ws), B, cin, H, W, B * H * W, 1.0, _stream()))
    if rc == -2:     # NQ_ERR_UNSUPPORTED: the caller runs the separate kernels
        return None
    L.check(rc, "head_forward_loss")
    return y, loss, dconv, db


_SIDE_STREAMS = {}


def _side_stream(device):
    key = torch.device(device).index
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
    return _SIDE_STREAMS[key]


class LayerPlan:
    """Everything the three launches of one decoder layer need, decided by plan_decoder from shapes alone.  Routes are
    "bf16x3" | "fp32", the weight gradient's also "swapped3", the data gradient's None where no launch happens (layer 0
    unless the embedding is trained).  H, W: the layer's INPUT size.  `dgrad` is the launch that turns this layer's
    conv-output gradient into the one of the layer below (layer 0: into d(embedding)), on this layer's transposed weight.
    The weight operands follow from the routes: the pre-split operand / its transposed form where fwd / dgrad is "bf16x3",
    the fp32 forward / backward operand where it is "fp32"."""
    __slots__ = ("k", "r", "act", "cin", "cout", "has_bias", "H", "W", "epi", "fwd", "dgrad", "wgrad", "x_split", "g_split",
                 "fwd_fmt", "dgrad_epi", "dgrad_r", "dgrad_fmt", "wgrad_fmt")


def plan_decoder(spec, wshapes, has_bias, B, H, W, want_emb_grad):
    """The launch plan of one decoder forward + backward: one LayerPlan per layer.  wshapes: [(cout, cin)], has_bias: [bool]
    per layer; B, H, W: the embedding's batch and spatial size.  A pure host function: no tensors, no GPU, only the library's
    memoised shape queries; spec.precision and NQ_SPLIT_IO are read at call time.

    _DecoderStackFn.forward calls it once per forward and stores the result on the node; the backward pass routes by that
    stored plan and asks the library nothing.  So a spec.precision edited between a node's forward and its backward does
    not re-route that node's weight gradients (nothing does that)."""
    n = len(spec.layers)
    use3 = spec.precision == "bf16x3"
    plan = []
    fio, bio, wio = [0] * n, [0] * n, [0] * n   # split {hi | lo} word capabilities: forward / data gradient / weight gradient
    for l, (k, r, act) in enumerate(spec.layers):
        p = LayerPlan()
        p.k, p.r, p.act, (p.cout, p.cin), p.has_bias, p.H, p.W = k, r, act, wshapes[l], bool(has_bias[l]), H, W
        cout, cin = p.cout, p.cin
        if l == n - 1:
            p.epi = EPI_TANH if spec.tanh_out else EPI_PLAIN
        else:
            p.epi = EPI_PS_GELU if act else EPI_PS if r > 1 else EPI_PLAIN
        p.fwd = "bf16x3" if use3 and conv3_supported(B, cin, H, W, cout, k) else "fp32"
        # layer 0's data gradient is only needed when the embedding itself is trained (FP32 trainer: the ConvNeXt encoder
        # sits below it, reference regress.py:259-266), and then stays on the fp32 kernel
        if l == 0:
            p.dgrad = "fp32" if want_emb_grad else None
        else:
            p.dgrad = "bf16x3" if use3 and conv3_supported(B, cout, H, W, cin, k) else "fp32"
        if use3 and conv_wgrad3_supported(B, cin, H, W, cout, k):
            p.wgrad = "bf16x3"
        elif use3 and conv_wgrad_swapped3_supported(B, cin, H, W, cout, k):
            p.wgrad = "swapped3"
        else:
            p.wgrad = "fp32"
        if p.fwd == "bf16x3":
            fio[l] = conv3_split_io(B, cin, H, W, cout, k)
        if p.dgrad == "bf16x3":
            bio[l] = conv3_split_io(B, cout, H, W, cin, k)
        if p.wgrad == "bf16x3":
            wio[l] = conv_wgrad3_split_io(B, cin, H, W, cout, k)
        below_act = l > 0 and spec.layers[l - 1][2]
        p.dgrad_epi, p.dgrad_r = (EPI_DGRAD_GELU, spec.layers[l - 1][1]) if below_act else (EPI_PLAIN, 1)
        # the head's data gradient (streaming vector kernel) can write split words
        if l == n - 1 and l > 0 and p.dgrad == "fp32" and below_act \
                and conv_split_out(B, cout, H, W, cin, k, p.dgrad_r, EPI_DGRAD_GELU):
            bio[l] = EPI_Y_SPLIT
        plan.append(p)
        if l == 0:
            H, W = H * spec.fc_hw[0], W * spec.fc_hw[1]
        H, W = H * r, W * r
    # Which tensors travel as split {hi | lo} words (NQ_SPLIT_IO=0: none): the input x_l of layer l (l >= 2: written by the
    # GELU epilogue of layer l - 1, read by layer l's forward patch staging and by its weight gradient) and the conv-output
    # gradient g_l (written by the data gradient of layer l + 1, read by layer l's weight gradient and data gradient) --
    # where EVERY kernel on both sides takes / writes that form.  Same values in the matrix pipe: identical results, except
    # that a weight gradient sums the bias gradient db from hi + lo of a split g_l (~2^-17 relative to the float path).
    split_on = use3 and os.environ.get("NQ_SPLIT_IO", "1") != "0"
    for l, p in enumerate(plan):
        below_act = l > 0 and plan[l - 1].act
        p.x_split = bool(split_on and l >= 2 and below_act and (fio[l - 1] & EPI_Y_SPLIT) and (fio[l] & EPI_X_SPLIT)
                         and (wio[l] & 1))
        p.g_split = bool(split_on and 1 <= l < n - 1 and (bio[l + 1] & EPI_Y_SPLIT) and (bio[l] & EPI_X_SPLIT) and (wio[l] & 2)
                         and below_act and not (l == 1 and spec.fc_hw != (1, 1)))
    # the fmt words of the launches: a side is split only where a bf16x3 kernel reads it (x_split / g_split imply that route)
    for l, p in enumerate(plan):
        p.fwd_fmt = (EPI_X_SPLIT if p.x_split else 0) | (EPI_Y_SPLIT if l + 1 < n and plan[l + 1].x_split else 0)
        p.dgrad_fmt = (EPI_X_SPLIT if p.g_split else 0) | (EPI_Y_SPLIT if l > 0 and plan[l - 1].g_split else 0)
        p.wgrad_fmt = (1 if p.x_split else 0) | (2 if p.g_split else 0)
    return plan


class _DecoderStackFn(Function):
    """Whole decoder (reference HNeRV.py:49-71 / NeRV.py:44-65) as ONE autograd node with an explicit schedule, the
    LayerPlans of plan_decoder.

    Every block's conv epilogue writes a = gelu(PixelShuffle(conv+bias)) and d = gelu'(...) from one erf (EPI_PS_GELU);
    the data-gradient kernel of the layer above multiplies by d and un-shuffles in its epilogue (EPI_DGRAD_GELU).  So
    per block: 1 launch forward, 2 backward (+ the small split-K reductions), no elementwise passes over activations.
    """

    @staticmethod
    def forward(ctx, emb, spec, *wb):
        x = _dev(emb, "embedding")
        n = len(spec.layers)
        Ws = [_dev(w, "weight") for w in wb[0::2]]
        bs = [_dev(b, "bias") if b is not None else None for b in wb[1::2]]
        plan = plan_decoder(spec, [tuple(W.shape[:2]) for W in Ws], [b is not None for b in bs], x.shape[0], x.shape[2],
                            x.shape[3], ctx.needs_input_grad[0])
        # every weight operand of the node, pre-split (bf16x3 routes) and fp32 (the others), is built by ONE launch before
        # the first convolution
        keys3 = [(l, t) for l, p in enumerate(plan) for t, route in ((False, p.fwd), (True, p.dgrad)) if route == "bf16x3"]
        keys32 = [l for l, p in enumerate(plan) if "fp32" in (p.fwd, p.dgrad)]
        ops3, ops32 = weight_layouts_all([(Ws[l], t) for l, t in keys3],
                                         [(Ws[l], plan[l].fwd == "fp32", plan[l].dgrad == "fp32") for l in keys32])
        ops3, ops32 = dict(zip(keys3, ops3)), dict(zip(keys32, ops32))
        saved_in, saved_z = [], []
        ctx.wbk, ctx.dims_b, ctx.w3t = [None] * n, [None] * n, [None] * n   # the data gradients' operands, per layer
        zprev = None         # gelu'(pre-activation) behind x, saved by the producing epilogue
        fused_loss = None
        for l, p in enumerate(plan):
            wt, dims, wbk, dims_b = ops32.get(l, (None,) * 4)
            if p.dgrad == "fp32":
                ctx.wbk[l], ctx.dims_b[l] = wbk, dims_b
            ctx.w3t[l] = ops3.get((l, True))
            if l == n - 1 and p.epi == EPI_TANH and p.fwd == "fp32" and getattr(_LOSS_TLS, "req", None) is not None:
                fused_loss = head_forward_loss_raw(x, wt, dims, bs[l], p.cout, p.k, *_LOSS_TLS.req)
            if fused_loss is not None:
                y, z = fused_loss[0], None
            elif p.fwd == "bf16x3":
                y, z = conv3_forward_raw(x, ops3[l, False], bs[l], p.cout, p.k, p.epi, p.r, fmt=p.fwd_fmt)
            else:
                y, z = conv_forward_raw(x, wt, dims, bs[l], p.cout, p.k, p.epi, p.r)
            saved_in.append(x)
            saved_z.append(zprev)
            x, zprev = (y, z) if p.epi == EPI_PS_GELU else (z, None) if p.epi == EPI_PS else (y, None)
            if l == 0 and spec.fc_hw != (1, 1):
                x = _space_from_channels(x, *spec.fc_hw).contiguous()
        ctx.spec, ctx.plan, ctx.n = spec, plan, n
        ctx.save_for_backward(x, *saved_in, *saved_z)
        # per-node state (reachable from outside as img.grad_fn.<name>): the data-parallel hook installed on this thread
        # when the forward ran, whether backward handed the arena to it, and the hand-over slot of the fused loss tail
        ctx.nq_arena, ctx.nq_arena_reduced = _arena_state(), False
        ctx.nq_head = _HeadHandoff() if spec.tanh_out else None
        if fused_loss is not None:   # the loss tail already ran behind the head: l2_loss_head_grad hands it out
            ctx.nq_head.loss, ctx.nq_head.dconv, ctx.nq_head.db = fused_loss[1], fused_loss[2], fused_loss[3]
            ctx.nq_head.version = fused_loss[2]._version
        return x

    @staticmethod
    def backward(ctx, g_img):
        hook = ctx.nq_arena[0]
        steps = _decoder_backward_steps(ctx, g_img)
        while True:
            try:
                part, last = next(steps)
            except StopIteration as done:
                return done.value
            if last is None:
                hook(part)
            else:
                hook(part, last)


def _decoder_backward_steps(ctx, g_img):
    """The backward pass of a decoder node as a GENERATOR: it yields (arena part, last) wherever a part of the flat gradient
    arena is complete and must be exchanged between data-parallel ranks (last = None: the whole arena at once), and
    returns the gradient tuple of _DecoderStackFn.backward.  The autograd node drives it and calls the installed hook at
    every yield; the captured data-parallel iteration (quantization/calib_model.py) drives it stage by stage, with the
    collectives launched eagerly between three replayed graphs.  Every route and flag comes from the plan the forward
    stored (ctx.plan); no support query is made here."""
    spec, plan, n = ctx.spec, ctx.plan, ctx.n
    saved = ctx.saved_tensors
    img, xs, zs = saved[0], saved[1:1 + n], saved[1 + n:]
    d_emb = None
    g = _dev(g_img, "grad")
    head_db = None
    head = ctx.nq_head
    if head is not None and head.loss is not None:
        # the fused loss tail ran behind the head but nobody took its result (l2_loss_head_grad was not called): the incoming
        # gradient is an ordinary d(loss)/d(image)
        head.dconv = head.db = head.loss = None
    if head is not None and head.dconv is not None:
        # l2_loss_head_grad handed over the gradient at the head conv's OUTPUT (tanh backward applied) and the head's
        # bias gradient.  Anything but that very tensor, unmodified, cannot be continued from: say so loudly.
        if head.dconv.data_ptr() != g.data_ptr() or g.shape != head.dconv.shape:
            raise RuntimeError("neuroquant_amd: the gradient returned by ops.l2_loss_head_grad must be passed to "
                               "backward() as it is (it already contains the tanh backward of this decoder)")
        dconv = g
        # scaled / edited in place since the hand-over: the pre-summed bias gradient no longer matches -> re-sum it
        head_db = head.db if g._version == head.version else None
        head.dconv = head.db = None
    elif spec.tanh_out:
        dconv = torch.empty_like(g)
        L.check(L.lib().nq_tanh_out_backward(_p(g), _p(img), _p(dconv), g.numel(), _stream()), "tanh_backward")
    else:
        dconv = g
    grads = [None] * (2 * n)
    # The weight gradients are off the critical path (only the data gradients chain): they run on a second HIP
    # stream so that their workgroups fill the partial last rounds ("tails") of the data-gradient kernels and the
    # launch gaps of the small deep layers.  Every dconv stays referenced until the streams are joined.
    main = torch.cuda.current_stream()
    side = _side_stream(g.device) if spec.overlap_wgrad else None
    keep = []

    # one flat arena for all weight/bias gradients when a data-parallel hook is installed (in-place collective)
    arena = views = None
    arena_hook, arena_two_phase = ctx.nq_arena
    if arena_hook is not None:
        sizes = []
        for p in plan:
            sizes += [p.cout * p.cin * p.k * p.k, p.cout if p.has_bias else 0]
        arena = torch.empty(sum(sizes), device=g.device, dtype=torch.float32)
        views, off = [], 0
        for l, p in enumerate(plan):
            wv = arena[off:off + sizes[2 * l]].view(p.cout, p.cin, p.k, p.k)
            off += sizes[2 * l]
            bv = arena[off:off + sizes[2 * l + 1]] if sizes[2 * l + 1] else None
            off += sizes[2 * l + 1]
            views.append((wv, bv))

    # the split-K weight-gradient kernels leave slabs; their fixed-order reductions run in ONE launch per group of
    # layers (`pending.flush()`: at the end of the backward pass, or before each part of the arena goes to the
    # data-parallel hook) instead of one ~10 us launch per layer.  Same sums in the same order: bit-identical.
    pending = PendingReductions() if side is None and os.environ.get("NQ_DEFER_REDUCE", "1") != "0" else None

    def wgrad(l, dconv):
        p = plan[l]
        out = views[l] if views is not None else None
        if p.wgrad == "bf16x3":
            return conv_wgrad3_raw(xs[l], dconv, p.cout, p.k, p.has_bias, out=out, defer=pending, fmt=p.wgrad_fmt)
        if p.wgrad == "swapped3":
            if l == n - 1 and p.has_bias and head_db is not None:   # bias gradient handed over by l2_loss_head_grad
                dw, _ = conv_wgrad_swapped3(xs[l], dconv, p.cout, p.k, False, out=out, defer=pending)
                if out is not None:
                    out[1].copy_(head_db)
                    return dw, out[1]
                return dw, head_db
            return conv_wgrad_swapped3(xs[l], dconv, p.cout, p.k, p.has_bias, out=out, defer=pending)
        return conv_wgrad_raw(xs[l], dconv, p.cout, p.k, p.has_bias, out=out, defer=pending)

    def dgrad(l, dconv):
        """conv-output gradient of layer l -> conv-output gradient of layer l - 1 (l >= 1)"""
        p = plan[l]
        if not plan[l - 1].act and plan[l - 1].r != 1:
            raise NotImplementedError("PixelShuffle without activation between decoder layers")
        # the layer below ends in GELU: d(pre-activation) = dgrad * gelu'(z), stored as ITS conv-output gradient
        zp = zs[l] if p.dgrad_epi == EPI_DGRAD_GELU else None
        if p.dgrad == "bf16x3":
            d, _ = conv3_forward_raw(dconv, ctx.w3t[l], None, p.cin, p.k, p.dgrad_epi, p.dgrad_r, zprev=zp, fmt=p.dgrad_fmt)
        else:
            d, _ = conv_forward_raw(dconv, ctx.wbk[l], ctx.dims_b[l], None, p.cin, p.k, p.dgrad_epi, p.dgrad_r, zprev=zp,
                                    fmt=p.dgrad_fmt)
        if not plan[l - 1].act and l == 1 and spec.fc_hw != (1, 1):
            d = _channels_from_space(d, *spec.fc_hw).contiguous()
        return d

    def emb_grad(dconv):   # d(embedding): plain data gradient through layer 0 (no activation below it)
        return conv_forward_raw(dconv, ctx.wbk[0], ctx.dims_b[0], None, plan[0].cin, plan[0].k, EPI_PLAIN, 1)[0]

    if arena is not None and arena_two_phase and n > 1:
        # Data-parallel schedule: the data-gradient chain first, then the weight gradients of the deep layers (most
        # of the parameters, a few per cent of the work) whose part of the arena is handed to the hook at once, then
        # the last layers' weight gradients (>= 80 % of the weight-gradient flops) while that collective is in
        # flight, then the rest of the arena.  Same kernels on the same operands as the single-GPU order: identical bits.
        dcs = [None] * n
        dcs[n - 1] = dconv
        for l in range(n - 1, 0, -1):
            dcs[l - 1] = dgrad(l, dcs[l])
        if plan[0].dgrad is not None:
            d_emb = emb_grad(dcs[0])
        flops = [p.cout * p.cin * p.k ** 2 * p.H * p.W for p in plan]
        split, late = n - 1, flops[n - 1]
        while split > 1 and late < 0.8 * sum(flops):
            split -= 1
            late += flops[split]
        for l in range(split):
            grads[2 * l], grads[2 * l + 1] = wgrad(l, dcs[l])
            dcs[l] = None
        off = sum(sizes[:2 * split])
        if pending is not None:
            pending.flush()
        yield arena[:off], False
        for l in range(split, n):
            grads[2 * l], grads[2 * l + 1] = wgrad(l, dcs[l])
            dcs[l] = None
        if pending is not None:
            pending.flush()
        yield arena[off:], True
        ctx.nq_arena_reduced = True
        return (d_emb, None) + tuple(grads)

    for l in range(n - 1, -1, -1):
        if side is not None:
            keep.append(dconv)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                dw, db = wgrad(l, dconv)
            for t in (dw, db):
                if t is not None:
                    t.record_stream(main)
        else:
            dw, db = wgrad(l, dconv)
        grads[2 * l], grads[2 * l + 1] = dw, db
        if l == 0:
            if plan[0].dgrad is not None:
                d_emb = emb_grad(dconv)
            break
        dconv = dgrad(l, dconv)
    if side is not None:
        main.wait_stream(side)
        keep.clear()
    if pending is not None:
        pending.flush()
    if arena is not None:
        yield arena, None
        ctx.nq_arena_reduced = True
    return (d_emb, None) + tuple(grads)


class _ManualNode:
    """Stand-in for the autograd context of _DecoderStackFn when the decoder is driven WITHOUT autograd (captured
    data-parallel iterations): forward fills it, decoder_backward_steps consumes it."""

    def __init__(self, n_inputs, want_emb_grad=False):
        self.needs_input_grad = (bool(want_emb_grad), False) + (True,) * n_inputs
        self.saved_tensors = ()

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors


def decoder_forward_manual(emb, spec: DecoderSpec, weights, two_phase=True):
    """decoder_stack without autograd: -> (image, node).  The node always collects its weight gradients in ONE flat arena
    and decoder_backward_steps(node, g) yields its parts for the caller to exchange (it calls no hook itself)."""
    flat = []
    for W, b in weights:
        flat += [W, b]
    node = _ManualNode(len(flat))
    with torch.no_grad():
        img = _DecoderStackFn.forward(node, emb, spec, *flat)
    node.nq_arena = ("manual", bool(two_phase))
    return img, node


def decoder_backward_steps(node, g_img):
    """Generator over the backward pass of a decoder_forward_manual node: yields (arena part, last | None) at the exchange
    points; StopIteration.value = (d_emb, None, dW0, db0, dW1, ...) as _DecoderStackFn.backward returns them."""
    return _decoder_backward_steps(node, g_img)


def decoder_stack(emb, spec: DecoderSpec, weights):
    """weights: [(W, b), ...] per layer (already fake-quantised).  Returns the output image."""
    flat = []
    for W, b in weights:
        flat += [W, b]
    return _DecoderStackFn.apply(emb, spec, *flat)


# ------------------------------------------------------------------------------------------ loss / metrics / frames
class _ScalarLossFn(Function):
    """A scalar loss of `pred` whose backward is grad * g.  launch(pred, tgt, want_grad) -> (loss, grad or None) issues the kernels;
    want_grad = `pred` needs a gradient (a launcher may compute the gradient regardless: its launches are its own affair)."""

    @staticmethod
    def forward(ctx, pred, tgt, launch):
        loss, grad = launch(pred, tgt, ctx.needs_input_grad[0])
        if grad is not None:
            ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None


def _l2_loss_launch(pred, tgt, want_grad):
    """lp_loss(pred, tgt, p=2): sum over channels, mean over batch*H*W (reference quantizer.py:66-71), and its gradient"""
    pred_d, tgt = _dev(pred.detach(), "pred"), _dev(tgt, "tgt")
    n = pred_d.numel()
    loss = torch.empty((), device=pred_d.device, dtype=torch.float32)
    dpred = torch.empty_like(pred_d) if want_grad else None
    ws = torch.empty(_q("nq_reduce_ws_floats", n), device=pred_d.device, dtype=torch.float32)
    L.check(L.lib().nq_l2_loss(_p(pred_d), _p(tgt), _p(loss), _p(dpred), _p(ws), n, n // pred_d.shape[1], 1.0, _stream()),
            "l2_loss")
    return loss, dpred


def l2_loss(pred, tgt):
    return _ScalarLossFn.apply(pred, tgt, _l2_loss_launch)


def l2_loss_and_grad(pred, tgt):
    """(loss, d loss / d pred) from ONE kernel, outside autograd: `pred.backward(dpred)` then feeds the decoder node
    directly (no ones-tensor, no elementwise multiply by the upstream gradient)."""
    return _l2_loss_launch(pred, tgt, True)


class _HeadHandoff:
    """Hand-over slot of the fused loss tail, owned by ONE decoder node (ctx.nq_head, reachable as img.grad_fn.nq_head):
    l2_loss_head_grad fills it with the gradient at the head conv's output and the head's bias gradient, the node's
    backward takes them when the incoming gradient is that very tensor (`version` = its in-place edit counter at the
    hand-over: an edited gradient is still continued from, but the bias gradient is summed again)."""
    __slots__ = ("dconv", "db", "version", "loss")

    def __init__(self):
        self.dconv = self.db = self.version = self.loss = None


def _handoff(pred, node=None):
    """The hand-over slot of the decoder node behind `pred` (node: the manual node of decoder_forward_manual, whose image has no
    autograd history), or None: only the tensor a tanh-headed decoder node returned carries one, and NQ_FUSED_LOSS=0 hides it."""
    head = getattr(node if node is not None else getattr(pred, "grad_fn", None), "nq_head", None)
    return head if isinstance(head, _HeadHandoff) and os.environ.get("NQ_FUSED_LOSS", "1") != "0" else None


def _hand_over(head, dconv, db):
    """Leave the gradient at the head conv's output and the head's bias gradient in the slot -> dconv.  (A result of
    ops.fused_head_loss that nobody asked for is dropped: the objective that hands over replaces it.)"""
    head.loss = None
    head.dconv, head.db, head.version = dconv, db, dconv._version
    return dconv


def _loss_target(what, pred, tgt, cache_u8, idx, typed=False):
    """The target of a loss launch on images `pred`: exactly one of float frames `tgt` and frames cache_u8[idx] / 255 of the uint8
    frame cache -> (tgt, cache_u8, idx) with the form not given None, tgt float32 and contiguous on the GPU, idx int64 and
    contiguous on pred's device.  ValueError for both, neither, or a target of another shape than pred.  A bad cache is a
    RuntimeError, except typed=True (the SSIM launchers): ValueError for a wrong type or shape, RuntimeError for a cache that is
    not contiguous on the GPU.  The VALUES of idx stay on the device, unchecked: inside [0, N) is the caller's responsibility."""
    if (tgt is None) == (cache_u8 is None):
        raise ValueError(f"{what} takes exactly one of tgt and cache_u8 + idx")
    if cache_u8 is None:
        if not typed:
            tgt = _dev(tgt, "tgt")
        elif not isinstance(tgt, torch.Tensor):
            raise ValueError(f"{what} takes a (B, C, H, W) target, got {type(tgt)}")
        if tuple(tgt.shape) != tuple(pred.shape):
            raise ValueError(f"{what}: pred {tuple(pred.shape)} and tgt {tuple(tgt.shape)} differ")
        return _dev(tgt.detach(), "tgt"), None, None
    bad = not isinstance(cache_u8, torch.Tensor) or cache_u8.dtype != torch.uint8 or cache_u8.dim() != 4 \
        or not isinstance(idx, torch.Tensor) or (typed and idx.dim() != 1)
    if bad and typed:
        raise ValueError(f"{what}: the frame cache must be a uint8 (N, C, H, W) tensor with a 1-d idx")
    tgt_shape = None if bad else (idx.numel(),) + tuple(cache_u8.shape[1:])
    if typed and tgt_shape != tuple(pred.shape):
        raise ValueError(f"{what}: pred {tuple(pred.shape)} and tgt {tgt_shape} differ")
    if tgt_shape != tuple(pred.shape) or not cache_u8.is_cuda or not cache_u8.is_contiguous():
        raise RuntimeError("frame cache must be a contiguous uint8 GPU tensor of the image's shape")
    return None, cache_u8, idx.to(device=pred.device, dtype=torch.int64).contiguous()


def l2_loss_tanh_head_raw(pred, tgt=None, cache_u8=None, idx=None):
    """One nq_l2_loss_tanh_head launch on an image `pred` = tanh(conv)*0.5+0.5: -> (loss, dconv, db) with lp_loss(pred,
    tgt, p=2), the gradient at the conv OUTPUT (tanh backward applied) and its per-channel sums (the head's bias
    gradient); the target is `tgt` or frames `cache_u8[idx]/255` read straight from the uint8 cache.  None when the
    kernel's tiling does not apply (H*W % 4096 != 0)."""
    pred_d = _dev(pred.detach(), "pred")
    if pred_d.dim() != 4:
        return None
    B, C, H, W = pred_d.shape
    if (H * W) % 4096 != 0 or C > 1024:
        return None
    tgt, cache_u8, idx = _loss_target("l2_loss_tanh_head", pred_d, tgt, cache_u8, idx)
    n = pred_d.numel()
    loss = torch.empty((), device=pred_d.device, dtype=torch.float32)
    dconv = torch.empty_like(pred_d)
    db = torch.empty(C, device=pred_d.device, dtype=torch.float32)
    ws = torch.empty(2 * _q("nq_reduce_ws_floats", n), device=pred_d.device, dtype=torch.float32)
    L.check(L.lib().nq_l2_loss_tanh_head(_p(pred_d), _p(tgt), _p(cache_u8), _p(idx), _p(loss), _p(dconv), _p(db), _p(ws),
                                         B, C, H * W, n // C, 1.0, _stream()), "l2_loss_tanh_head")
    return loss, dconv, db


def l2_loss_head_grad(pred, tgt=None, cache_u8=None, idx=None, node=None):
    """lp_loss(pred, tgt, p=2) for `pred` = the image a tanh-headed `decoder_stack` just returned, fused with what its
    backward does first: returns (loss, g) where `pred.backward(g)` continues at the head convolution -- g is the
    gradient at the head conv's OUTPUT (tanh backward applied) and the head's bias gradient is handed over with it
    (one pass over the image instead of loss + tanh backward + channel sums; the target can be read straight from the
    uint8 frame cache).  The hand-over lives on pred's own autograd node, so g belongs to THIS decoder call only and
    must reach backward() as returned.  Returns None when `pred` is not such an image (no graph recorded, another
    producer) or the fused kernel does not apply; the caller then uses l2_loss_and_grad."""
    head = _handoff(pred, node)
    if head is None:
        return None
    if head.loss is not None:   # computed behind the head convolution (ops.fused_head_loss): nothing to launch
        loss, head.loss = head.loss, None
        return loss, head.dconv
    out = l2_loss_tanh_head_raw(pred, tgt, cache_u8, idx)
    return None if out is None else (out[0], _hand_over(head, out[1], out[2]))


# ---- the same tail in the 8-bit YUV 4:2:0 domain (include/nq_hip.h: nq_yuv420_loss) ----
YUV_LOSS_WEIGHTS = (6.0, 1.0, 1.0)
yuv420_loss_launches = 0    # nq_yuv420_loss launches issued (or captured) by this process: the default paths issue none


def _loss_weights(what, weights, n):
    """-> the weights of a loss as floats; ValueError naming `what` unless they are n finite numbers >= 0 with a positive sum"""
    try:
        w = tuple(float(v) for v in weights)
    except (TypeError, ValueError):
        w = ()
    if len(w) != n or not all(math.isfinite(v) and v >= 0.0 for v in w) or not sum(w) > 0.0:
        raise ValueError(f"{what}: weights must be {('two', 'three')[n - 2]} finite numbers >= 0 with a positive sum, got {weights!r}")
    return w


def _mse_plus_args(what, pred_shape, tgt_shape, weights, least, sizes):
    """the checks of an MSE + (1 - similarity) loss on images whose sides are at least `least` -> its two weights as floats"""
    if len(pred_shape) != 4 or min(pred_shape[:2]) <= 0 or min(pred_shape[2:]) < least:
        raise ValueError(f"{what} takes (B, C, H, W) images {sizes}, got {tuple(pred_shape)}")
    if tuple(tgt_shape) != tuple(pred_shape):
        raise ValueError(f"{what}: pred {tuple(pred_shape)} and tgt {tuple(tgt_shape)} differ")
    return _loss_weights(what, weights, 2)


def yuv420_loss_args(what, shape, matrix, full_range, weights):
    """-> (matrix code, range code, (wy, wu, wv)); ValueError naming `what` before anything is launched"""
    if len(shape) != 4 or shape[1] != 3 or shape[0] <= 0:
        raise ValueError(f"{what} takes (B, 3, H, W) images, got {tuple(shape)}")
    _, m, fr = _yuv_args(what, shape[2], shape[3], matrix, full_range)
    return m, fr, _loss_weights(what, weights, 3)


def yuv420_loss_raw(pred, tgt=None, cache_u8=None, idx=None, matrix="bt709", full_range=False, weights=YUV_LOSS_WEIGHTS,
                    head=False):
    """One nq_yuv420_loss launch pair on images `pred` (B, 3, H, W), H and W even -> (loss4, grad, db): loss4 = (L, MSE_Y, MSE_U,
    MSE_V) with L = 3 (wY MSE_Y + wU MSE_U + wV MSE_V) / (wY + wU + wV) over the unrounded 8-bit 4:2:0 codes / 255; the target is
    `tgt` or frames `cache_u8[idx] / 255` read straight from the uint8 cache.  head=False: grad = dL/dpred, db = None.
    head=True (`pred` = tanh(conv) * 0.5 + 0.5): grad = the gradient at the conv OUTPUT and db its per-channel sums (the head's
    bias gradient), as l2_loss_tanh_head_raw.  ValueError for a bad shape, matrix or weights before any launch."""
    global yuv420_loss_launches
    if not isinstance(pred, torch.Tensor):
        raise ValueError(f"yuv420_loss takes (B, 3, H, W) images, got {type(pred)}")
    m, fr, w = yuv420_loss_args("yuv420_loss", pred.shape, matrix, full_range, weights)
    pred_d = _dev(pred.detach(), "pred")
    B, C, H, W = pred_d.shape
    tgt, cache_u8, idx = _loss_target("yuv420_loss", pred_d, tgt, cache_u8, idx)
    loss4 = torch.empty(4, device=pred_d.device, dtype=torch.float32)
    grad = torch.empty_like(pred_d)
    db = torch.empty(3, device=pred_d.device, dtype=torch.float32) if head else None
    ws = torch.empty(_q("nq_yuv420_loss_ws_floats", B, H, W), device=pred_d.device, dtype=torch.float32)
    yuv420_loss_launches += 1
    L.check(_timed("yuv420_loss", lambda: L.lib().nq_yuv420_loss(
        _p(pred_d), _p(tgt), _p(cache_u8), _p(idx), _p(loss4), _p(grad), _p(db), _p(ws), B, H, W, m, fr, w[0], w[1], w[2], 1.0,
        _stream())), "yuv420_loss")
    return loss4, grad, db


def yuv420_loss(pred, tgt, matrix="bt709", full_range=False, weights=YUV_LOSS_WEIGHTS):
    """Differentiable L of yuv420_loss_raw (w.r.t. `pred`): the weighted plane MSEs of the 8-bit YUV 4:2:0 codes, on the scale
    of l2_loss (the trainer divides both by 3)."""
    full_range, weights = bool(full_range), tuple(weights)

    def launch(pred, tgt, want_grad):
        loss4, grad, _ = yuv420_loss_raw(pred, tgt=tgt, matrix=matrix, full_range=full_range, weights=weights)
        return loss4[0].clone(), grad
    return _ScalarLossFn.apply(pred, tgt, launch)


def yuv420_loss_head_grad(pred, tgt=None, cache_u8=None, idx=None, matrix="bt709", full_range=False,
                          weights=YUV_LOSS_WEIGHTS, node=None):
    """l2_loss_head_grad for the YUV 4:2:0 objective: -> (loss4, g) where `pred.backward(g)` (or decoder_backward_steps(node,
    g)) continues the backward pass.  When `pred` carries the hand-over slot of a tanh-headed decoder node, g is the
    gradient at the head conv's OUTPUT and the head's bias gradient is handed over with it; otherwise g = dL/dpred and the
    ordinary backward runs.  Never None: the kernel has no tiling restriction."""
    head = _handoff(pred, node)
    loss4, g, db = yuv420_loss_raw(pred, tgt, cache_u8, idx, matrix, full_range, weights, head=head is not None)
    return loss4, (g if head is None else _hand_over(head, g, db))


# ---- MSE + single-scale SSIM, the reference's ssim / Fusion1 / 3 / 5 losses (include/nq_hip.h: nq_ssim_loss) ----
SSIM_LOSS_TILE = (8, 118)   # rows x columns a workgroup of csrc/ssim_loss.hip owns (SL_TH, SL_TW): the tests' edge shapes


def ssim_loss_args(what, pred_shape, tgt_shape, w_mse, w_ssim):
    """-> (w_mse, w_ssim) as floats; ValueError naming `what` before anything is launched"""
    return _mse_plus_args(what, pred_shape, tgt_shape, (w_mse, w_ssim), 11, "with H, W >= 11")


def _mse_plus_launch(entry, what, pred, tgt, w_mse, w_sim, want_grad, grad_scale=1.0):
    """One nq_ssim_loss / nq_msssim_loss call (entry "ssim_loss" / "msssim_loss") -> (loss3, grad or None, ws): ws[:B] holds the
    per-frame SSIM / MS-SSIM"""
    if not isinstance(pred, torch.Tensor) or not isinstance(tgt, torch.Tensor):
        raise ValueError(f"{what} takes two (B, C, H, W) tensors, got {type(pred)} and {type(tgt)}")
    w = (ssim_loss_args if entry == "ssim_loss" else ms_ssim_loss_args)(what, pred.shape, tgt.shape, w_mse, w_sim)
    pred_d, tgt = _dev(pred.detach(), "pred"), _dev(tgt.detach(), "tgt")
    B, C, H, W = pred_d.shape
    loss3 = torch.empty(3, device=pred_d.device, dtype=torch.float32)
    grad = torch.empty_like(pred_d) if want_grad else None
    ws = torch.empty(_q(f"nq_{entry}_ws_floats", B, C, H, W), device=pred_d.device, dtype=torch.float32)
    L.check(_timed(entry, lambda: getattr(L.lib(), "nq_" + entry)(_p(pred_d), _p(tgt), _p(loss3), _p(grad), _p(ws), B, C, H, W, w[0],
                                                                  w[1], float(grad_scale), _stream())), entry)
    return loss3, grad, ws


def ssim_loss_raw(pred, tgt, w_mse, w_ssim, want_grad=True):
    """One nq_ssim_loss call on images `pred`, `tgt` (B, C, H, W), H, W >= 11 -> (loss3, grad): loss3 = (L, mean MSE, mean SSIM)
    with L = mean_b [w_mse * MSE_b + w_ssim * (1 - SSIM_b)], SSIM the single-scale pytorch_msssim.ssim(pred, tgt, data_range=1,
    size_average=False) (11-tap Gaussian window, valid filtering; reference utils.py:119-130); grad = dL/dpred, exact, or None
    with want_grad=False (the forward launch alone: the same loss3 bits).  Bit-identical from call to call.  ValueError for a bad
    shape or bad weights before any launch."""
    loss3, grad, _ = _mse_plus_launch("ssim_loss", "ssim_loss", pred, tgt, w_mse, w_ssim, want_grad)
    return loss3, grad


def ssim_loss(pred, tgt, w_mse=0.0, w_ssim=1.0):
    """Differentiable L of ssim_loss_raw (w.r.t. `pred`): the reference's per-frame loss followed by .mean()."""
    w_mse, w_ssim = float(w_mse), float(w_ssim)

    def launch(pred, tgt, want_grad):
        loss3, grad = ssim_loss_raw(pred, tgt, w_mse, w_ssim)
        return loss3[0].clone(), grad
    return _ScalarLossFn.apply(pred, tgt, launch)


ssim_loss_head_launches = 0    # nq_ssim_loss_head calls issued (or captured) by this process: the default paths issue none


def ssim_loss_head_raw(pred, tgt=None, cache_u8=None, idx=None, w_mse=0.0, w_ssim=1.0, head=False):
    """One nq_ssim_loss_head call on images `pred` (B, C, H, W), H, W >= 11 -> (loss3, grad, db): loss3 = (C * L, mean MSE, mean
    SSIM) with L of ssim_loss_raw (the factor C puts weights (1, 0) on the scale of lp_loss(p=2), as the 3 of yuv420_loss_raw);
    the target is `tgt` or frames `cache_u8[idx] / 255` read straight from the uint8 cache.  head=False: grad = C * dL/dpred,
    db = None.  head=True (`pred` = tanh(conv) * 0.5 + 0.5): grad = the gradient at the conv OUTPUT and db its per-channel sums
    (the head's bias gradient), as l2_loss_tanh_head_raw.  ValueError for a bad shape, target or weights before any launch.
    The VALUES of idx are not among what is checked: they stay on the device (a host read would stop a capture), and keeping
    them inside [0, N) is the caller's responsibility, as for l2_loss_tanh_head_raw and yuv420_loss_raw."""
    global ssim_loss_head_launches
    if not isinstance(pred, torch.Tensor):
        raise ValueError(f"ssim_loss_head takes (B, C, H, W) images, got {type(pred)}")
    w = ssim_loss_args("ssim_loss_head", pred.shape, pred.shape, w_mse, w_ssim)
    tgt, cache_u8, idx = _loss_target("ssim_loss_head", pred, tgt, cache_u8, idx, typed=True)
    pred_d = _dev(pred.detach(), "pred")
    B, C, H, W = pred_d.shape
    loss3 = torch.empty(3, device=pred_d.device, dtype=torch.float32)
    grad = torch.empty_like(pred_d)
    db = torch.empty(C, device=pred_d.device, dtype=torch.float32) if head else None
    ws = torch.empty(_q("nq_ssim_loss_head_ws_floats", B, C, H, W), device=pred_d.device, dtype=torch.float32)
    ssim_loss_head_launches += 1
    L.check(_timed("ssim_loss_head", lambda: L.lib().nq_ssim_loss_head(
        _p(pred_d), _p(tgt), _p(cache_u8), _p(idx), _p(loss3), _p(grad), _p(db), _p(ws), B, C, H, W, w[0], w[1], float(C),
        _stream())), "ssim_loss_head")
    return loss3, grad, db


def ssim_loss_head_grad(pred, tgt=None, cache_u8=None, idx=None, w_mse=0.0, w_ssim=1.0, node=None):
    """l2_loss_head_grad for the MSE + SSIM objective: -> (loss3, g) where `pred.backward(g)` (or decoder_backward_steps(node,
    g)) continues the backward pass.  When `pred` carries the hand-over slot of a tanh-headed decoder node, g is the
    gradient at the head conv's OUTPUT and the head's bias gradient is handed over with it; otherwise g = C * dL/dpred and the
    ordinary backward runs.  Never None: the kernel has no tiling restriction."""
    head = _handoff(pred, node)
    loss3, g, db = ssim_loss_head_raw(pred, tgt, cache_u8, idx, w_mse, w_ssim, head=head is not None)
    return loss3, (g if head is None else _hand_over(head, g, db))


# ---- MSE + five-scale MS-SSIM (include/nq_hip.h: nq_msssim_loss) ----
MSSSIM_LOSS_LAUNCHES = 11      # kernel launches of one nq_msssim_loss call with a gradient: 5 forward, 1 finish, 5 backward
msssim_loss_head_launches = 0  # ops.msssim_loss_head_grad calls issued (or captured) by this process: the default paths issue none


def ms_ssim_loss_args(what, pred_shape, tgt_shape, w_mse, w_ms):
    """-> (w_mse, w_ms) as floats; ValueError naming `what` before anything is launched"""
    return _mse_plus_args(what, pred_shape, tgt_shape, (w_mse, w_ms), 161, "whose smaller side exceeds (11 - 1) * 2**4 = 160")


def ms_ssim_loss_raw(pred, tgt, w_mse, w_ms, want_grad=True):
    """One nq_msssim_loss call on images `pred`, `tgt` (B, C, H, W), min(H, W) > 160 -> (loss3, grad): loss3 = (L, mean MSE, mean
    MS-SSIM) with L = mean_b [w_mse * MSE_b + w_ms * (1 - MS_b)], MS_b the five-scale MS-SSIM that ops.ms_ssim reports (the
    definition of pytorch_msssim.ms_ssim(pred, tgt, data_range=1, size_average=False)); grad = dL/dpred, exact, or None with
    want_grad=False (the forward launches alone: the same loss3 bits).  A (frame, channel) plane on which the relu of a scale
    is active has M = 0 and, by this project's rule, no MS-SSIM gradient (autograd would give NaN).  Bit-identical from call
    to call.  ValueError for a bad shape or bad weights before any launch."""
    loss3, grad, _ = _mse_plus_launch("msssim_loss", "ms_ssim_loss", pred, tgt, w_mse, w_ms, want_grad)
    return loss3, grad


def ms_ssim_loss(pred, tgt, w_mse=0.0, w_ms=1.0):
    """Differentiable L of ms_ssim_loss_raw (w.r.t. `pred`).  Where `pred` needs no gradient (torch.no_grad, a detached image) the
    call is forward only: six launches, no derivative maps, the same loss bits."""
    w_mse, w_ms = float(w_mse), float(w_ms)

    def launch(pred, tgt, want_grad):
        loss3, grad = ms_ssim_loss_raw(pred, tgt, w_mse, w_ms, want_grad=want_grad)
        return loss3[0].clone(), grad
    return _ScalarLossFn.apply(pred, tgt, launch)


def msssim_loss_head_grad(img_out, tgt=None, cache_u8=None, idx=None, node=None, w_mse=0.0, w_ms=1.0):
    """ssim_loss_head_grad for the MSE + MS-SSIM objective: -> (loss3, dimg) with loss3 = (C * L, mean MSE, mean MS-SSIM) (the
    factor C puts weights (1, 0) on the scale of lp_loss(p = 2)) and `img_out.backward(dimg)` (or decoder_backward_steps(node,
    dimg)) continuing the backward pass.  The target is `tgt` or the frames `cache_u8[idx] / 255`, gathered by
    nq_gather_frames_u8.  With the hand-over slot of a tanh-headed decoder node, dimg is the gradient at the head conv's OUTPUT
    (nq_tanh_out_backward of C * dL/dimg) and the head's bias gradient (nq_channel_sum of it) is handed over with it; otherwise
    dimg = C * dL/dimg.  There is no fused head variant of this kernel.  Everything stays on the stream, nothing is read by the
    host.  ValueError for a bad shape, target or weights before any launch."""
    global msssim_loss_head_launches
    if not isinstance(img_out, torch.Tensor):
        raise ValueError(f"msssim_loss_head_grad takes (B, C, H, W) images, got {type(img_out)}")
    w = ms_ssim_loss_args("msssim_loss_head_grad", img_out.shape, img_out.shape, w_mse, w_ms)
    tgt, cache_u8, idx = _loss_target("msssim_loss_head_grad", img_out, tgt, cache_u8, idx, typed=True)
    if not img_out.is_cuda:
        raise RuntimeError("neuroquant_amd: msssim_loss_head_grad needs GPU tensors")
    if cache_u8 is not None:
        tgt = gather_frames_u8(cache_u8, idx)
    C = img_out.shape[1]
    msssim_loss_head_launches += 1
    loss3, g, _ = _mse_plus_launch("msssim_loss", "msssim_loss_head_grad", img_out, tgt, w[0], w[1], True, grad_scale=float(C))
    loss3[:1].mul_(float(C))       # the float L times C, one more rounding, on the stream
    head = _handoff(img_out, node)
    if head is None:
        return loss3, g
    img_d = _dev(img_out.detach(), "img_out")
    dconv = torch.empty_like(g)
    L.check(L.lib().nq_tanh_out_backward(_p(g), _p(img_d), _p(dconv), g.numel(), _stream()), "tanh_backward")
    return loss3, _hand_over(head, dconv, channel_sum(dconv))


def ssim(out, gt):
    """per-frame single-scale SSIM of (F, C, H, W) images -> (F,) fp32 (pytorch_msssim.ssim(out, gt, data_range=1,
    size_average=False)); a frame's value depends on that frame's bytes only.  Forward only (inputs are detached)."""
    _, _, ws = _mse_plus_launch("ssim_loss", "ssim", out, gt, 0.0, 1.0, False)
    return ws[:out.shape[0]].clone()


def frame_psnr(out, gt):
    """per-frame PSNR (reference utils.py:148-151): -10*log10(mean((out-gt)^2) + 1e-9)."""
    out, gt = _dev(out.detach()), _dev(gt.detach())
    frames = out.shape[0]
    flen = out.numel() // frames
    sse = torch.empty(frames, device=out.device, dtype=torch.float32)
    L.check(L.lib().nq_frame_sse(_p(out), _p(gt), _p(sse), frames, flen, _stream()), "frame_sse")
    return -10 * torch.log10(sse / flen + 1e-9)


def ms_ssim(out, gt):
    """per-frame MS-SSIM of (F, C, H, W) images in [0, 1] -> (F,) fp32 (reference utils.py:158-164:
    pytorch_msssim.ms_ssim(out, gt, data_range=1, size_average=False)): five scales, 11-tap Gaussian window (sigma 1.5),
    valid filtering, 2x2 average pooling between scales, weights (0.0448, 0.2856, 0.3001, 0.2363, 0.1333); the definition is
    spelled out at nq_ms_ssim in include/nq_hip.h.  One HIP launch per scale + a fixed-order finishing launch on the
    current stream: bit-identical from call to call, a frame's value does not depend on the other frames of the call.
    Not differentiable (inputs are detached).  ValueError when min(H, W) <= 160 (the package's assert).

    Parity with the pip package's last bits is NOT pinned: pytorch_msssim is not available where this project is built
    and tested; the tests hold this op to a float64 restatement of the definition (tests/msssim_ref.py)."""
    out, gt = _dev(out.detach(), "out"), _dev(gt.detach(), "gt")
    if out.dim() != 4 or out.shape != gt.shape:
        raise RuntimeError(f"neuroquant_amd: ms_ssim takes two (F, C, H, W) tensors of one shape, got {tuple(out.shape)} and "
                           f"{tuple(gt.shape)}")
    F_, C, H, W = out.shape
    if min(H, W) <= 160:
        raise ValueError(f"ms_ssim: the smaller side of the image must exceed (11 - 1) * 2**4 = 160, got {H} x {W}")
    res = torch.empty(F_, device=out.device, dtype=torch.float32)
    ws = torch.empty(_q("nq_ms_ssim_ws_floats", F_, C, H, W), device=out.device, dtype=torch.float32)
    L.check(L.lib().nq_ms_ssim(_p(out), _p(gt), _p(res), _p(ws), F_, C, H, W, _stream()), "ms_ssim")
    return res


def gather_frames_u8(frames_u8: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """float frames[idx] / 255 from a GPU-resident uint8 cache (reference videosets/datasets.py:19-24)."""
    if not frames_u8.is_cuda or frames_u8.dtype != torch.uint8 or not frames_u8.is_contiguous():
        raise RuntimeError("frame cache must be a contiguous uint8 GPU tensor")
    idx = idx.to(device=frames_u8.device, dtype=torch.int64).contiguous()
    n = idx.numel()
    flen = frames_u8[0].numel()
    out = torch.empty((n,) + tuple(frames_u8.shape[1:]), device=frames_u8.device, dtype=torch.float32)
    L.check(L.lib().nq_gather_frames_u8(_p(frames_u8), _p(idx), _p(out), n, flen, _stream()), "gather_frames")
    return out


# ------------------------------------------------------------------------------------------ packed bit stream
def packed_words(n: int, n_bits: int) -> int:
    """32-bit words that n levels of n_bits bits occupy (0 for n <= 0 or n_bits outside 1..8)."""
    return int(L.lib().nq_packed_words(int(n), int(n_bits)))


def _dev_as(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"neuroquant_amd: {name} must live on the GPU (no CPU fallback exists)")
    if t.dtype != dtype:
        raise RuntimeError(f"neuroquant_amd: {name} must be {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def pack_levels(levels_u8: torch.Tensor, n_bits: int) -> torch.Tensor:
    """uint8 levels (any shape, flattened) -> int32 words of the packed stream (bit order: include/nq_hip.h).
    ValueError for an empty tensor, n_bits outside 1..8 or a level that does not fit n_bits bits."""
    lv = _dev_as(levels_u8, torch.uint8, "levels").reshape(-1)
    if not 1 <= int(n_bits) <= 8 or lv.numel() == 0:
        raise ValueError(f"pack_levels: n_bits must be 1..8 and levels non-empty, got n_bits={n_bits}, {lv.numel()} levels")
    if int(lv.max()) >= 2 ** int(n_bits):
        raise ValueError(f"pack_levels: level {int(lv.max())} does not fit {n_bits} bits")
    words = torch.empty(packed_words(lv.numel(), n_bits), device=lv.device, dtype=torch.int32)
    L.check(L.lib().nq_pack_levels(_p(lv), _p(words), lv.numel(), int(n_bits), _stream()), "pack_levels")
    return words


def _dequant_scales(what, delta, zp, shape):
    """delta / zero_point of a dequantising decode on the GPU, checked against `shape`: one value per shape[0] (channel-wise) or
    a single value -> (delta, zp, shape as a tuple of ints)"""
    delta, zp = _dev(delta, "delta"), _dev(zp, "zero_point")
    shape = tuple(int(s) for s in shape)
    if delta.numel() != zp.numel() or delta.numel() not in (1, shape[0]):
        raise ValueError(f"{what}: delta / zero_point must hold one value per output channel or a single value")
    return delta, zp, shape


def unpack_dequant(words: torch.Tensor, delta: torch.Tensor, zp: torch.Tensor, shape, n_bits: int) -> torch.Tensor:
    """packed words -> fp32 tensor of `shape`: (level - zp) * delta, the quantisers' own expression.  delta / zp hold one value
    per shape[0] (channel-wise) or a single value."""
    words = _dev_as(words, torch.int32, "words")
    delta, zp, shape = _dequant_scales("unpack_dequant", delta, zp, shape)
    n = math.prod(shape)
    if not 1 <= int(n_bits) <= 8 or n <= 0:
        raise ValueError(f"unpack_dequant: n_bits must be 1..8 and the shape non-empty, got n_bits={n_bits}, shape {shape}")
    if words.numel() < packed_words(n, n_bits):
        raise ValueError(f"unpack_dequant: {words.numel()} words cannot hold {n} levels of {n_bits} bits")
    rows = delta.numel()
    w = torch.empty(shape, device=words.device, dtype=torch.float32)
    L.check(L.lib().nq_unpack_dequant(_p(words), _p(delta), _p(zp), _p(w), rows, n // rows, int(n_bits), _stream()),
            "unpack_dequant")
    return w


def frames_to_u8(x: torch.Tensor, layout: str = "chw") -> torch.Tensor:
    """(n, C, H, W) fp32 -> uint8 round(clamp(x, 0, 1) * 255) (nearest even, NaN -> 0): (n, C, H, W) for layout 'chw',
    (n, H, W, C) for 'hwc' (what image writers take)."""
    if layout not in ("chw", "hwc"):
        raise ValueError(f"frames_to_u8: layout must be 'chw' or 'hwc', got {layout!r}")
    x = _dev(x.detach(), "x")
    if x.dim() != 4 or x.numel() == 0:
        raise ValueError(f"frames_to_u8 takes a non-empty (n, C, H, W) tensor, got {tuple(x.shape)}")
    n, C, H, W = x.shape
    out = torch.empty((n, C, H, W) if layout == "chw" else (n, H, W, C), device=x.device, dtype=torch.uint8)
    L.check(L.lib().nq_frames_to_u8(_p(x), _p(out), n, C, H * W, 0 if layout == "chw" else 1, _stream()), "frames_to_u8")
    return out


# ------------------------------------------------------------------------------------------ 8-bit YUV 4:2:0 frames
YUV_MATRICES = {"bt601": 0, "bt709": 1}


def yuv420_frame_bytes(H: int, W: int) -> int:
    """bytes of one I420 frame, H * W * 3 / 2 (0 for non-positive or odd sizes)."""
    return int(L.lib().nq_yuv420_frame_bytes(int(H), int(W)))


def _yuv_args(what, H, W, matrix, full_range=False):
    """-> (frame bytes, matrix code, range code); ValueError naming `what` for odd / non-positive sizes or an unknown matrix"""
    if matrix not in YUV_MATRICES:
        raise ValueError(f"{what}: matrix must be one of {sorted(YUV_MATRICES)}, got {matrix!r}")
    H, W = int(H), int(W)
    fb = H * W * 3 // 2 if H > 0 and W > 0 and not (H | W) & 1 else 0    # nq_yuv420_frame_bytes, without the call
    if fb <= 0:
        raise ValueError(f"{what}: 4:2:0 frames need positive even H and W, got {H} x {W}")
    return fb, YUV_MATRICES[matrix], 1 if full_range else 0


def _yuv_frames(what, buf, fb, H, W):
    """a (n, frame bytes) uint8 tensor (one frame may come flat) -> (n, frame bytes); ValueError otherwise"""
    if not isinstance(buf, torch.Tensor) or buf.dtype != torch.uint8:
        raise ValueError(f"{what} takes uint8 I420 frames, got {getattr(buf, 'dtype', type(buf))}")
    if buf.dim() == 1:
        buf = buf[None]
    if buf.dim() != 2 or buf.shape[0] == 0 or buf.shape[1] != fb:
        raise ValueError(f"{what}: {H} x {W} frames are (n, {fb}) bytes, got {tuple(buf.shape)}")
    return buf


def frames_to_yuv420(x: torch.Tensor, matrix: str = "bt709", full_range: bool = False) -> torch.Tensor:
    """(n, 3, H, W) fp32 RGB -> uint8 (n, H * W * 3 / 2): I420 frames (Y, U, V planes), the payload of a .y4m / .yuv frame.
    NaN -> 0 and clamp to [0, 1] as frames_to_u8; chroma is the mean of each 2 x 2 block; one rounding (include/nq_hip.h)."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or x.shape[0] == 0:
        raise ValueError("frames_to_yuv420 takes a non-empty (n, 3, H, W) float32 tensor, got "
                         f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}")
    n, _, H, W = x.shape
    fb, m, fr = _yuv_args("frames_to_yuv420", H, W, matrix, full_range)
    x = _dev(x.detach(), "x")
    out = torch.empty((n, fb), device=x.device, dtype=torch.uint8)
    L.check(L.lib().nq_frames_to_yuv420(_p(x), _p(out), n, H, W, m, fr, _stream()), "frames_to_yuv420")
    return out


def yuv420_to_rgb_u8(buf: torch.Tensor, H: int, W: int, matrix: str = "bt709", full_range: bool = False) -> torch.Tensor:
    """uint8 I420 frames (n, H * W * 3 / 2) -> uint8 (n, 3, H, W) planar RGB; each chroma sample serves its 2 x 2 block."""
    fb, m, fr = _yuv_args("yuv420_to_rgb_u8", H, W, matrix, full_range)
    buf = _dev_as(_yuv_frames("yuv420_to_rgb_u8", buf, fb, H, W), torch.uint8, "frames")
    n = buf.shape[0]
    out = torch.empty((n, 3, int(H), int(W)), device=buf.device, dtype=torch.uint8)
    L.check(L.lib().nq_yuv420_to_rgb_u8(_p(buf), _p(out), n, int(H), int(W), m, fr, _stream()), "yuv420_to_rgb_u8")
    return out


def yuv420_sse(a: torch.Tensor, b: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """exact sums of squared code differences of two sets of I420 frames -> int64 (n, 3): per frame, planes Y, U, V."""
    fb, _, _ = _yuv_args("yuv420_sse", H, W, "bt709")
    a, b = _yuv_frames("yuv420_sse", a, fb, H, W), _yuv_frames("yuv420_sse", b, fb, H, W)
    if a.shape != b.shape or a.device != b.device:
        raise ValueError(f"yuv420_sse: the two sets of frames differ: {tuple(a.shape)} and {tuple(b.shape)}")
    a, b = _dev_as(a, torch.uint8, "frames"), _dev_as(b, torch.uint8, "frames")
    n = a.shape[0]
    sse = torch.empty((n, 3), device=a.device, dtype=torch.int64)   # sums stay far below 2^63: the bytes of a uint64 (n, 3)
    L.check(L.lib().nq_yuv420_sse(_p(a), _p(b), _p(sse), n, int(H), int(W), _stream()), "yuv420_sse")
    return sse


def yuv420_psnr(a: torch.Tensor, b: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """PSNR of the 8-bit Y, U and V planes -> float64 (n, 3): 10 log10(255^2 * plane_pixels / sse), inf where sse = 0."""
    sse = yuv420_sse(a, b, H, W).double()
    px = torch.tensor([H * W, H * W // 4, H * W // 4], device=sse.device, dtype=torch.float64)
    return 10.0 * torch.log10(255.0 ** 2 * px / sse)


# ------------------------------------------------------------------------------------------ entropy-coded levels (rANS)
def rans_chunks(n: int, chunk: int) -> int:
    """chunks a tensor of n levels is cut into (0 for n <= 0, chunk <= 0 or chunk not a multiple of 64)."""
    return int(L.lib().nq_rans_chunks(int(n), int(chunk)))


def _rans_args(words, states, offsets, freq, n, n_bits, chunk, trusted, what):
    """The four coded arrays as the kernel takes them: 16-bit words and frequencies travel as int16, 32-bit states and offsets
    as int32 (the bit patterns of the file's u16 / u32).  Sizes are checked here; unless `trusted` (the caller has validated
    the offsets on the host, as the player does) the offsets are checked on the device, which costs one synchronisation:
    the kernel bounds a chunk's reads by its own offsets, so they must lie inside `words`."""
    words, freq = _dev_as(words, torch.int16, "words").reshape(-1), _dev_as(freq, torch.int16, "freq").reshape(-1)
    states, offsets = _dev_as(states, torch.int32, "states").reshape(-1), _dev_as(offsets, torch.int32, "offsets").reshape(-1)
    chunks = rans_chunks(n, chunk) if 1 <= int(n_bits) <= 8 else 0
    if chunks <= 0:
        raise ValueError(f"{what}: need n > 0, n_bits in 1..8 and chunk a positive multiple of 64, got n={n}, n_bits={n_bits}, "
                         f"chunk={chunk}")
    if freq.numel() != 2 ** int(n_bits) or states.numel() != 64 * chunks or offsets.numel() != chunks + 1:
        raise ValueError(f"{what}: {chunks} chunks of {n_bits}-bit levels need {2 ** int(n_bits)} frequencies, {64 * chunks} states "
                         f"and {chunks + 1} offsets, got {freq.numel()}, {states.numel()} and {offsets.numel()}")
    if not trusted:
        o = offsets.long() & 0xFFFFFFFF
        if int(o[0]) != 0 or int(o[-1]) != words.numel() or bool((o[1:] < o[:-1]).any()):
            raise ValueError(f"{what}: offsets must start at 0, never decrease and end at the number of words ({words.numel()})")
    if words.numel() == 0:   # a constant tensor costs no word; the entry still wants a pointer
        words = torch.zeros(1, device=states.device, dtype=torch.int16)
    return words, states, offsets, freq


def rans_decode(words, states, offsets, freq, n: int, n_bits: int, chunk: int, trusted: bool = False) -> torch.Tensor:
    """rANS-coded levels (bitstream.rans_encode writes them) -> n uint8 levels."""
    words, states, offsets, freq = _rans_args(words, states, offsets, freq, n, n_bits, chunk, trusted, "rans_decode")
    lv = torch.empty(int(n), device=states.device, dtype=torch.uint8)
    L.check(L.lib().nq_rans_decode(_p(words), _p(states), _p(offsets), _p(freq), int(n), int(n_bits), int(chunk), None, None, 1,
                                   _p(lv), None, _stream()), "rans_decode")
    return lv


def rans_decode_dequant(words, states, offsets, freq, delta: torch.Tensor, zp: torch.Tensor, shape, n_bits: int, chunk: int,
                        trusted: bool = False) -> torch.Tensor:
    """rANS-coded levels -> fp32 tensor of `shape`: (level - zp) * delta, bit-identical to `unpack_dequant` of the same levels.
    delta / zp hold one value per shape[0] or a single value."""
    delta, zp, shape = _dequant_scales("rans_decode_dequant", delta, zp, shape)
    n = math.prod(shape)
    words, states, offsets, freq = _rans_args(words, states, offsets, freq, n, n_bits, chunk, trusted, "rans_decode_dequant")
    w = torch.empty(shape, device=states.device, dtype=torch.float32)
    L.check(L.lib().nq_rans_decode(_p(words), _p(states), _p(offsets), _p(freq), n, int(n_bits), int(chunk), _p(delta), _p(zp),
                                   n // delta.numel(), None, _p(w), _stream()), "rans_decode_dequant")
    return w


# ------------------------------------------------------------------------------------------ quantised embeddings
def _embed_args(what, shape, delta, zp, n_bits, temporal):
    shape = tuple(int(s) for s in shape)
    if len(shape) != 4 or min(shape) <= 0:
        raise ValueError(f"{what} takes non-empty (N, C, h, w) embeddings, got shape {shape}")
    if not 2 <= int(n_bits) <= 8:
        raise ValueError(f"{what}: n_bits must be 2..8, got {n_bits}")
    delta, zp = _dev(delta, "delta").reshape(-1), _dev(zp, "zero_point").reshape(-1)
    if delta.numel() != shape[1] or zp.numel() != shape[1]:
        raise ValueError(f"{what}: delta / zero_point must hold one value per embedding channel ({shape[1]}), got "
                         f"{delta.numel()} / {zp.numel()}")
    return shape, delta, zp, int(n_bits), int(bool(temporal))


def embed_symbols(x: torch.Tensor, delta: torch.Tensor, zp: torch.Tensor, n_bits: int, temporal: bool):
    """(N, C, h, w) fp32 embeddings -> (levels, symbols), uint8 (N, C*h*w) each: level = clamp(rint(x / delta[c]) + zp[c], 0,
    2^n_bits - 1) with one delta / zp per channel (the UAQ element); symbols are the levels, or (temporal) frame 0's levels and
    the differences to the previous frame's modulo 2^n_bits.  One launch."""
    x = _dev(x.detach(), "x")
    (N, C, h, w), delta, zp, n_bits, temporal = _embed_args("embed_symbols", x.shape, delta, zp, n_bits, temporal)
    levels = torch.empty((N, C * h * w), device=x.device, dtype=torch.uint8)
    symbols = torch.empty_like(levels)
    L.check(L.lib().nq_embed_symbols(_p(x), _p(delta), _p(zp), N, C, h * w, n_bits, temporal, _p(levels), _p(symbols), _stream()),
            "embed_symbols")
    return levels, symbols


def embed_restore(symbols_f32: torch.Tensor, delta: torch.Tensor, zp: torch.Tensor, shape, n_bits: int, temporal: bool) -> torch.Tensor:
    """symbols as floats (exact integers, N * C*h*w of them: what `unpack_dequant` / `rans_decode_dequant` give with a step of
    one and a zero point of zero) -> fp32 embeddings of `shape` (N, C, h, w): the levels rebuilt frame after frame, then
    (level - zp[c]) * delta[c], the expression of `unpack_dequant`."""
    sym = _dev(symbols_f32, "symbols").reshape(-1)
    (N, C, h, w), delta, zp, n_bits, temporal = _embed_args("embed_restore", shape, delta, zp, n_bits, temporal)
    if sym.numel() != N * C * h * w:
        raise ValueError(f"embed_restore: {sym.numel()} symbols for embeddings of shape {(N, C, h, w)}")
    out = torch.empty((N, C, h, w), device=sym.device, dtype=torch.float32)
    L.check(L.lib().nq_embed_restore(_p(sym), _p(delta), _p(zp), N, C, h * w, n_bits, temporal, _p(out), _stream()), "embed_restore")
    return out


# ------------------------------------------------------------------------------------------ bit allocation
def rows_dot(V: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """out[r] = <V[r], g> for the K <= 8 rows of V, in float64 (exact products, fixed summation order: bit-identical from call
    to call).  V: (K, ...) fp32, g: fp32 with the elements of one row."""
    V, g = _dev(V.detach(), "V"), _dev(g.detach(), "g")
    K, n = (V.shape[0], g.numel()) if V.dim() else (0, 0)
    if not 1 <= K <= 8 or n < 1 or V.numel() != K * n:
        raise ValueError(f"rows_dot: V must hold 1..8 rows of g's {n} elements, got {tuple(V.shape)} against {tuple(g.shape)}")
    out = torch.empty(K, device=V.device, dtype=torch.float64)
    ws = torch.empty(_q("nq_rows_dot_ws_bytes", K, n) // 8, device=V.device, dtype=torch.float64)
    L.check(L.lib().nq_rows_dot(_p(V), _p(g), _p(out), K, n, _p(ws), _stream()), "rows_dot")
    return out


def bit_search(G: torch.Tensor, size_bits: torch.Tensor, budget_bits: int):
    """Exhaustive search of the K^L allocations of an (L K) x (L K) Omega table G (float64) under sum_l size_bits[l][c_l] <=
    budget_bits (size_bits: (L, K) int64, non-negative) -> (omega, index), index = sum_l c_l K^l; (inf, None) when nothing
    fits.  Ties go to the lowest index; the sum order is the one of tests/bit_search_ref.py, so the two agree to the bit."""
    G = _dev_as(G, torch.float64, "G")
    size_bits = _dev_as(size_bits, torch.int64, "size_bits")
    if size_bits.dim() != 2 or G.dim() != 2 or G.shape[0] != G.shape[1] or G.shape[0] != size_bits.numel() or G.numel() == 0:
        raise ValueError(f"bit_search: G must be (L K, L K) for size_bits (L, K), got {tuple(G.shape)} and {tuple(size_bits.shape)}")
    n_layers, K = size_bits.shape
    budget_bits = int(budget_bits)
    if not 0 <= budget_bits < 2 ** 64 or bool((size_bits < 0).any()):
        raise ValueError("bit_search: sizes and the budget must be non-negative and below 2^64")
    ws_bytes = _q("nq_bit_search_ws_bytes", n_layers, K)
    ws = torch.empty(max(ws_bytes // 8, 1), device=G.device, dtype=torch.float64)
    omega = torch.empty(1, device=G.device, dtype=torch.float64)
    index = torch.empty(1, device=G.device, dtype=torch.int64)     # the bits of the entry's uint64
    L.check(L.lib().nq_bit_search(_p(G), _p(size_bits), n_layers, K, budget_bits, _p(omega), _p(index), _p(ws), _stream()),
            "bit_search")
    ix = int(index) & 0xFFFFFFFFFFFFFFFF
    return float(omega), (None if ix == 0xFFFFFFFFFFFFFFFF else ix)

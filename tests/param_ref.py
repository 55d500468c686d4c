"""Plain CPU restatements and input generators of the parameter-side tests (tests/test_param_side_edges.py, GPU) -- test
infrastructure, not collected, not product code.

Restatements: what oracle/nq_oracle.py lacks, in the reference's fp32 op order where the HIP kernel claims bit-exactness and
in float64 where it sums.  tests/test_param_ref_cpu.py anchors each of them (torch.optim.Adam, the recorded goldens, the
oracle), so the GPU tests do not rest on untested helpers.

Generators: every input of the GPU file that meets an AdaRound kernel (the single-tensor cases, the multi-tensor and the
fused launches) comes from here, at a fixed seed, so that the CPU file can assert the stability conditions on exactly those
inputs.  The other inputs of the GPU file (the 1 048 577-element UAQ case, the transform, the prologue, the reductions) are
drawn in the GPU file itself: their comparisons are bit-exact or plain sums, with nothing to keep away from.
The indicator terms of the quantisers are discontinuities (the clamp mask
xi in [0, qmax], the hard-sigmoid mask lin in [0, 1], the hard rounding alpha >= 0); the GPU tests never mask a mismatching
element, the generators keep every element away from the edges instead:
  * |lin| and |lin - 1| are at least LIN_MARGIN (the sigmoid differs by an ulp or two between libm and the GPU's OCML);
  * no indicator changes when alpha moves by 2 ulp either way;
  * no fp32 rounding of xi = (floor(x / delta) + h) + zp turns a move of H_ULPS in the soft target h into a jump of xi (a
    rounding tie of the same kind as rint's: with 8 bits an ulp of xi is 1.5e-5, two orders above the sigmoid's error);
  * where an Adam step follows, the two terms of d(alpha) do not cancel below 1/CANCEL of their magnitudes (Adam divides
    the gradient by its own magnitude: a gradient of rounding noise would become a step of +-lr).
rint / floor edges of x / delta get no margin on frac(x / delta), and the CPU file asserts none.  That rests on one thing
only: every kernel is handed the ORACLE's delta and zero point (the single-tensor test also compares the GPU's own scales
with them, bit for bit; the multi-tensor and fused tests do not compute scales on the GPU at all), the division is
correctly rounded on both sides, and rint(x / delta) and floor(x / delta) are each compared bit for bit and unmasked on
these very inputs (uaq_forward, the hard forward, x_quant).  A kernel whose quotient differed in the last bit next to an
edge would fail there; the toleranced comparisons reuse the same quotient.  Exact ties and exact integers are in the
inputs on purpose: the constant rows and the sentinels (a row's extremum sits on the last grid point).
"""
import math

import torch
import torch.nn.functional as F

from oracle import nq_oracle as O

GAMMA, ZETA = O.GAMMA, O.ZETA
LIN_MARGIN = 1e-5
H_ULPS = 4e-7        # more than the soft targets of the two sides differ by (the sigmoid within an ulp or two, times 1.2)
XI_JUMP = 2e-6       # a rounding of xi that turns a move of H_ULPS in h into more than this counts as a tie
CANCEL = 30.0

# tolerances of the project (tests/test_hip_parity.py: test_adaround_kernels, test_round_regulariser_kernels, test_adam_kernel)
DALPHA_RTOL, DALPHA_ATOL = 1e-5, 1e-7      # atol per unit of max|gy| * max(delta)
REG_RTOL, REG_ATOL = 2e-5, 1e-9            # atol at regulariser weight 0.01
SOFT_RTOL, SOFT_ATOL = 1e-6, 2e-6          # atol per unit of max(delta)
ALPHA0_RTOL, ALPHA0_ATOL = 2e-5, 2e-6
ADAM_RTOL, ADAM_ATOL = 1e-6, 5e-7
# Adam's moments.  The C ABI carries beta1 / beta2 as fp32 and the kernels form 1 - beta from those; torch rounds the double
# 1 - beta to fp32.  For the default betas the two differ, relative, by 2.4e-7 (0.9) and 1.29e-5 (0.999): computed below, not
# measured.  Every term of m and of v carries that factor; on top, four fp32 roundings of 6e-8 per step and side, over
# at most three steps: 1.5e-6 at worst, of which m (whose terms cancel) also gets the gradient's bound through the recursion.
BETA1_DEV = abs((1 - float(torch.tensor(0.9, dtype=torch.float32))) / (1 - 0.9) - 1) + 7.6e-7        # 1.0e-6
BETA2_DEV = abs((1 - float(torch.tensor(0.999, dtype=torch.float32))) / (1 - 0.999) - 1) + 2e-6      # 1.5e-5
SUM_RTOL = 1e-5                            # of sum |term| (the project's bar is 1e-4; the issue asks to aim an order tighter)


# ---------------------------------------------------------------------------------------------- Adam
def adam_step(p, g, m, v, lr, t, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch/optim/adam.py _single_tensor_adam (no weight decay, no amsgrad), step t >= 1, in place on fp32 tensors."""
    m.lerp_(g, 1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1, bc2 = 1 - beta1 ** t, 1 - beta2 ** t
    denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
    p.addcdiv_(m, denom, value=-(lr / bc1))


def adam_scalars(lr, t, beta1=0.9, beta2=0.999):
    """(lr / (1 - beta1^t), sqrt(1 - beta2^t)): the two per-step scalars the captured iterations read from device memory"""
    return lr / (1 - beta1 ** t), math.sqrt(1 - beta2 ** t)


# ---------------------------------------------------------------------------------------------- AdaRound pieces
def lin_of(alpha):
    return torch.sigmoid(alpha) * (ZETA - GAMMA) + GAMMA


def reg_dalpha(alpha, b, weight):
    """d/d(alpha) of weight * sum(1 - |2h - 1|^b), h = clamp(lin, 0, 1) (calib_model.py:39-47): dR/dh * h', fp32."""
    s = torch.sigmoid(alpha)
    lin = s * (ZETA - GAMMA) + GAMMA
    h = torch.clamp(lin, 0, 1)
    hp = (ZETA - GAMMA) * (s * (1 - s)) * ((lin >= 0) & (lin <= 1)).to(alpha.dtype)
    c = h - 0.5
    dRdh = -weight * (b * (c.abs() * 2).pow(b - 1)) * 2 * torch.sign(c)
    return dRdh * hp


def round_loss_terms(alpha, b):
    """the summands of the rounding regulariser (before the weight), fp32"""
    return 1 - ((O.soft_targets(alpha) - 0.5).abs() * 2).pow(b)


def dalpha_terms(x, gy, alpha, delta, zp, n_levels, reg_weight=0.0, reg_b=0.0):
    """(data term, regulariser term, bound): d(alpha) = data + regulariser; bound = what a correct kernel may differ by, element
    by element, from the project's figures applied to each term (a relative figure on the sum would be wrong where they cancel)."""
    t1 = O.adaround_dalpha(x, gy, alpha, delta, zp, n_levels)
    bound = DALPHA_RTOL * t1.abs() + DALPHA_ATOL * float(gy.abs().max()) * float(delta.max())
    if reg_weight:
        t2 = reg_dalpha(alpha, reg_b, reg_weight)
        bound = bound + REG_RTOL * t2.abs() + REG_ATOL * (reg_weight / 0.01)
    else:
        t2 = torch.zeros_like(t1)
    return t1, t2, bound


def soft_bound(y, delta):
    return SOFT_RTOL * y.abs() + SOFT_ATOL * float(delta.max())


def uaq_ddelta_terms(x, gy, delta, zp, n_levels):
    """summands of O.uaq_ddelta, fp32 (the closed form of d(sum(gy * y)) / d(delta))"""
    u = x / delta
    x_int = u.round() + zp
    inside = ((x_int >= 0) & (x_int <= n_levels - 1)).to(x.dtype)
    x_q = torch.clamp(x_int, 0, n_levels - 1)
    return gy * ((x_q - zp) - inside * u)


def uaq_dx(x, gy, delta, zp, n_levels):
    """straight-through d/dx of the UAQ fake-quant, by autograd through the oracle (round_ste, quantizer.py:53-57)"""
    xc = x.clone().requires_grad_(True)
    (O.uaq_fake_quant(xc, delta, zp, n_levels) * gy).sum().backward()
    return xc.grad


def indicators(x, alpha, delta, zp, n_levels):
    """every 0/1 term of the AdaRound forward / backward at this alpha, stacked"""
    lin = lin_of(alpha)
    h = torch.clamp(lin, 0, 1)
    xi = torch.floor(x / delta) + h + zp
    xh = torch.floor(x / delta) + (alpha >= 0).float() + zp
    return torch.stack(((xi >= 0) & (xi <= n_levels - 1), (lin >= 0) & (lin <= 1), alpha >= 0,
                        (xh >= 0) & (xh <= n_levels - 1)))


def ulp_step(a, k):
    """a moved by k ulp (k may be negative)"""
    out = a.clone()
    for _ in range(abs(k)):
        out = torch.nextafter(out, torch.full_like(out, math.inf if k > 0 else -math.inf))
    return out


def unstable(x, alpha, delta, zp, n_levels):
    """elements that violate a stability condition of the module docstring (without the Adam one)"""
    lin = lin_of(alpha)
    bad = (lin.abs() < LIN_MARGIN) | ((lin - 1).abs() < LIN_MARGIN)
    here = indicators(x, alpha, delta, zp, n_levels)
    for k in (-2, 2):
        bad |= (indicators(x, ulp_step(alpha, k), delta, zp, n_levels) != here).any(0)
    # rounding ties of the soft forward's own additions: xi = (floor(x / delta) + h) + zp is rounded to fp32 twice, and next to
    # a zero point of 128 or more an ulp of xi is 1.5e-5 -- h is then in effect rounded to that grid, and a soft target H_ULPS
    # away (an ulp or two of the sigmoid) can land on the neighbouring grid point, 50 times the difference in h
    h = torch.clamp(lin, 0, 1)
    fl = torch.floor(x / delta)
    xi = (fl + h) + zp
    for dh in (-H_ULPS, H_ULPS):
        bad |= ((((fl + torch.clamp(h + dh, 0, 1)) + zp) - xi).abs() > XI_JUMP) & (h > 0) & (h < 1)
    return bad


def cancelling(t1, t2):
    g = t1 + t2
    return (g != 0) & (g.abs() * CANCEL < t1.abs() + t2.abs())


class AdaAdamRef:
    """Reference trajectory of `d(alpha) (+ regulariser gradient), then Adam on alpha` over several steps, with the bound each
    of alpha / m / v may differ by and the elements that violate a stability condition at any step."""

    def __init__(self, x, alpha, delta, zp, n_levels, lr):
        self.x, self.delta, self.zp, self.nl, self.lr = x, delta, zp, n_levels, lr
        self.alpha = alpha.clone()
        self.m, self.v = torch.zeros_like(alpha), torch.zeros_like(alpha)
        self.bm, self.bv = torch.zeros_like(alpha), torch.zeros_like(alpha)
        self.t = 0
        self.bad = torch.zeros(alpha.shape, dtype=torch.bool)

    def step(self, g_t, reg_weight, reg_b):
        """g_t: the gradient that meets alpha (transform domain where there is a transform)"""
        self.t += 1
        self.bad |= unstable(self.x, self.alpha, self.delta, self.zp, self.nl)
        t1, t2, bg = dalpha_terms(self.x, g_t, self.alpha, self.delta, self.zp, self.nl, reg_weight, reg_b)
        self.bad |= cancelling(t1, t2)
        g = t1 + t2
        if self.t > 1:
            # alpha itself was held to Adam's tolerance after the step before, da = ADAM_RTOL |alpha| + ADAM_ATOL.  The data
            # term is proportional to s (1 - s), whose logarithmic derivative 1 - 2 s is at most 1: it moves by at most
            # da |t1|.  The regulariser term moves by up to (b - 1) * 0.6 / t per unit of alpha, ~40 where it is not
            # negligible -> 1e-4 of it covers the drift.
            bg = bg + (ADAM_RTOL * self.alpha.abs() + ADAM_ATOL) * t1.abs() + 1e-4 * t2.abs()
        self.bm = 0.9 * self.bm + 0.1 * bg
        self.bv = 0.999 * self.bv + 0.001 * (2 * g.abs() * bg + bg * bg)
        adam_step(self.alpha, g, self.m, self.v, self.lr, self.t)
        self.bm = self.bm + BETA1_DEV * self.m.abs()
        self.bv = self.bv + BETA2_DEV * self.v
        return g


# ---------------------------------------------------------------------------------------------- fused chain
def fwht_pad(g, n):
    """H of the gradient zero-padded along C_in to n (the transform is its own transpose)"""
    return O.hadamard_along_cin(F.pad(g, (0, 0, 0, 0, 0, n - g.shape[1])))


def fq_fwht_forward(x, alpha, delta, zp, n_levels, soft, c_in):
    """H(Q(x))[:, :c_in] (quant_layer.py:70-71) and the bound it may differ by: the transform's entries are +-1/sqrt(n), so
    an output is off by at most sum|error of Q| / sqrt(n) (zero for the hard rounding: Q is bit-exact, H in the oracle's order)."""
    y, _ = O.adaround_fake_quant(x, alpha, delta, zp, n_levels, soft)
    out = O.hadamard_along_cin(y)[:, :c_in].contiguous()
    if not soft:
        return out, torch.zeros_like(out)
    b = (soft_bound(y, delta).sum(1, keepdim=True) + 1e-6 * y.abs().sum(1, keepdim=True)) / math.sqrt(x.shape[1])
    return out, b.expand(-1, c_in, -1, -1)


# ---------------------------------------------------------------------------------------------- step prologue
def step_prologue(order_tab, scal_tab, step):
    return order_tab[step].clone(), scal_tab[step].clone()


def step_gather(order_tab, step, table):
    """out[t] = table[clamp(order_tab[step][t], 0, rows - 1)]"""
    return table[order_tab[step].clamp(0, table.shape[0] - 1)]


# ---------------------------------------------------------------------------------------------- reductions
def channel_sum64(x):
    """(sums, sums of magnitudes) per channel of (B, C, ...) in float64"""
    xd = x.double().flatten(2)
    return xd.sum((0, 2)), xd.abs().sum((0, 2))


def frame_sse64(out, gt):
    t = (out - gt).flatten(1)
    t = (t * t).double()
    return t.sum(1)


def l2_loss64(pred, tgt):
    """lp_loss(p = 2) (quantizer.py:66-71): sum over channels, mean over the rest -> (loss in float64 from the fp32 terms,
    its gradient with the coefficient 2 / mean_count rounded to fp32 as the kernel does)"""
    mean_count = pred.numel() // pred.shape[1]
    d = pred - tgt
    loss = (d * d).double().sum() / mean_count
    return loss, torch.tensor(2.0 / mean_count, dtype=torch.float32) * d


# ---------------------------------------------------------------------------------------------- generators
ROW_KINDS = ("random", "positive", "negative", "constant", "x20", "x1e-3")
ROW_SCALE = {"random": 1.0, "positive": 1.0, "negative": 1.0, "x20": 20.0, "x1e-3": 1e-3}
CONSTANT = 0.37
SENTINEL_LAST, SENTINEL_FIRST = 4.75, 5.5     # in units of the row's scale: beyond every random element of the row


def row_kinds(rows, row_len):
    """kind of every row: the cycle of ROW_KINDS, started at (rows + row_len) % 6 -- most shapes of the tests have two or three
    rows, and every kind has to occur at row lengths past one reduction pass (256) and past one block per row (1024)"""
    return [ROW_KINDS[(rows + row_len + r) % 6] for r in range(rows)]


def edge_rows(g, rows, row_len):
    """(rows, row_len, 1, 1) weight whose rows are of the kinds of edge_weight of tests/golden/make_golden.py (random,
    all-positive, all-negative, constant, x20, x1e-3; row_kinds() says which row is which), with a sentinel in the last element
    of every row and in the first of the next, so a row read one element off, or with its neighbour's scale, shows.

    The sentinel is of the row's own kind, so that the kind holds for the WHOLE row: +-(SENTINEL + r / 8) times the row's scale
    (the row's extremum: its min / max / delta come from it), positive in a positive row, negative in a negative one, last
    element positive and first negative in a random one; a constant row has none -- its neighbours' sentinels sit right
    beside it."""
    kinds = row_kinds(rows, row_len)
    w = torch.randn(rows, row_len, generator=g)
    for r, kind in enumerate(kinds):
        if kind == "positive":
            w[r] = w[r].abs() + 0.01
        elif kind == "negative":
            w[r] = -w[r].abs() - 0.01
        elif kind == "constant":
            w[r] = CONSTANT
        else:
            w[r] = w[r] * ROW_SCALE[kind]
    for r, kind in enumerate(kinds):
        if kind == "constant":
            continue
        if r < rows - 1:
            w[r, -1] = (-1.0 if kind == "negative" else 1.0) * ROW_SCALE[kind] * (SENTINEL_LAST + 0.125 * r)
        if r > 0:                  # after the row's last element: in a row of one element the first one is what stays
            w[r, 0] = (1.0 if kind == "positive" else -1.0) * ROW_SCALE[kind] * (SENTINEL_FIRST + 0.125 * r)
    return w.view(rows, row_len, 1, 1)


def stable_alpha(g, x, delta, zp, n_levels, spread=3.0):
    """rounding variables over the whole range (saturated both ways, and between), nudged off the edges"""
    alpha = torch.randn(x.shape, generator=g) * spread
    for _ in range(20):
        bad = unstable(x, alpha, delta, zp, n_levels)
        if not bad.any():
            return alpha
        alpha[bad] += 0.037
    raise AssertionError("stable_alpha did not converge")


def stable_ada_adam(x, alpha, delta, zp, n_levels, lr, grads, reg_weight, reg_bs):
    """alpha nudged until the whole reference trajectory (one gradient of `grads` and one reg_b per step) is stable, with
    the regulariser on and with it gated off (the two trajectories part after the first step)"""
    alpha = alpha.clone()
    for _ in range(40):
        bad = torch.zeros(alpha.shape, dtype=torch.bool)
        for rw in sorted({reg_weight, 0.0}):
            ref = AdaAdamRef(x, alpha, delta, zp, n_levels, lr)
            for g_t, rb in zip(grads, reg_bs):
                ref.step(g_t, rw, rb)
            bad |= ref.bad
        if not bad.any():
            return alpha
        alpha[bad] += 0.037
    raise AssertionError("stable_ada_adam did not converge")


def adam_case(seed=61):
    """plain Adam over the segment sizes of MULTI_SEGS: parameters and three gradients of two magnitudes each"""
    g = torch.Generator().manual_seed(seed)
    shapes = [(s[0] * s[1],) if len(s) == 2 else s for s in MULTI_SEGS]
    ps = [torch.randn(s, generator=g) for s in shapes]
    grads = [[torch.randn(s, generator=g) * (10.0 if (k + i) % 3 == 0 else 0.1) for i, s in enumerate(shapes)] for k in range(3)]
    return ps, grads


# segments of the multi-tensor launches: (rows, row_len) per-row weights, (n,) scalar-scale biases.  19 of them: the launches
# take 16 per chunk.  row_len 1..3: the division branch of the row lookup; 5..7: a row edge inside a thread's four elements;
# n = 1023 / 1024 / 1025 / 2051: the block prefix of the segments behind; both chunks hold per-row segments behind others.
MULTI_SEGS = [(5, 1), (7, 2), (9, 3), (6, 5), (6, 6), (6, 7), (3, 341), (4, 256), (5, 205), (7, 293), (1,), (37,),
              (2, 1100), (3, 4), (11, 45), (1, 63), (2, 2049), (1027,), (9, 3)]
MULTI_LR = 3e-3
MULTI_REG_W = 0.01
MULTI_REG_BS = (7.3, 4.0)


def multi_case(seed=41):
    """-> list of dicts, one per segment of MULTI_SEGS: x, delta, zp (oracle's 'max' init, fp16 round trip), n_levels, alpha
    (stable for the forward, the backward at both reg_b and the two Adam steps), two gradients, soft flag, reg weight."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, seg in enumerate(MULTI_SEGS):
        nl = 2 ** (2, 4, 8, 3, 6)[i % 5]
        if len(seg) == 2:
            x = edge_rows(g, *seg)
            d0, z0 = O.scale_init_max(x, nl, True)
            rw = MULTI_REG_W
        else:
            x = torch.randn(seg, generator=g) * 0.3
            d0, z0 = O.scale_init_max(x, nl, True)       # 1-D: one scalar pair of shape (1,)
            rw = 0.0
        d, z, _ = O.adaround_init(x, d0, z0)
        gys = [torch.randn(x.shape, generator=g) * (0.5 if k == 0 else 0.2) for k in range(2)]
        alpha = stable_alpha(g, x, d, z, nl)
        alpha = stable_ada_adam(x, alpha, d, z, nl, MULTI_LR, gys, rw, MULTI_REG_BS)
        out.append(dict(x=x, d0=d0, z0=z0, d=d, z=z, nl=nl, alpha=alpha, gys=gys, soft=(i % 3) != 0, rw=rw))
    return out


# fused fake-quant + FWHT launches: (n, inner) within ops.fq_fwht_fusable, c_in in {1, n/2+1, n}
FUSED_NK = [(1, 1), (1, 9), (1, 25), (2, 1), (2, 9), (2, 25), (64, 1), (64, 9), (64, 25), (512, 1), (512, 9), (1024, 1)]


def fwht_opb(n, inner, tile=8192, cols=16):
    """outer rows per workgroup of the FWHT tile kernels (the launcher's formula, neuroquant_amd/csrc/fwht.hip)"""
    return max(1, min(tile // (n * inner), (cols + inner - 1) // inner))


def fused_shapes():
    """(c_out, n, k, c_in) of every weight segment: c_out = OPB + 1 (one full tile and a one-row tile; OPB is 1 for the long rows)"""
    shapes = []
    for n, inner in FUSED_NK:
        k = int(math.isqrt(inner))
        for c_in in sorted({1, n // 2 + 1, n} & set(range(1, n + 1))):
            shapes.append((fwht_opb(n, inner) + 1, n, k, c_in))
    return shapes


def fused_case(per_row, seed=53):
    """-> list of dicts, weight segments with a bias segment after each: transform-domain x, alpha, delta / zp (per output
    channel or one scalar), spatial gradients of two steps and their transforms; stable like multi_case."""
    g = torch.Generator().manual_seed(seed + int(per_row))
    out = []
    for i, (co, n, k, c_in) in enumerate(fused_shapes()):
        nl = 2 ** (4, 8, 2, 6)[i % 4]
        x = torch.randn(co, n, k, k, generator=g)
        d0, z0 = O.scale_init_max(x, nl, per_row)
        d, z, _ = O.adaround_init(x, d0, z0)
        gys = [torch.randn(co, c_in, k, k, generator=g) * 0.3 for _ in range(2)]
        gts = [fwht_pad(gy, n) for gy in gys]
        alpha = stable_alpha(g, x, d, z, nl)
        alpha = stable_ada_adam(x, alpha, d, z, nl, MULTI_LR, gts, MULTI_REG_W, MULTI_REG_BS)
        out.append(dict(x=x, d=d, z=z, nl=nl, alpha=alpha, gys=gys, gts=gts, n=n, c_in=c_in, soft=(i % 4) != 1, rw=MULTI_REG_W))
        bn = (1, 5, 2049)[i % 3]
        b = torch.randn(bn, generator=g) * 0.3
        bd0, bz0 = O.scale_init_max(b, nl, True)
        bd, bz, _ = O.adaround_init(b, bd0, bz0)
        bgs = [torch.randn(bn, generator=g) * 0.3 for _ in range(2)]
        ba = stable_alpha(g, b, bd, bz, nl)
        ba = stable_ada_adam(b, ba, bd, bz, nl, MULTI_LR, bgs, 0.0, MULTI_REG_BS)
        out.append(dict(x=b, d=bd, z=bz, nl=nl, alpha=ba, gys=bgs, gts=bgs, n=0, c_in=0, soft=True, rw=0.0))
    return out


# single-tensor quantiser kernels
SINGLE_SHAPES = [(1, 1), (3, 3), (2, 255), (2, 256), (3, 257), (2, 1023), (2, 1024), (3, 1025), (2, 2049), (5, 4097)]
SINGLE_BITS = (2, 4, 8)
SINGLE_REG = (0.01, 7.3)     # (weight, b)


def single_case(rows, row_len, per_row, nb):
    """inputs of one single-tensor case: x, the oracle's scales (UAQ 'max' init; after AdaRound's fp16 round trip), a gradient,
    a stable alpha"""
    g = torch.Generator().manual_seed(1000 * rows + row_len + 7 * nb + int(per_row))
    nl = 2 ** nb
    x = edge_rows(g, rows, row_len)
    d0, z0 = O.scale_init_max(x, nl, per_row)
    d, z, a0 = O.adaround_init(x, d0, z0)
    gy = torch.randn(x.shape, generator=g)
    alpha = stable_alpha(g, x, d, z, nl)
    return dict(x=x, d0=d0, z0=z0, d=d, z=z, a0=a0, gy=gy, alpha=alpha, nl=nl)

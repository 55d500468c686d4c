/* nq_hip.h -- C ABI of libnqhip.so: the MI355X (gfx950) kernels behind NeuroQuant's network-wise
 * calibration hot path.
 *
 * The reference (Eric-qi/NeuroQuant) has no FFI layer: its boundary is the Python object API of
 * quantization/{quantizer,quant_layer,quant_model,calib_model}.py and models/{HNeRV,NeRV}.py.  The Python
 * host in neuroquant_amd/ keeps that API and reaches every entry point below through ctypes on
 * torch.cuda.current_stream().  Each entry point names the reference code (file:line under
 * /root/reference) whose arithmetic it replaces.
 *
 * Conventions (all entry points):
 *   - plain C: device pointers + sizes, no torch types; fp32 tensors, contiguous, NCHW / OIHW;
 *   - no allocation, no ownership transfer, no host synchronisation: the caller passes outputs and
 *     workspaces; work is enqueued on `stream` (a hipStream_t) and the call returns immediately;
 *   - returns NQ_OK (0) or a negative NQ_ERR_* code; nothing throws across the boundary;
 *   - re-entrant from any thread and device; the only thing the library remembers is, per kernel and per device, that
 *     the >64 KB dynamic-LDS opt-in has been granted (lock-free, idempotent); pointers must be 16-byte aligned unless
 *     stated otherwise.
 *
 * "rows x row_len" tensors: a weight (C_out, C_in, k, k) is rows=C_out, row_len=C_in*k*k; a bias is
 * rows=1, row_len=C_out.  per_row=1 -> delta/zp hold one value per row (channel-wise weight),
 * per_row=0 -> one scalar for the whole tensor (bias, layer-wise weight)  (quantizer.py:129-153).
 */
#ifndef NQ_HIP_H
#define NQ_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* nq_stream_t; /* hipStream_t */

/* The library is built with -fvisibility=hidden: exactly the entry points declared in this header are exported
 * (`nm -D --defined-only libnqhip.so` == this file; checked by tests/test_cabi_cpu.py). */
#define NQ_API __attribute__((visibility("default")))

#define NQ_OK 0
#define NQ_ERR_INVALID (-1)     /* bad argument (null pointer, non power-of-two length, size <= 0 ...) */
#define NQ_ERR_UNSUPPORTED (-2) /* shape outside what the kernels are built for */
#define NQ_ERR_LAUNCH (-3)      /* HIP reported a launch error */

/* 7.  History: v4 added the fused launches marked "ABI v4" below, v5 the split {hi | lo} word interchange.  v6 only removed:
 * the *_slabs / *_fmt weight-gradient entries (now the `seg` / `fmt` arguments of nq_conv_wgrad, nq_conv_wgrad3 and
 * nq_conv_wgrad3_swapped), the GELU-on-load option of the fp32 kernels (in_gelu / x_gelu: nothing used it), and the
 * "workspace of the exchanged problem > 4 floats" idiom (now nq_conv_wgrad3_swapped_ws_floats / _supported).  v7 added nq_conv_forward3_plan. */
NQ_API int nq_abi_version(void);
NQ_API const char* nq_error_string(int code);

/* ---------------------------------------------------------------- quantiser parameter side ---- */

/* UniformAffineQuantizer.init_quantization_scale, 'max' branch (quantizer.py:127-168): per row
 * delta = max((max(x,0)-min(x,0))/(n_levels-1), 1e-8) (division in double, stored fp32),
 * zp = rint(-min/delta).  One value per row is written; a bias / layer-wise tensor is rows=1. */
NQ_API int nq_scale_init_max(const float* x, int64_t rows, int64_t row_len, int n_levels, float* delta, float* zp,
                      nq_stream_t stream);

/* UniformAffineQuantizer.init_quantization_scale, 'mse' / 'l1' / 'gaussian' (quantizer.py:170-220, 227-234).
 * THE DEFINITION, shared by the kernels (csrc/scale_init.hip), ops and the tests' restatement (tests/scale_init_ref.py).
 * A row is one output channel, or the whole tensor (rows=1); it has n = row_len elements; K = n_levels.
 *
 * Search ('mse': p = 3.5, 'l1': p = 1).  All fp32, uncontracted, IEEE division, round-half-even, unless marked double:
 *   x_max, x_min   the row's maximum and minimum (0 is NOT included, unlike 'max')
 *   candidates i = 0..9:   f_i = (float)(1.0 - i*0.05) [double inside], hi = x_max*f_i, lo = x_min*f_i,
 *                          delta_i = max((hi - lo) / (float)(K - 1), 1e-8f), zp_i = rint((-lo) / delta_i)
 *   per element:           q = clamp(rint(x / delta_i) + zp_i, 0, K - 1), xq = (q - zp_i)*delta_i, t = |x - xq|
 *   score [double]:        s_i = (sum of term) / n, term = (double)t for p = 1, pow((double)t, p) otherwise
 *   winner:                the lowest i with s_i < s_j for every earlier j, starting from 1e10 (strict <, as the reference).
 *                          A row none of whose scores is below 1e10 (a NaN or Inf in the row) has no winner: choice = -1 and
 *                          delta = zp = NaN.
 * The reference sums the scores in fp32; the double sum is this project's definition, so that the result does not depend on
 * an order of summation.
 *
 * 'gaussian', the reference's quirk kept -- the VARIANCE where a standard deviation was surely meant, so it clips hard:
 *   mu = mean, var = unbiased variance (divisor n - 1), two passes (the mean, then the squared deviations from the unrounded
 *   mean), accumulated in double, each rounded once to fp32;  x_min = min(mu - 6*var, 0), x_max = max(mu + 6*var, 0),
 *   delta = max((x_max - x_min) / (float)(K - 1), 1e-8f), zp = rint((-x_min) / delta).  A row of one element has no variance:
 *   NaN, as in the reference.
 *
 * delta, zp: rows floats.  choice: rows int32.  scores (may be NULL): rows x 10 doubles.  stats (may be NULL): rows x {mu, var}.
 * ws: at least nq_scale_init_ws_bytes(rows, row_len) bytes, 8-byte aligned; that query returns NQ_ERR_INVALID for sizes the
 * entries refuse.  2 <= n_levels <= 65536, p finite and > 0.  The launch plan depends on (rows, row_len) only and nothing is
 * accumulated atomically: two calls on the same data give the same bits.  One launch for rows of up to 8192 elements (x read
 * once), three for longer rows, which are cut into pieces of 8192 elements (x read twice). */
NQ_API int64_t nq_scale_init_ws_bytes(int64_t rows, int64_t row_len);
NQ_API int nq_scale_init_search(const float* x, int64_t rows, int64_t row_len, int n_levels, double p, float* delta, float* zp,
                         int* choice, double* scores, void* ws, nq_stream_t stream);
NQ_API int nq_scale_init_gaussian(const float* x, int64_t rows, int64_t row_len, int n_levels, float* delta, float* zp, float* stats,
                           void* ws, nq_stream_t stream);

/* UniformAffineQuantizer.forward (quantizer.py:117-119): y = (clamp(rint(x/delta)+zp, 0, L-1) - zp)*delta. */
NQ_API int nq_uaq_forward(const float* x, const float* delta, const float* zp, float* y, int64_t rows, int64_t row_len,
                   int per_row, int n_levels, nq_stream_t stream);

/* Backward of the above (round_ste, quantizer.py:53-57): ddelta[row] = sum gy*((xq-zp) -
 * 1{0<=rint(x/delta)+zp<=L-1} * x/delta), overwritten (rows values, or 1 if !per_row); dx (may be NULL; same shape as x)
 * = gy * 1{0<=rint(x/delta)+zp<=L-1}, the straight-through gradient w.r.t. the quantiser input. */
NQ_API int nq_uaq_backward(const float* x, const float* gy, const float* delta, const float* zp, float* ddelta, float* dx,
                    int64_t rows, int64_t row_len, int per_row, int n_levels, nq_stream_t stream);

/* AdaRoundQuantizer.__init__/init_alpha (quantizer.py:264-265, 305-314): delta/zp through an fp16 round
 * trip, alpha = -log((zeta-gamma)/(frac(x/delta)-gamma) - 1).  delta_out/zp_out have the size of delta_in. */
NQ_API int nq_adaround_init(const float* x, const float* delta_in, const float* zp_in, float* delta_out, float* zp_out,
                     float* alpha, int64_t rows, int64_t row_len, int per_row, nq_stream_t stream);

/* AdaRoundQuantizer.forward 'learned_hard_sigmoid' (quantizer.py:288-300): soft!=0 -> floor(x/delta)+h(alpha),
 * else floor(x/delta)+1{alpha>=0}; xq (may be NULL) receives the clamped integer grid value x_quant. */
NQ_API int nq_adaround_forward(const float* x, const float* alpha, const float* delta, const float* zp, float* y, float* xq,
                        int64_t rows, int64_t row_len, int per_row, int n_levels, int soft, nq_stream_t stream);

/* d/dalpha of the soft forward, plus (reg_weight != 0) the gradient of the rounding regulariser
 * reg_weight * sum(1 - |2h(alpha)-1|^reg_b) (calib_model.py:39-47).  dalpha is overwritten. */
NQ_API int nq_adaround_backward(const float* x, const float* gy, const float* alpha, const float* delta, const float* zp,
                         float* dalpha, int64_t rows, int64_t row_len, int per_row, int n_levels, float reg_weight,
                         float reg_b, nq_stream_t stream);

/* Value of the regulariser over one alpha tensor: out[0] (+)= weight*sum(1-|2h-1|^b) (calib_model.py:45).
 * ws: >= nq_reduce_ws_floats(n) floats of scratch; accumulate!=0 adds to out[0]. Deterministic. */
NQ_API int64_t nq_reduce_ws_floats(int64_t n);
NQ_API int nq_round_loss(const float* alpha, int64_t n, float b, float weight, float* ws, float* out, int accumulate,
                  nq_stream_t stream);

/* Gradient of the regulariser alone: dalpha (+)= gscale[0] * weight * d/dalpha sum(1-|2h-1|^b); gscale is a
 * device scalar (the upstream gradient of the loss term) or NULL for 1. */
NQ_API int nq_round_loss_backward(const float* alpha, int64_t n, float b, float weight, const float* gscale, float* dalpha,
                           int accumulate, nq_stream_t stream);

/* torch.optim.Adam single-tensor step, no weight decay / amsgrad (used by calib_model.py:134, 195):
 * m += (g-m)*(1-beta1); v = v*beta2 + (1-beta2)*g*g; p -= step_size * m / (sqrt(v)/bc2_sqrt + eps),
 * step_size = lr/(1-beta1^t), bc2_sqrt = sqrt(1-beta2^t) computed by the host in double. */
NQ_API int nq_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float step_size, float beta1, float beta2,
                 float eps, float bc2_sqrt, nq_stream_t stream);

/* ---- multi-tensor variants: ONE launch for all layers (the per-iteration parameter side is 14 small tensors; 42
 * launch-bound kernels become 3).  `segs` is a HOST array (copied into the kernel arguments, <= 16 segments per launch,
 * longer lists are chunked); every pointer inside is a device pointer.  The single-tensor entry points above are
 * one-segment launches of the same kernels. */
typedef struct nq_ada_seg {
  const float* x;      /* weights (rows x row_len) */
  const float* gy;     /* backward only: gradient w.r.t. the fake-quantised output */
  const float* alpha;
  const float* delta;  /* (rows) when per_row, else (1) */
  const float* zp;
  float* out;          /* forward: fake-quantised weights; backward: d(alpha) (+ regulariser gradient) */
  int64_t rows, row_len;
  int per_row, n_levels, soft; /* soft = soft_targets (forward only) */
  float reg_weight;    /* backward only: regulariser weight lambda, 0 = none (bias quantisers, warm-up) */
} nq_ada_seg;
typedef struct nq_adam_seg {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
} nq_adam_seg;
/* d(alpha) (+ regulariser gradient where reg_weight != 0) and torch.optim.Adam's update of alpha in ONE pass over the
 * rounding variables (calib_model.py:170-226: loss.backward(); optimizer.step()): per element the arithmetic of
 * nq_adaround_backward_multi followed by nq_adam_step_multi, d(alpha) is never stored; alpha, m, v are updated in place and
 * bit-identical to the two launches.  dyn != NULL: {reg_b, regulariser gate, lr/(1-beta1^t), sqrt(1-beta2^t)} are read from
 * that device array (nq_step_prologue) instead of the host arguments. */
typedef struct nq_ada_adam_seg {
  const float* x;
  const float* gy;
  float* alpha;
  const float* delta;
  const float* zp;
  float* m;
  float* v;
  int64_t rows, row_len;
  int per_row, n_levels;
  float reg_weight;
} nq_ada_adam_seg;
NQ_API int nq_adaround_adam_multi(const nq_ada_adam_seg* segs, int nseg, float reg_b, float step_size, float beta1, float beta2, float eps,
                           float bc2_sqrt, const float* dyn, nq_stream_t stream);
NQ_API int nq_adaround_forward_multi(const nq_ada_seg* segs, int nseg, nq_stream_t stream);
/* The UAQ fake-quant (nq_uaq_forward) / its d(delta) (nq_uaq_backward without dx) for several tensors in one launch:
 * phase 1 of the calibration (calib_model.py:119-165).  Uses x, gy (backward), delta, zp, out (forward: y; backward:
 * d(delta), one value per reduction row), rows, row_len, per_row, n_levels of nq_ada_seg; alpha / soft / reg_weight are
 * ignored.  nq_uaq_forward / nq_uaq_backward are one-segment launches of the same kernels. */
NQ_API int nq_uaq_forward_multi(const nq_ada_seg* segs, int nseg, nq_stream_t stream);
NQ_API int nq_uaq_backward_multi(const nq_ada_seg* segs, int nseg, nq_stream_t stream);
NQ_API int nq_adaround_backward_multi(const nq_ada_seg* segs, int nseg, float reg_b, nq_stream_t stream);
NQ_API int nq_adam_step_multi(const nq_adam_seg* segs, int nseg, float step_size, float beta1, float beta2, float eps,
                       float bc2_sqrt, nq_stream_t stream);

/* ---- captured iterations (hipGraph): what changes from one calibration iteration to the next is the batch (frame
 * indices), the temperature b / regulariser gate (LinearTempDecay + warm-up, calib_model.py:62-81) and Adam's two bias
 * corrections.  The host writes them for a whole epoch into device tables once; nq_step_prologue copies row *step into
 * fixed slots (cur_idx: B int64 frame indices; cur_scal: nscal floats) and increments *step, and the _dyn variants read
 * their scalars from cur_scal = {reg_b, regulariser gate (0 or 1), lr/(1-beta1^t), sqrt(1-beta2^t)} instead of from
 * host arguments -- same values, same arithmetic, so a replayed iteration is bit-identical to an eagerly launched one. */
NQ_API int nq_step_prologue(const int64_t* order, const float* scal, int* step, int64_t* cur_idx, float* cur_scal, int B, int nscal,
                     nq_stream_t stream);
/* The same, plus the batch's rows of a table gathered in the same launch: out[t] = table[cur_idx[t]] (row_len floats each),
 * i.e. the decoder inputs cali_data[idx] (calib_model.py:150, :201) without a separate index_select launch. */
NQ_API int nq_step_prologue_gather(const int64_t* order, const float* scal, int* step, int64_t* cur_idx, float* cur_scal, int B, int nscal,
                            const float* table, int64_t table_rows, int64_t row_len, float* out, nq_stream_t stream);
NQ_API int nq_adaround_backward_multi_dyn(const nq_ada_seg* segs, int nseg, const float* dyn, nq_stream_t stream);
NQ_API int nq_adam_step_multi_dyn(const nq_adam_seg* segs, int nseg, const float* dyn, float beta1, float beta2, float eps,
                           nq_stream_t stream);

/* Orthonormal Walsh-Hadamard transform along the middle axis (hadamard_along_channel_weight,
 * quant_layer.py:16-22, with the zero-padding of :45-49 and the slice of :71 folded in):
 * x is [outer][n_in][inner] (read as zero for index >= n_in), y is [outer][n_out][inner], transform
 * length n = 2^k <= 1024, n_in <= n, n_out <= n.  x and y must not alias. */
NQ_API int nq_fwht(const float* x, float* y, int64_t outer, int n, int64_t inner, int n_in, int n_out, nq_stream_t stream);

/* nq_fwht for several tensors in ONE launch (all layers of a decoder); `segs` is a host array, the pointers inside are
 * device pointers; fields as the arguments of nq_fwht (same arithmetic, bit-identical results). */
typedef struct nq_fwht_seg {
  const float* x;
  float* y;
  int64_t outer, inner;
  int n, n_in, n_out;
} nq_fwht_seg;
NQ_API int nq_fwht_multi(const nq_fwht_seg* segs, int nseg, nq_stream_t stream);

/* The AdaRound fake-quant fused with the transform (ABI v4; QuantModule.forward with hadamard=True, quant_layer.py:70-71, and
 * its backward + Adam, calib_model.py:170-226): one launch per direction for all layers of a decoder.
 *   nq_adaround_fwht_multi        y = H(Q(x))[:, :c_in] per weight tensor (x, alpha: (outer, n, inner) transform-domain weight and
 *                                 its rounding variables; y: (outer, c_in, inner)); a segment with n == 0 is a plain tensor
 *                                 (a bias: y = Q(x), outer * inner elements, one scalar delta / zp)
 *   nq_fwht_adaround_adam_multi   g = H(pad(gy)) (gy: (outer, c_in, inner)), then d(alpha) (+ regulariser gradient, reg_weight)
 *                                 and Adam's update of alpha / m / v in place; scalars and `dyn` as nq_adaround_adam_multi
 * Bit-identical to nq_adaround_forward_multi + nq_fwht_multi and to nq_fwht_multi + nq_adaround_adam_multi (same butterflies,
 * same per-element arithmetic); the transform-domain tensors no longer cross HBM between the two.  Rows with n * inner >
 * 8192 are NQ_ERR_UNSUPPORTED (callers use the separate launches). */
typedef struct nq_fq_fwht_seg {
  const float* x;
  float* alpha;
  const float* delta;
  const float* zp;
  float* m;          /* backward only */
  float* v;
  const float* gy;   /* backward only */
  float* y;          /* forward only */
  int64_t outer, inner;
  int n, c_in, per_row, n_levels, soft;
  float reg_weight;
} nq_fq_fwht_seg;
NQ_API int nq_adaround_fwht_multi(const nq_fq_fwht_seg* segs, int nseg, nq_stream_t stream);
NQ_API int nq_fwht_adaround_adam_multi(const nq_fq_fwht_seg* segs, int nseg, float reg_b, float step_size, float beta1, float beta2,
                                float eps, float bc2_sqrt, const float* dyn, nq_stream_t stream);

/* ---------------------------------------------------------------- convolution side ------------ */

/* Re-layout an OIHW weight (Cout,Cin,k,k) into the two GEMM operands the conv kernels read:
 *   wt_fwd [krows_fwd][ld_fwd]: row (ci*k+kh)*k+kw, column co            (forward)
 *   wt_bwd [krows_bwd][ld_bwd]: row (co*k+kh)*k+kw, column ci, taps flipped (data gradient)
 * rows/columns beyond the real extents are written as zero.  Either output may be NULL. */
NQ_API int nq_weight_layouts(const float* w, float* wt_fwd, float* wt_bwd, int Cout, int Cin, int k, int krows_fwd,
                      int ld_fwd, int krows_bwd, int ld_bwd, nq_stream_t stream);

/* nq_weight_layouts for several layers in ONE launch (the per-layer form is launch-bound); `segs` is a host array, the
 * pointers inside are device pointers; wt_fwd / wt_bwd may be NULL per segment; dims as for nq_weight_layouts. */
typedef struct nq_wl_seg {
  const float* w;
  float* wt_fwd;
  float* wt_bwd;
  int Cout, Cin, k, krows_fwd, ld_fwd, krows_bwd, ld_bwd;
} nq_wl_seg;
NQ_API int nq_weight_layouts_multi(const nq_wl_seg* segs, int nseg, nq_stream_t stream);

/* Padded operand sizes the conv kernels expect for a (Cin -> Cout, k) convolution. */
NQ_API int nq_conv_operand_dims(int Cin, int Cout, int k, int* krows, int* ld);

/* Implicit-GEMM convolution on the fp32 MFMA pipe (replaces F.conv2d in QuantModule.forward,
 * quant_layer.py:80, fused with what follows it in the decoder):
 *   stride 1, padding k/2, x (B,Cin,H,W), wt = wt_fwd layout from nq_weight_layouts, bias (Cout) or NULL.
 *   epilogue NQ_EPI_PLAIN     : y (B,Cout,H,W) = conv + bias
 *            NQ_EPI_PS_GELU   : PixelShuffle(r) + exact-erf GELU (quant_block.py:31-35, _layers.py:20-36):
 *                               with v = shuffled conv+bias, (B,Cout/r^2,H*r,W*r): y = gelu(v) and z = gelu'(v), the
 *                               derivative saved for the backward pass (one erf serves both; no backward kernel
 *                               evaluates erf/exp again)
 *            NQ_EPI_TANH      : y = tanh(conv+bias)*0.5+0.5 (OutImg, _layers.py:10-16)
 * The data gradient of a convolution is the same call with wt = wt_bwd and Cin/Cout swapped.
 * ws: scratch of >= nq_conv_forward_ws_floats(...) floats (may be NULL when that is 0): layers with few pixel
 * tiles split their K loop across workgroups; the partial sums are added in fixed order (deterministic). */
#define NQ_EPI_PLAIN 0
#define NQ_EPI_PS_GELU 1
#define NQ_EPI_TANH 2
#define NQ_EPI_PS 3         /* PixelShuffle(r) only: z = shuffled conv+bias (no activation) */
#define NQ_EPI_DGRAD_GELU 4 /* data gradient: y = conv * zprev, zprev (B,Cout,H,W) = the z a NQ_EPI_PS_GELU forward saved
                             * (= gelu' of the pre-activation), stored PixelUnshuffle(r)-ed, i.e. as the
                             * (B,Cout*r*r,H/r,W/r) output gradient of the convolution below */
/* Split {hi | lo} word interchange between the bf16x3 kernels (ABI v5; OR-ed into `epilogue`): a float v travels as one
 * 32-bit word {bf16 hi = bf16(v) in the upper half, bf16 lo = bf16(v - hi) in the lower half}, i.e. the two operands the
 * bf16x3 kernels derive from v when they stage it -- a consumer that is handed the word re-packs halves instead of converting.
 * Same bytes per element, same NCHW indexing, same results bit for bit.
 *   NQ_EPI_X_SPLIT : the input x of nq_conv_forward3 holds such words        (where nq_conv3_split_io has the bit)
 *   NQ_EPI_Y_SPLIT : the output y is written as such words (never z)         (nq_conv3_split_io / nq_conv_split_out)
 * nq_split_words converts a float tensor to that form (elementwise; for callers that feed such a kernel themselves). */
#define NQ_EPI_X_SPLIT 0x100
#define NQ_EPI_Y_SPLIT 0x200
NQ_API int nq_split_words(const float* x, float* y, int64_t n, nq_stream_t stream);
NQ_API int64_t nq_conv_forward_ws_floats(int B, int Cin, int H, int W, int Cout, int k);
/* 1 when nq_conv_forward can write y as split words (NQ_EPI_Y_SPLIT) for this call: the streaming data gradient of the head */
NQ_API int nq_conv_split_out(int B, int Cin, int H, int W, int Cout, int k, int r, int epilogue, int has_bias);
NQ_API int nq_conv_forward(const float* x, const float* wt, const float* bias, float* y, float* z, float* ws, int B, int Cin, int H,
                    int W, int Cout, int k, int krows, int ld, int r, int epilogue, const float* zprev, nq_stream_t stream);
/* The launch plan nq_conv_forward will use for this call (additive to ABI v7; pure host function): which kernel family and which
 * of its builds.  Not a second derivation: the launch, this query, nq_conv_forward_ws_floats and nq_conv_split_out read ONE
 * resolution of the call (route_fwd, csrc/conv.hip, with the head's choices resolved in csrc/conv_head.hip); the head's environment
 * knobs (NQ_HEAD_FWD, NQ_HEAD_RD, NQ_HEAD_DGRAD, NQ_HEAD_DG_R) are read per call, by the query as by the launch.  `epilogue`
 * without the split-word bits.  NQ_ERR_INVALID for whatever arguments nq_conv_forward rejects as invalid by their values (sizes,
 * epilogue, r) or out == NULL, NQ_ERR_UNSUPPORTED for k outside {1,3,5}, B > 65535 or a knob that names a build that is not compiled. */
#define NQ_CONV_IGEMM 1          /* conv_igemm: 4 x 32-pixel tiles x 16*mi channels per workgroup, fp32 MFMA */
#define NQ_CONV_TINY 2           /* tiny_pw_fwd: 1x1 over <= 256 pixels, a thread (or ksl threads) per output */
#define NQ_CONV_HEAD_FWD 3       /* head_fwd2: streaming head forward (3x3, 3 channels, W % 4 == 0) */
#define NQ_CONV_HEAD_FWD_LDS 4   /* head_fwd: LDS-staged head forward (<= 4 output channels) */
#define NQ_CONV_HEAD_DGRAD 5     /* head_dgrad2: streaming head data gradient (3x3, 3 channels, r == 2) */
#define NQ_CONV_HEAD_DGRAD_LDS 6 /* head_dgrad: LDS-staged head data gradient (<= 4 input channels, no bias) */
typedef struct nq_conv_plan {
  int kernel;     /* NQ_CONV_* */
  int mi;         /* implicit GEMM: 16*mi = channel tile; 0 for the other families, like the next three */
  int ncg;        /* channel groups of its K loop: Cin / CI rounded up, CI = 16 / 8 / 4 for k = 1 / 3 / 5 */
  int nsplit;     /* splits of the K loop over workgroups; > 1: slabs in ws, nq_conv_splitk_finish writes y / z */
  int finish;     /* build of the finish kernel: 0 none, 1 a thread per output, 8 eight threads per output */
  int ksl;        /* tiny: threads per output; else 0 */
  int rows;       /* streaming head kernels: output rows per wave (the compiled R); else 0 */
  int hd_ks, hd_r2, hd_co, hd_px; /* LDS-staged head kernels: kernel size (both), and of head_dgrad_kernel<KS, R2, CO, PX> the rest */
  int split_out;  /* nq_conv_split_out of this call */
  int64_t ws_floats; /* nq_conv_forward_ws_floats of the shape: what ws must hold whatever the epilogue */
} nq_conv_plan;
NQ_API int nq_conv_forward_plan(int B, int Cin, int H, int W, int Cout, int k, int r, int epilogue, int has_bias, nq_conv_plan* out);

/* ---- "bf16x3" variant of nq_conv_forward: fp32-equivalent accuracy on the BF16 matrix pipe ------------------------
 * Every fp32 operand is split into bf16 hi + lo and each product formed as hi*hi + hi*lo + lo*hi with fp32
 * accumulation (v_mfma_f32_16x16x32_bf16): relative error ~2^-16 per product before accumulation, i.e. the same
 * order as the fp32 rounding noise of these K~1000 contractions; 5.3x the fp32-MFMA rate.  k in {3,5} only.
 *   nq_conv3_supported    : 1 when the shape is served by this path (enough workgroups, > 4 channels each side)
 *   nq_conv3_weight_bytes : size of the pre-split operand of a (Cin -> Cout, k) convolution
 *   nq_weight_layout3     : builds it from the OIHW weight w; transposed = 1 builds the operand of the data gradient
 *                           (then Cin/Cout are those of the gradient convolution: Cin = w's C_out, Cout = w's C_in)
 *   nq_conv_forward3      : same contract as nq_conv_forward (epilogues, zprev); ws = nq_conv_forward3_ws_floats
 *                           floats (0 -> may be NULL): deep low-resolution layers are split over channel chunks */
NQ_API int nq_conv3_supported(int B, int Cin, int H, int W, int Cout, int k);
/* bit mask NQ_EPI_X_SPLIT | NQ_EPI_Y_SPLIT: the sides of nq_conv_forward3 that may travel as split words for this shape */
NQ_API int nq_conv3_split_io(int B, int Cin, int H, int W, int Cout, int k);
NQ_API int64_t nq_conv_forward3_ws_floats(int B, int Cin, int H, int W, int Cout, int k);
NQ_API int64_t nq_conv3_weight_bytes(int Cin, int Cout, int k);
NQ_API int nq_weight_layout3(const float* w, void* wt3, int Cin, int Cout, int k, int transposed, nq_stream_t stream);
/* several operands (all layers, forward and data-gradient) in ONE launch; `segs` is a host array, pointers inside are
 * device pointers; Cin/Cout/transposed per segment as for nq_weight_layout3 */
typedef struct nq_wl3_seg {
  const float* w;
  void* wt3;
  int Cin, Cout, k, transposed;
} nq_wl3_seg;
NQ_API int nq_weight_layout3_multi(const nq_wl3_seg* segs, int nseg, nq_stream_t stream);
/* nq_weight_layout3_multi + nq_weight_layouts_multi in ONE launch (ABI v4): every operand a decoder needs per iteration, the
 * same bytes as the two calls (which it falls back to when a table does not fit one kernel-argument block). */
NQ_API int nq_weight_layouts_all(const nq_wl3_seg* segs3, int n3, const nq_wl_seg* segsf, int nf, nq_stream_t stream);
/* The launch plan nq_conv_forward3 will use for this shape (ABI v7; pure host function, the same for every epilogue): which kernel
 * and which of its builds, the split over 16-channel chunks and the LDS of the launch.  It is not a second derivation: the launch,
 * this query, nq_conv3_supported, nq_conv3_split_io and nq_conv_forward3_ws_floats all read ONE resolution of the shape
 * (route_fwd3, csrc/conv3.hip; the weight-gradient entries likewise read route_wgrad3).  Answered for every valid shape --
 * nq_conv_forward3 launches whatever it is handed -- with `supported` = nq_conv3_supported, i.e. whether callers should route
 * the shape here at all.  A few-pixel shape whose wave-private patches would need more than 160 KiB of LDS is not given to the
 * few-pixel kernel: it takes the tiled kernel (and is `supported` only where that one fills the chip).
 * NQ_ERR_INVALID for k outside {3,5}, a non-positive size or out == NULL. */
#define NQ_CONV3_TILED 1 /* conv_igemm3: 8 x 32-pixel tiles x 16*mi channels per workgroup */
#define NQ_CONV3_FLAT 2  /* conv_flat3: the pixels of all frames as one flat GEMM dimension (<= 512 pixels, W <= 32) */
typedef struct nq_conv3_plan {
  int kernel;          /* NQ_CONV3_TILED or NQ_CONV3_FLAT */
  int supported;       /* nq_conv3_supported */
  int split_io;        /* nq_conv3_split_io */
  int mi;              /* 16*mi = channel tile of the weight operand (nq_weight_layout3) and of the tiled kernel */
  int waves;           /* tiled: waves per SIMD its build is compiled for (2, or 3 for mi <= 3 on a short K loop); few-pixel: 0 */
  int flat_nw, flat_nb, flat_mi; /* few-pixel: waves, 16-pixel blocks, 16-channel blocks per workgroup; tiled: 0 */
  int nsplit;          /* splits of the K loop over workgroups; > 1: slabs in ws, nq_conv_splitk_finish writes y / z */
  int per_split;       /* 16-channel chunks per split (the last split takes what is left) */
  int tail;            /* last chunk by the channels c it holds: 0 c > 12 (a full chunk's k-steps), 3 c <= 12, 2 c <= 8, 1 c <= 4 */
  int lds_bytes;       /* dynamic LDS of the launch ... */
  int lds_bytes_dgrad; /* ... and with NQ_EPI_DGRAD_GELU (the unsplit tiled kernel with mi <= 4 transposes its tile through LDS) */
} nq_conv3_plan;
NQ_API int nq_conv_forward3_plan(int B, int Cin, int H, int W, int Cout, int k, nq_conv3_plan* out);
NQ_API int nq_conv_forward3(const float* x, const void* wt3, const float* bias, float* y, float* z, const float* zprev, float* ws, int B,
                     int Cin, int H, int W, int Cout, int k, int r, int epilogue, nq_stream_t stream);
/* ---- "levels" forward for decoded bit streams: integer weights, two BF16 MFMAs per product (additive to ABI v7) ----
 * A stored weight is W[co][..] = n[co][..] * scale[co] with n = level - zero_point an INTEGER, |n| <= 255 for 2..8 bits.  bf16
 * carries an 8-bit significand and so holds every integer up to 256 exactly: n_hi = n, n_lo = 0.  The per-channel scale commutes
 * with the sum over K, hence
 *     y[co] = scale[co] * sum_k n[co][k] * (x_hi[k] + x_lo[k]) + bias[co]
 * with the products n*x_hi and n*x_lo only (the bf16x3 term a_lo*b_hi is zero, and neither the rounding of W to hi + lo nor the
 * dropped lo*lo term exists), the scale applied once per output and the bias added after it (two roundings, not contracted).
 *   nq_conv3_levels_supported : 1 exactly where nq_conv_forward3_plan reports kernel == NQ_CONV3_TILED, supported and nsplit == 1
 *                               (the same single resolution of the shape; pure host function)
 *   nq_conv_forward3_levels   : wt = the nq_weight_layout3 operand (transposed = 0) of the OIHW tensor n -- every entry must be an
 *                               integer of magnitude <= 256, else n is NOT exact and the result is wrong --, scale (Cout);
 *                               epilogues NQ_EPI_PLAIN / PS_GELU / TANH / PS with the outputs of nq_conv_forward3, floats in and
 *                               out.  NQ_ERR_INVALID: a null x / wt / scale, a missing y / z, a non-positive size,
 *                               NQ_EPI_DGRAD_GELU.  NQ_ERR_UNSUPPORTED: k outside {3,5}, a split-word bit, B > 65535, a shape
 *                               for which nq_conv3_levels_supported is 0. */
NQ_API int nq_conv3_levels_supported(int B, int Cin, int H, int W, int Cout, int k);
NQ_API int nq_conv_forward3_levels(const float* x, const void* wt, const float* scale, const float* bias, float* y, float* z, int B,
                                   int Cin, int H, int W, int Cout, int k, int r, int epilogue, nq_stream_t stream);
/* ---- "half" forward for decoded bit streams: the same integers against HALF-PRECISION activations, one F16 MFMA per product
 * (additive to ABI v7).  An APPROXIMATION, about ten times outside the bf16x3 bounds; opt-in.
 *     y[co] = scale[co] * sum_k n[co][k] * f16(x[k]) + bias[co]
 * n is exact in IEEE half as it is in bf16 (|n| <= 256 < 2048); x is rounded ONCE to half, round-to-nearest-even; fp32
 * accumulation, scale, bias and epilogues as nq_conv_forward3_levels.
 *   nq_weight_layout3_f16       : the operand: the byte layout, slots and size (nq_conv3_weight_bytes) of nq_weight_layout3
 *                                 (transposed = 0) with the hi plane holding IEEE halves and an all-zero lo plane.  NQ_ERR_INVALID
 *                                 as nq_weight_layout3.  Every entry of w must be an integer of magnitude <= 256.
 *   nq_conv_forward3_levels_f16 : the launch; the arguments, their checks (made before any device call) and their codes are
 *                                 nq_conv_forward3_levels', plus sat_flag, one device word (NQ_ERR_INVALID when null): a finite
 *                                 activation of magnitude > 65504 is clamped to +-65504 instead of becoming an infinity and the
 *                                 launch then stores 1 to *sat_flag; it never stores 0 (the caller clears the word).  NaN and
 *                                 infinite activations pass unchanged and leave the flag alone.
 * Eligibility is exactly nq_conv3_levels_supported: there is no second query. */
NQ_API int nq_weight_layout3_f16(const float* w, void* wt, int Cin, int Cout, int k, nq_stream_t stream);
NQ_API int nq_conv_forward3_levels_f16(const float* x, const void* wt, const float* scale, const float* bias, float* y, float* z,
                                       unsigned* sat_flag, int B, int Cin, int H, int W, int Cout, int k, int r, int epilogue,
                                       nq_stream_t stream);

/* Weight + bias gradient of the same convolution: dw (Cout,Cin,k,k), db (Cout) (db may be NULL), from x (B,Cin,H,W) and
 * dy (B,Cout,H,W).  ws: scratch of >= nq_conv_wgrad_ws_floats(...) floats.  Deterministic (fixed split-K order).
 * The kernels split K over workgroups into slabs and finish with a fixed-order reduction launch.  seg == NULL: both run.
 * seg != NULL (deferred reduction): ONLY the split kernel runs and *seg describes the pending reduction (slab / dw / db
 * pointers stay owned by the caller until it ran); nq_wgrad_reduce_multi performs up to 16 pending reductions per launch,
 * each with the same summation order -- results are bit-identical to the seg == NULL call.  seg->nsplit == 0 on return:
 * the kernel wrote dw / db itself (few-pixel problems), nothing is pending.  The three entries below share this contract. */
typedef struct nq_wgr_seg {
  const float* slab;     /* [nsplit][co_pad][n_pad] */
  const float* slab_db;  /* [nsplit][co_pad] or NULL */
  float* dw;
  float* db;             /* or NULL */
  int Cout, N, co_pad, n_pad, nsplit;
  int swap_kk;           /* > 0: role-swapped problem, dw[ci][co][kk-1-tap] = R[co][ci][tap] (nq_conv_wgrad3_swapped) */
  int sg;                /* split groups per output (1, 4 or 16): fixes the summation order */
} nq_wgr_seg;
NQ_API int64_t nq_conv_wgrad_ws_floats(int B, int Cin, int H, int W, int Cout, int k);
NQ_API int nq_conv_wgrad(const float* x, const float* dy, float* dw, float* db, float* ws, int B, int Cin, int H, int W, int Cout,
                  int k, nq_wgr_seg* seg, nq_stream_t stream);
/* The launch plan nq_conv_wgrad will use for this shape (additive to ABI v7; pure host function; the launch and
 * nq_conv_wgrad_ws_floats read the same resolution, route_wgrad in csrc/conv.hip).  NQ_ERR_INVALID for a non-positive size or
 * out == NULL, NQ_ERR_UNSUPPORTED for k outside {1,3,5}. */
#define NQ_CONV_WGRAD_MFMA 1 /* conv_wgrad<mi, ni>: 16*mi channels x 64*ni columns per workgroup, K split over nsplit workgroups */
#define NQ_CONV_WGRAD_TINY 2 /* tiny_pw_wgrad: 1x1 over <= 256 pixels, a thread per weight, writes dw / db itself */
typedef struct nq_conv_wgrad_plan_t {
  int kernel;     /* NQ_CONV_WGRAD_* */
  int mi, ni;     /* the build; 0 for the tiny kernel, like the next five */
  int co_pad, n_pad; /* slab dimensions: Cout and Cin*k*k rounded up to whole tiles */
  int nsplit;     /* K splits = slabs */
  int nseg;       /* 32-pixel row segments the splits divide among themselves */
  int tiny_px8;   /* tiny: 1 where H*W % 8 == 0 (its eight-pixel loop); else 0 */
  int64_t ws_floats; /* nq_conv_wgrad_ws_floats */
} nq_conv_wgrad_plan_t;
NQ_API int nq_conv_wgrad_plan(int B, int Cin, int H, int W, int Cout, int k, nq_conv_wgrad_plan_t* out);

/* bf16x3 variant of nq_conv_wgrad, k in {3,5}: */
NQ_API int nq_conv_wgrad3_supported(int B, int Cin, int H, int W, int Cout, int k);
NQ_API int64_t nq_conv_wgrad3_ws_floats(int B, int Cin, int H, int W, int Cout, int k);   /* 4 (a token) for few-pixel shapes */
/* The launch plan nq_conv_wgrad3 will use for this shape (pure host function): MT = 16*mi channels x NT = 64*ni columns per
 * workgroup, nsplit K-splits, pc != 0 -> the 8-wave producer/consumer kernel (32-bit buffer offsets: only for operands
 * below 2 GiB), pc == 0 -> the 4-wave kernel (64-bit pointers). */
NQ_API int nq_conv_wgrad3_plan(int B, int Cin, int H, int W, int Cout, int k, int* mi, int* ni, int* nsplit, int* pc);
/* fmt != 0: operands as split {hi | lo} words (see NQ_EPI_X_SPLIT): bit 0 -- x, bit 1 -- dy, only the bits
 * nq_conv_wgrad3_split_io returns for the shape (the row-segment producer/consumer kernel; other bits: NQ_ERR_UNSUPPORTED).
 * dw is bit-identical to the float call on the un-split tensors; db sums hi + lo of every dy value (what the matrix pipe
 * sees of it). */
NQ_API int nq_conv_wgrad3_split_io(int B, int Cin, int H, int W, int Cout, int k);
NQ_API int nq_conv_wgrad3(const float* x, const float* dy, float* dw, float* db, float* ws, int B, int Cin, int H, int W, int Cout,
                   int k, int fmt, nq_wgr_seg* seg, nq_stream_t stream);
/* The same weight gradient dw (Cout,Cin,k,k) for a convolution with very FEW output channels (the 3-channel head, HNeRV.py:42)
 * by exchanged operand roles: R[ci][(co,tap)] = sum_p x[ci][p] * dy[co][p+tap] is the weight gradient of the convolution
 * dy -> x-channels and dW[co][ci][tap] = R[ci][co][k*k-1-tap]; the big tensor x is then the un-shifted GEMM operand read
 * exactly once.  No bias gradient (use nq_channel_sum on dy).  All three take the arguments of the ORIGINAL layer:
 *   nq_conv_wgrad3_swapped_ws_floats : size of ws -- the slabs of the exchanged problem's plan; 0 exactly where the launch is
 *                                      NQ_ERR_UNSUPPORTED (the few-pixel kernel owns the exchanged shape: no exchanged form)
 *   nq_conv_wgrad3_swapped_supported : 1 where callers should route here (like nq_conv3_supported, narrower than what the
 *                                      launch accepts): Cout <= 4 < Cin, Cout*k*k <= 64, the exchanged problem is
 *                                      nq_conv_wgrad3_supported and the workspace size above is not 0 */
NQ_API int64_t nq_conv_wgrad3_swapped_ws_floats(int B, int Cin, int H, int W, int Cout, int k);
NQ_API int nq_conv_wgrad3_swapped_supported(int B, int Cin, int H, int W, int Cout, int k);
NQ_API int nq_conv_wgrad3_swapped(const float* x, const float* dy, float* dw, float* ws, int B, int Cin, int H, int W, int Cout, int k,
                           nq_wgr_seg* seg, nq_stream_t stream);
NQ_API int nq_wgrad_reduce_multi(const nq_wgr_seg* segs, int nseg, nq_stream_t stream);

/* Backward of PixelShuffle(r)+GELU: dconv (B,C*r*r,H,W) = unshuffle(da * z), da and z (B,C,H*r,W*r), z = the saved
 * derivative output of a NQ_EPI_PS_GELU forward. */
NQ_API int nq_ps_gelu_backward(const float* da, const float* z, float* dconv, int B, int C, int H, int W, int r,
                        nq_stream_t stream);

/* Backward of OutImg 'tanh': dconv = dimg * 0.5 * (1 - t^2), t = 2*img - 1. */
NQ_API int nq_tanh_out_backward(const float* dimg, const float* img, float* dconv, int64_t n, nq_stream_t stream);

/* lp_loss p=2 (quantizer.py:66-71): loss[0] = sum_{b,c,h,w}(pred-tgt)^2 / (B*H*W); dpred (may be NULL) =
 * 2*(pred-tgt)/(B*H*W) * gscale.  ws: >= nq_reduce_ws_floats(n) floats.  Deterministic. */
NQ_API int nq_l2_loss(const float* pred, const float* tgt, float* loss, float* dpred, float* ws, int64_t n, int64_t mean_count,
               float gscale, nq_stream_t stream);

/* Per-channel sums of an NCHW tensor, out[c] = sum_{b,h,w} x[b][c][h][w] (bias gradient of a convolution);
 * ws: >= 512*C floats.  Deterministic. */
NQ_API int nq_channel_sum(const float* x, float* out, float* ws, int B, int C, int64_t HW, nq_stream_t stream);

/* nq_l2_loss + nq_tanh_out_backward + nq_channel_sum of a tanh-headed decoder in one pass over the image (the tail of
 * calib_model.py:219-226 for OutImg 'tanh', models/_layers.py): loss[0] as nq_l2_loss (bit-identical), dconv (B,C,H,W) =
 * [2*(pred-tgt)/(B*H*W)*gscale] * 0.5 * (1 - (2*pred-1)^2) = the gradient at the head conv's output, db[c] = sum of dconv
 * over frames and pixels (the head's bias gradient).  The target is either float frames `tgt` (B,C,H,W) or the uint8
 * frame cache `cache_u8` (N,C,H,W) with frame indices idx[B] (tgt = cache[idx]/255, videosets/datasets.py:19-24);
 * exactly one of the two is non-NULL.  ws: >= 2*nq_reduce_ws_floats(B*C*HW) floats.  NQ_ERR_UNSUPPORTED unless
 * HW % 4096 == 0 (callers then use the three separate entry points).  Deterministic. */
NQ_API int nq_l2_loss_tanh_head(const float* pred, const float* tgt, const uint8_t* cache_u8, const int64_t* idx, float* loss,
                         float* dconv, float* db, float* ws, int B, int C, int64_t HW, int64_t mean_count, float gscale,
                         nq_stream_t stream);

/* The decoder's 3-channel tanh head (HNeRV.py:42, 64-66; NeRV.py:37, 58-60; OutImg models/_layers.py:10-16) AND the loss
 * tail of nq_l2_loss_tanh_head in one pass over the image (ABI v4): y (B,3,H,W) = tanh(conv3x3(x, w) + bias) * 0.5 + 0.5 is
 * still written; loss, dconv and db as nq_l2_loss_tanh_head defines them (the same per-element arithmetic; the loss and db
 * are summed per image strip and then in strip order: deterministic, last-bit different from the chunked sums of
 * nq_l2_loss_tanh_head).  wt / ld: the fp32 forward operand of nq_weight_layouts for the (Cin -> 3, k = 3) head.
 * ws: nq_head_forward_loss_ws_floats(B, H, W) floats.  NQ_ERR_UNSUPPORTED unless W % 4 == 0, ld % 4 == 0 and x < 4 GiB
 * (callers then run nq_conv_forward + nq_l2_loss_tanh_head). */
NQ_API int64_t nq_head_forward_loss_ws_floats(int B, int H, int W);
NQ_API int nq_head_forward_loss(const float* x, const float* wt, int ld, const float* bias, float* y, const float* tgt,
                         const uint8_t* cache_u8, const int64_t* idx, float* loss, float* dconv, float* db, float* ws, int B,
                         int Cin, int H, int W, int64_t mean_count, float gscale, nq_stream_t stream);

/* Per-frame PSNR pieces (utils.py:148-151): sse[f] = sum over one frame of (out-gt)^2, frames of frame_len floats. */
NQ_API int nq_frame_sse(const float* out, const float* gt, float* sse, int64_t frames, int64_t frame_len, nq_stream_t stream);

/* Per-frame MS-SSIM (utils.py:158-164 -> pytorch_msssim.ms_ssim(X, Y, data_range=1, size_average=False); evaluated beside
 * the PSNR at calibrate_network.py:109-137): out / gt (frames, C, H, W) fp32 in [0, 1] -> msssim (frames).  Five scales; per
 * scale an 11-tap Gaussian window (sigma 1.5, float32 taps), separable, valid, along H then along W, of x, y, xx, yy, xy;
 * cs = mean((2 s12 + C2) / (s1 + s2 + C2)), ssim = mean((2 m1 m2 + C1) / (m1^2 + m2^2 + C1) * cs_map), C1 = 0.01^2, C2 = 0.03^2;
 * between scales avg_pool2d(2, 2, padding (h % 2, w % 2)) with divisor 4; result = mean over channels of
 * prod_s relu(cs_s or ssim_5) ^ (0.0448, 0.2856, 0.3001, 0.2363, 0.1333).  One launch per scale (it also writes the pooled
 * images of the next one) + one finishing launch that adds the per-workgroup partial sums in a fixed order: no atomics,
 * bit-identical from call to call and independent of the other frames of the call.  Variances are taken about a
 * per-workgroup pivot, so the last bits differ from a literal fp32 evaluation; parity with the pip package's last bits
 * is not pinned (the package is not available where this library is built and tested: the yardstick is a float64
 * restatement of the definition, tests/msssim_ref.py).  ws: nq_ms_ssim_ws_floats(frames, C, H, W) floats (the pooled
 * pyramids of both images + the partial sums; 0 for arguments nq_ms_ssim rejects).  NQ_ERR_INVALID for null pointers,
 * non-positive sizes and min(H, W) <= 160 (the package's assert), all checked before the device is touched;
 * NQ_ERR_UNSUPPORTED for frames * C > 65535. */
NQ_API int64_t nq_ms_ssim_ws_floats(int64_t frames, int C, int H, int W);
NQ_API int nq_ms_ssim(const float* out, const float* gt, float* msssim, float* ws, int64_t frames, int C, int H, int W,
               nq_stream_t stream);

/* Frame gather: dst[i] = float(src_u8[idx[i]]) / 255 for frames of frame_len bytes (videosets/datasets.py:19-24);
 * idx is a device int64 array of n entries. */
NQ_API int nq_gather_frames_u8(const uint8_t* src, const int64_t* idx, float* dst, int64_t n, int64_t frame_len,
                        nq_stream_t stream);

/* ---- twice-differentiable elementwise pieces of the decoder (ABI v4): the Omega bit-allocation criterion differentiates
 * the decoder twice (Hessian-vector products by double backward, methods/bit_assign.py:57-118, 171-217), through
 * PixelShuffle, the exact-erf GELU (models/_layers.py:20-36, 104-105) and OutImg's tanh (models/_layers.py:10-16).
 *   nq_act_dd        y[i] = f(x[i]) * (g ? g[i] : 1) * (g2 ? g2[i] : 1);  mode 0 / 1 / 2: gelu, gelu', gelu''
 *                    (gelu'' = phi(x) (2 - x^2));  mode 3 / 4 / 5: t = tanh(x): 0.5 t + 0.5, 0.5 (1 - t^2), -t (1 - t^2)
 *   nq_pixel_shuffle inverse = 0: (B, C*r*r, H, W) -> (B, C, H*r, W*r) (torch.nn.PixelShuffle); inverse = 1: the un-shuffle
 *   nq_bias_add      y[b][c][p] = (x ? x[b][c][p] : 0) + bias[c]  (the bias term of F.conv2d, quant_layer.py:80; x = NULL
 *                    broadcasts the bias: the backward of a channel sum) */
NQ_API int nq_act_dd(const float* x, const float* g, const float* g2, float* y, int64_t n, int mode, nq_stream_t stream);
NQ_API int nq_pixel_shuffle(const float* x, float* y, int B, int C, int H, int W, int r, int inverse, nq_stream_t stream);
NQ_API int nq_bias_add(const float* x, const float* bias, float* y, int B, int C, int64_t HW, nq_stream_t stream);

/* ---- packed bit stream (additions are backward compatible: nq_abi_version() stays 7) ----
 * Bit order: level i of a b-bit tensor occupies bits [i*b, (i+1)*b) of the stream; bit j of the stream is bit j % 32 of
 * 32-bit word j / 32 (words are little-endian in a file), so a level straddles two words whenever b does not divide 32.
 *   nq_packed_words   ceil(n * n_bits / 32); 0 for n <= 0 or n_bits outside 1..8.
 *   nq_pack_levels    levels (n bytes, one level each; any alignment) -> words (nq_packed_words(n, n_bits), 4-byte aligned).
 *                     A level is masked to n_bits bits; unused high bits of the last word are zero; every word has exactly
 *                     one writer (a thread packs 32 levels into n_bits words): no atomics, bit-identical from call to call.
 *   nq_unpack_dequant w[r][j] = ((float)level[r * row_len + j] - zp[r]) * delta[r], in that order, uncontracted: the expression
 *                     of nq_uaq_forward / nq_adaround_forward (quantizer.py:117-119, 300), so the weights a player rebuilds are
 *                     the quantiser's bit for bit.  rows = C_out with one delta / zp per row, rows = 1 for a layer-wise
 *                     tensor or a bias.  No word at or beyond nq_packed_words(rows * row_len, n_bits) is read.
 *   nq_frames_to_u8   dst = (uint8) rint(min(max(src, 0), 1) * 255), round to nearest even (torch.round), NaN -> 0.  src is
 *                     (n, C, HW) fp32; layout 0 writes (n, C, HW) (planar), layout 1 writes (n, HW, C) (interleaved, what
 *                     image writers take).  16-byte loads and dword stores when src is 16-byte and dst 4-byte aligned and,
 *                     for layout 1, C == 3 and HW % 4 == 0 (C == 1 is planar); otherwise one byte per thread.
 * NQ_ERR_INVALID for null pointers, non-positive sizes, n_bits outside 1..8, layout outside {0, 1} and element counts past
 * int64, all checked before the device is touched; NQ_ERR_UNSUPPORTED for more than 2^31 - 1 workgroups. */
NQ_API int64_t nq_packed_words(int64_t n, int n_bits);
NQ_API int nq_pack_levels(const uint8_t* levels, uint32_t* words, int64_t n, int n_bits, nq_stream_t stream);
NQ_API int nq_unpack_dequant(const uint32_t* words, const float* delta, const float* zp, float* w, int64_t rows, int64_t row_len,
                      int n_bits, nq_stream_t stream);
NQ_API int nq_frames_to_u8(const float* src, uint8_t* dst, int64_t n, int C, int64_t HW, int layout, nq_stream_t stream);

/* ---- 8-bit YUV 4:2:0 frames (additive: nq_abi_version() stays 7) ----
 * A frame is I420: the Y plane H x W, then U (H/2) x (W/2), then V, one byte per sample: the payload of a .y4m / .yuv frame.
 * matrix 0 is BT.601 (Kr = 0.299, Kb = 0.114), 1 is BT.709 (Kr = 0.2126, Kb = 0.0722); Kg = 1 - Kr - Kb.  full_range 0 is
 * limited ("video") range, Y in 16..235 and chroma in 16..240; 1 is full range.  All arithmetic is fp32 in the order written
 * here, uncontracted; every derived constant (icb = 1/(2(1-Kb)), icr = 1/(2(1-Kr)), c_r = 2(1-Kr), c_b = 2(1-Kb),
 * c_gb = Kb c_b / Kg, c_gr = Kr c_r / Kg, 1/219, 1/224, 1/255) is formed in double and rounded once to float.
 *   nq_yuv420_frame_bytes  H * W * 3 / 2; 0 for non-positive or odd H or W and for a product past int64.  Pure host function.
 *   nq_frames_to_yuv420    src: (n, 3, H, W) fp32 planar RGB; dst: n frames.  Per pixel NaN -> 0, then clamp to [0, 1] (the rule
 *                          of nq_frames_to_u8); y = (Kr r + Kg g) + Kb b; cb = (b - y) icb; cr = (r - y) icr.  The chroma of a
 *                          2 x 2 block is ((c00 + c01) + (c10 + c11)) * 0.25, row 0 first, left before right.  Limited range:
 *                          Y = rint(16 + 219 y), U = rint(128 + 224 cb), V likewise from cr; full range: Y = rint(255 y),
 *                          U = rint(128 + 255 cb).  Product, then sum, then round to nearest even, then clamp to [0, 255].
 *                          With W % 8 == 0, src 16-byte and dst 8-byte aligned a thread takes 2 rows x 8 columns (16-byte
 *                          loads, 8-byte Y stores, dword chroma stores); otherwise one thread per 2 x 2 block, scalar loads,
 *                          byte stores.  Every byte has one writer: bit-identical from call to call.
 *   nq_yuv420_to_rgb_u8    the inverse, for ground truth: src n frames (any byte is legal), dst uint8 (n, 3, H, W) planar.  Each
 *                          chroma sample serves its 2 x 2 block.  Limited range: y = (Y - 16) (1/219), cb = (U - 128) (1/224);
 *                          full range: y = Y (1/255), cb = (U - 128) (1/255); cr from V as cb from U.  r = y + c_r cr;
 *                          b = y + c_b cb; g = (y - c_gb cb) - c_gr cr; code = rint(min(max(., 0), 1) * 255).  Vector path
 *                          with W % 8 == 0 and both pointers 8-byte aligned.
 *   nq_yuv420_sse          a, b: n frames each; sse: uint64 (n, 3), the exact sum of squared code differences per frame and
 *                          plane (Y, U, V).  The entry zeroes sse on the stream; workgroups reduce in registers and LDS and
 *                          add one 64-bit partial per plane with a global atomic add.  Integer sums do not depend on the
 *                          order: bit-identical from call to call.  sse is 8-byte aligned.
 * NQ_ERR_INVALID, before the device is touched, for null pointers, n <= 0, non-positive or odd H or W, matrix or full_range
 * outside {0, 1} and n * H * W * 3 past int64; NQ_ERR_UNSUPPORTED for more than 2^31 - 1 workgroups. */
NQ_API int64_t nq_yuv420_frame_bytes(int64_t H, int64_t W);
NQ_API int nq_frames_to_yuv420(const float* src, uint8_t* dst, int64_t n, int H, int W, int matrix, int full_range,
                        nq_stream_t stream);
NQ_API int nq_yuv420_to_rgb_u8(const uint8_t* src, uint8_t* dst, int64_t n, int H, int W, int matrix, int full_range,
                        nq_stream_t stream);
NQ_API int nq_yuv420_sse(const uint8_t* a, const uint8_t* b, uint64_t* sse, int64_t n, int H, int W, nq_stream_t stream);

/* ---- reconstruction loss in the 8-bit YUV 4:2:0 domain (additive: nq_abi_version() stays 7) ----
 * pred, tgt: (B, 3, H, W) fp32 planar RGB, H and W even; matrix / full_range as above; weights wy, wu, wv >= 0 with a positive
 * sum.  The transform is linear, so it is applied to d = pred - tgt (offsets cancel, nothing is clamped), fp32, uncontracted:
 *   dy = (Kr d_r + Kg d_g) + Kb d_b;  dcb = (d_b - dy) icb;  dcr = (d_r - dy) icr          per pixel
 *   eY = sY dy per pixel;  eU = sC mean2x2(dcb), eV = sC mean2x2(dcr) per 2 x 2 block, the box of nq_frames_to_yuv420
 *   sY = 219/255, sC = 224/255 in limited range, both 1 in full range: errors are 8-bit code units / 255
 *   MSE_Y = sum eY^2 / (B H W);  MSE_U = sum eU^2 / (B H W / 4);  MSE_V likewise
 *   L = 3 (wy MSE_Y + wu MSE_U + wv MSE_V) / (wy + wu + wv)      (3: the scale of nq_l2_loss, a sum over three channels)
 * -10 log10(MSE_plane) is the plane PSNR of the unrounded codes nq_frames_to_yuv420 would round.
 *   loss[4] = {L, MSE_Y, MSE_U, MSE_V}.  A zero weight removes its plane from L and from the gradient exactly.
 *   Target: exactly one of `tgt` and `cache_u8` (N, 3, H, W) + idx[B] is non-NULL; tgt = cache[idx[b]] / 255, the arithmetic of
 *   nq_gather_frames_u8.
 *   db == NULL: grad (B, 3, H, W) = gscale dL/dpred, exact: a pixel receives its own luma term and a quarter of its block's two
 *   chroma terms.  db != NULL (tanh head, the contract of nq_l2_loss_tanh_head): grad = that value * 0.5 * (1 - (2 pred - 1)^2),
 *   the gradient at the head conv's output, bit-identical to nq_tanh_out_backward of the db == NULL result; db[3] = its sums over
 *   frames and pixels.
 *   ws: nq_yuv420_loss_ws_floats(B, H, W) floats (0 for arguments the entry refuses).  One streaming launch (2 rows x 4 columns
 *   per thread with 16-byte accesses when W % 4 == 0, pred / tgt / grad are 16-byte and the cache 4-byte aligned; else one thread
 *   per 2 x 2 block) + one launch that adds the workgroups' partial sums in a fixed order: no atomics, bit-identical from call
 *   to call.
 * NQ_ERR_INVALID, before the device is touched, for null pointers, both or neither target, non-positive or odd H or W, B <= 0,
 * matrix or full_range outside {0, 1}, a negative or non-finite weight, a zero weight sum and B * 3 * H * W past int64;
 * NQ_ERR_UNSUPPORTED for more than 2^31 - 1 workgroups. */
NQ_API int64_t nq_yuv420_loss_ws_floats(int B, int H, int W);
NQ_API int nq_yuv420_loss(const float* pred, const float* tgt, const uint8_t* cache_u8, const int64_t* idx, float* loss, float* grad,
                   float* db, float* ws, int B, int H, int W, int matrix, int full_range, float wy, float wu, float wv,
                   float gscale, nq_stream_t stream);

/* ---- MSE + single-scale SSIM training loss with its exact gradient (additive: nq_abi_version() stays 7) ----
 * The reference's `ssim`, `Fusion1`, `Fusion3` and `Fusion5` losses (reference utils.py:119-130): w_mse * mse + w_ssim * (1 -
 * pytorch_msssim.ssim(X, Y, data_range=1, size_average=False)) per frame, then the mean over frames.
 * X = pred, Y = tgt: (B, C, H, W) fp32, H, W >= 11.  Window g: 11 taps, sigma 1.5, taps evaluated in float32; g* filters
 * separably and valid, along H then W, each channel on its own.  C1 = 1e-4, C2 = 9e-4, no relu.  Per plane
 *   mu_x = g*X, mu_y = g*Y, Sxx = g*(X^2), Syy = g*(Y^2), Sxy = g*(XY)
 *   A1 = 2 mu_x mu_y + C1, A2 = 2 (Sxy - mu_x mu_y) + C2, B1 = mu_x^2 + mu_y^2 + C1, B2 = (Sxx - mu_x^2) + (Syy - mu_y^2) + C2
 *   S = A1 A2 / (B1 B2) on the (H - 10) x (W - 10) valid region, N = (H - 10)(W - 10);  SSIM_b = mean over channels of mean S
 *   L = mean_b [ w_mse mean_{c,h,w} (X - Y)^2 + w_ssim (1 - SSIM_b) ]
 *   loss3[3] = {L, mean MSE, mean SSIM}; after the call ws[0 .. B) holds SSIM_b of every frame.
 * Gradient, with the five moments as the independent quantities and gT* the adjoint of the valid filter (the same window
 * over the map zero-extended by 10 on every side, an H x W result):
 *   P = dS/d mu_x = 2 mu_y (A2 - A1) / (B1 B2) + 2 mu_x S (1 / B2 - 1 / B1),  Q = dS/d Sxx = -S / B2,  R = dS/d Sxy = 2 A1 / (B1 B2)
 *   dL/dX = w_mse 2 (X - Y) / (B C H W) - w_ssim / (B C N) (gT*P + 2 X gT*Q + Y gT*R)
 *   grad != NULL: grad (B, C, H, W) = grad_scale dL/dX.  grad == NULL: forward only, P, Q, R are not written.
 * Three launches: forward (S, P, Q, R and one partial sum of S and of (X - Y)^2 per workgroup; moments about a per-workgroup
 * pivot as nq_ms_ssim), backward (a gather, every gradient element has one writer), and one that adds the partial sums in a
 * fixed order in double.  No atomics: bit-identical from call to call, a frame's SSIM depends on that frame's bytes only.
 * pred == tgt gives SSIM = 1, MSE = 0 and a zero gradient exactly.
 *   ws: nq_ssim_loss_ws_floats(B, C, H, W) floats (0 for arguments the entry refuses).
 * NQ_ERR_INVALID, before the device is touched, for null pred / tgt / loss3 / ws, non-positive B or C, H or W below 11, a
 * negative or non-finite weight, a non-finite grad_scale and an element count past int64; NQ_ERR_UNSUPPORTED for B * C > 65535. */
NQ_API int64_t nq_ssim_loss_ws_floats(int B, int C, int H, int W);
NQ_API int nq_ssim_loss(const float* pred, const float* tgt, float* loss3, float* grad, float* ws, int B, int C, int H, int W,
                 float w_mse, float w_ssim, float grad_scale, nq_stream_t stream);

/* ---- the same loss as the tail of a calibration iteration (additive: nq_abi_version() stays 7) ----
 * L, MSE, SSIM and dL/dX as nq_ssim_loss defines them, with what nq_l2_loss_tanh_head and nq_yuv420_loss hand over:
 *   loss3[3] = {scale L (the float L of nq_ssim_loss times scale, one more rounding), mean MSE, mean SSIM}; ws[0 .. B) holds
 *   SSIM_b.  The calibration engine passes scale = C: weights (1, 0) then give the value and gradient of lp_loss(p = 2).
 *   Target: exactly one of `tgt` (B, C, H, W) and `cache_u8` (N, C, H, W) + idx[B] is non-NULL; tgt = cache[idx[b]] / 255, the
 *   arithmetic of nq_gather_frames_u8, converted while the forward and the backward launch stage their tiles (no float copy of
 *   the target is written).  The VALUES of idx are the caller's responsibility, as for nq_l2_loss_tanh_head and nq_yuv420_loss:
 *   they live on the device and are not read by the host (that would stop a capture), an index outside [0, N) reads outside
 *   the cache.
 *   db == NULL: grad (B, C, H, W) = scale dL/dX (grad == NULL: forward only).  With a float target every output but loss3[0]
 *   equals nq_ssim_loss(grad_scale = scale) bit for bit.
 *   db != NULL (X = tanh(conv) * 0.5 + 0.5; grad must be given): grad = that value * 0.5 * (1 - (2 X - 1)^2), the gradient at
 *   the head conv's output, bit-identical to nq_tanh_out_backward of the db == NULL result; db[C] = its sums over frames and
 *   pixels: every backward workgroup (one tile of one (frame, channel) plane) adds its results in double and stores one float,
 *   the finishing launch adds those per channel, frame by frame, in double.
 * At most three launches (forward, backward, finish: 1 + C workgroups with db), no atomics, no host read, no launch argument
 * that depends on device data: bit-identical from call to call and capturable in a hipGraph.
 *   ws: nq_ssim_loss_head_ws_floats(B, C, H, W) floats = nq_ssim_loss_ws_floats + B C ceil(H / 8) ceil(W / 118) (0 for
 *   arguments the entry refuses).
 * NQ_ERR_INVALID, before the device is touched, for what nq_ssim_loss refuses, both or neither target, a cache without idx
 * and db without grad; NQ_ERR_UNSUPPORTED for B * C > 65535. */
NQ_API int64_t nq_ssim_loss_head_ws_floats(int B, int C, int H, int W);
NQ_API int nq_ssim_loss_head(const float* pred, const float* tgt, const uint8_t* cache_u8, const int64_t* idx, float* loss3,
                      float* grad, float* db, float* ws, int B, int C, int H, int W, float w_mse, float w_ssim, float scale,
                      nq_stream_t stream);

/* ---- MSE + five-scale MS-SSIM training loss with its exact gradient (additive: nq_abi_version() stays 7) ----
 * X_1 = pred, Y_1 = tgt: (B, C, H, W) fp32, min(H, W) > 160.  Scales s = 1 .. 5 of h_s x w_s pixels:
 *   X_{s+1} = avg_pool2d(X_s, 2, 2, padding (h_s % 2, w_s % 2)), divisor 4 (the padding counts), as nq_ms_ssim; the same for Y.
 *   Window, valid separable filter g*, C1, C2, A1, A2, B1, B2 as nq_ssim_loss states them; per scale the maps
 *   cs = A2 / B2 and ssim = A1 A2 / (B1 B2) on the (h_s - 10) x (w_s - 10) valid region, N_s its pixel count.
 *   v_s(b, c) = mean cs (s = 1 .. 4), mean ssim (s = 5);  w = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
 *   M(b, c) = prod_s relu(v_s)^(w_s),  MS_b = mean_c M(b, c),  MSE_b = mean_{c,h,w} (X - Y)^2
 *   L = mean_b [ w_mse MSE_b + w_ms (1 - MS_b) ]
 *   loss3[3] = {L, mean MSE, mean MS-SSIM}; after the call ws[0 .. B) holds MS_b of every frame.
 * Gradient.  On a plane where every v_s > 0: dL/dv_s = -(w_ms / (B C)) w_s M / v_s.  With the five moments as the independent
 * quantities and gT* the adjoint of the valid filter (nq_ssim_loss), the derivative maps of scale s are
 *   s = 5: P, Q, R of nq_ssim_loss;   s < 5 (the luminance factor dropped): P = d cs / d mu_x = 2 (mu_x cs - mu_y) / B2,
 *   Q = d cs / d Sxx = -cs / B2,  R = d cs / d Sxy = 2 / B2
 *   own_s = dL/dv_s / N_s (gT*P + 2 X_s gT*Q + Y_s gT*R)
 *   G_s = own_s + up(G_{s+1}),  up(G)[i, j] = G[(i + h_s % 2) / 2, (j + w_s % 2) / 2] / 4  (the exact adjoint of the pooling)
 *   dL/dX = G_1 + w_mse 2 (X - Y) / (B C H W)
 * On a plane where some v_s <= 0 the relu is active and M = 0 exactly; the MS-SSIM part of that plane's gradient is DEFINED as
 * exactly zero at every scale (autograd through 0^w gives NaN there).
 *   grad != NULL: grad (B, C, H, W) = grad_scale dL/dX.  grad == NULL: forward only, no derivative map is written, the same
 *   loss3 bits.
 * Eleven launches (six forward only): one forward launch per scale (the next scale's pooled images, the derivative maps, one
 * partial sum per workgroup), one finishing launch (partial sums added in a fixed order in double; v_s, M, the coefficients
 * grad_scale dL/dv_s / N_s and the clamp, written to the workspace), one backward launch per scale from 5 down to 1 (a gather,
 * every element one writer).  No atomics, no host read between launches: bit-identical from call to call, capturable in a
 * hipGraph; a frame's MS_b depends on that frame's bytes only.  pred == tgt gives MS-SSIM = 1, MSE = 0 and a zero gradient exactly.
 *   ws: nq_msssim_loss_ws_floats(B, C, H, W) floats (0 for arguments the entry refuses) =
 *       B + 5 B C + B C T_1 + sum_s B C T_s + 3 sum_{s>1} B C h_s w_s + 3 sum_s B C N_s,  T_s = ceil((h_s - 10) / 8) ceil((w_s - 10) / 118).
 * NQ_ERR_INVALID, before the device is touched, for null pred / tgt / loss3 / ws, non-positive sizes, min(H, W) <= 160, a
 * negative or non-finite weight, both weights zero, a non-finite grad_scale and an element count past int64;
 * NQ_ERR_UNSUPPORTED for B * C > 65535. */
NQ_API int64_t nq_msssim_loss_ws_floats(int B, int C, int H, int W);
NQ_API int nq_msssim_loss(const float* pred, const float* tgt, float* loss3, float* grad, float* ws, int B, int C, int H, int W,
                   float w_mse, float w_ms, float grad_scale, nq_stream_t stream);

/* Entropy-coded levels: 64-lane interleaved rANS, one frequency table per tensor (probabilities in units of
 * 1 / 4096), 32-bit states >= 2^16, 16-bit words.  The n levels (flat, C order) are cut into chunks of `chunk` symbols (a
 * multiple of 64, the last may be short); lane l of a chunk owns its symbols l, l + 64, ...  One wavefront decodes one chunk.
 *   nq_rans_chunks   ceil(n / chunk); 0 for n <= 0, chunk <= 0 or chunk not a multiple of 64.  Pure host function.
 *   nq_rans_decode   words: every chunk's 16-bit words, chunk after chunk; states: 64 per chunk; offsets: chunks + 1 entries,
 *                    chunk c owns words [offsets[c], offsets[c + 1]); freq: 2^n_bits entries that sum to 4096.  Outputs, either
 *                    may be NULL but not both: levels[i] (one byte each) and w[i] = ((float)level[i] - zp[i / row_len]) *
 *                    delta[i / row_len], the expression of the unpacking entry above, so the floats equal the packed path's bit
 *                    for bit (delta / zp may be NULL when w is).  All pointers are device pointers.  A word index at or past
 *                    the chunk's own word count reads as 0 and every table lookup is in range whatever freq holds; the caller
 *                    guarantees that offsets never decrease and end at the number of words, and that words is non-NULL even
 *                    when no chunk owns a word.
 * NQ_ERR_INVALID, before the device is touched, for null pointers, n <= 0, n_bits outside 1..8, chunk <= 0 or not a multiple
 * of 64, row_len <= 0 and both outputs NULL; NQ_ERR_UNSUPPORTED for n >= 2^32 (32-bit offsets) or more than 2^31 - 1
 * workgroups. */
NQ_API int64_t nq_rans_chunks(int64_t n, int64_t chunk);
NQ_API int nq_rans_decode(const uint16_t* words, const uint32_t* states, const uint32_t* offsets, const uint16_t* freq, int64_t n,
                   int n_bits, int64_t chunk, const float* delta, const float* zp, int64_t row_len, uint8_t* levels, float* w,
                   nq_stream_t stream);

/* ---- quantised, temporally coded frame embeddings (additive: nq_abi_version() stays 7) ----
 * x is (N, C, HW) fp32: N frames, C embedding channels, HW positions, E = C * HW values per frame; delta / zp hold one value
 * per channel.  level[t][e] = clamp(rint(x[t][e] / delta[c]) + zp[c], 0, 2^n_bits - 1) with c = e / HW, in fp32 and
 * uncontracted: the level of nq_uaq_forward.  Symbols are frame-major (N, E): temporal = 0: sym[t] = level[t]; temporal = 1:
 * sym[0] = level[0], sym[t] = (level[t] - level[t - 1]) mod 2^n_bits.
 *   nq_embed_symbols  one launch, one thread per value (a thread recomputes its predecessor's level from x[t - 1]): writes
 *                     the N * E levels and the N * E symbols, one byte each.  A NaN gives level 0.
 *   nq_embed_restore  sym holds the N * E symbols as floats (exact integers: what nq_unpack_dequant / nq_rans_decode write
 *                     with a step of one and a zero point of zero); a float outside [0, 255] is clamped, then masked to
 *                     n_bits bits.  level[t] = temporal ? (level[t - 1] + sym[t]) & (2^n_bits - 1) : sym[t];
 *                     out[t][e] = ((float)level[t][e] - zp[c]) * delta[c], the expression of nq_unpack_dequant.  One thread
 *                     per column e, sequential over t.
 * NQ_ERR_INVALID, before the device is touched, for null pointers, non-positive sizes, n_bits outside 2..8 and temporal
 * outside {0, 1}; NQ_ERR_UNSUPPORTED for N * C * HW past int64 or more than 2^31 - 1 workgroups. */
NQ_API int nq_embed_symbols(const float* x, const float* delta, const float* zp, int64_t N, int64_t C, int64_t HW, int n_bits,
                     int temporal, uint8_t* levels, uint8_t* symbols, nq_stream_t stream);
NQ_API int nq_embed_restore(const float* sym, const float* delta, const float* zp, int64_t N, int64_t C, int64_t HW, int n_bits,
                     int temporal, float* out, nq_stream_t stream);

/* ---- bit allocation under a size budget (additive: nq_abi_version() stays 7) ----
 * The Omega score of an allocation is a quadratic form: with K bit choices for each of L layers, the (L K) x (L K) Gram matrix
 * G[(l,c),(m,d)] = <v_l(c), (H v_m(d))_l> of the per-layer perturbations gives Omega(b) = sum_l sum_m G[(l,b_l),(m,b_m)].
 *   nq_rows_dot     out[r] = sum_i V[r * n + i] * g[i] for r < K, 1 <= K <= 8: the K entries G[(l,.), j] from layer l's slice g of
 *                   H e_j.  Every product is formed in float64 (exact: 24 x 24 bits); the sums are float64 in a fixed order
 *                   (per-thread strided partial sums, a wave tree, one partial per workgroup in ws, a finishing launch that adds
 *                   the partials in index order): no atomics, bit-identical from call to call.  g is read once for all K rows.
 *                   ws: nq_rows_dot_ws_bytes(K, n) bytes (0 for arguments the entry refuses), 8-byte aligned.
 *   nq_bit_search   G: (L K) x (L K) row-major, row / column (l, c) at l K + c; size_bits: L x K.  A candidate is the
 *                   mixed-radix index sum_l c_l K^l (layer 0 least significant).  Over every candidate with
 *                   sum_l size_bits[l][c_l] <= budget_bits (the sum saturates at 2^64 - 1), Omega is summed from 0.0 with l
 *                   ascending in the outer and m ascending in the inner loop by plain float64 additions, and the lexicographic
 *                   minimum of (Omega, index) is kept: ties go to the lowest index, a NaN Omega is never selected.  Nothing
 *                   fits: best_index = UINT64_MAX, best_omega = +inf.  G and size_bits are staged in LDS; workgroup minima go
 *                   to ws (nq_bit_search_ws_bytes(L, K) bytes, 8-byte aligned; 0 for shapes the entry refuses), a finishing
 *                   launch reduces them.  best_omega / best_index are device pointers to one element each.
 * NQ_ERR_INVALID, before the device is touched, for null pointers, L < 1, K < 1, K > 8 and n < 1; NQ_ERR_UNSUPPORTED for L > 12,
 * K^L >= 2^32 and an (L K)^2 table past 64 KB of LDS. */
NQ_API int64_t nq_rows_dot_ws_bytes(int K, int64_t n);
NQ_API int nq_rows_dot(const float* V, const float* g, double* out, int K, int64_t n, double* ws, nq_stream_t stream);
NQ_API int64_t nq_bit_search_ws_bytes(int L, int K);
NQ_API int nq_bit_search(const double* G, const uint64_t* size_bits, int L, int K, uint64_t budget_bits, double* best_omega,
                  uint64_t* best_index, void* ws, nq_stream_t stream);

/* ---- rate-aware calibration: the entropy cost of the stored levels (additive: nq_abi_version() stays 7) ----
 * THE definition.  For a weight tensor with n = rows * row_len elements, K = n_levels (4 .. 256), per-row or scalar delta / zp,
 * everything per element in fp32 and uncontracted unless stated:
 *   f_i    = floor(x_i / delta)                              the float expression of nq_adaround_forward
 *   lo_i   = clamp((f_i + 0) + zp, 0, K - 1),  hi_i = clamp((f_i + 1) + zp, 0, K - 1)
 *   l_i    = alpha_i >= 0 ? hi_i : lo_i                      the hard level: bit for bit the xq nq_adaround_forward(soft = 0) writes
 *   c_k    = #{i : l_i = k}                                  int32
 *   cost_k = log2((n + K) / (c_k + 1)) bits                  evaluated in double, rounded once to float (Laplace smoothing: an
 *                                                            unused level has a finite price)
 *   s = sigmoid(alpha_i), lin = 1.2 s - 0.1, h_i = clamp(lin, 0, 1), h'_i = (0 <= lin <= 1) ? 1.2 (s (1 - s)) : 0
 *                                                            the expressions of nq_adaround_backward
 *   R_soft = sum_i (1 - h_i) cost[lo_i] + h_i cost[hi_i]     bits
 *   R_hard = sum_k c_k cost_k                                bits, cost_k the float table entry, summed in double for k ascending,
 *                                                            rounded once to float; R_soft equals it when every h_i is 0 or 1
 *   d(alpha)_i += ((gate * scale) * (cost[hi_i] - cost[lo_i])) * h'_i        the table is a constant of the derivative
 * gate = dyn[1], the regulariser gate of nq_step_prologue's slots, read on the device, or 1 when dyn == NULL; callers pass
 * scale = lambda / P with P the pixels of the clip (frames * H * W), which makes the term lambda * bpp.  gate * scale == 0 stores
 * nothing to dalpha (it stays bit for bit what it was).  Only weight quantisers take part, as for the rounding regulariser; in a
 * Hadamard model x / alpha are the padded transform-domain tensors: what the file stores.
 *
 * nq_level_rate: `segs` is a host array, the pointers inside are device pointers; lists longer than 16 tensors are chunked
 * (seg_table.h).  Per chunk FOUR launches: (1) a histogram -- each workgroup counts the levels of its 4096 elements in LDS with
 * integer LDS adds (8 padded copies of the table per wave, so that a dominating level costs an 8-way, not a 64-way, serialised
 * add) and writes K partial counts to ws; (2) a finish -- one workgroup per tensor adds the partial counts in workgroup order and
 * writes counts, cost and rate[1] = R_hard; (3) the rate pass -- one pass over x, alpha, delta, zp that adds the gradient into
 * dalpha (skipped when dalpha == NULL) and writes one partial sum of R_soft per workgroup to ws; (4) a sum -- one workgroup adds
 * each tensor's partials in a fixed order in double, writes rate[0] = R_soft and continues total[0] / total[1] = the float sums
 * of R_soft / R_hard over the tensors in list order ((0 + r_0) + r_1 ...).  No global atomics, no float atomics, no host read
 * between launches, no launch argument that depends on device data: bit-identical from call to call, capturable in a hipGraph.
 *   ws: the sum over the call's tensors of nq_level_rate_ws_words(rows * row_len, n_levels) 4-byte words, 16-byte aligned;
 *       nq_level_rate_ws_words(n, K) = ceil(n / 4096) * (K + 1), 0 for n <= 0 or K outside 4 .. 256 or a product past int64.
 *       ws_words is what the caller allocated: less than the call needs is NQ_ERR_INVALID.
 * NQ_ERR_INVALID, before the device is touched and whatever the position of the tensor in the list, for null pointers (dalpha and
 * dyn may be NULL), non-positive sizes, a row past 2^31 - 1 elements, n_levels outside 4 .. 256, a negative or non-finite scale
 * and an element count or workspace past int64. */
typedef struct nq_rate_seg {
  const float* x;      /* weights (rows x row_len) */
  const float* alpha;
  const float* delta;  /* (rows) when per_row, else (1) */
  const float* zp;
  float* dalpha;       /* d(alpha) to add the gradient to, or NULL */
  int32_t* counts;     /* out: n_levels */
  float* cost;         /* out: n_levels */
  float* rate;         /* out: {R_soft, R_hard} */
  int64_t rows, row_len;
  int per_row, n_levels;
} nq_rate_seg;
NQ_API int64_t nq_level_rate_ws_words(int64_t n, int n_levels);
NQ_API int nq_level_rate(const nq_rate_seg* segs, int nseg, float scale, const float* dyn, float* total, void* ws, int64_t ws_words,
                  nq_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NQ_HIP_H */

// Parameter-side kernels: scale init, uniform-affine and AdaRound fake-quant (forward / backward),
// rounding regulariser, Adam.  All HBM-bound elementwise / row-reduction work; compiled with
// -ffp-contract=off so that the arithmetic is the reference's op-by-op fp32 sequence
// (quantization/quantizer.py, calib_model.py:39-47).
#include "nq_common.h"
#include "quant_elem.h"
#include "seg_table.h"

namespace {

constexpr int TPB = 256;
constexpr int EPT = 4;  // elements per thread per block chunk

// ------------------------------------------------------------------------------------------------
// scale init: one workgroup per row (quantizer.py:156-168)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void scale_init_kernel(const float* __restrict__ x, int64_t row_len, int n_levels,
                                                         float* __restrict__ delta, float* __restrict__ zp) {
  __shared__ float smin[4], smax[4];
  const float* xr = x + (int64_t)blockIdx.x * row_len;
  float mn = 0.f, mx = 0.f;  // min(x_min, 0), max(x_max, 0)
  for (int64_t i = threadIdx.x; i < row_len; i += TPB) {
    float v = xr[i];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  mn = nq_wave_min(mn);
  mx = nq_wave_max(mx);
  if ((threadIdx.x & 63) == 0) {
    smin[threadIdx.x >> 6] = mn;
    smax[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < TPB / 64; ++i) {
      mn = fminf(mn, smin[i]);
      mx = fmaxf(mx, smax[i]);
    }
    // Python-double division, then cast to fp32 (quantizer.py:163)
    float d = (float)(((double)mx - (double)mn) / (double)(n_levels - 1));
    d = fmaxf(d, 1e-8f);
    delta[blockIdx.x] = d;
    zp[blockIdx.x] = rintf((-mn) / d);
  }
}

// ------------------------------------------------------------------------------------------------
// AdaRound init
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float half_round_trip(float v) { return (float)(_Float16)v; }  // round-to-nearest-even, like Tensor.half()

__global__ void adaround_scale_kernel(const float* __restrict__ din, const float* __restrict__ zin,
                                      float* __restrict__ dout, float* __restrict__ zout, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    dout[i] = half_round_trip(din[i]);  // quantizer.py:264
    zout[i] = half_round_trip(zin[i]);  // quantizer.py:265
  }
}

__global__ __launch_bounds__(TPB) void adaround_alpha_init_kernel(const float* __restrict__ x,
                                                                  const float* __restrict__ delta,
                                                                  float* __restrict__ alpha, int64_t n, int64_t row_len,
                                                                  int per_row) {
  int64_t i = (int64_t)blockIdx.x * (TPB * EPT) + threadIdx.x;
#pragma unroll
  for (int e = 0; e < EPT; ++e, i += TPB) {
    if (i < n) {
      float u = x[i] / delta[per_row ? i / row_len : 0];
      float rest = u - floorf(u);
      alpha[i] = -logf((NQ_ZETA - NQ_GAMMA) / (rest - NQ_GAMMA) - 1.0f);  // quantizer.py:312
    }
  }
}

// ------------------------------------------------------------------------------------------------
// deterministic two-stage sums
// ------------------------------------------------------------------------------------------------
constexpr int RED_CHUNK = NQ_RED_CHUNK;

__global__ __launch_bounds__(TPB) void round_loss_stage1(const float* __restrict__ alpha, int64_t n, float b,
                                                         float* __restrict__ ws) {
  __shared__ float red[16];
  int64_t i0 = (int64_t)blockIdx.x * RED_CHUNK;
  float acc = 0.f;
  for (int k = 0; k < 16; ++k) {
    int64_t i = i0 + k * TPB + threadIdx.x;
    if (i < n) {
      float h = fminf(fmaxf(soft_target_lin(alpha[i]), 0.f), 1.f);
      acc += 1.f - powf(fabsf(h - 0.5f) * 2.f, b);
    }
  }
  float s = nq_block_sum(acc, red);
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}

__global__ __launch_bounds__(TPB) void round_loss_bwd_kernel(const float* __restrict__ alpha, int64_t n, float b,
                                                             float weight, const float* __restrict__ gscale,
                                                             float* __restrict__ dalpha, int accumulate) {
  int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  float s = nq_sigmoid(alpha[i]);
  float lin = s * (NQ_ZETA - NQ_GAMMA) + NQ_GAMMA;
  float h = fminf(fmaxf(lin, 0.f), 1.f);
  float hp = (lin >= 0.f && lin <= 1.f) ? (NQ_ZETA - NQ_GAMMA) * (s * (1.f - s)) : 0.f;
  float c = h - 0.5f;
  float sg = (c > 0.f) ? 1.f : ((c < 0.f) ? -1.f : 0.f);
  float g = -(weight * (gscale ? gscale[0] : 1.f)) * (b * powf(fabsf(c) * 2.f, b - 1.f)) * 2.f * sg * hp;
  dalpha[i] = accumulate ? dalpha[i] + g : g;
}

// ------------------------------------------------------------------------------------------------
// The quantisers and Adam: ONE launch for all layers' weight and bias tensors (14 per decoder) over a segment table
// (seg_table.h); a workgroup works on 1024 consecutive elements of its segment's tensor.  The single-tensor entries are
// one-segment launches of the same kernels.
// ------------------------------------------------------------------------------------------------
struct AdaSegD {
  const float* x;
  const float* gy;
  const float* alpha;
  const float* delta;
  const float* zp;
  float* out;
  int64_t n;
  int row_len, per_row, soft;
  float qmax, reg_weight;
  int vec;  // every pointer of the segment is 16-byte aligned -> 16-byte accesses
  float* xq;  // nq_adaround_forward's x_quant output (the XQ instantiation only)
};
struct AdamSegD {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
  int vec;
};
struct AdaAdamSegD {
  const float* x;
  const float* gy;
  float* alpha;
  const float* delta;
  const float* zp;
  float* m;
  float* v;
  int64_t n;
  int row_len, per_row;
  float qmax, reg_weight;
  int vec;
};
struct UaqSegD {
  const float* x;
  const float* gy;      // backward
  const float* delta;
  const float* zp;
  float* out;           // forward: y; backward: d(delta)
  int64_t n;            // forward: elements
  int64_t rows;         // backward: reduction rows
  int row_len, per_row;
  float qmax;
  float* dx;            // nq_uaq_backward's gradient w.r.t. x (the DX instantiation only)
};

// A thread owns 4 CONSECUTIVE elements i0 .. i0 + 3 of its segment (one 16-byte load / store per tensor when the segment's
// pointers are 16-byte aligned: these kernels are bound by the number of memory instructions, 23 -> 10 us for the 2.65 M
// elements of HNeRV-3M), else -- and in the segment's last, partial group -- element by element.
struct Quad {
  // ONE 16-byte access in the compiler's eyes too: a float4 is four scalars to it until late, and it moved the fourth, which
  // the element-by-element path also touches, out of both paths (a 12-byte and a 4-byte access)
  typedef float V4 __attribute__((ext_vector_type(4)));
  int64_t i0, n, row0, row_len;
  int rem0, per_row;
  bool vec;
  static __device__ __forceinline__ int64_t first(int blk) { return (int64_t)blk * (TPB * EPT) + 4 * threadIdx.x; }
  __device__ __forceinline__ Quad(int64_t i0_, int64_t n_, int vec_ok)
      : i0(i0_), n(n_), row0(0), row_len(1), rem0(0), per_row(0), vec(vec_ok && (i0_ + 3 < n_)) {}
  // v[a][j] = p[a][i0 + j] for the N arrays p[0 .. N), 0 past the end
  template <int N>
  __device__ __forceinline__ void load(const float* const* p, float (*v)[4]) const {
    if (vec) {
#pragma unroll
      for (int a = 0; a < N; ++a) {
        const V4 t = *reinterpret_cast<const V4*>(p[a] + i0);
        v[a][0] = t.x; v[a][1] = t.y; v[a][2] = t.z; v[a][3] = t.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = i0 + j < n;
#pragma unroll
        for (int a = 0; a < N; ++a) v[a][j] = in ? p[a][i0 + j] : 0.f;
      }
    }
  }
  template <int N>
  __device__ __forceinline__ void store(float* const* p, const float (*v)[4]) const {
    if (vec) {
#pragma unroll
      for (int a = 0; a < N; ++a) *reinterpret_cast<V4*>(p[a] + i0) = V4{v[a][0], v[a][1], v[a][2], v[a][3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i0 + j < n) {
#pragma unroll
          for (int a = 0; a < N; ++a) p[a][i0 + j] = v[a][j];
        }
    }
  }
  // Row of delta / zp for element i0 + j: rows of >= 4 elements are crossed at most once inside the group; 0 past the end.
  // set_rows comes AFTER load in the kernels, so that the loads are issued before the division and not ~180 instructions
  // behind it.  row_len is held in 64 bits: widened only inside the per_row branch, the compiler filled the other branch's
  // copy from registers of the pending loads -- a full wait right behind them (adaround_adam_multi_kernel 21.1 -> 22.0 us).
  __device__ __forceinline__ void set_rows(int per_row_, int row_len_) {
    per_row = per_row_;
    row_len = row_len_;
    row0 = per_row ? i0 / row_len : 0;
    rem0 = per_row ? (int)(i0 - row0 * row_len) : 0;
  }
  __device__ __forceinline__ int64_t row(int j) const {
    int64_t r = 0;
    if (per_row) r = (row_len >= 4) ? row0 + ((rem0 + j >= row_len) ? 1 : 0) : (i0 + j) / row_len;
    if (i0 + j >= n) r = 0;
    return r;
  }
};

// XQ: also store the clamped integer grid value (forward only; the calibration step never does)
template <bool BWD, bool XQ>
__global__ __launch_bounds__(TPB) void adaround_multi_kernel(NqSegTable<AdaSegD> t, float reg_b, const float* __restrict__ dyn) {
  int blk;
  const int k = t.find(blockIdx.x, blk);
  const AdaSegD& sg = t.s[k];
  const int64_t i0 = Quad::first(blk);
  if (i0 >= sg.n) return;
  Quad q(i0, sg.n, sg.vec);
  constexpr int X = 0, A = 1, GY = 2, OUT = 0, XQO = 1;
  const float* const src[3] = {sg.x, sg.alpha, sg.gy};
  float* const dst[2] = {sg.out, sg.xq};
  float in[3][4], out[2][4];
  q.load<BWD ? 3 : 2>(src, in);
  q.set_rows(sg.per_row, sg.row_len);
  const StepScalars sc(BWD ? dyn : nullptr, reg_b, 0.f, 0.f);
  const float rw = sc.reg_weight(sg.reg_weight);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t row = q.row(j);
    const float d = sg.delta[row], z = sg.zp[row];
    if constexpr (BWD) out[OUT][j] = ada_bwd_elem(in[X][j], in[GY][j], in[A][j], d, z, sg.qmax, rw, sc.reg_b);
    else out[OUT][j] = ada_fwd_elem(in[X][j], in[A][j], d, z, sg.qmax, sg.soft, out[XQO][j]);
  }
  q.store<XQ ? 2 : 1>(dst, out);
}

__global__ __launch_bounds__(TPB) void adam_multi_kernel(NqSegTable<AdamSegD> t, float step_size, float beta1, float beta2,
                                                         float eps, float bc2_sqrt, const float* __restrict__ dyn) {
  const StepScalars sc(dyn, 0.f, step_size, bc2_sqrt);
  int blk;
  const int k = t.find(blockIdx.x, blk);
  const AdamSegD& sg = t.s[k];
  const int64_t i0 = Quad::first(blk);
  if (i0 >= sg.n) return;
  const Quad q(i0, sg.n, sg.vec);
  // (not Quad's scalar path: a partial group loads and stores nothing past the end, element by element)
  if (q.vec) {
    constexpr int G = 0, M = 1, V = 2, P = 3;
    const float* const src[4] = {sg.g, sg.m, sg.v, sg.p};
    float* const dst[3] = {sg.m, sg.v, sg.p};
    float a[4][4];
    q.load<4>(src, a);
#pragma unroll
    for (int j = 0; j < 4; ++j) adam_elem(a[G][j], a[M][j], a[V][j], a[P][j], sc.step_size, beta1, beta2, eps, sc.bc2_sqrt);
    q.store<3>(dst, a + M);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i0 + j < sg.n) {
        const int64_t i = i0 + j;
        float m = sg.m[i], v = sg.v[i], p = sg.p[i];
        adam_elem(sg.g[i], m, v, p, sc.step_size, beta1, beta2, eps, sc.bc2_sqrt);
        sg.m[i] = m;
        sg.v[i] = v;
        sg.p[i] = p;
      }
  }
}

// d(alpha) (+ regulariser gradient) and the Adam update of alpha in ONE pass (round 3): alpha is both the input of the
// fake-quant backward and Adam's parameter, so d(alpha) never goes to memory (x, gy, alpha, m, v: 85 MB per HNeRV-3M
// iteration instead of 117 MB in two launches).
__global__ __launch_bounds__(TPB) void adaround_adam_multi_kernel(NqSegTable<AdaAdamSegD> t, float reg_b, float step_size,
                                                                  float beta1, float beta2, float eps, float bc2_sqrt,
                                                                  const float* __restrict__ dyn) {
  const StepScalars sc(dyn, reg_b, step_size, bc2_sqrt);
  int blk;
  const int k = t.find(blockIdx.x, blk);
  const AdaAdamSegD& sg = t.s[k];
  const int64_t i0 = Quad::first(blk);
  if (i0 >= sg.n) return;
  Quad q(i0, sg.n, sg.vec);
  // rows in load order (x and alpha are needed first); the new alpha gets the row behind m and v: one store of three rows
  constexpr int X = 0, A = 1, GY = 2, M = 3, V = 4, ANEW = 5;
  const float* const src[5] = {sg.x, sg.alpha, sg.gy, sg.m, sg.v};
  float* const dst[3] = {sg.m, sg.v, sg.alpha};
  float a[6][4];
  q.load<5>(src, a);
  q.set_rows(sg.per_row, sg.row_len);
  const float rw = sc.reg_weight(sg.reg_weight);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t row = q.row(j);
    const float g = ada_bwd_elem(a[X][j], a[GY][j], a[A][j], sg.delta[row], sg.zp[row], sg.qmax, rw, sc.reg_b);
    a[ANEW][j] = a[A][j];
    adam_elem(g, a[M][j], a[V][j], a[ANEW][j], sc.step_size, beta1, beta2, eps, sc.bc2_sqrt);
  }
  q.store<3>(dst, a + M);
}

// UAQ fake-quant of several tensors in ONE launch (phase 1 of the calibration, calib_model.py:119-165): the forward per
// element, the backward one workgroup per reduction row.
__global__ __launch_bounds__(TPB) void uaq_fwd_multi_kernel(NqSegTable<UaqSegD> t) {
  int blk;
  const int k = t.find(blockIdx.x, blk);
  const UaqSegD& sg = t.s[k];
  int64_t i = (int64_t)blk * (TPB * EPT) + threadIdx.x;
#pragma unroll
  for (int e = 0; e < EPT; ++e, i += TPB) {
    if (i < sg.n) {
      const int64_t row = sg.per_row ? i / sg.row_len : 0;
      sg.out[i] = uaq_fwd_elem(sg.x[i], sg.delta[row], sg.zp[row], sg.qmax);
    }
  }
}
// DX: also store the straight-through gradient w.r.t. the quantiser input (the calibration step never does)
template <bool DX>
__global__ __launch_bounds__(TPB) void uaq_bwd_multi_kernel(NqSegTable<UaqSegD> t) {
  __shared__ float red[16];
  int blk;
  const int k = t.find(blockIdx.x, blk);
  const UaqSegD& sg = t.s[k];
  const int64_t row = blk;
  const float d = sg.delta[row], z = sg.zp[row];
  const int64_t base = row * sg.row_len;
  float acc = 0.f;
  for (int64_t i = threadIdx.x; i < sg.row_len; i += TPB) {
    float inside;
    const float g = sg.gy[base + i];
    acc += uaq_bwd_term(sg.x[base + i], g, d, z, sg.qmax, inside);
    // round_ste (quantizer.py:53-57, 117-119): autograd multiplies by delta (dequantisation), masks by the clamp and
    // divides by delta again (x/delta): (g*d)/d, not g, in fp32
    if (DX) sg.dx[base + i] = inside != 0.f ? (g * d) / d : 0.f;
  }
  float s = nq_block_sum(acc, red);
  if (threadIdx.x == 0) sg.out[row] = s;
}

// ------------------------------------------------------------------------------------------------
// host segment -> device segment; each returns the segment's workgroups or NQ_ERR_*
// ------------------------------------------------------------------------------------------------
inline int64_t quad_blocks(int64_t n) { return (n + TPB * EPT - 1) / (TPB * EPT); }
template <class... P>
inline int aligned16(P... p) { return ((... | (uintptr_t)p) & 15) == 0; }

int64_t ada_fill(const nq_ada_seg& h, bool bwd, float* xq, AdaSegD& d) {
  if (!h.x || !h.alpha || !h.delta || !h.zp || !h.out || (bwd && !h.gy) || h.rows <= 0 || h.row_len <= 0 ||
      h.row_len > 0x7fffffffLL)
    return NQ_ERR_INVALID;
  d.x = h.x; d.gy = h.gy; d.alpha = h.alpha; d.delta = h.delta; d.zp = h.zp; d.out = h.out; d.xq = xq;
  d.n = h.rows * h.row_len; d.row_len = (int)h.row_len; d.per_row = h.per_row; d.soft = h.soft;
  d.qmax = (float)(h.n_levels - 1); d.reg_weight = h.reg_weight;
  d.vec = aligned16(h.x, h.alpha, h.out, bwd ? h.gy : h.x, xq);
  return quad_blocks(d.n);
}

int64_t ada_adam_fill(const nq_ada_adam_seg& h, AdaAdamSegD& d) {
  if (!h.x || !h.gy || !h.alpha || !h.delta || !h.zp || !h.m || !h.v || h.rows <= 0 || h.row_len <= 0 ||
      h.row_len > 0x7fffffffLL)
    return NQ_ERR_INVALID;
  d.x = h.x; d.gy = h.gy; d.alpha = h.alpha; d.delta = h.delta; d.zp = h.zp; d.m = h.m; d.v = h.v;
  d.n = h.rows * h.row_len; d.row_len = (int)h.row_len; d.per_row = h.per_row;
  d.qmax = (float)(h.n_levels - 1); d.reg_weight = h.reg_weight;
  d.vec = aligned16(h.x, h.gy, h.alpha, h.m, h.v);
  return quad_blocks(d.n);
}

int64_t adam_fill(const nq_adam_seg& h, AdamSegD& d) {
  if (!h.p || !h.g || !h.m || !h.v || h.n <= 0) return NQ_ERR_INVALID;
  d.p = h.p; d.g = h.g; d.m = h.m; d.v = h.v; d.n = h.n;
  d.vec = aligned16(h.p, h.g, h.m, h.v);
  return quad_blocks(h.n);
}

int64_t uaq_fill(const nq_ada_seg& h, bool bwd, float* dx, UaqSegD& d) {
  if (!h.x || !h.delta || !h.zp || !h.out || (bwd && !h.gy) || h.rows <= 0 || h.row_len <= 0) return NQ_ERR_INVALID;
  d.x = h.x; d.gy = h.gy; d.delta = h.delta; d.zp = h.zp; d.out = h.out; d.dx = dx;
  d.n = h.rows * h.row_len;
  // per_row = 0: the whole tensor is one reduction row with one scale
  d.rows = h.per_row ? h.rows : 1;
  const int64_t rl = h.per_row ? h.row_len : h.rows * h.row_len;
  if (rl > 0x7fffffffLL) return NQ_ERR_INVALID;
  d.row_len = (int)rl; d.per_row = h.per_row; d.qmax = (float)(h.n_levels - 1);
  return bwd ? d.rows : quad_blocks(d.n);
}

// xq / dx: the one output of a single-tensor entry that the multi-tensor entries lack (NULL there)
int ada_multi(const nq_ada_seg* segs, int nseg, float reg_b, const float* dyn, bool bwd, float* xq, nq_stream_t stream) {
  return NqSegTable<AdaSegD>::launch_all(
      segs, nseg, [&](int i, AdaSegD& d) { return ada_fill(segs[i], bwd, xq, d); },
      [&](const NqSegTable<AdaSegD>& t, unsigned blocks) {
        const auto kernel = bwd ? adaround_multi_kernel<true, false>
                                : (xq ? adaround_multi_kernel<false, true> : adaround_multi_kernel<false, false>);
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(TPB), 0, nq_s(stream), t, reg_b, dyn);
      });
}

int uaq_multi(const nq_ada_seg* segs, int nseg, bool bwd, float* dx, nq_stream_t stream) {
  return NqSegTable<UaqSegD>::launch_all(
      segs, nseg, [&](int i, UaqSegD& d) { return uaq_fill(segs[i], bwd, dx, d); },
      [&](const NqSegTable<UaqSegD>& t, unsigned blocks) {
        const auto kernel = !bwd ? uaq_fwd_multi_kernel : (dx ? uaq_bwd_multi_kernel<true> : uaq_bwd_multi_kernel<false>);
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(TPB), 0, nq_s(stream), t);
      });
}

int adam_multi(const nq_adam_seg* segs, int nseg, float step_size, float beta1, float beta2, float eps, float bc2_sqrt,
               const float* dyn, nq_stream_t stream) {
  return NqSegTable<AdamSegD>::launch_all(
      segs, nseg, [&](int i, AdamSegD& d) { return adam_fill(segs[i], d); },
      [&](const NqSegTable<AdamSegD>& t, unsigned blocks) {
        hipLaunchKernelGGL(adam_multi_kernel, dim3(blocks), dim3(TPB), 0, nq_s(stream), t, step_size, beta1, beta2, eps,
                           bc2_sqrt, dyn);
      });
}

}  // namespace

extern "C" {

int nq_abi_version(void) { return 7; }

const char* nq_error_string(int code) {
  switch (code) {
    case NQ_OK: return "ok";
    case NQ_ERR_INVALID: return "invalid argument";
    case NQ_ERR_UNSUPPORTED: return "unsupported shape";
    case NQ_ERR_LAUNCH: return "HIP launch error";
    default: return "unknown error";
  }
}

int nq_scale_init_max(const float* x, int64_t rows, int64_t row_len, int n_levels, float* delta, float* zp,
                      nq_stream_t stream) {
  if (!x || !delta || !zp || rows <= 0 || row_len <= 0 || n_levels < 2) return NQ_ERR_INVALID;
  hipLaunchKernelGGL(scale_init_kernel, dim3((unsigned)rows), dim3(TPB), 0, nq_s(stream), x, row_len, n_levels, delta,
                     zp);
  return nq_launch_status();
}

int nq_uaq_forward(const float* x, const float* delta, const float* zp, float* y, int64_t rows, int64_t row_len,
                   int per_row, int n_levels, nq_stream_t stream) {
  const nq_ada_seg h{x, nullptr, nullptr, delta, zp, y, rows, row_len, per_row, n_levels, 0, 0.f};
  return uaq_multi(&h, 1, false, nullptr, stream);
}

int nq_uaq_backward(const float* x, const float* gy, const float* delta, const float* zp, float* ddelta, float* dx,
                    int64_t rows, int64_t row_len, int per_row, int n_levels, nq_stream_t stream) {
  const nq_ada_seg h{x, gy, nullptr, delta, zp, ddelta, rows, row_len, per_row, n_levels, 0, 0.f};
  return uaq_multi(&h, 1, true, dx, stream);
}

int nq_uaq_forward_multi(const nq_ada_seg* segs, int nseg, nq_stream_t stream) {
  return uaq_multi(segs, nseg, false, nullptr, stream);
}
int nq_uaq_backward_multi(const nq_ada_seg* segs, int nseg, nq_stream_t stream) {
  return uaq_multi(segs, nseg, true, nullptr, stream);
}

int nq_adaround_init(const float* x, const float* delta_in, const float* zp_in, float* delta_out, float* zp_out,
                     float* alpha, int64_t rows, int64_t row_len, int per_row, nq_stream_t stream) {
  if (!x || !delta_in || !zp_in || !delta_out || !zp_out || !alpha || rows <= 0 || row_len <= 0) return NQ_ERR_INVALID;
  const int64_t n = rows * row_len, ns = per_row ? rows : 1;
  if (quad_blocks(n) > 0x7fffffffLL) return NQ_ERR_INVALID;
  hipLaunchKernelGGL(adaround_scale_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, nq_s(stream), delta_in,
                     zp_in, delta_out, zp_out, ns);
  hipLaunchKernelGGL(adaround_alpha_init_kernel, dim3((unsigned)quad_blocks(n)), dim3(TPB), 0, nq_s(stream), x, delta_out,
                     alpha, n, row_len, per_row);
  return nq_launch_status();
}

int nq_adaround_forward(const float* x, const float* alpha, const float* delta, const float* zp, float* y, float* xq,
                        int64_t rows, int64_t row_len, int per_row, int n_levels, int soft, nq_stream_t stream) {
  const nq_ada_seg h{x, nullptr, alpha, delta, zp, y, rows, row_len, per_row, n_levels, soft, 0.f};
  return ada_multi(&h, 1, 0.f, nullptr, false, xq, stream);
}

int nq_adaround_backward(const float* x, const float* gy, const float* alpha, const float* delta, const float* zp,
                         float* dalpha, int64_t rows, int64_t row_len, int per_row, int n_levels, float reg_weight,
                         float reg_b, nq_stream_t stream) {
  const nq_ada_seg h{x, gy, alpha, delta, zp, dalpha, rows, row_len, per_row, n_levels, 0, reg_weight};
  return ada_multi(&h, 1, reg_b, nullptr, true, nullptr, stream);
}

int nq_adaround_forward_multi(const nq_ada_seg* segs, int nseg, nq_stream_t stream) {
  return ada_multi(segs, nseg, 0.f, nullptr, false, nullptr, stream);
}

int nq_adaround_backward_multi(const nq_ada_seg* segs, int nseg, float reg_b, nq_stream_t stream) {
  return ada_multi(segs, nseg, reg_b, nullptr, true, nullptr, stream);
}

int nq_adaround_backward_multi_dyn(const nq_ada_seg* segs, int nseg, const float* dyn, nq_stream_t stream) {
  if (!dyn) return NQ_ERR_INVALID;
  return ada_multi(segs, nseg, 0.f, dyn, true, nullptr, stream);
}

int nq_adaround_adam_multi(const nq_ada_adam_seg* segs, int nseg, float reg_b, float step_size, float beta1, float beta2, float eps,
                           float bc2_sqrt, const float* dyn, nq_stream_t stream) {
  return NqSegTable<AdaAdamSegD>::launch_all(
      segs, nseg, [&](int i, AdaAdamSegD& d) { return ada_adam_fill(segs[i], d); },
      [&](const NqSegTable<AdaAdamSegD>& t, unsigned blocks) {
        hipLaunchKernelGGL(adaround_adam_multi_kernel, dim3(blocks), dim3(TPB), 0, nq_s(stream), t, reg_b, step_size, beta1,
                           beta2, eps, bc2_sqrt, dyn);
      });
}

int64_t nq_reduce_ws_floats(int64_t n) { return n <= 0 ? 1 : (n + RED_CHUNK - 1) / RED_CHUNK; }

int nq_round_loss(const float* alpha, int64_t n, float b, float weight, float* ws, float* out, int accumulate,
                  nq_stream_t stream) {
  if (!alpha || !ws || !out || n <= 0) return NQ_ERR_INVALID;
  int64_t parts = nq_reduce_ws_floats(n);
  hipLaunchKernelGGL(round_loss_stage1, dim3((unsigned)parts), dim3(TPB), 0, nq_s(stream), alpha, n, b, ws);
  hipLaunchKernelGGL(nq_sum_stage2, dim3(1), dim3(TPB), 0, nq_s(stream), ws, parts, weight, out, accumulate);
  return nq_launch_status();
}

int nq_round_loss_backward(const float* alpha, int64_t n, float b, float weight, const float* gscale, float* dalpha,
                           int accumulate, nq_stream_t stream) {
  if (!alpha || !dalpha || n <= 0) return NQ_ERR_INVALID;
  hipLaunchKernelGGL(round_loss_bwd_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, nq_s(stream), alpha, n,
                     b, weight, gscale, dalpha, accumulate);
  return nq_launch_status();
}

int nq_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float step_size, float beta1, float beta2,
                 float eps, float bc2_sqrt, nq_stream_t stream) {
  const nq_adam_seg h{p, g, m, v, n};
  return adam_multi(&h, 1, step_size, beta1, beta2, eps, bc2_sqrt, nullptr, stream);
}

int nq_adam_step_multi(const nq_adam_seg* segs, int nseg, float step_size, float beta1, float beta2, float eps,
                       float bc2_sqrt, nq_stream_t stream) {
  return adam_multi(segs, nseg, step_size, beta1, beta2, eps, bc2_sqrt, nullptr, stream);
}

int nq_adam_step_multi_dyn(const nq_adam_seg* segs, int nseg, const float* dyn, float beta1, float beta2, float eps,
                           nq_stream_t stream) {
  if (!dyn) return NQ_ERR_INVALID;
  return adam_multi(segs, nseg, 0.f, beta1, beta2, eps, 1.f, dyn, stream);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// the step prologue of captured iterations
// ------------------------------------------------------------------------------------------------
namespace {

// One block: copies row `*step` of the per-step tables into the fixed "current step" slots every other kernel of the
// iteration reads, then advances the counter -- the only thing that changes between two replays of a captured iteration.
__global__ __launch_bounds__(256) void step_prologue_kernel(const int64_t* __restrict__ order, const float* __restrict__ scal,
                                                            int* __restrict__ step, int64_t* __restrict__ cur_idx,
                                                            float* __restrict__ cur_scal, int B, int nscal) {
  const int s = *step;
  const int t = threadIdx.x;
  int64_t vi = 0;
  float vs = 0.f;
  if (t < B) vi = order[(int64_t)s * B + t];
  if (t < nscal) vs = scal[(int64_t)s * nscal + t];
  __syncthreads();   // every thread has read *step before it is advanced
  if (t < B) cur_idx[t] = vi;
  if (t < nscal) cur_scal[t] = vs;
  if (t == 0) *step = s + 1;
}

// The prologue plus the gather of the batch's decoder inputs: blocks 1.. copy out[t] = table[order[step*B + t]] (they read
// the step counter BEFORE block 0 can have advanced it?  No ordering exists between blocks, so block 0 does NOT advance it
// here: every block reads *step, and the counter is advanced by the LAST block to finish -- a ticket in step[1]).
__global__ __launch_bounds__(256) void step_prologue_gather_kernel(const int64_t* __restrict__ order, const float* __restrict__ scal,
                                                                   int* __restrict__ step, int64_t* __restrict__ cur_idx,
                                                                   float* __restrict__ cur_scal, int B, int nscal,
                                                                   const float* __restrict__ table, int64_t table_rows,
                                                                   int64_t row_len, float* __restrict__ out) {
  __shared__ int last;
  const int s = __hip_atomic_load(step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int t = threadIdx.x;
  if (blockIdx.x == 0) {
    if (t < B) cur_idx[t] = order[(int64_t)s * B + t];
    if (t < nscal) cur_scal[t] = scal[(int64_t)s * nscal + t];
  } else {
    const int64_t per = ((int64_t)B * row_len + (gridDim.x - 2)) / (gridDim.x - 1);   // elements per gather block
    const int64_t lo = (int64_t)(blockIdx.x - 1) * per, hi = min(lo + per, (int64_t)B * row_len);
    for (int64_t e = lo + t; e < hi; e += 256) {
      const int64_t f = e / row_len, j = e - f * row_len;
      int64_t idx = order[(int64_t)s * B + f];
      idx = idx < 0 ? 0 : (idx >= table_rows ? table_rows - 1 : idx);
      out[e] = table[idx * row_len + j];
    }
  }
  // the last block to arrive advances the step counter and re-arms the ticket (nobody reads *step after its ticket)
  __syncthreads();
  if (t == 0) last = (atomicAdd(step + 1, 1) == (int)gridDim.x - 1);
  __syncthreads();
  if (last && t == 0) {
    step[1] = 0;
    __hip_atomic_store(step, s + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace

extern "C" {

int nq_step_prologue(const int64_t* order, const float* scal, int* step, int64_t* cur_idx, float* cur_scal, int B, int nscal,
                     nq_stream_t stream) {
  if (!order || !scal || !step || !cur_idx || !cur_scal || B <= 0 || B > 256 || nscal <= 0 || nscal > 256) return NQ_ERR_INVALID;
  hipLaunchKernelGGL(step_prologue_kernel, dim3(1), dim3(256), 0, nq_s(stream), order, scal, step, cur_idx, cur_scal, B, nscal);
  return nq_launch_status();
}

int nq_step_prologue_gather(const int64_t* order, const float* scal, int* step, int64_t* cur_idx, float* cur_scal, int B, int nscal,
                            const float* table, int64_t table_rows, int64_t row_len, float* out, nq_stream_t stream) {
  if (!order || !scal || !step || !cur_idx || !cur_scal || B <= 0 || B > 256 || nscal <= 0 || nscal > 256 || !table || !out ||
      table_rows <= 0 || row_len <= 0)
    return NQ_ERR_INVALID;
  // step = {counter, ticket}: two ints (the caller zeroes both)
  const int64_t total = (int64_t)B * row_len;
  int gb = (int)((total + 4095) / 4096);
  if (gb < 1) gb = 1;
  if (gb > 64) gb = 64;
  hipLaunchKernelGGL(step_prologue_gather_kernel, dim3(1 + gb), dim3(256), 0, nq_s(stream), order, scal, step, cur_idx, cur_scal, B,
                     nscal, table, table_rows, row_len, out);
  return nq_launch_status();
}

}  // extern "C"

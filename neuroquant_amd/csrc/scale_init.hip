// Scale init by search and by the row's moments (the definition is in include/nq_hip.h above
// nq_scale_init_search): UniformAffineQuantizer.init_quantization_scale for scale_method 'mse' / 'l1' / 'gaussian'
// (reference quantizer.py:170-220, 227-234).  The reference scores ten clipped ranges per output channel with a Python loop
// of small torch ops; here every candidate of a row is scored in ONE pass over the row, ten double accumulators per lane.
//
// Launch plan -- a function of (rows, row_len) only, so two calls give the same bits:
//   row_len <= WAVE_MAX    one wave per row, four rows per workgroup, the row in LDS                  (1 launch)
//   row_len <= BLOCK_MAX   one workgroup per row, the row in LDS                                     (1 launch)
//   longer                 rows cut into CHUNK-element pieces, one workgroup each: the row's range (or sum) per piece, the ten
//                          partial scores (or the squared deviations) per piece, one finishing workgroup per row  (3 launches)
// x is read from HBM once on the first two routes and twice on the third.  No atomics; every sum is a lane-strided double
// accumulation, a wave64 shuffle tree and a fixed-order pass over the waves / pieces.  Compiled with -ffp-contract=off: the
// fp32 element arithmetic is the definition's, op by op.
#include "nq_common.h"

#include <cmath>

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int NC = 10;                    // candidates: the range scaled by 1.00, 0.95 ... 0.55
constexpr int WAVE_MAX = 512;             // longest row a wave keeps in its quarter of the workgroup's LDS (2 KB)
constexpr int BLOCK_MAX = 8192;           // longest row a workgroup keeps in LDS (32 KB)
constexpr int CHUNK = 8192;               // elements per workgroup of a row that is cut
constexpr int MAXK = 65536;
constexpr int64_t MAX_BLOCKS = (1LL << 24) - 1;   // blocks * TPB stays below 2^32 work-items

enum Route { ROUTE_WAVE = 0, ROUTE_BLOCK = 1, ROUTE_CHUNK = 2 };

struct Plan {
  int route;
  int64_t nchunk;   // pieces per row (1 unless ROUTE_CHUNK)
  int64_t blocks;   // workgroups of the scoring launch
};

// false: sizes the entries refuse
inline bool make_plan(int64_t rows, int64_t row_len, Plan& p) {
  if (rows <= 0 || row_len <= 0 || rows > INT64_MAX / row_len) return false;
  p.nchunk = 1;
  if (row_len <= WAVE_MAX) {
    p.route = ROUTE_WAVE;
    p.blocks = rows / WAVES + (rows % WAVES != 0);
  } else if (row_len <= BLOCK_MAX) {
    p.route = ROUTE_BLOCK;
    p.blocks = rows;
  } else {
    p.route = ROUTE_CHUNK;
    p.nchunk = row_len / CHUNK + (row_len % CHUNK != 0);
    if (rows > MAX_BLOCKS / p.nchunk) return false;
    p.blocks = rows * p.nchunk;
  }
  return p.blocks <= MAX_BLOCKS;
}

// the workspace of a cut row: per piece 8 bytes of statistics {min, max} / {sum}, then NC doubles of partial scores
constexpr int64_t WS_PER_CHUNK = 8 + NC * 8;

struct Cand {
  float d[NC], z[NC];
};

__device__ __forceinline__ void candidates(float x_max, float x_min, int K, Cand& c) {
  const float km1 = (float)(K - 1);
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const float f = (float)(1.0 - (double)i * 0.05);
    const float hi = x_max * f, lo = x_min * f;
    const float d = fmaxf((hi - lo) / km1, 1e-8f);
    c.d[i] = d;
    c.z[i] = rintf((-lo) / d);
  }
}

// one element into the ten sums.  A NaN element leaves the clamp as level 0 and comes back as |NaN - xq| = NaN.
__device__ __forceinline__ void score(float x, const Cand& c, float qmax, double p, bool p_is_1, double (&acc)[NC]) {
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const float q = fminf(fmaxf(rintf(x / c.d[i]) + c.z[i], 0.f), qmax);
    const float xq = (q - c.z[i]) * c.d[i];
    const float t = fabsf(x - xq);
    acc[i] += p_is_1 ? (double)t : pow((double)t, p);
  }
}

__device__ __forceinline__ double wave_sum_d(double v) {   // valid in lane 0
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_min_all(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max_all(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// workgroup-wide range, in every thread
__device__ __forceinline__ void block_minmax_all(float& mn, float& mx, float* smem /* 2 * WAVES */) {
  mn = wave_min_all(mn);
  mx = wave_max_all(mx);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    smem[threadIdx.x >> 6] = mn;
    smem[WAVES + (threadIdx.x >> 6)] = mx;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    mn = fminf(mn, smem[w]);
    mx = fmaxf(mx, smem[WAVES + w]);
  }
}

// workgroup-wide sum in a fixed order, in every thread
__device__ __forceinline__ double block_sum_d_all(double v, double* smem /* WAVES */) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = 0.0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) r += smem[w];
  return r;
}

// ten workgroup-wide sums; valid in thread 0
__device__ __forceinline__ void block_sum_nc(double (&acc)[NC], double* smem /* WAVES * NC */) {
#pragma unroll
  for (int i = 0; i < NC; ++i) acc[i] = wave_sum_d(acc[i]);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < NC; ++i) smem[(threadIdx.x >> 6) * NC + i] = acc[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      double r = 0.0;
      for (int w = 0; w < WAVES; ++w) r += smem[w * NC + i];
      acc[i] = r;
    }
  }
}

struct SearchOut {
  float* delta;
  float* zp;
  int* choice;
  double* scores;   // may be null
};

// the lowest candidate whose score is below every earlier one, from 1e10 (quantizer.py:173-186); none: choice -1, NaN scales
__device__ __forceinline__ void search_finish(const double (&sum)[NC], int64_t n, const Cand& c, int64_t row, const SearchOut& o) {
  double best = 1e10;
  int win = -1;
  float d = __builtin_nanf(""), z = __builtin_nanf("");
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const double s = sum[i] / (double)n;
    if (o.scores) o.scores[row * NC + i] = s;
    if (s < best) {
      best = s;
      win = i;
      d = c.d[i];
      z = c.z[i];
    }
  }
  o.choice[row] = win;
  o.delta[row] = d;
  o.zp[row] = z;
}

// 'gaussian' (quantizer.py:188-203): the range is mean -+ 6 * VARIANCE, the reference's quirk.  min / max / clamp as the
// reference's Python min(), max() and torch.max() order their arguments, so that a NaN (a row of one element) stays a NaN.
__device__ __forceinline__ void gauss_finish(double sum, double ss, int64_t n, int K, int64_t row, float* delta, float* zp, float* stats) {
  const float mu = (float)(sum / (double)n);
  const float var = (float)(ss / (double)(n - 1));
  const float s6 = 6.f * var;
  const float a = mu - s6, b = mu + s6;
  const float x_min = (0.f < a) ? 0.f : a;
  const float x_max = (0.f > b) ? 0.f : b;
  float d = (x_max - x_min) / (float)(K - 1);
  d = (d < 1e-8f) ? 1e-8f : d;
  delta[row] = d;
  zp[row] = rintf((-x_min) / d);
  if (stats) {
    stats[2 * row] = mu;
    stats[2 * row + 1] = var;
  }
}

// ---------------------------------------------------------------------------------------------- route 1: a wave per row
__global__ __launch_bounds__(TPB) void search_wave_kernel(const float* __restrict__ x, int64_t rows, int row_len, int K, double p,
                                                          SearchOut o) {
  __shared__ float rows_lds[WAVES][WAVE_MAX];
  const int64_t row = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;   // whole waves leave; nothing below synchronises the workgroup
  const int lane = threadIdx.x & 63;
  const float* xr = x + row * row_len;
  float* rowv = rows_lds[threadIdx.x >> 6];
  float mn = INFINITY, mx = -INFINITY;
  for (int j = lane; j < row_len; j += 64) {
    const float v = xr[j];
    rowv[j] = v;
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  mn = wave_min_all(mn);
  mx = wave_max_all(mx);
  Cand c;
  candidates(mx, mn, K, c);
  const float qmax = (float)(K - 1);
  const bool p1 = p == 1.0;
  double acc[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i) acc[i] = 0.0;
#pragma unroll 1
  for (int j = lane; j < row_len; j += 64) score(rowv[j], c, qmax, p, p1, acc);   // each lane reads what it wrote
#pragma unroll
  for (int i = 0; i < NC; ++i) acc[i] = wave_sum_d(acc[i]);
  if (lane == 0) search_finish(acc, row_len, c, row, o);
}

__global__ __launch_bounds__(TPB) void gauss_wave_kernel(const float* __restrict__ x, int64_t rows, int row_len, int K,
                                                         float* __restrict__ delta, float* __restrict__ zp, float* __restrict__ stats) {
  __shared__ float rows_lds[WAVES][WAVE_MAX];
  const int64_t row = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const float* xr = x + row * row_len;
  float* rowv = rows_lds[threadIdx.x >> 6];
  double s = 0.0;
  for (int j = lane; j < row_len; j += 64) {
    const float v = xr[j];
    rowv[j] = v;
    s += (double)v;
  }
  s = __shfl(wave_sum_d(s), 0, 64);
  const double mean = s / (double)row_len;
  double ss = 0.0;
  for (int j = lane; j < row_len; j += 64) {
    const double dv = (double)rowv[j] - mean;
    ss += dv * dv;
  }
  ss = wave_sum_d(ss);
  if (lane == 0) gauss_finish(s, ss, row_len, K, row, delta, zp, stats);
}

// ----------------------------------------------------------------------------------------- route 2: a workgroup per row
__global__ __launch_bounds__(TPB) void search_block_kernel(const float* __restrict__ x, int row_len, int K, double p, SearchOut o) {
  __shared__ float rowv[BLOCK_MAX];
  __shared__ float mm[2 * WAVES];
  __shared__ double red[WAVES * NC];
  const int64_t row = blockIdx.x;
  const float* xr = x + row * row_len;
  float mn = INFINITY, mx = -INFINITY;
  for (int j = threadIdx.x; j < row_len; j += TPB) {
    const float v = xr[j];
    rowv[j] = v;
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  block_minmax_all(mn, mx, mm);
  Cand c;
  candidates(mx, mn, K, c);
  const float qmax = (float)(K - 1);
  const bool p1 = p == 1.0;
  double acc[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i) acc[i] = 0.0;
#pragma unroll 1
  for (int j = threadIdx.x; j < row_len; j += TPB) score(rowv[j], c, qmax, p, p1, acc);   // each thread reads what it wrote
  block_sum_nc(acc, red);
  if (threadIdx.x == 0) search_finish(acc, row_len, c, row, o);
}

__global__ __launch_bounds__(TPB) void gauss_block_kernel(const float* __restrict__ x, int row_len, int K, float* __restrict__ delta,
                                                          float* __restrict__ zp, float* __restrict__ stats) {
  __shared__ float rowv[BLOCK_MAX];
  __shared__ double red[WAVES];
  const int64_t row = blockIdx.x;
  const float* xr = x + row * row_len;
  double s = 0.0;
  for (int j = threadIdx.x; j < row_len; j += TPB) {
    const float v = xr[j];
    rowv[j] = v;
    s += (double)v;
  }
  s = block_sum_d_all(s, red);
  const double mean = s / (double)row_len;
  double ss = 0.0;
  for (int j = threadIdx.x; j < row_len; j += TPB) {
    const double dv = (double)rowv[j] - mean;
    ss += dv * dv;
  }
  ss = block_sum_d_all(ss, red);
  if (threadIdx.x == 0) gauss_finish(s, ss, row_len, K, row, delta, zp, stats);
}

// ------------------------------------------------------------------------------------------------- route 3: rows in pieces
// piece b of the launch: row b / nchunk, elements [lo, hi) of it
struct Piece {
  int64_t row, lo, hi;
  __device__ __forceinline__ Piece(int64_t b, int64_t nchunk, int64_t row_len) {
    row = b / nchunk;
    lo = (b - row * nchunk) * CHUNK;
    hi = lo + CHUNK < row_len ? lo + CHUNK : row_len;
  }
};

// the row's range from the ranges of its pieces, in every thread
__device__ __forceinline__ void row_minmax(const float* __restrict__ st, int64_t nchunk, float& mn, float& mx, float* smem) {
  mn = INFINITY;
  mx = -INFINITY;
  for (int64_t k = threadIdx.x; k < nchunk; k += TPB) {
    mn = fminf(mn, st[2 * k]);
    mx = fmaxf(mx, st[2 * k + 1]);
  }
  block_minmax_all(mn, mx, smem);
}
// the sum of one double per piece, `stride` doubles apart, in every thread; the same order wherever it is called
__device__ __forceinline__ double row_sum(const double* __restrict__ part, int64_t nchunk, int stride, double* smem) {
  double a = 0.0;
  for (int64_t k = threadIdx.x; k < nchunk; k += TPB) a += part[k * stride];
  return block_sum_d_all(a, smem);
}

__global__ __launch_bounds__(TPB) void chunk_minmax_kernel(const float* __restrict__ x, int64_t row_len, int64_t nchunk,
                                                           float* __restrict__ st) {
  __shared__ float mm[2 * WAVES];
  const Piece pc(blockIdx.x, nchunk, row_len);
  const float* xr = x + pc.row * row_len;
  float mn = INFINITY, mx = -INFINITY;
  for (int64_t j = pc.lo + threadIdx.x; j < pc.hi; j += TPB) {
    const float v = xr[j];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  block_minmax_all(mn, mx, mm);
  if (threadIdx.x == 0) {
    st[2 * (int64_t)blockIdx.x] = mn;
    st[2 * (int64_t)blockIdx.x + 1] = mx;
  }
}

__global__ __launch_bounds__(TPB) void search_chunk_kernel(const float* __restrict__ x, int64_t row_len, int64_t nchunk, int K, double p,
                                                           const float* __restrict__ st, double* __restrict__ part) {
  __shared__ float mm[2 * WAVES];
  __shared__ double red[WAVES * NC];
  const Piece pc(blockIdx.x, nchunk, row_len);
  const float* xr = x + pc.row * row_len;
  float mn, mx;
  row_minmax(st + 2 * pc.row * nchunk, nchunk, mn, mx, mm);
  Cand c;
  candidates(mx, mn, K, c);
  const float qmax = (float)(K - 1);
  const bool p1 = p == 1.0;
  double acc[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i) acc[i] = 0.0;
#pragma unroll 1
  for (int64_t j = pc.lo + threadIdx.x; j < pc.hi; j += TPB) score(xr[j], c, qmax, p, p1, acc);
  block_sum_nc(acc, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < NC; ++i) part[(int64_t)blockIdx.x * NC + i] = acc[i];
  }
}

__global__ __launch_bounds__(TPB) void search_rows_kernel(int64_t row_len, int64_t nchunk, int K, const float* __restrict__ st,
                                                          const double* __restrict__ part, SearchOut o) {
  __shared__ float mm[2 * WAVES];
  __shared__ double red[WAVES];
  const int64_t row = blockIdx.x;
  float mn, mx;
  row_minmax(st + 2 * row * nchunk, nchunk, mn, mx, mm);
  Cand c;
  candidates(mx, mn, K, c);
  double sum[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i) sum[i] = row_sum(part + row * nchunk * NC + i, nchunk, NC, red);
  if (threadIdx.x == 0) search_finish(sum, row_len, c, row, o);
}

__global__ __launch_bounds__(TPB) void chunk_sum_kernel(const float* __restrict__ x, int64_t row_len, int64_t nchunk,
                                                        double* __restrict__ st) {
  __shared__ double red[WAVES];
  const Piece pc(blockIdx.x, nchunk, row_len);
  const float* xr = x + pc.row * row_len;
  double s = 0.0;
  for (int64_t j = pc.lo + threadIdx.x; j < pc.hi; j += TPB) s += (double)xr[j];
  s = block_sum_d_all(s, red);
  if (threadIdx.x == 0) st[blockIdx.x] = s;
}

__global__ __launch_bounds__(TPB) void gauss_chunk_kernel(const float* __restrict__ x, int64_t row_len, int64_t nchunk,
                                                          const double* __restrict__ st, double* __restrict__ part) {
  __shared__ double red[WAVES];
  const Piece pc(blockIdx.x, nchunk, row_len);
  const float* xr = x + pc.row * row_len;
  const double mean = row_sum(st + pc.row * nchunk, nchunk, 1, red) / (double)row_len;
  double ss = 0.0;
  for (int64_t j = pc.lo + threadIdx.x; j < pc.hi; j += TPB) {
    const double dv = (double)xr[j] - mean;
    ss += dv * dv;
  }
  ss = block_sum_d_all(ss, red);
  if (threadIdx.x == 0) part[blockIdx.x] = ss;
}

__global__ __launch_bounds__(TPB) void gauss_rows_kernel(int64_t row_len, int64_t nchunk, int K, const double* __restrict__ st,
                                                         const double* __restrict__ part, float* __restrict__ delta,
                                                         float* __restrict__ zp, float* __restrict__ stats) {
  __shared__ double red[WAVES];
  const int64_t row = blockIdx.x;
  const double s = row_sum(st + row * nchunk, nchunk, 1, red);
  const double ss = row_sum(part + row * nchunk, nchunk, 1, red);
  if (threadIdx.x == 0) gauss_finish(s, ss, row_len, K, row, delta, zp, stats);
}

}  // namespace

extern "C" {

int64_t nq_scale_init_ws_bytes(int64_t rows, int64_t row_len) {
  Plan pl;
  if (!make_plan(rows, row_len, pl)) return NQ_ERR_INVALID;
  return pl.route == ROUTE_CHUNK ? pl.blocks * WS_PER_CHUNK : 16;
}

int nq_scale_init_search(const float* x, int64_t rows, int64_t row_len, int n_levels, double p, float* delta, float* zp, int* choice,
                         double* scores, void* ws, nq_stream_t stream) {
  Plan pl;
  if (!x || !delta || !zp || !choice || !ws || n_levels < 2 || n_levels > MAXK || !std::isfinite(p) || p <= 0.0) return NQ_ERR_INVALID;
  if (!make_plan(rows, row_len, pl)) return NQ_ERR_INVALID;
  const SearchOut o{delta, zp, choice, scores};
  const dim3 grid((unsigned)pl.blocks), block(TPB);
  hipStream_t s = nq_s(stream);
  if (pl.route == ROUTE_WAVE) {
    hipLaunchKernelGGL(search_wave_kernel, grid, block, 0, s, x, rows, (int)row_len, n_levels, p, o);
  } else if (pl.route == ROUTE_BLOCK) {
    hipLaunchKernelGGL(search_block_kernel, grid, block, 0, s, x, (int)row_len, n_levels, p, o);
  } else {
    float* st = static_cast<float*>(ws);
    double* part = reinterpret_cast<double*>(static_cast<char*>(ws) + pl.blocks * 8);
    hipLaunchKernelGGL(chunk_minmax_kernel, grid, block, 0, s, x, row_len, pl.nchunk, st);
    hipLaunchKernelGGL(search_chunk_kernel, grid, block, 0, s, x, row_len, pl.nchunk, n_levels, p, st, part);
    hipLaunchKernelGGL(search_rows_kernel, dim3((unsigned)rows), block, 0, s, row_len, pl.nchunk, n_levels, st, part, o);
  }
  return nq_launch_status();
}

int nq_scale_init_gaussian(const float* x, int64_t rows, int64_t row_len, int n_levels, float* delta, float* zp, float* stats, void* ws,
                           nq_stream_t stream) {
  Plan pl;
  if (!x || !delta || !zp || !ws || n_levels < 2 || n_levels > MAXK) return NQ_ERR_INVALID;
  if (!make_plan(rows, row_len, pl)) return NQ_ERR_INVALID;
  const dim3 grid((unsigned)pl.blocks), block(TPB);
  hipStream_t s = nq_s(stream);
  if (pl.route == ROUTE_WAVE) {
    hipLaunchKernelGGL(gauss_wave_kernel, grid, block, 0, s, x, rows, (int)row_len, n_levels, delta, zp, stats);
  } else if (pl.route == ROUTE_BLOCK) {
    hipLaunchKernelGGL(gauss_block_kernel, grid, block, 0, s, x, (int)row_len, n_levels, delta, zp, stats);
  } else {
    double* st = static_cast<double*>(ws);
    double* part = st + pl.blocks;
    hipLaunchKernelGGL(chunk_sum_kernel, grid, block, 0, s, x, row_len, pl.nchunk, st);
    hipLaunchKernelGGL(gauss_chunk_kernel, grid, block, 0, s, x, row_len, pl.nchunk, st, part);
    hipLaunchKernelGGL(gauss_rows_kernel, dim3((unsigned)rows), block, 0, s, row_len, pl.nchunk, n_levels, st, part, delta, zp, stats);
  }
  return nq_launch_status();
}

}  // extern "C"

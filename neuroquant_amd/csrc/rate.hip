// Rate-aware calibration (the definition is in include/nq_hip.h above nq_level_rate): the entropy cost of the
// levels a bit stream stores -- a histogram of the hard levels, the per-level price under a static model, the soft rate of
// the rounding variables and its gradient w.r.t. alpha.  Four launches per segment table, no global atomics, every sum in a
// fixed order.  Compiled with -ffp-contract=off: the level is nq_adaround_forward's expression, bit for bit.
#include "nq_common.h"
#include "seg_table.h"

#include <cmath>

namespace {

constexpr int TPB = 256;
constexpr int SPAN = 4096;            // elements per workgroup: 4 groups of 256 threads x 4 consecutive elements
constexpr int GROUPS = SPAN / (TPB * 4);
constexpr int COPIES = 8;             // histogram copies per wave: lane & 7 picks one
constexpr int MAXK = 256, MINK = 4;
constexpr int NCOPY = (TPB / 64) * COPIES;

struct RateSegD {
  const float* x;
  const float* alpha;
  const float* delta;
  const float* zp;
  float* dalpha;
  int* counts;
  float* cost;
  float* rate;
  int* ws_hist;      // [nblk][K] partial counts
  float* ws_part;    // [nblk] partial sums of R_soft
  int64_t n;
  int row_len, per_row, K, nblk;
  int vec;           // x, alpha (and dalpha) are 16-byte aligned
};
using RateTable = NqSegTable<RateSegD>;

typedef float V4 __attribute__((ext_vector_type(4)));

// 4 consecutive elements from i0, 0 past the end
__device__ __forceinline__ void load4(const float* __restrict__ p, int64_t i0, int64_t n, bool vec, float (&v)[4]) {
  if (vec) {
    const V4 t = *reinterpret_cast<const V4*>(p + i0);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (i0 + j < n) ? p[i0 + j] : 0.f;
  }
}

// delta / zp row of the 4 elements from i0 (rows of >= 4 elements are crossed at most once inside the group)
struct Rows {
  int64_t i0, row0;
  int row_len, rem0, per_row;
  __device__ __forceinline__ Rows(int64_t i0_, int per_row_, int row_len_) : i0(i0_), row0(0), row_len(row_len_), rem0(0), per_row(per_row_) {
    if (per_row) {
      row0 = i0 / row_len;
      rem0 = (int)(i0 - row0 * row_len);
    }
  }
  __device__ __forceinline__ int64_t row(int j) const {
    if (!per_row) return 0;
    return row_len >= 4 ? row0 + ((rem0 + j >= row_len) ? 1 : 0) : (i0 + j) / row_len;
  }
};

// the two neighbouring levels of an element as table indices in [0, K - 1] (whatever x, delta and zp hold: a NaN gives 0)
__device__ __forceinline__ void levels(float xv, float d, float z, float qmax, int& lo, int& hi) {
  const float f = floorf(xv / d);
  const float l = fminf(fmaxf((f + 0.f) + z, 0.f), qmax);
  const float h = fminf(fmaxf((f + 1.f) + z, 0.f), qmax);
  const int K1 = (int)qmax;
  lo = min(max((int)l, 0), K1);
  hi = min(max((int)h, 0), K1);
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
// block-wide sum in double, fixed order; valid in thread 0
__device__ __forceinline__ double block_sum_d(double v, double* smem /* TPB / 64 */) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < TPB / 64; ++i) r += smem[i];
  return r;
}

// (1) K partial counts per workgroup.  LDS: NCOPY copies of the table with a stride of K + 1 words, so that the same level in
// the 8 copies of a wave falls on 8 different banks.
__global__ __launch_bounds__(TPB) void rate_hist_kernel(RateTable t) {
  __shared__ int hist[NCOPY * (MAXK + 1)];
  int blk;
  const int k = t.find(blockIdx.x, blk);
  const RateSegD& sg = t.s[k];
  const int K = sg.K, stride = K + 1;
  for (int i = threadIdx.x; i < NCOPY * stride; i += TPB) hist[i] = 0;
  __syncthreads();
  int* mine = hist + ((threadIdx.x >> 6) * COPIES + (threadIdx.x & (COPIES - 1))) * stride;
  const float qmax = (float)(K - 1);
#pragma unroll
  for (int g = 0; g < GROUPS; ++g) {
    const int64_t i0 = (int64_t)blk * SPAN + g * (TPB * 4) + 4 * threadIdx.x;
    if (i0 < sg.n) {
      const bool vec = sg.vec && (i0 + 3 < sg.n);
      float xv[4], av[4];
      load4(sg.x, i0, sg.n, vec, xv);
      load4(sg.alpha, i0, sg.n, vec, av);
      const Rows rows(i0, sg.per_row, sg.row_len);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (i0 + j < sg.n) {
          const int64_t r = rows.row(j);
          int lo, hi;
          levels(xv[j], sg.delta[r], sg.zp[r], qmax, lo, hi);
          atomicAdd(mine + (av[j] >= 0.f ? hi : lo), 1);
        }
      }
    }
  }
  __syncthreads();
  for (int lv = threadIdx.x; lv < K; lv += TPB) {
    int c = 0;
#pragma unroll 4
    for (int cp = 0; cp < NCOPY; ++cp) c += hist[cp * stride + lv];
    sg.ws_hist[(int64_t)blk * K + lv] = c;
  }
}

// (2) one workgroup per tensor: counts, the cost table, R_hard
__global__ __launch_bounds__(TPB) void rate_finish_kernel(RateTable t) {
  __shared__ double term[MAXK];
  const RateSegD& sg = t.s[blockIdx.x];
  const int K = sg.K, lv = threadIdx.x;
  if (lv < K) {
    int c = 0;
    for (int b = 0; b < sg.nblk; ++b) c += sg.ws_hist[(int64_t)b * K + lv];
    const float cost = (float)log2(((double)sg.n + (double)K) / ((double)c + 1.0));
    sg.counts[lv] = c;
    sg.cost[lv] = cost;
    term[lv] = (double)c * (double)cost;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = 0.0;
    for (int i = 0; i < K; ++i) r += term[i];
    sg.rate[1] = (float)r;
  }
}

// (3) the gradient into d(alpha) and one partial sum of R_soft per workgroup
__global__ __launch_bounds__(TPB) void rate_pass_kernel(RateTable t, float scale, const float* __restrict__ dyn) {
  __shared__ float cost[MAXK];
  __shared__ double red[TPB / 64];
  int blk;
  const int k = t.find(blockIdx.x, blk);
  const RateSegD& sg = t.s[k];
  const int K = sg.K;
  for (int i = threadIdx.x; i < K; i += TPB) cost[i] = sg.cost[i];
  __syncthreads();
  const float gs = (dyn ? dyn[1] : 1.f) * scale;
  const bool grad = sg.dalpha != nullptr && gs != 0.f;
  const float qmax = (float)(K - 1);
  float acc = 0.f;
#pragma unroll
  for (int g = 0; g < GROUPS; ++g) {
    const int64_t i0 = (int64_t)blk * SPAN + g * (TPB * 4) + 4 * threadIdx.x;
    if (i0 < sg.n) {
      const bool vec = sg.vec && (i0 + 3 < sg.n);
      float xv[4], av[4], dv[4] = {0.f, 0.f, 0.f, 0.f};
      load4(sg.x, i0, sg.n, vec, xv);
      load4(sg.alpha, i0, sg.n, vec, av);
      if (grad) load4(sg.dalpha, i0, sg.n, vec, dv);
      const Rows rows(i0, sg.per_row, sg.row_len);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (i0 + j < sg.n) {
          const int64_t r = rows.row(j);
          int lo, hi;
          levels(xv[j], sg.delta[r], sg.zp[r], qmax, lo, hi);
          const float s = nq_sigmoid(av[j]);
          const float lin = s * (NQ_ZETA - NQ_GAMMA) + NQ_GAMMA;
          const float h = fminf(fmaxf(lin, 0.f), 1.f);
          const float hp = (lin >= 0.f && lin <= 1.f) ? (NQ_ZETA - NQ_GAMMA) * (s * (1.f - s)) : 0.f;
          const float cl = cost[lo], ch = cost[hi];
          acc += (1.f - h) * cl + h * ch;
          if (grad) dv[j] = dv[j] + (gs * (ch - cl)) * hp;
        }
      }
      if (grad) {
        if (vec) {
          *reinterpret_cast<V4*>(sg.dalpha + i0) = V4{dv[0], dv[1], dv[2], dv[3]};
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (i0 + j < sg.n) sg.dalpha[i0 + j] = dv[j];
        }
      }
    }
  }
  const double s = block_sum_d((double)acc, red);
  if (threadIdx.x == 0) sg.ws_part[blk] = (float)s;
}

// (4) one workgroup: R_soft per tensor (partials in a fixed order, in double) and the running totals over the list
__global__ __launch_bounds__(TPB) void rate_sum_kernel(RateTable t, float* __restrict__ total, int first) {
  __shared__ double red[TPB / 64];
  float ts = first ? 0.f : total[0], th = first ? 0.f : total[1];   // (read by thread 0 only where it matters)
  for (int k = 0; k < t.nseg; ++k) {
    const RateSegD& sg = t.s[k];
    double acc = 0.0;
    for (int b = threadIdx.x; b < sg.nblk; b += TPB) acc += (double)sg.ws_part[b];
    const double s = block_sum_d(acc, red);
    if (threadIdx.x == 0) {
      const float rs = (float)s;
      sg.rate[0] = rs;
      ts = ts + rs;
      th = th + sg.rate[1];
    }
  }
  if (threadIdx.x == 0) {
    total[0] = ts;
    total[1] = th;
  }
}

inline int64_t rate_blocks(int64_t n) { return (n + SPAN - 1) / SPAN; }

// elements of a segment, or -1 for sizes the entry refuses
inline int64_t rate_elems(const nq_rate_seg& h) {
  if (h.rows <= 0 || h.row_len <= 0 || h.row_len > 0x7fffffffLL || h.rows > INT64_MAX / h.row_len) return -1;
  return h.rows * h.row_len;
}

}  // namespace

extern "C" {

int64_t nq_level_rate_ws_words(int64_t n, int n_levels) {
  if (n <= 0 || n_levels < MINK || n_levels > MAXK) return 0;
  const int64_t nb = n / SPAN + (n % SPAN != 0);
  if (nb > INT64_MAX / (n_levels + 1)) return 0;
  return nb * (n_levels + 1);
}

int nq_level_rate(const nq_rate_seg* segs, int nseg, float scale, const float* dyn, float* total, void* ws, int64_t ws_words,
                  nq_stream_t stream) {
  if (!segs || nseg <= 0 || !total || !ws || ws_words <= 0 || !std::isfinite(scale) || scale < 0.f) return NQ_ERR_INVALID;
  // every tensor is checked before the first launch
  int64_t need = 0;
  for (int i = 0; i < nseg; ++i) {
    const nq_rate_seg& h = segs[i];
    if (!h.x || !h.alpha || !h.delta || !h.zp || !h.counts || !h.cost || !h.rate) return NQ_ERR_INVALID;
    if (h.n_levels < MINK || h.n_levels > MAXK) return NQ_ERR_INVALID;
    const int64_t n = rate_elems(h);
    if (n < 0) return NQ_ERR_INVALID;
    const int64_t w = nq_level_rate_ws_words(n, h.n_levels);
    if (w <= 0 || need > INT64_MAX / 4 - w) return NQ_ERR_INVALID;   // the byte count fits int64 too
    need += w;
  }
  if (need > ws_words) return NQ_ERR_INVALID;
  int* base = static_cast<int*>(ws);
  int64_t off = 0;
  int first = 1;
  return RateTable::launch_all(
      segs, nseg,
      [&](int i, RateSegD& d) -> int64_t {
        const nq_rate_seg& h = segs[i];
        d.x = h.x; d.alpha = h.alpha; d.delta = h.delta; d.zp = h.zp; d.dalpha = h.dalpha;
        d.counts = h.counts; d.cost = h.cost; d.rate = h.rate;
        d.n = h.rows * h.row_len; d.row_len = (int)h.row_len; d.per_row = h.per_row ? 1 : 0; d.K = h.n_levels;
        const int64_t nb = rate_blocks(d.n);
        if (nb > 0x7fffffffLL) return NQ_ERR_INVALID;
        d.nblk = (int)nb;
        d.ws_hist = base + off;
        d.ws_part = reinterpret_cast<float*>(base + off + nb * h.n_levels);
        off += nb * (h.n_levels + 1);
        d.vec = (((uintptr_t)h.x | (uintptr_t)h.alpha | (uintptr_t)h.dalpha) & 15) == 0;
        return nb;
      },
      [&](const RateTable& t, unsigned blocks) {
        hipLaunchKernelGGL(rate_hist_kernel, dim3(blocks), dim3(TPB), 0, nq_s(stream), t);
        hipLaunchKernelGGL(rate_finish_kernel, dim3((unsigned)t.nseg), dim3(TPB), 0, nq_s(stream), t);
        hipLaunchKernelGGL(rate_pass_kernel, dim3(blocks), dim3(TPB), 0, nq_s(stream), t, scale, dyn);
        hipLaunchKernelGGL(rate_sum_kernel, dim3(1), dim3(TPB), 0, nq_s(stream), t, total, first);
        first = 0;
      });
}

}  // extern "C"

// Bit allocation under a size budget: the two kernels around the exact Omega table.
//
// The Omega score of an allocation b = (b_0 .. b_{L-1}) is the quadratic form v^T H v of the concatenated per-layer
// perturbations v_l(b_l) = W_l - Q_{b_l}(W_l).  With K bit choices per layer and the n = L K directions e_{l,c} (v_l(c) on
// layer l, zero elsewhere), the Gram matrix G[(l,c),(m,d)] = <e_{l,c}, H e_{m,d}> gives
//     Omega(b) = sum_l sum_m G[(l,b_l),(m,b_m)]                                        exactly, for all K^L allocations.
//
//   nq_rows_dot    the Gram assembly: after one second-order pass, layer l's slice g of H e_j against the K perturbations of
//                  layer l (the rows of V) -> the K entries G[(l,.), j].  Products of two floats are exact in float64; the sums
//                  are float64 in a fixed order (per-thread strided partial sums, a wave tree, the waves of a workgroup in
//                  order, one partial per workgroup, then the workgroups' partials in index order): no atomics, the same
//                  bits from call to call.  g is read once for all K rows.
//   nq_bit_search  the search: every allocation is a mixed-radix index (layer 0 = least significant digit).  A thread decodes
//                  the first index of a run of consecutive indices once and then steps its digits like an odometer; G and the
//                  size table sit in LDS (L K <= 80 whenever K^L < 2^32, i.e. at most 50 KB + 640 B).  Omega of a candidate is
//                  summed l ascending (outer), m ascending (inner), from 0.0, by plain float64 additions -- the order of the
//                  host restatement, so the two compare with ==.  The minimum is lexicographic in (Omega, index): ties go to the
//                  lowest index, a NaN Omega never wins (every comparison with it is false).
#include "nq_common.h"

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / NQ_WAVE;

// ------------------------------------------------------------------------------------------------ rows_dot
constexpr int RD_MAXK = 8;
constexpr int64_t RD_MIN_SPAN = 4096;     // elements per workgroup (16 per thread) ...
constexpr int64_t RD_MAX_BLOCKS = 1024;   // ... grown so that no more than this many partials per row are left to the finish

struct RdPlan {
  int64_t span, blocks;
};

inline RdPlan rd_plan(int64_t n) {
  int64_t span = (n + RD_MAX_BLOCKS - 1) / RD_MAX_BLOCKS;
  span = (span + TPB - 1) / TPB * TPB;
  if (span < RD_MIN_SPAN) span = RD_MIN_SPAN;
  return {span, (n + span - 1) / span};
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// workgroup b owns elements [b span, min(n, (b + 1) span)); ws[r * gridDim.x + b] = its partial sum of row r
__global__ __launch_bounds__(TPB) void rows_dot_kernel(const float* __restrict__ V, const float* __restrict__ g,
                                                       double* __restrict__ ws, int K, int64_t n, int64_t span) {
  __shared__ double s_part[RD_MAXK][WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t lo = (int64_t)blockIdx.x * span;
  const int64_t hi = lo + span < n ? lo + span : n;
  double acc[RD_MAXK];
#pragma unroll
  for (int r = 0; r < RD_MAXK; ++r) acc[r] = 0.0;
  for (int64_t i = lo + tid; i < hi; i += TPB) {
    const double gi = (double)g[i];
#pragma unroll
    for (int r = 0; r < RD_MAXK; ++r)
      if (r < K) acc[r] += (double)V[(int64_t)r * n + i] * gi;
  }
#pragma unroll
  for (int r = 0; r < RD_MAXK; ++r) {
    if (r < K) {   // K is uniform: whole waves take the branch together
      const double s = wave_sum_d(acc[r]);
      if (lane == 0) s_part[r][wave] = s;
    }
  }
  __syncthreads();
  if (tid < K) {
    double s = 0.0;
    for (int w = 0; w < WAVES; ++w) s += s_part[tid][w];
    ws[(int64_t)tid * gridDim.x + blockIdx.x] = s;
  }
}

// one wavefront; thread r adds row r's partials in index order
__global__ __launch_bounds__(64) void rows_dot_finish_kernel(const double* __restrict__ ws, double* __restrict__ out, int K,
                                                             int64_t blocks) {
  const int r = threadIdx.x;
  if (r >= K) return;
  double s = 0.0;
  for (int64_t b = 0; b < blocks; ++b) s += ws[(int64_t)r * blocks + b];
  out[r] = s;
}

// ------------------------------------------------------------------------------------------------ bit_search
constexpr int BS_MAXL = 12;
constexpr int BS_RUN = 8;                  // consecutive indices per odometer run
constexpr int64_t BS_MAX_BLOCKS = 4096;    // the grid strides over the runs beyond this many workgroups
constexpr size_t BS_LDS_LIMIT = 64 * 1024;

struct Best {
  double omega;
  uint64_t index;
};

// lexicographic (omega, index); false whenever a.omega is NaN
__device__ __forceinline__ bool better(double ao, uint64_t ai, double bo, uint64_t bi) { return ao < bo || (ao == bo && ai < bi); }

__device__ __forceinline__ void wave_min(double& o, uint64_t& ix) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const double oo = __shfl_down(o, d, 64);
    const uint64_t oi = (uint64_t)__shfl_down((unsigned long long)ix, d, 64);
    if (better(oo, oi, o, ix)) {
      o = oo;
      ix = oi;
    }
  }
}

// minimum over the workgroup, valid in thread 0
__device__ __forceinline__ void block_min(double& o, uint64_t& ix, double* s_o, uint64_t* s_i) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  wave_min(o, ix);
  if (lane == 0) {
    s_o[wave] = o;
    s_i[wave] = ix;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < WAVES; ++w)
      if (better(s_o[w], s_i[w], o, ix)) {
        o = s_o[w];
        ix = s_i[w];
      }
}

inline size_t bs_lds_bytes(int L, int K) {
  const size_t n = (size_t)L * (size_t)K;
  return n * n * sizeof(double) + n * sizeof(uint64_t);
}

// K^L, or 0 when it reaches 2^32
inline uint64_t bs_total(int L, int K) {
  uint64_t t = 1;
  for (int l = 0; l < L; ++l) {
    t *= (uint64_t)K;
    if (t >= (1ull << 32)) return 0;
  }
  return t;
}

inline int64_t bs_blocks(uint64_t total) {
  const uint64_t runs = (total + BS_RUN - 1) / BS_RUN;
  const uint64_t blocks = (runs + TPB - 1) / TPB;
  return (int64_t)(blocks < (uint64_t)BS_MAX_BLOCKS ? blocks : (uint64_t)BS_MAX_BLOCKS);
}

template <int L>
__global__ __launch_bounds__(TPB) void bit_search_kernel(const double* __restrict__ G, const uint64_t* __restrict__ size_bits,
                                                         int K, uint32_t total, uint64_t budget, Best* __restrict__ ws) {
  extern __shared__ double s_dyn[];
  __shared__ double s_o[WAVES];
  __shared__ uint64_t s_i[WAVES];
  const int n = L * K;
  double* sG = s_dyn;                                      // n x n
  uint64_t* sS = reinterpret_cast<uint64_t*>(s_dyn + n * n);   // n
  for (int i = threadIdx.x; i < n * n; i += TPB) sG[i] = G[i];
  for (int i = threadIdx.x; i < n; i += TPB) sS[i] = size_bits[i];
  __syncthreads();

  double best_o = __builtin_inf();
  uint64_t best_i = ~0ull;
  const uint64_t runs = ((uint64_t)total + BS_RUN - 1) / BS_RUN;
  const uint64_t stride = (uint64_t)gridDim.x * TPB;
  // a thread's runs ascend, and so do the indices inside a run: a strict '<' keeps the lowest index among its ties
  for (uint64_t run = (uint64_t)blockIdx.x * TPB + threadIdx.x; run < runs; run += stride) {
    const uint32_t first = (uint32_t)(run * BS_RUN);
    const uint32_t cnt = total - first < (uint32_t)BS_RUN ? total - first : (uint32_t)BS_RUN;
    int col[L];                                            // col[l] = l K + digit l: the candidate's row / column of G
    uint32_t rest = first;
#pragma unroll
    for (int l = 0; l < L; ++l) {
      col[l] = l * K + (int)(rest % (uint32_t)K);
      rest /= (uint32_t)K;
    }
    for (uint32_t s = 0; s < cnt; ++s) {
      uint64_t size = 0;
#pragma unroll
      for (int l = 0; l < L; ++l) {
        const uint64_t t = size + sS[col[l]];
        size = t < size ? ~0ull : t;                       // saturate: a wrapped sum must not pass for a small one
      }
      if (size <= budget) {
        double omega = 0.0;
#pragma unroll
        for (int l = 0; l < L; ++l) {
          const double* row = sG + col[l] * n;
#pragma unroll
          for (int m = 0; m < L; ++m) omega += row[col[m]];
        }
        if (omega < best_o) {
          best_o = omega;
          best_i = (uint64_t)first + s;
        }
      }
      bool carry = true;                                   // next index: digit 0 steps, a digit that reaches K wraps and carries
#pragma unroll
      for (int l = 0; l < L; ++l) {
        if (carry) {
          const int next = col[l] + 1;
          carry = next == (l + 1) * K;
          col[l] = carry ? l * K : next;
        }
      }
    }
  }
  block_min(best_o, best_i, s_o, s_i);
  if (threadIdx.x == 0) ws[blockIdx.x] = Best{best_o, best_i};
}

__global__ __launch_bounds__(TPB) void bit_search_finish_kernel(const Best* __restrict__ ws, int64_t blocks,
                                                                double* __restrict__ best_omega, uint64_t* __restrict__ best_index) {
  __shared__ double s_o[WAVES];
  __shared__ uint64_t s_i[WAVES];
  double o = __builtin_inf();
  uint64_t ix = ~0ull;
  for (int64_t b = threadIdx.x; b < blocks; b += TPB) {
    const Best c = ws[b];
    if (better(c.omega, c.index, o, ix)) {
      o = c.omega;
      ix = c.index;
    }
  }
  block_min(o, ix, s_o, s_i);
  if (threadIdx.x == 0) {
    best_omega[0] = o;
    best_index[0] = ix;
  }
}

template <int L>
void bs_launch(const double* G, const uint64_t* size_bits, int K, uint32_t total, uint64_t budget, Best* ws, int64_t blocks,
              size_t lds, hipStream_t s) {
  hipLaunchKernelGGL(bit_search_kernel<L>, dim3((unsigned)blocks), dim3(TPB), lds, s, G, size_bits, K, total, budget, ws);
}

}  // namespace

extern "C" {

int64_t nq_rows_dot_ws_bytes(int K, int64_t n) {
  if (K < 1 || K > RD_MAXK || n < 1) return 0;
  return (int64_t)K * rd_plan(n).blocks * (int64_t)sizeof(double);
}

int nq_rows_dot(const float* V, const float* g, double* out, int K, int64_t n, double* ws, nq_stream_t stream) {
  if (!V || !g || !out || !ws || K < 1 || K > RD_MAXK || n < 1) return NQ_ERR_INVALID;
  if (n > (int64_t)0x7fffffffffffffffLL / RD_MAXK) return NQ_ERR_UNSUPPORTED;   // r * n + i stays inside int64
  const RdPlan p = rd_plan(n);
  hipLaunchKernelGGL(rows_dot_kernel, dim3((unsigned)p.blocks), dim3(TPB), 0, nq_s(stream), V, g, ws, K, n, p.span);
  hipLaunchKernelGGL(rows_dot_finish_kernel, dim3(1), dim3(64), 0, nq_s(stream), ws, out, K, p.blocks);
  return nq_launch_status();
}

int64_t nq_bit_search_ws_bytes(int L, int K) {
  if (L < 1 || L > BS_MAXL || K < 1 || K > 8) return 0;
  const uint64_t total = bs_total(L, K);
  if (!total || bs_lds_bytes(L, K) > BS_LDS_LIMIT) return 0;
  return bs_blocks(total) * (int64_t)sizeof(Best);
}

int nq_bit_search(const double* G, const uint64_t* size_bits, int L, int K, uint64_t budget_bits, double* best_omega,
                  uint64_t* best_index, void* ws, nq_stream_t stream) {
  if (!G || !size_bits || !best_omega || !best_index || !ws || L < 1 || K < 1 || K > 8) return NQ_ERR_INVALID;
  if (L > BS_MAXL) return NQ_ERR_UNSUPPORTED;
  const uint64_t total64 = bs_total(L, K);
  const size_t lds = bs_lds_bytes(L, K);
  if (!total64 || lds > BS_LDS_LIMIT) return NQ_ERR_UNSUPPORTED;
  const uint32_t total = (uint32_t)total64;
  const int64_t blocks = bs_blocks(total64);
  Best* part = static_cast<Best*>(ws);
  hipStream_t s = nq_s(stream);
  switch (L) {
    case 1: bs_launch<1>(G, size_bits, K, total, budget_bits, part, blocks, lds, s); break;
    case 2: bs_launch<2>(G, size_bits, K, total, budget_bits, part, blocks, lds, s); break;
    case 3: bs_launch<3>(G, size_bits, K, total, budget_bits, part, blocks, lds, s); break;
    case 4: bs_launch<4>(G, size_bits, K, total, budget_bits, part, blocks, lds, s); break;
    case 5: bs_launch<5>(G, size_bits, K, total, budget_bits, part, blocks, lds, s); break;
    case 6: bs_launch<6>(G, size_bits, K, total, budget_bits, part, blocks, lds, s); break;
    case 7: bs_launch<7>(G, size_bits, K, total, budget_bits, part, blocks, lds, s); break;
    case 8: bs_launch<8>(G, size_bits, K, total, budget_bits, part, blocks, lds, s); break;
    case 9: bs_launch<9>(G, size_bits, K, total, budget_bits, part, blocks, lds, s); break;
    case 10: bs_launch<10>(G, size_bits, K, total, budget_bits, part, blocks, lds, s); break;
    case 11: bs_launch<11>(G, size_bits, K, total, budget_bits, part, blocks, lds, s); break;
    default: bs_launch<12>(G, size_bits, K, total, budget_bits, part, blocks, lds, s); break;
  }
  hipLaunchKernelGGL(bit_search_finish_kernel, dim3(1), dim3(TPB), 0, s, part, blocks, best_omega, best_index);
  return nq_launch_status();
}

}  // extern "C"

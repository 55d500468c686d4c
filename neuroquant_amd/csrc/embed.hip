// Quantised, temporally coded frame embeddings of an HNeRV stream.
//
// The embeddings are x[N][C][HW] (frame, channel, position), E = C * HW values per frame, one (delta, zero_point) pair per
// channel.  A level is the UAQ element of quant_elem.h, level = clamp(rint(x / delta[c]) + zp[c], 0, 2^b - 1); a file stores
// symbols, frame-major (N, E): the levels themselves, or (temporal) frame 0's levels and, for t > 0, the difference to the
// previous frame's level modulo 2^b.  nq_embed_symbols forms them in one fully parallel launch (a thread recomputes its
// predecessor's level from x[t - 1]); nq_embed_restore undoes the differences, one thread per column e, sequential over t
// (neighbouring threads touch neighbouring addresses in every step), and dequantises with the expression of
// nq_unpack_dequant.  It runs once per file on at most a few 10^5 values: no scan.
#include "nq_common.h"

namespace {

constexpr int TPB = 256;

// the level of quant_elem.h's uaq_fwd_elem, before it is scaled back
__device__ __forceinline__ uint32_t embed_level(float xv, float d, float z, float qmax) {
  const float xi = rintf(xv / d) + z;
  return (uint32_t)fminf(fmaxf(xi, 0.f), qmax);   // NaN -> 0 (fmaxf returns the other operand)
}

// One thread per value i = t * E + e.
__global__ __launch_bounds__(TPB) void embed_symbols_kernel(const float* __restrict__ x, const float* __restrict__ delta,
                                                            const float* __restrict__ zp, uint8_t* __restrict__ levels,
                                                            uint8_t* __restrict__ symbols, int64_t n, int64_t E, int64_t HW,
                                                            int n_bits, int temporal) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const int64_t t = i / E;
  const int64_t c = (i - t * E) / HW;
  const float d = delta[c], z = zp[c];
  const uint32_t mask = (1u << n_bits) - 1u;
  const float qmax = (float)mask;
  const uint32_t lv = embed_level(x[i], d, z, qmax);
  uint32_t s = lv;
  if (temporal && t > 0) s = (lv - embed_level(x[i - E], d, z, qmax)) & mask;
  levels[i] = (uint8_t)lv;
  symbols[i] = (uint8_t)s;
}

// One thread per column e, t = 0 .. N - 1 in order.  A symbol arrives as a float that holds an integer in [0, 2^b); anything
// else (a file can hold anything) is clamped to [0, 255] and masked, so the level is always in range.
__global__ __launch_bounds__(TPB) void embed_restore_kernel(const float* __restrict__ sym, const float* __restrict__ delta,
                                                            const float* __restrict__ zp, float* __restrict__ out, int64_t N,
                                                            int64_t E, int64_t HW, int n_bits, int temporal) {
  const int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (e >= E) return;
  const int64_t c = e / HW;
  const float d = delta[c], z = zp[c];
  const uint32_t mask = (1u << n_bits) - 1u;
  uint32_t lv = 0;
  for (int64_t t = 0; t < N; ++t) {
    const int64_t i = t * E + e;
    const uint32_t s = (uint32_t)fminf(fmaxf(sym[i], 0.f), 255.f);
    lv = (temporal ? lv + s : s) & mask;
    out[i] = ((float)lv - z) * d;
  }
}

inline bool grid_ok(int64_t blocks) { return blocks > 0 && blocks <= 0x7fffffffLL; }

// 0, or the error both entries give for these sizes; E and n = N * E on success
inline int embed_sizes(int64_t N, int64_t C, int64_t HW, int n_bits, int temporal, int64_t& E, int64_t& n) {
  if (N <= 0 || C <= 0 || HW <= 0 || n_bits < 2 || n_bits > 8 || (temporal != 0 && temporal != 1)) return NQ_ERR_INVALID;
  if (C > INT64_MAX / HW) return NQ_ERR_UNSUPPORTED;
  E = C * HW;
  if (N > INT64_MAX / E) return NQ_ERR_UNSUPPORTED;
  n = N * E;
  return NQ_OK;
}

}  // namespace

extern "C" {

int nq_embed_symbols(const float* x, const float* delta, const float* zp, int64_t N, int64_t C, int64_t HW, int n_bits,
                     int temporal, uint8_t* levels, uint8_t* symbols, nq_stream_t stream) {
  if (!x || !delta || !zp || !levels || !symbols) return NQ_ERR_INVALID;
  int64_t E = 0, n = 0;
  const int rc = embed_sizes(N, C, HW, n_bits, temporal, E, n);
  if (rc != NQ_OK) return rc;
  const int64_t blocks = (n + TPB - 1) / TPB;
  if (n > INT64_MAX - TPB || !grid_ok(blocks)) return NQ_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(embed_symbols_kernel, dim3((unsigned)blocks), dim3(TPB), 0, nq_s(stream), x, delta, zp, levels, symbols, n,
                     E, HW, n_bits, temporal);
  return nq_launch_status();
}

int nq_embed_restore(const float* sym, const float* delta, const float* zp, int64_t N, int64_t C, int64_t HW, int n_bits,
                     int temporal, float* out, nq_stream_t stream) {
  if (!sym || !delta || !zp || !out) return NQ_ERR_INVALID;
  int64_t E = 0, n = 0;
  const int rc = embed_sizes(N, C, HW, n_bits, temporal, E, n);
  if (rc != NQ_OK) return rc;
  const int64_t blocks = (E + TPB - 1) / TPB;
  if (E > INT64_MAX - TPB || !grid_ok(blocks)) return NQ_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(embed_restore_kernel, dim3((unsigned)blocks), dim3(TPB), 0, nq_s(stream), sym, delta, zp, out, N, E, HW,
                     n_bits, temporal);
  return nq_launch_status();
}

}  // extern "C"

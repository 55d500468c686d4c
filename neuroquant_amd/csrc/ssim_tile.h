// The tile, the window and the two filter passes that ssim_loss.hip and msssim_loss.hip share: a workgroup
// of 256 threads owns an 8 x 118 tile, stages 18 x 128 inputs in LDS, filters along H into LDS (thread = column x group of 4
// rows) and along W in registers (thread = row x group of 4 columns).  Window products are explicit fused multiply-adds with
// the taps in rising order; both files are compiled with -ffp-contract=off, so everything else rounds operation by operation.
// Everything here sits in an unnamed namespace: each file that includes it gets its own copy, with internal linkage.
#pragma once
#include <cstdint>

#include "nq_common.h"

namespace {

constexpr int SL_WIN = 11, SL_HALO = SL_WIN - 1;
constexpr int SL_TH = 8, SL_TW = 118;                             // tile a workgroup owns
constexpr int SL_IH = SL_TH + SL_HALO, SL_IW = SL_TW + SL_HALO;   // staged tile: 18 x 128
constexpr int SL_VS = SL_IW + 4;                                  // row stride of the H-filtered maps (16-byte reads run 4 past)
constexpr int SL_TPB = 256;
constexpr int SL_RG = 4;                                          // rows / columns one thread filters at a time
constexpr int SL_NCG = (SL_TW + SL_RG - 1) / SL_RG;               // column groups of a tile row: 30
static_assert(SL_IW * (SL_TH / SL_RG) == SL_TPB, "one (column, row group) per thread in the H pass");
static_assert(SL_IH % (SL_TPB / SL_IW) == 0, "the staging loop covers the tile's rows exactly");
static_assert(SL_TH * SL_NCG <= SL_TPB, "one (row, column group) per thread in the W pass");
static_assert((SL_NCG - 1) * SL_RG + SL_RG + SL_HALO + 2 <= SL_VS, "the W pass reads inside a row of the filtered maps");

// the window and its sums as msssim.hip states them: exp(-(i-5)^2 / (2 * 1.5^2)) / sum, evaluated in float32; the taps add up
// to G = 0.999999969266355, G^2 in two dimensions
__constant__ float sl_g[SL_WIN] = {0x1.0d957p-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f,
                                   0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d957p-10f};
constexpr float SL_D2 = 6.146728898e-08f;       // 1 - G^2
constexpr float SL_G2D2 = 6.146728520e-08f;     // G^2 (1 - G^2)

// what the shift by the pivots (p of x, q of y) took from g*(xy) - (g*x)(g*y); a = g*x', b = g*y'
__device__ __forceinline__ float sl_shift_term(float p, float q, float a, float b) {
  return SL_D2 * (q * a + p * b) + (p * q) * SL_G2D2;
}

// ---- along H: thread = (column, group of 4 rows); 14 staged rows feed 4 x NM sums, taps in rising order.
//      `value(r, c, m)` hands over the NM quantities of staged element (r, c). ----
template <int NM, typename V>
__device__ __forceinline__ void sl_filter_h(float (*sv)[SL_TH][SL_VS], V value) {
  const int c = threadIdx.x & (SL_IW - 1), r0 = (threadIdx.x / SL_IW) * SL_RG;
  float acc[SL_RG][NM];
#pragma unroll
  for (int j = 0; j < SL_RG; ++j)
#pragma unroll
    for (int q = 0; q < NM; ++q) acc[j][q] = 0.f;
#pragma unroll
  for (int r = 0; r < SL_RG + SL_HALO; ++r) {
    float m[NM];
    value(r0 + r, c, m);
#pragma unroll
    for (int j = 0; j < SL_RG; ++j) {
      const int t = r - j;
      if (t >= 0 && t < SL_WIN) {
#pragma unroll
        for (int q = 0; q < NM; ++q) acc[j][q] = __builtin_fmaf(sl_g[t], m[q], acc[j][q]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < SL_RG; ++j)
#pragma unroll
    for (int q = 0; q < NM; ++q) sv[q][r0 + j][c] = acc[j][q];
}

// ---- along W: row r, columns c0 .. c0 + 3 of the tile from columns c0 .. c0 + 13 of the H-filtered maps ----
template <int NM>
__device__ __forceinline__ void sl_filter_w(const float (*sv)[SL_TH][SL_VS], int r, int c0, float (*acc)[NM]) {
#pragma unroll
  for (int q = 0; q < NM; ++q) {
    float v[SL_RG + SL_HALO + 2];
#pragma unroll
    for (int k = 0; k < (SL_RG + SL_HALO + 2) / 4; ++k) {
      const float4 t = *reinterpret_cast<const float4*>(&sv[q][r][c0 + 4 * k]);
      v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w;
    }
#pragma unroll
    for (int j = 0; j < SL_RG; ++j) {
      float a = 0.f;
#pragma unroll
      for (int t = 0; t < SL_WIN; ++t) a = __builtin_fmaf(sl_g[t], v[j + t], a);
      acc[j][q] = a;
    }
  }
}

__device__ __forceinline__ double sl_wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// Sums of a and of b over the workgroup (a multiple of 64 threads, at most 256) in a fixed order; valid in thread 0.
__device__ __forceinline__ void sl_block_sum2(double& a, double& b, double (*red)[2]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  a = sl_wave_sum_d(a);
  b = sl_wave_sum_d(b);
  if (lane == 0) {
    red[wave][0] = a;
    red[wave][1] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int i = 1; i < nw; ++i) {
      a += red[i][0];
      b += red[i][1];
    }
}

}  // namespace

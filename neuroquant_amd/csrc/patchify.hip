// The HNeRV encoder's downsampling stages (reference models/_layers.py: ConvNeXt.downsample_layers) for the trainer: a
// stride-s, kernel-s "patchify" convolution fused with the channels-first LayerNorm next to it, forward and backward in fp32,
// NCHW in and out.  The definition is in include/nq_hip.h (nq_patchify_ln_forward), the design in DESIGN.md §28.
//
//   forward   pf_stats        'pre' only: mu and rstd of every input pixel, one pixel per lane, coalesced channel planes
//             pf_product      (MODE 0 / 1) the product over gathered patches on the 16x16x4 fp32 MFMA, 16 output pixels per
//                             wave and all C_out rows in the accumulators; 'pre' normalises on the operand load, 'post' runs
//                             the LayerNorm on the accumulators and saves mu, rstd per output pixel
//   backward  pf_product      (MODE 2, 'post') y again from x, the LayerNorm backward on the accumulators -> g = dL/dy (NCHW,
//                             workspace) and the per-channel partial sums of d ln_w, d ln_b
//             pf_dgrad        dx = W^T g per (tile, kernel row): the 16 rows of an accumulator tile are 16 channels of ONE input
//                             pixel, so the 'pre' LayerNorm backward runs on the accumulators and dx is written directly;
//                             zeroes the ignored remainder rows and columns
//             pf_wgrad        d conv_w and d conv_b (a column of ones) with the output pixels as the K dimension, per wave one
//                             partial of a 64-column chunk
//             pf_finish       every parameter gradient = the sum of its partials in partial order, in double
//
// MFMA 16x16x4 fp32 operand layout (wave64, lane l, li = l % 16, kq = l / 16): A[li][k = kq], B[k = kq][n = li],
// D[m = 4 kq + r][n = li] in accumulator register r.  The forward's k <-> (c, i, j) map is
// c = 4 g + kq, one step per (i, g, j): a lane's s steps of one (i, g) read ONE row segment x[c][s h_o + i][s w_o .. + s - 1]
// and ONE segment conv_w[o][c][i][0 .. s - 1] (16-byte loads at s = 4, 8-byte loads at s = 2, scalar loads otherwise).
#include "nq_common.h"

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int PF_MAXG = 256;       // workgroups of pf_product / pf_dgrad at most (the per-channel partials)
constexpr int PF_WSPLIT = 32;      // pixel splits of pf_wgrad at most
constexpr int PF_KTW = 4;          // 16-column tiles of conv_w's gradient per pf_wgrad workgroup
constexpr int PF_WPART_CAP = 1 << 19;   // pf_wgrad: splits * C_out (K + 1) stays below this (4 wave partials per split)

__device__ __forceinline__ v4f pf_mfma(float a, float b, v4f c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

struct PfDims {
  int N, Cin, H, W, Cout, Ho, Wo, K;
  int64_t HW, HoWo;
  int P, ntiles;      // output pixels N Ho Wo, 16-pixel tiles
  int ksplit;         // pf_product: 1 (a wave per tile) or 4 (the waves of a workgroup split the channel groups of one tile)
  int xvec;           // row segments of x / mu / rstd are aligned for the vector load of this s
};

// s consecutive floats at p (zeros unless ok); one 16- / 8-byte load where the segment is aligned for it
template <int S>
__device__ __forceinline__ void pf_seg(float (&v)[S], const float* __restrict__ p, bool ok, bool vec) {
  if constexpr (S == 4) {
    if (vec) {
      const float4 t = ok ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
      v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
      return;
    }
  }
  if constexpr (S == 2) {
    if (vec) {
      const float2 t = ok ? *reinterpret_cast<const float2*>(p) : make_float2(0.f, 0.f);
      v[0] = t.x, v[1] = t.y;
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < S; ++j) v[j] = ok ? p[j] : 0.f;
}

// sum over the 16 lanes that share kq (the pixels of a tile); every lane of the group gets it, in a fixed order
__device__ __forceinline__ float pf_sum16(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 8, 64);
  return v;
}
// sum over the 4 lanes li, li + 16, li + 32, li + 48 that hold the channels of one pixel
__device__ __forceinline__ float pf_sum_kq(float v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

struct PfPix {
  int n, ho, wo, hw;
  bool valid;
};
__device__ __forceinline__ PfPix pf_pixel(int q, const PfDims& d) {
  PfPix p;
  p.valid = q < d.P;
  const int qq = p.valid ? q : 0;
  p.n = qq / (int)d.HoWo;
  p.hw = qq - p.n * (int)d.HoWo;
  p.ho = p.hw / d.Wo;
  p.wo = p.hw - p.ho * d.Wo;
  return p;
}

// ---- 'pre' forward, pass 1: LayerNorm statistics of every input pixel ----
__global__ __launch_bounds__(256) void pf_stats(const float* __restrict__ x, float* __restrict__ mu, float* __restrict__ rstd, int C,
                                                int64_t HW, int64_t total) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= total) return;
  const int64_t n = q / HW, hw = q - n * HW;
  const float* __restrict__ p = x + n * C * HW + hw;
  float s = 0.f;
  for (int c = 0; c < C; ++c) s += p[(int64_t)c * HW];
  const float mean = s / (float)C;
  float v = 0.f;
  for (int c = 0; c < C; ++c) {
    const float e = p[(int64_t)c * HW] - mean;
    v = __builtin_fmaf(e, e, v);
  }
  mu[q] = mean;
  rstd[q] = 1.0f / sqrtf(v / (float)C + 1e-6f);
}

// ---- the product over gathered patches.  MODE 0: out = LNcf(conv(x)) ('post' forward), 1: out = conv(LNcf(x)) ('pre'
// forward), 2: 'post' backward, y again and g = the LayerNorm backward of dy ----
template <int CT, int S, int MODE>
__global__ __launch_bounds__(256) void pf_product(const float* __restrict__ x, const float* __restrict__ w,
                                                  const float* __restrict__ cb, const float* __restrict__ ln_w,
                                                  const float* __restrict__ ln_b, float* mu, float* rstd,
                                                  const float* __restrict__ dy, float* __restrict__ out,
                                                  float* __restrict__ chanpart, PfDims d) {
  constexpr bool PRE = MODE == 1;
  __shared__ float part[3][CT * 256];     // ksplit = 4: the accumulators of waves 1 .. 3, [ct][r][lane]
  __shared__ float red[4][2][CT * 16];    // MODE 2: per-wave channel sums
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, kq = lane >> 4;
  const int ks = d.ksplit, CG = (d.Cin + 3) >> 2;
  const bool owner = ks == 1 || wave == 0;
  float pc[2][CT][4];   // MODE 2: d ln_w, d ln_b of channel ct 16 + 4 kq + r over this lane's pixels
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) pc[k][ct][r] = 0.f;
  // ksplit = 4: every wave of the workgroup walks the same tiles (uniform barriers); ksplit = 1: a tile per wave, no barrier
  const int t0 = ks == 1 ? blockIdx.x * 4 + wave : blockIdx.x, tstep = ks == 1 ? gridDim.x * 4 : gridDim.x;
  for (int t = t0; t < d.ntiles; t += tstep) {
    const int q = t * 16 + li;
    const PfPix px = pf_pixel(q, d);
    v4f acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[ct] = v4f{0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < S; ++i) {
      const int64_t rowoff = (int64_t)(S * px.ho + i) * d.W + S * px.wo;   // of the row segment within a plane
      float m[S], rs[S];
      if constexpr (PRE) {
        pf_seg<S>(m, mu + (int64_t)px.n * d.HW + rowoff, px.valid, d.xvec);
        pf_seg<S>(rs, rstd + (int64_t)px.n * d.HW + rowoff, px.valid, d.xvec);
      }
      for (int g = ks == 1 ? 0 : wave; g < CG; g += ks) {
        const int c = 4 * g + kq;
        const bool cv = c < d.Cin, bv = cv && px.valid;
        float b[S];
        pf_seg<S>(b, x + ((int64_t)px.n * d.Cin + (cv ? c : 0)) * d.HW + rowoff, bv, d.xvec);
        if constexpr (PRE) {
          const float lw = cv ? ln_w[c] : 0.f, lb = cv ? ln_b[c] : 0.f;
#pragma unroll
          for (int j = 0; j < S; ++j) b[j] = bv ? __builtin_fmaf((b[j] - m[j]) * rs[j], lw, lb) : 0.f;
        }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const int o = ct * 16 + li;
          const bool ov = cv && o < d.Cout;
          float a[S];
          pf_seg<S>(a, w + (int64_t)(ov ? o : 0) * d.K + ((cv ? c : 0) * S + i) * S, ov, true);
#pragma unroll
          for (int j = 0; j < S; ++j) acc[ct] = pf_mfma(a[j], b[j], acc[ct]);
        }
      }
    }
    if (ks != 1) {   // sum the four channel-group shares in wave order
      if (wave)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) part[wave - 1][(ct * 4 + r) * 64 + lane] = acc[ct][r];
      __syncthreads();
      if (!wave)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int e = (ct * 4 + r) * 64 + lane;
            acc[ct][r] = ((acc[ct][r] + part[0][e]) + part[1][e]) + part[2][e];
          }
      __syncthreads();
    }
    if (!owner) continue;
    // y[o][pixel] with o = ct 16 + 4 kq + r: a pixel's channels sit in 4 registers x CT tiles x the 4 lanes li + 16 kq
    float y[CT][4];
    float s = 0.f;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = ct * 16 + 4 * kq + r;
        const bool ov = o < d.Cout;
        y[ct][r] = ov ? acc[ct][r] + cb[o] : 0.f;
        s += y[ct][r];
      }
    if constexpr (MODE == 1) {
      if (px.valid)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int o = ct * 16 + 4 * kq + r;
            if (o < d.Cout) out[((int64_t)px.n * d.Cout + o) * d.HoWo + px.hw] = y[ct][r];
          }
    } else if constexpr (MODE == 0) {
      const float inv = 1.0f / (float)d.Cout;
      const float mean = pf_sum_kq(s) * inv;
      float v = 0.f;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool ov = ct * 16 + 4 * kq + r < d.Cout;
          y[ct][r] = ov ? y[ct][r] - mean : 0.f;
          v = __builtin_fmaf(y[ct][r], y[ct][r], v);
        }
      const float rsd = 1.0f / sqrtf(pf_sum_kq(v) * inv + 1e-6f);
      if (px.valid) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int o = ct * 16 + 4 * kq + r;
            if (o < d.Cout) out[((int64_t)px.n * d.Cout + o) * d.HoWo + px.hw] = __builtin_fmaf(y[ct][r] * rsd, ln_w[o], ln_b[o]);
          }
        if (kq == 0) mu[q] = mean, rstd[q] = rsd;
      }
    } else {
      const float mean = px.valid ? mu[q] : 0.f, rsd = px.valid ? rstd[q] : 0.f;
      float dyh[CT][4], s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int o = ct * 16 + 4 * kq + r;
          const bool ov = px.valid && o < d.Cout;
          const float dyv = ov ? dy[((int64_t)px.n * d.Cout + o) * d.HoWo + px.hw] : 0.f;
          y[ct][r] = ov ? (y[ct][r] - mean) * rsd : 0.f;     // yhat
          pc[0][ct][r] = __builtin_fmaf(dyv, y[ct][r], pc[0][ct][r]);
          pc[1][ct][r] += dyv;
          dyh[ct][r] = ov ? dyv * ln_w[o] : 0.f;
          s1 += dyh[ct][r];
          s2 = __builtin_fmaf(dyh[ct][r], y[ct][r], s2);
        }
      const float inv = 1.0f / (float)d.Cout;
      s1 = pf_sum_kq(s1) * inv;
      s2 = pf_sum_kq(s2) * inv;
      if (px.valid)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int o = ct * 16 + 4 * kq + r;
            if (o < d.Cout) out[((int64_t)px.n * d.Cout + o) * d.HoWo + px.hw] = rsd * ((dyh[ct][r] - s1) - y[ct][r] * s2);
          }
    }
  }
  if constexpr (MODE == 2) {
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = pf_sum16(pc[k][ct][r]);
          if (li == 0) red[wave][k][ct * 16 + 4 * kq + r] = v;
        }
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * CT * 16; e += 256) {
      const int k = e / (CT * 16), o = e - k * (CT * 16);
      if (o < d.Cout) chanpart[((int64_t)blockIdx.x * 2 + k) * d.Cout + o] = ((red[0][k][o] + red[1][k][o]) + red[2][k][o]) + red[3][k][o];
    }
  }
}

// ---- data gradient: item (tile, i) per wave; acc[j][cti] = dz[c = cti 16 + 4 kq + r] of input pixel (s h_o + i, s w_o + j).
// PRE: g = dy, the LayerNorm backward on the accumulators, per-channel partial sums of d ln_w, d ln_b per workgroup ----
template <int CTI, int S, bool PRE>
__global__ __launch_bounds__(256) void pf_dgrad(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ w,
                                                const float* __restrict__ mu, const float* __restrict__ rstd,
                                                const float* __restrict__ ln_w, float* __restrict__ dx, float* __restrict__ chanpart,
                                                PfDims d) {
  __shared__ float red[4][2][CTI * 16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, kq = lane >> 4;
  float pc[2][CTI][4];
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int cti = 0; cti < CTI; ++cti)
#pragma unroll
      for (int r = 0; r < 4; ++r) pc[k][cti][r] = 0.f;
  const int64_t items = (int64_t)d.ntiles * S;
  for (int64_t it = (int64_t)blockIdx.x * 4 + wave; it < items; it += (int64_t)gridDim.x * 4) {
    const int t = (int)(it / S), i = (int)(it - (int64_t)t * S);
    const PfPix px = pf_pixel(t * 16 + li, d);
    v4f acc[S][CTI];
#pragma unroll
    for (int j = 0; j < S; ++j)
#pragma unroll
      for (int cti = 0; cti < CTI; ++cti) acc[j][cti] = v4f{0.f, 0.f, 0.f, 0.f};
    for (int tt = 0; tt < d.Cout / 4; ++tt) {
      const int o = 4 * tt + kq;
      const float b = px.valid ? g[((int64_t)px.n * d.Cout + o) * d.HoWo + px.hw] : 0.f;
#pragma unroll
      for (int cti = 0; cti < CTI; ++cti) {
        const int c = cti * 16 + li;
        const bool cv = c < d.Cin;
        float a[S];
        pf_seg<S>(a, w + (int64_t)o * d.K + ((cv ? c : 0) * S + i) * S, cv, true);
#pragma unroll
        for (int j = 0; j < S; ++j) acc[j][cti] = pf_mfma(a[j], b, acc[j][cti]);
      }
    }
    const int64_t rowoff = (int64_t)(S * px.ho + i) * d.W + S * px.wo;
#pragma unroll
    for (int j = 0; j < S; ++j) {
      if constexpr (PRE) {
        const int64_t pix = (int64_t)px.n * d.HW + rowoff + j;
        const float m = px.valid ? mu[pix] : 0.f, rs = px.valid ? rstd[pix] : 0.f;
        float xh[CTI][4], dxh[CTI][4], s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int cti = 0; cti < CTI; ++cti)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = cti * 16 + 4 * kq + r;
            const bool cv = px.valid && c < d.Cin;
            const float xv = cv ? x[((int64_t)px.n * d.Cin + c) * d.HW + rowoff + j] : 0.f;
            const float dz = cv ? acc[j][cti][r] : 0.f;
            xh[cti][r] = cv ? (xv - m) * rs : 0.f;
            pc[0][cti][r] = __builtin_fmaf(dz, xh[cti][r], pc[0][cti][r]);
            pc[1][cti][r] += dz;
            dxh[cti][r] = cv ? dz * ln_w[c] : 0.f;
            s1 += dxh[cti][r];
            s2 = __builtin_fmaf(dxh[cti][r], xh[cti][r], s2);
          }
        const float inv = 1.0f / (float)d.Cin;
        s1 = pf_sum_kq(s1) * inv;
        s2 = pf_sum_kq(s2) * inv;
        if (px.valid && dx)
#pragma unroll
          for (int cti = 0; cti < CTI; ++cti)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int c = cti * 16 + 4 * kq + r;
              if (c < d.Cin) dx[((int64_t)px.n * d.Cin + c) * d.HW + rowoff + j] = rs * ((dxh[cti][r] - s1) - xh[cti][r] * s2);
            }
      } else {
        if (px.valid)
#pragma unroll
          for (int cti = 0; cti < CTI; ++cti)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int c = cti * 16 + 4 * kq + r;
              if (c < d.Cin) dx[((int64_t)px.n * d.Cin + c) * d.HW + rowoff + j] = acc[j][cti][r];
            }
      }
    }
  }
  // the remainder the convolution never read: rows past s Ho of every plane, then columns past s Wo of the rows above
  if (dx) {
    const int RH = d.H - S * d.Ho, RW = d.W - S * d.Wo;
    const int64_t rows_e = (int64_t)RH * d.W, R = rows_e + (int64_t)S * d.Ho * RW, total = R * d.N * d.Cin;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
      const int64_t plane = e / R;
      int64_t r = e - plane * R, h, ww;
      if (r < rows_e) {
        h = S * d.Ho + r / d.W, ww = r % d.W;
      } else {
        r -= rows_e;
        h = r / RW, ww = S * d.Wo + r % RW;
      }
      dx[plane * d.HW + h * d.W + ww] = 0.f;
    }
  }
  if constexpr (PRE) {
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int cti = 0; cti < CTI; ++cti)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = pf_sum16(pc[k][cti][r]);
          if (li == 0) red[wave][k][cti * 16 + 4 * kq + r] = v;
        }
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * CTI * 16; e += 256) {
      const int k = e / (CTI * 16), c = e - k * (CTI * 16);
      if (c < d.Cin) chanpart[((int64_t)blockIdx.x * 2 + k) * d.Cin + c] = ((red[0][k][c] + red[1][k][c]) + red[2][k][c]) + red[3][k][c];
    }
  }
}

// ---- weight gradient: workgroup (pixel split, chunk of 64 columns k of [conv_w | 1]) -> per wave one partial of
// dW[o][k] = sum_p g[o][p] z[k][p]; column K is the bias gradient (z = 1).  PRE: z = LNcf(x) on the load ----
template <int CT, int S, bool PRE>
__global__ __launch_bounds__(256) void pf_wgrad(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ mu,
                                                const float* __restrict__ rstd, const float* __restrict__ ln_w,
                                                const float* __restrict__ ln_b, float* __restrict__ wpart, PfDims d) {
  constexpr int LDP = 17;
  __shared__ float sg[4][CT * 16 * LDP];   // per wave g[o][p] of its tile
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, kq = lane >> 4;
  float* S_g = sg[wave];
  // this lane's columns k = kbase + kt 16 + li: 1 = a tap (c, i, j) of the patch, 2 = the column of ones, 0 = padding
  int kind[PF_KTW], poff[PF_KTW];
  int64_t xoff[PF_KTW];
  float lw[PF_KTW], lb[PF_KTW];
#pragma unroll
  for (int kt = 0; kt < PF_KTW; ++kt) {
    const int k = (blockIdx.y * PF_KTW + kt) * 16 + li;
    kind[kt] = k < d.K ? 1 : k == d.K ? 2 : 0;
    const int kk = k < d.K ? k : 0;
    const int c = kk / (S * S), ij = kk - c * (S * S), i = ij / S, j = ij - i * S;
    poff[kt] = i * d.W + j;
    xoff[kt] = (int64_t)c * d.HW + poff[kt];
    lw[kt] = PRE ? ln_w[c] : 1.f;
    lb[kt] = PRE ? ln_b[c] : 0.f;
  }
  v4f acc[PF_KTW][CT];
#pragma unroll
  for (int kt = 0; kt < PF_KTW; ++kt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[kt][ct] = v4f{0.f, 0.f, 0.f, 0.f};
  // every wave of the workgroup runs the same number of rounds (a tile past the end is all zeros): the barriers are uniform
  for (int base = blockIdx.x * 4; base < d.ntiles; base += gridDim.x * 4) {
    const int t = base + wave;
    const PfPix px = pf_pixel(t < d.ntiles ? t * 16 + li : d.P, d);
#pragma unroll
    for (int e = 0; e < CT * 4; ++e) {
      const int o = 4 * e + kq;
      S_g[o * LDP + li] = (px.valid && o < d.Cout) ? g[((int64_t)px.n * d.Cout + o) * d.HoWo + px.hw] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int t4 = 0; t4 < 4; ++t4) {
      const int p = 4 * t4 + kq;
      const PfPix pp = pf_pixel(t < d.ntiles ? t * 16 + p : d.P, d);
      const int64_t pixoff = (int64_t)(S * pp.ho) * d.W + S * pp.wo;
      float b[PF_KTW];
#pragma unroll
      for (int kt = 0; kt < PF_KTW; ++kt) {
        float v = 0.f;
        if (pp.valid && kind[kt] == 1) {
          v = x[(int64_t)pp.n * d.Cin * d.HW + xoff[kt] + pixoff];
          if constexpr (PRE) {
            const int64_t pix = (int64_t)pp.n * d.HW + pixoff + poff[kt];
            v = __builtin_fmaf((v - mu[pix]) * rstd[pix], lw[kt], lb[kt]);
          }
        } else if (pp.valid && kind[kt] == 2) {
          v = 1.f;
        }
        b[kt] = v;
      }
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const float a = S_g[(ct * 16 + li) * LDP + p];
#pragma unroll
        for (int kt = 0; kt < PF_KTW; ++kt) acc[kt][ct] = pf_mfma(a, b[kt], acc[kt][ct]);
      }
    }
    __syncthreads();
  }
  float* __restrict__ o_ = wpart + ((int64_t)blockIdx.x * 4 + wave) * ((int64_t)d.Cout * (d.K + 1));
#pragma unroll
  for (int kt = 0; kt < PF_KTW; ++kt) {
    const int k = (blockIdx.y * PF_KTW + kt) * 16 + li;
    if (k <= d.K)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int o = ct * 16 + 4 * kq + r;
          if (o < d.Cout) o_[(int64_t)o * (d.K + 1) + k] = acc[kt][ct][r];
        }
  }
}

// ---- finish: element e of {[d conv_w | d conv_b][o][K + 1] | d ln_w | d ln_b} ----
__global__ __launch_bounds__(256) void pf_finish(const float* __restrict__ wpart, int np, const float* __restrict__ chanpart, int ng,
                                                 int Cout, int K, int Cl, float* __restrict__ d_w, float* __restrict__ d_b,
                                                 float* __restrict__ d_ln_w, float* __restrict__ d_ln_b) {
  const int wsz = Cout * (K + 1);
  int e = blockIdx.x * 256 + threadIdx.x;
  double s = 0.0;
  if (e < wsz) {
    for (int p = 0; p < np; ++p) s += (double)wpart[(int64_t)p * wsz + e];
    const int o = e / (K + 1), k = e - o * (K + 1);
    if (k < K) d_w[o * K + k] = (float)s;
    else d_b[o] = (float)s;
    return;
  }
  e -= wsz;
  if (e < 2 * Cl) {
    for (int p = 0; p < ng; ++p) s += (double)chanpart[(int64_t)p * 2 * Cl + e];
    (e < Cl ? d_ln_w : d_ln_b)[e < Cl ? e : e - Cl] = (float)s;
  }
}

// ---- host: one plan per shape, shared by the workspace query and the launches ----
struct PfPlan {
  PfDims d;
  int pre;
  int Gf;                 // workgroups of pf_product
  int Gd;                 // workgroups of pf_dgrad
  int Gc;                 // per-channel partials: Gd ('pre') or Gf ('post')
  int Sw, nchunk;         // pf_wgrad: pixel splits (4 Sw wave partials), 64-column chunks
  int64_t off_chan, off_w, ws_floats;   // float offsets into the workspace (g of 'post' at 0)
};

int pf_plan(int N, int Cin, int H, int W, int Cout, int s, int order, PfPlan& p) {
  if (order != NQ_PATCHIFY_POST && order != NQ_PATCHIFY_PRE) return NQ_ERR_INVALID;
  if (s < 2 || s > 5 || N < 1 || H < s || W < s) return NQ_ERR_INVALID;
  if (Cout < 8 || Cout > 64 || (Cout & 7)) return NQ_ERR_INVALID;
  const bool cin8 = Cin >= 8 && Cin <= 64 && !(Cin & 7);
  if (!(cin8 || (Cin == 3 && order == NQ_PATCHIFY_POST))) return NQ_ERR_INVALID;
  const int Ho = H / s, Wo = W / s;
  const int64_t HW = (int64_t)H * W, HoWo = (int64_t)Ho * Wo, lim = (int64_t)1 << 31;
  if (HW >= lim || HW * Cin >= lim || HW * Cin * N >= lim || HoWo * Cout * N >= lim) return NQ_ERR_INVALID;
  const int64_t P = HoWo * N;
  PfDims& d = p.d;
  d = PfDims{N, Cin, H, W, Cout, Ho, Wo, Cin * s * s, HW, HoWo, (int)P, (int)((P + 15) / 16), 1, 0};
  d.xvec = (s == 4 || s == 2) && W % s == 0;
  d.ksplit = (d.ntiles < 1024 && (Cin + 3) / 4 >= 4) ? 4 : 1;
  p.pre = order == NQ_PATCHIFY_PRE;
  const int64_t wgf = d.ksplit == 1 ? (d.ntiles + 3) / 4 : d.ntiles, wgd = ((int64_t)d.ntiles * s + 3) / 4;
  p.Gf = (int)(wgf < PF_MAXG ? wgf : PF_MAXG);
  p.Gd = (int)(wgd < PF_MAXG ? wgd : PF_MAXG);
  p.Gc = p.pre ? p.Gd : p.Gf;
  const int wsz = Cout * (d.K + 1);
  int sw = (d.ntiles + 3) / 4;
  if (sw > PF_WSPLIT) sw = PF_WSPLIT;
  const int cap = PF_WPART_CAP / wsz > 1 ? PF_WPART_CAP / wsz : 1;
  p.Sw = sw < cap ? sw : cap;
  p.nchunk = (d.K + 1 + 16 * PF_KTW - 1) / (16 * PF_KTW);
  p.off_chan = p.pre ? 0 : P * Cout;
  p.off_w = p.off_chan + (int64_t)p.Gc * 2 * (p.pre ? Cin : Cout);
  p.ws_floats = p.off_w + (int64_t)p.Sw * 4 * wsz;
  return NQ_OK;
}

bool pf_aligned(const void* a) { return a && (reinterpret_cast<uintptr_t>(a) & 15) == 0; }

#define PF_S_SWITCH(S, CALL)                       \
  switch (S) {                                     \
    case 2: { constexpr int SS = 2; CALL; } break; \
    case 3: { constexpr int SS = 3; CALL; } break; \
    case 4: { constexpr int SS = 4; CALL; } break; \
    default: { constexpr int SS = 5; CALL; } break; \
  }
// TT = 16-row tiles of C (1 .. 4), SS = s
#define PF_DISPATCH(C, S, CALL)                                  \
  switch (((C) + 15) / 16) {                                     \
    case 1: { constexpr int TT = 1; PF_S_SWITCH(S, CALL) } break; \
    case 2: { constexpr int TT = 2; PF_S_SWITCH(S, CALL) } break; \
    case 3: { constexpr int TT = 3; PF_S_SWITCH(S, CALL) } break; \
    default: { constexpr int TT = 4; PF_S_SWITCH(S, CALL) } break; \
  }

template <int CT, int S>
void pf_launch_product(int mode, const float* x, const float* w, const float* cb, const float* ln_w, const float* ln_b, float* mu,
                       float* rstd, const float* dy, float* out, float* chanpart, const PfPlan& p, hipStream_t st) {
  if (mode == 0) pf_product<CT, S, 0><<<p.Gf, 256, 0, st>>>(x, w, cb, ln_w, ln_b, mu, rstd, dy, out, chanpart, p.d);
  else if (mode == 1) pf_product<CT, S, 1><<<p.Gf, 256, 0, st>>>(x, w, cb, ln_w, ln_b, mu, rstd, dy, out, chanpart, p.d);
  else pf_product<CT, S, 2><<<p.Gf, 256, 0, st>>>(x, w, cb, ln_w, ln_b, mu, rstd, dy, out, chanpart, p.d);
}

template <int CTI, int S>
void pf_launch_dgrad(const float* g, const float* x, const float* w, const float* mu, const float* rstd, const float* ln_w,
                     float* dx, float* chanpart, const PfPlan& p, hipStream_t st) {
  if (p.pre) pf_dgrad<CTI, S, true><<<p.Gd, 256, 0, st>>>(g, x, w, mu, rstd, ln_w, dx, chanpart, p.d);
  else pf_dgrad<CTI, S, false><<<p.Gd, 256, 0, st>>>(g, x, w, mu, rstd, ln_w, dx, chanpart, p.d);
}

template <int CT, int S>
void pf_launch_wgrad(const float* g, const float* x, const float* mu, const float* rstd, const float* ln_w, const float* ln_b,
                     float* wpart, const PfPlan& p, hipStream_t st) {
  const dim3 grid(p.Sw, p.nchunk);
  if (p.pre) pf_wgrad<CT, S, true><<<grid, 256, 0, st>>>(g, x, mu, rstd, ln_w, ln_b, wpart, p.d);
  else pf_wgrad<CT, S, false><<<grid, 256, 0, st>>>(g, x, mu, rstd, ln_w, ln_b, wpart, p.d);
}

}  // namespace

extern "C" {

NQ_API int64_t nq_patchify_ln_ws_bytes(int N, int Cin, int H, int W, int Cout, int s, int order) {
  PfPlan p;
  return pf_plan(N, Cin, H, W, Cout, s, order, p) == NQ_OK ? p.ws_floats * 4 : 0;
}

NQ_API int nq_patchify_ln_forward(const float* x, const float* conv_w, const float* conv_b, const float* ln_w, const float* ln_b,
                                  float* out, float* mu, float* rstd, int N, int Cin, int H, int W, int Cout, int s, int order,
                                  nq_stream_t stream) {
  PfPlan p;
  int rc = pf_plan(N, Cin, H, W, Cout, s, order, p);
  if (rc != NQ_OK) return rc;
  for (const void* a : {(const void*)x, (const void*)conv_w, (const void*)conv_b, (const void*)ln_w, (const void*)ln_b,
                        (const void*)out, (const void*)mu, (const void*)rstd})
    if (!pf_aligned(a)) return NQ_ERR_INVALID;
  hipStream_t st = nq_s(stream);
  if (p.pre) {
    const int64_t total = (int64_t)N * p.d.HW;
    pf_stats<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(x, mu, rstd, Cin, p.d.HW, total);
  }
  PF_DISPATCH(Cout, s, (pf_launch_product<TT, SS>(p.pre, x, conv_w, conv_b, ln_w, ln_b, mu, rstd, nullptr, out, nullptr, p, st)))
  return nq_launch_status();
}

NQ_API int nq_patchify_ln_backward(const float* dy, const float* x, const float* mu, const float* rstd, const float* conv_w,
                                   const float* conv_b, const float* ln_w, const float* ln_b, float* dx, float* d_conv_w,
                                   float* d_conv_b, float* d_ln_w, float* d_ln_b, void* ws, int64_t ws_bytes, int N, int Cin, int H,
                                   int W, int Cout, int s, int order, nq_stream_t stream) {
  PfPlan p;
  int rc = pf_plan(N, Cin, H, W, Cout, s, order, p);
  if (rc != NQ_OK) return rc;
  for (const void* a : {(const void*)dy, (const void*)x, (const void*)mu, (const void*)rstd, (const void*)conv_w, (const void*)conv_b,
                        (const void*)ln_w, (const void*)ln_b, (const void*)ws})
    if (!pf_aligned(a)) return NQ_ERR_INVALID;
  if (dx && !pf_aligned(dx)) return NQ_ERR_INVALID;
  for (const void* a : {(const void*)d_conv_w, (const void*)d_conv_b, (const void*)d_ln_w, (const void*)d_ln_b})
    if (!a) return NQ_ERR_INVALID;
  if (ws_bytes < p.ws_floats * 4) return NQ_ERR_INVALID;
  float* wsf = static_cast<float*>(ws);
  float* chanpart = wsf + p.off_chan;
  hipStream_t st = nq_s(stream);
  const float* g = dy;   // what the two products of the backward contract with: dy ('pre') or dL/d conv(x) ('post')
  if (!p.pre) {
    PF_DISPATCH(Cout, s, (pf_launch_product<TT, SS>(2, x, conv_w, conv_b, ln_w, ln_b, const_cast<float*>(mu),
                                                     const_cast<float*>(rstd), dy, wsf, chanpart, p, st)))
    g = wsf;
  }
  if (p.pre || dx) PF_DISPATCH(Cin, s, (pf_launch_dgrad<TT, SS>(g, x, conv_w, mu, rstd, ln_w, dx, chanpart, p, st)))
  PF_DISPATCH(Cout, s, (pf_launch_wgrad<TT, SS>(g, x, mu, rstd, ln_w, ln_b, wsf + p.off_w, p, st)))
  const int nout = Cout * (p.d.K + 1) + 2 * (p.pre ? Cin : Cout);
  pf_finish<<<(nout + 255) / 256, 256, 0, st>>>(wsf + p.off_w, 4 * p.Sw, chanpart, p.Gc, Cout, p.d.K, p.pre ? Cin : Cout, d_conv_w,
                                                d_conv_b, d_ln_w, d_ln_b);
  return nq_launch_status();
}

}  // extern "C"

// ConvNeXt encoder block (reference models/_layers.py: Block) for the trainer: forward and backward in fp32, NCHW in and
// out.  The definition is in include/nq_hip.h (nq_convnext_block_forward), the design in DESIGN.md §27.
//
//   forward   cx_dwln_fwd   depthwise 7x7 + LayerNorm statistics, one pixel per lane, the C outputs of a pixel in registers;
//                           writes xhat (channels-last) and rstd
//             cx_mlp_fwd    both pointwise products of 16 pixels per wave on the 16x16x4 fp32 MFMA; W1 and W2 in LDS in
//                           fragment order; the hidden chunk goes from the accumulators of the first product through GELU
//                           into the B operand of the second
//   backward  cx_mlp_bwd    per 16 pixels: h again, dh = (W2^T g) . gelu'(h), da = W1^T dh, m again (for d gamma), the
//                           LayerNorm backward -> du (NCHW, workspace) and the per-channel partial sums
//             cx_wgrad      per hidden chunk of 16: dW1, dW2, db1 with the pixels as the K dimension, partial per wave
//             cx_dw_bwd     dx = dy + corr(du, flipped dw_w), the 49-tap weight gradient and the bias gradient per tile
//             cx_finish     every parameter gradient = the sum of its partials in partial order, in double
//
// MFMA 16x16x4 fp32 operand layout (wave64, lane l, i = l % 16, kq = l / 16): A[i][k = kq], B[k = kq][n = i],
// D[m = 4 kq + r][n = i] in accumulator register r.  The hidden chunk hT[j][p] (j = hidden row, p = pixel) therefore sits
// as hT[4 kq + r][i]: register r of all lanes IS a B operand (k = kq, n = i) of the product over j, for the k <-> j map
// j = 4 kq + r -- the A operand of that step is W2[c][j0 + 4 kq + r], one float4 of a row of W2 per lane for r = 0..3.
#include "nq_common.h"

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int CX_TH = 8, CX_TW = 32;                  // pixels of a depthwise tile (256 lanes)
constexpr int CX_PH = CX_TH + 6, CX_PW = CX_TW + 6;   // ... with the 3-pixel halo
constexpr int CX_MAXG = 256;                          // workgroups of cx_mlp_fwd / cx_mlp_bwd at most
constexpr int CX_WSPLIT = 16;                         // pixel splits of cx_wgrad at most: 64 wave partials

__device__ __forceinline__ v4f cx_mfma(float a, float b, v4f c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

struct CxDims {
  int64_t P, HW;      // pixels N*H*W, pixels of a plane
  int ntiles;         // 16-pixel tiles
};

// stage one channel's tile + halo (zero outside the image) of plane `xp`
__device__ __forceinline__ void cx_stage(float* tile, const float* __restrict__ xp, int h0, int w0, int H, int W) {
  for (int e = threadIdx.x; e < CX_PH * CX_PW; e += 256) {
    const int r = e / CX_PW, q = e - r * CX_PW;
    const int hh = h0 + r - 3, ww = w0 + q - 3;
    tile[e] = (hh >= 0 && hh < H && ww >= 0 && ww < W) ? xp[(int64_t)hh * W + ww] : 0.f;
  }
}

// ---- forward A: depthwise 7x7 + LayerNorm statistics ----
template <int C>
__global__ __launch_bounds__(256) void cx_dwln_fwd(const float* __restrict__ x, const float* __restrict__ dw_w,
                                                   const float* __restrict__ dw_b, float* __restrict__ xhat,
                                                   float* __restrict__ rstd, int H, int W) {
  __shared__ float tile[CX_PH * CX_PW];
  const int n = blockIdx.z, h0 = blockIdx.y * CX_TH, w0 = blockIdx.x * CX_TW;
  const int tx = threadIdx.x % CX_TW, ty = threadIdx.x / CX_TW;
  const int64_t HW = (int64_t)H * W;
  float u[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    __syncthreads();
    cx_stage(tile, x + ((int64_t)n * C + c) * HW, h0, w0, H, W);
    __syncthreads();
    const float* __restrict__ wp = dw_w + c * 49;
    float acc = dw_b[c];
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
      for (int j = 0; j < 7; ++j) acc = __builtin_fmaf(tile[(ty + i) * CX_PW + tx + j], wp[i * 7 + j], acc);
    u[c] = acc;
  }
  float mean = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) mean += u[c];
  mean *= 1.0f / C;
  float var = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    u[c] -= mean;
    var = __builtin_fmaf(u[c], u[c], var);
  }
  const float rs = 1.0f / sqrtf(var * (1.0f / C) + 1e-6f);
  const int h = h0 + ty, w = w0 + tx;
  if (h < H && w < W) {
    const int64_t q = (int64_t)n * HW + (int64_t)h * W + w;
    float4* __restrict__ o = reinterpret_cast<float4*>(xhat + q * C);
#pragma unroll
    for (int c = 0; c < C; c += 4) o[c / 4] = make_float4(u[c] * rs, u[c + 1] * rs, u[c + 2] * rs, u[c + 3] * rs);
    rstd[q] = rs;
  }
}

// the B operand of the products over c for pixel q: a[p][c] = xhat ln_w + ln_b at c = kq (C/4) + s (any k <-> c map serves,
// the A operand uses the same one; this one makes both operands contiguous runs of a row)
template <int C>
__device__ __forceinline__ void cx_load_a(float (&aB)[C / 4], const float* __restrict__ xhat, const float* __restrict__ ln_w,
                                          const float* __restrict__ ln_b, int64_t q, bool valid, int kq) {
  constexpr int KQ = C / 4;
#pragma unroll
  for (int s = 0; s < KQ; ++s) {
    const int c = kq * KQ + s;
    aB[s] = valid ? __builtin_fmaf(xhat[q * C + c], ln_w[c], ln_b[c]) : 0.f;
  }
}

// ---- forward B: out = x + gamma (W2 gelu(W1 a + b1) + b2) ----
template <int C>
__global__ __launch_bounds__(256) void cx_mlp_fwd(const float* __restrict__ x, const float* __restrict__ xhat,
                                                  const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                  const float* __restrict__ w1, const float* __restrict__ b1,
                                                  const float* __restrict__ w2, const float* __restrict__ b2,
                                                  const float* __restrict__ gamma, float* __restrict__ out, CxDims d) {
  constexpr int KQ = C / 4, NJ = C / 4, CT = (C + 15) / 16, HID = 4 * C;
  extern __shared__ float lds[];
  float* F1 = lds;                 // [jc][s][lane]      = W1[jc 16 + i][kq KQ + s]
  float* F2 = lds + NJ * KQ * 64;  // [jc][ct][lane][r]  = W2[ct 16 + i][jc 16 + 4 kq + r], 0 for rows >= C
  for (int e = threadIdx.x; e < NJ * KQ * 64; e += 256) {
    const int l = e & 63, s = (e >> 6) % KQ, jc = (e >> 6) / KQ;
    F1[e] = w1[(jc * 16 + (l & 15)) * C + (l >> 4) * KQ + s];
  }
  for (int e = threadIdx.x; e < NJ * CT * 256; e += 256) {
    const int r = e & 3, l = (e >> 2) & 63, ct = (e >> 8) % CT, jc = (e >> 8) / CT;
    const int c = ct * 16 + (l & 15), j = jc * 16 + 4 * (l >> 4) + r;
    F2[e] = c < C ? w2[c * HID + j] : 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, kq = lane >> 4;
  for (int t = blockIdx.x * 4 + wave; t < d.ntiles; t += gridDim.x * 4) {
    const int64_t q = (int64_t)t * 16 + i;
    const bool valid = q < d.P;
    float aB[KQ];
    cx_load_a<C>(aB, xhat, ln_w, ln_b, q, valid, kq);
    v4f m[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) m[ct] = v4f{0.f, 0.f, 0.f, 0.f};
    for (int jc = 0; jc < NJ; ++jc) {
      v4f h = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KQ; ++s) h = cx_mfma(F1[(jc * KQ + s) * 64 + lane], aB[s], h);
      const float4 bv = *reinterpret_cast<const float4*>(b1 + jc * 16 + 4 * kq);
      float ge[4], dge;
      nq_gelu_pair(h[0] + bv.x, ge[0], dge);
      nq_gelu_pair(h[1] + bv.y, ge[1], dge);
      nq_gelu_pair(h[2] + bv.z, ge[2], dge);
      nq_gelu_pair(h[3] + bv.w, ge[3], dge);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const float4 f = reinterpret_cast<const float4*>(F2)[(jc * CT + ct) * 64 + lane];
        m[ct] = cx_mfma(f.x, ge[0], m[ct]);
        m[ct] = cx_mfma(f.y, ge[1], m[ct]);
        m[ct] = cx_mfma(f.z, ge[2], m[ct]);
        m[ct] = cx_mfma(f.w, ge[3], m[ct]);
      }
    }
    if (valid) {
      const int64_t n = q / d.HW, hw = q - n * d.HW;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = ct * 16 + 4 * kq + r;
          if (c < C) {
            const int64_t idx = (n * C + c) * d.HW + hw;
            out[idx] = x[idx] + gamma[c] * (m[ct][r] + b2[c]);
          }
        }
    }
  }
}

// sum over the 16 lanes that share kq (the pixels of a tile); every lane of the group gets it, in a fixed order
__device__ __forceinline__ float cx_sum16(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 8, 64);
  return v;
}

// the hidden chunk jc of 16 pixels from registers: ge = gelu(h), dh = (W2^T g) . gelu'(h), both as hT[4 kq + r][i]
template <int C>
__device__ __forceinline__ void cx_hidden(const float (&w1f)[C / 4], const float (&w2tf)[C / 4], const float (&aB)[C / 4],
                                          const float (&gB)[C / 4], const float* __restrict__ b1, int jc, int kq, float (&ge)[4],
                                          float (&dh)[4]) {
  v4f h = {0.f, 0.f, 0.f, 0.f}, dg = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < C / 4; ++s) {
    h = cx_mfma(w1f[s], aB[s], h);
    dg = cx_mfma(w2tf[s], gB[s], dg);
  }
  const float4 bv = *reinterpret_cast<const float4*>(b1 + jc * 16 + 4 * kq);
  const float b[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float dge;
    nq_gelu_pair(h[r] + b[r], ge[r], dge);
    dh[r] = dg[r] * dge;
  }
}

// A operands of the two products over c for hidden rows jc 16 + i: W1[j][kq KQ + s] and W2[kq KQ + s][j]
template <int C>
__device__ __forceinline__ void cx_load_wfrag(float (&w1f)[C / 4], float (&w2tf)[C / 4], const float* __restrict__ w1,
                                              const float* __restrict__ w2, int jc, int i, int kq) {
  constexpr int KQ = C / 4;
#pragma unroll
  for (int s = 0; s < KQ; ++s) {
    w1f[s] = w1[(jc * 16 + i) * C + kq * KQ + s];
    w2tf[s] = w2[(kq * KQ + s) * (4 * C) + jc * 16 + i];
  }
}

// g[p][c] = gamma[c] dy[p][c] at c = kq (C/4) + s
template <int C>
__device__ __forceinline__ void cx_load_g(float (&gB)[C / 4], const float* __restrict__ dy, const float* __restrict__ gamma,
                                          int64_t q, bool valid, int kq, const CxDims& d) {
  constexpr int KQ = C / 4;
  const int64_t n = valid ? q / d.HW : 0, hw = valid ? q - n * d.HW : 0;
#pragma unroll
  for (int s = 0; s < KQ; ++s) {
    const int c = kq * KQ + s;
    gB[s] = valid ? gamma[c] * dy[(n * C + c) * d.HW + hw] : 0.f;
  }
}

// ---- backward, data side: du (NCHW) and the partial sums of d gamma, d b2, d ln_w, d ln_b per workgroup ----
template <int C>
__global__ __launch_bounds__(256) void cx_mlp_bwd(const float* __restrict__ dy, const float* __restrict__ xhat,
                                                  const float* __restrict__ rstd, const float* __restrict__ ln_w,
                                                  const float* __restrict__ ln_b, const float* __restrict__ w1,
                                                  const float* __restrict__ b1, const float* __restrict__ w2,
                                                  const float* __restrict__ b2, const float* __restrict__ gamma,
                                                  float* __restrict__ du, float* __restrict__ chanpart, CxDims d) {
  constexpr int KQ = C / 4, NJ = C / 4, CT = (C + 15) / 16, HID = 4 * C;
  __shared__ float red[4][4][CT * 16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, kq = lane >> 4;
  float pc[4][CT][4];   // d gamma, d b2, d ln_w, d ln_b of channel ct 16 + 4 kq + r over this lane's pixels
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) pc[k][ct][r] = 0.f;
  for (int t = blockIdx.x * 4 + wave; t < d.ntiles; t += gridDim.x * 4) {
    const int64_t q = (int64_t)t * 16 + i;
    const bool valid = q < d.P;
    float aB[KQ], gB[KQ];
    cx_load_a<C>(aB, xhat, ln_w, ln_b, q, valid, kq);
    cx_load_g<C>(gB, dy, gamma, q, valid, kq, d);
    v4f m[CT], da[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) m[ct] = da[ct] = v4f{0.f, 0.f, 0.f, 0.f};
    for (int jc = 0; jc < NJ; ++jc) {
      float w1f[KQ], w2tf[KQ], ge[4], dh[4];
      cx_load_wfrag<C>(w1f, w2tf, w1, w2, jc, i, kq);
      cx_hidden<C>(w1f, w2tf, aB, gB, b1, jc, kq, ge, dh);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const int c = ct * 16 + i;
        const bool cv = c < C;
        const int cc = cv ? c : 0;
        const float4 f = *reinterpret_cast<const float4*>(w2 + cc * HID + jc * 16 + 4 * kq);
        const float z = cv ? 1.f : 0.f;
        m[ct] = cx_mfma(f.x * z, ge[0], m[ct]);
        m[ct] = cx_mfma(f.y * z, ge[1], m[ct]);
        m[ct] = cx_mfma(f.z * z, ge[2], m[ct]);
        m[ct] = cx_mfma(f.w * z, ge[3], m[ct]);
#pragma unroll
        for (int r = 0; r < 4; ++r) da[ct] = cx_mfma(w1[(jc * 16 + 4 * kq + r) * C + cc] * z, dh[r], da[ct]);
      }
    }
    // LayerNorm backward of pixel q: its C channels are spread over the 4 lanes i, i + 16, i + 32, i + 48
    const int64_t n = valid ? q / d.HW : 0, hw = valid ? q - n * d.HW : 0;
    float xh[CT][4], dxh[CT][4], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int c0 = ct * 16 + 4 * kq;
      const bool cv = valid && c0 < C;
      const float4 xv = cv ? *reinterpret_cast<const float4*>(xhat + q * C + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
      xh[ct][0] = xv.x, xh[ct][1] = xv.y, xh[ct][2] = xv.z, xh[ct][3] = xv.w;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = cv ? c0 + r : 0;
        const float dyv = cv ? dy[(n * C + c) * d.HW + hw] : 0.f;
        const float dav = cv ? da[ct][r] : 0.f;
        pc[0][ct][r] = __builtin_fmaf(dyv, m[ct][r] + b2[c], pc[0][ct][r]);
        pc[1][ct][r] = __builtin_fmaf(dyv, gamma[c], pc[1][ct][r]);
        pc[2][ct][r] = __builtin_fmaf(dav, xh[ct][r], pc[2][ct][r]);
        pc[3][ct][r] += dav;
        dxh[ct][r] = dav * ln_w[c];
        s1 += dxh[ct][r];
        s2 = __builtin_fmaf(dxh[ct][r], xh[ct][r], s2);
      }
    }
    s1 += __shfl_xor(s1, 16, 64);
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 16, 64);
    s2 += __shfl_xor(s2, 32, 64);
    s1 *= 1.0f / C;
    s2 *= 1.0f / C;
    if (valid) {
      const float rs = rstd[q];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = ct * 16 + 4 * kq + r;
          if (c < C) du[(n * C + c) * d.HW + hw] = rs * ((dxh[ct][r] - s1) - xh[ct][r] * s2);
        }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = cx_sum16(pc[k][ct][r]);
        if (i == 0) red[wave][k][ct * 16 + 4 * kq + r] = v;
      }
  __syncthreads();
  for (int e = threadIdx.x; e < 4 * CT * 16; e += 256) {
    const int k = e / (CT * 16), c = e - k * (CT * 16);
    if (c < C) chanpart[((int64_t)blockIdx.x * 4 + k) * C + c] = ((red[0][k][c] + red[1][k][c]) + red[2][k][c]) + red[3][k][c];
  }
}

// ---- backward, weight side: workgroup (split, jc) -> per wave one partial of dW1[jc 16 .. +16][:], dW2[:][jc 16 .. +16], db1 ----
template <int C>
__global__ __launch_bounds__(256) void cx_wgrad(const float* __restrict__ dy, const float* __restrict__ xhat,
                                                const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                const float* __restrict__ w1, const float* __restrict__ b1,
                                                const float* __restrict__ w2, const float* __restrict__ gamma,
                                                float* __restrict__ wpart, CxDims d) {
  constexpr int KQ = C / 4, CT = (C + 15) / 16, HID = 4 * C, LDC = C + 1, LDP = 17;
  constexpr int WAVE_FLOATS = 2 * 16 * LDP + 2 * 16 * LDC;
  __shared__ float sm[4][WAVE_FLOATS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, kq = lane >> 4, jc = blockIdx.y;
  float* Sdh = sm[wave];          // dh[j][p]
  float* Sge = Sdh + 16 * LDP;    // gelu(h)[j][p]
  float* Sa = Sge + 16 * LDP;     // a[p][c]
  float* Sg = Sa + 16 * LDC;      // g[p][c]
  float w1f[KQ], w2tf[KQ];
  cx_load_wfrag<C>(w1f, w2tf, w1, w2, jc, i, kq);
  v4f acc1[CT], acc2[CT];         // [j = 4 kq + r][c = ct 16 + i] of dW1 and of dW2^T
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc1[ct] = acc2[ct] = v4f{0.f, 0.f, 0.f, 0.f};
  float db[4] = {0.f, 0.f, 0.f, 0.f};
  // every wave of the workgroup runs the same number of rounds (a tile past the end is all zeros): the barriers are uniform
  for (int base = blockIdx.x * 4; base < d.ntiles; base += gridDim.x * 4) {
    const int64_t q = (int64_t)(base + wave) * 16 + i;
    const bool valid = q < d.P;
    float aB[KQ], gB[KQ], ge[4], dh[4];
    cx_load_a<C>(aB, xhat, ln_w, ln_b, q, valid, kq);
    cx_load_g<C>(gB, dy, gamma, q, valid, kq, d);
    cx_hidden<C>(w1f, w2tf, aB, gB, b1, jc, kq, ge, dh);
#pragma unroll
    for (int s = 0; s < KQ; ++s) {
      Sa[i * LDC + kq * KQ + s] = aB[s];
      Sg[i * LDC + kq * KQ + s] = gB[s];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ge[r] = valid ? ge[r] : 0.f;   // gelu(b1) of a pixel past the end meets g = 0 anyway; keep the tile clean
      Sdh[(4 * kq + r) * LDP + i] = dh[r];
      Sge[(4 * kq + r) * LDP + i] = ge[r];
      db[r] += dh[r];
    }
    __syncthreads();
#pragma unroll
    for (int t4 = 0; t4 < 4; ++t4) {
      const int p = 4 * t4 + kq;
      const float a1 = Sdh[i * LDP + p], a2 = Sge[i * LDP + p];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const int c = ct * 16 + i;
        const bool cv = c < C;
        const int cc = cv ? c : 0;
        const float ba = Sa[p * LDC + cc], bg = Sg[p * LDC + cc];
        acc1[ct] = cx_mfma(a1, cv ? ba : 0.f, acc1[ct]);
        acc2[ct] = cx_mfma(a2, cv ? bg : 0.f, acc2[ct]);
      }
    }
    __syncthreads();
  }
  float* __restrict__ o = wpart + ((int64_t)blockIdx.x * 4 + wave) * (2 * HID * C + HID);
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int c = ct * 16 + i;
    if (c < C) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = jc * 16 + 4 * kq + r;
        o[j * C + c] = acc1[ct][r];
        o[HID * C + c * HID + j] = acc2[ct][r];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float v = cx_sum16(db[r]);
    if (i == 0) o[2 * HID * C + jc * 16 + 4 * kq + r] = v;
  }
}

// ---- backward of the depthwise convolution: workgroup (tile, c, n) ----
__global__ __launch_bounds__(256) void cx_dw_bwd(const float* __restrict__ du, const float* __restrict__ x,
                                                 const float* __restrict__ dy, const float* __restrict__ dw_w,
                                                 float* __restrict__ dx, float* __restrict__ dwpart, int C, int H, int W,
                                                 int tiles_x) {
  __shared__ float sdu[CX_PH * CX_PW], sx[CX_PH * CX_PW], red[4][50];
  const int tb = blockIdx.x, c = blockIdx.y, n = blockIdx.z;
  const int h0 = (tb / tiles_x) * CX_TH, w0 = (tb % tiles_x) * CX_TW;
  const int tx = threadIdx.x % CX_TW, ty = threadIdx.x / CX_TW;
  const int64_t plane = ((int64_t)n * C + c) * ((int64_t)H * W);
  cx_stage(sdu, du + plane, h0, w0, H, W);
  cx_stage(sx, x + plane, h0, w0, H, W);
  __syncthreads();
  const float* __restrict__ wp = dw_w + c * 49;
  const int h = h0 + ty, w = w0 + tx;
  if (h < H && w < W) {
    // u[h'][w'] = sum x[h' + i - 3][w' + j - 3] w[i][j]  =>  dx[h][w] = dy + sum du[h - i + 3][w - j + 3] w[i][j]
    float acc = dy[plane + (int64_t)h * W + w];
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
      for (int j = 0; j < 7; ++j) acc = __builtin_fmaf(sdu[(ty + 6 - i) * CX_PW + tx + 6 - j], wp[i * 7 + j], acc);
    dx[plane + (int64_t)h * W + w] = acc;
  }
  // lane t < 49 of wave v: tap t over the 64 pixels of tile rows 2 v, 2 v + 1; lane 49: the bias gradient
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane < 50) {
    const int ti = lane < 49 ? lane / 7 : 3, tj = lane < 49 ? lane % 7 : 3;
    float acc = 0.f;
    for (int p = 0; p < 64; ++p) {
      const int py = 2 * wave + (p >> 5), px = p & 31;
      const float g = sdu[(py + 3) * CX_PW + px + 3];
      const float v = lane < 49 ? sx[(py + ti) * CX_PW + px + tj] : 1.f;
      acc = __builtin_fmaf(g, v, acc);
    }
    red[wave][lane] = acc;
  }
  __syncthreads();
  if (threadIdx.x < 50)
    dwpart[(((int64_t)n * gridDim.x + tb) * C + c) * 50 + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// ---- finish: element e of {dW1 | dW2 | db1 | d gamma | d b2 | d ln_w | d ln_b | (d dw_w, d dw_b)[c][50]} ----
struct CxGrads {
  float *d_w1, *d_b1, *d_w2, *d_b2, *d_gamma, *d_ln_w, *d_ln_b, *d_dw_w, *d_dw_b;
};
__global__ __launch_bounds__(256) void cx_finish(const float* __restrict__ wpart, int np, const float* __restrict__ chanpart,
                                                 int ng, const float* __restrict__ dwpart, int nt, int C, CxGrads g) {
  const int HID = 4 * C, wsz = 2 * HID * C + HID;
  int e = blockIdx.x * 256 + threadIdx.x;
  double s = 0.0;
  if (e < wsz) {
    for (int p = 0; p < np; ++p) s += (double)wpart[(int64_t)p * wsz + e];
    if (e < HID * C) g.d_w1[e] = (float)s;
    else if (e < 2 * HID * C) g.d_w2[e - HID * C] = (float)s;
    else g.d_b1[e - 2 * HID * C] = (float)s;
    return;
  }
  e -= wsz;
  if (e < 4 * C) {
    for (int p = 0; p < ng; ++p) s += (double)chanpart[(int64_t)p * 4 * C + e];
    const int k = e / C, c = e - k * C;
    (k == 0 ? g.d_gamma : k == 1 ? g.d_b2 : k == 2 ? g.d_ln_w : g.d_ln_b)[c] = (float)s;
    return;
  }
  e -= 4 * C;
  if (e < 50 * C) {
    for (int p = 0; p < nt; ++p) s += (double)dwpart[(int64_t)p * 50 * C + e];
    const int c = e / 50, t = e - c * 50;
    if (t < 49) g.d_dw_w[c * 49 + t] = (float)s;
    else g.d_dw_b[c] = (float)s;
  }
}

// ---- host: one plan per shape, shared by the workspace query and the launches ----
struct CxPlan {
  CxDims d;
  int tiles_x, tiles_y;
  int G;                  // workgroups of cx_mlp_fwd / cx_mlp_bwd
  int S;                  // pixel splits of cx_wgrad (4 S wave partials)
  int64_t T;              // depthwise tiles N * tiles_y * tiles_x
  int64_t off_chan, off_w, off_dw, ws_floats;   // float offsets into the workspace (du at 0)
};

int cx_plan(int N, int C, int H, int W, CxPlan& p) {
  if (N < 1 || H < 1 || W < 1 || C < 8 || C > 64 || (C & 7)) return NQ_ERR_INVALID;
  const int64_t HW = (int64_t)H * W;
  if (HW > (INT64_MAX / 256) / N) return NQ_ERR_INVALID;
  const int64_t P = HW * N, ntiles = (P + 15) / 16;
  p.tiles_x = (W + CX_TW - 1) / CX_TW;
  p.tiles_y = (H + CX_TH - 1) / CX_TH;
  if (N > 65535 || ntiles > INT32_MAX || p.tiles_y > 65535 || (int64_t)p.tiles_x * p.tiles_y > INT32_MAX) return NQ_ERR_UNSUPPORTED;
  p.d = CxDims{P, HW, (int)ntiles};
  const int64_t wg = (ntiles + 3) / 4;
  p.G = (int)(wg < CX_MAXG ? wg : CX_MAXG);
  p.S = (int)(wg < CX_WSPLIT ? wg : CX_WSPLIT);
  p.T = (int64_t)N * p.tiles_y * p.tiles_x;
  if (p.T > INT32_MAX) return NQ_ERR_UNSUPPORTED;
  p.off_chan = P * C;
  p.off_w = p.off_chan + (int64_t)p.G * 4 * C;
  p.off_dw = p.off_w + (int64_t)p.S * 4 * (8 * C * C + 4 * C);
  p.ws_floats = p.off_dw + p.T * 50 * C;
  return NQ_OK;
}

bool cx_aligned(const void* a) { return a && (reinterpret_cast<uintptr_t>(a) & 15) == 0; }

template <int C>
int cx_forward(const float* x, const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b, const float* w1,
               const float* b1, const float* w2, const float* b2, const float* gamma, float* out, float* xhat, float* rstd, int N,
               int H, int W, const CxPlan& p, hipStream_t st) {
  constexpr int CT = (C + 15) / 16;
  const size_t lds = sizeof(float) * ((size_t)4 * C * C + (size_t)(C / 4) * CT * 256);
  int rc = nq_lds_optin<cx_mlp_fwd<C>>(lds);
  if (rc != NQ_OK) return rc;
  cx_dwln_fwd<C><<<dim3(p.tiles_x, p.tiles_y, N), 256, 0, st>>>(x, dw_w, dw_b, xhat, rstd, H, W);
  cx_mlp_fwd<C><<<p.G, 256, lds, st>>>(x, xhat, ln_w, ln_b, w1, b1, w2, b2, gamma, out, p.d);
  return nq_launch_status();
}

template <int C>
int cx_backward(const float* dy, const float* xhat, const float* rstd, const float* ln_w, const float* ln_b, const float* w1,
                const float* b1, const float* w2, const float* b2, const float* gamma, float* ws, const CxPlan& p, hipStream_t st) {
  cx_mlp_bwd<C><<<p.G, 256, 0, st>>>(dy, xhat, rstd, ln_w, ln_b, w1, b1, w2, b2, gamma, ws, ws + p.off_chan, p.d);
  cx_wgrad<C><<<dim3(p.S, C / 4), 256, 0, st>>>(dy, xhat, ln_w, ln_b, w1, b1, w2, gamma, ws + p.off_w, p.d);
  return NQ_OK;
}

#define CX_DISPATCH(C, CALL)     \
  switch (C) {                   \
    case 8: { constexpr int CC = 8; CALL; } break;   \
    case 16: { constexpr int CC = 16; CALL; } break; \
    case 24: { constexpr int CC = 24; CALL; } break; \
    case 32: { constexpr int CC = 32; CALL; } break; \
    case 40: { constexpr int CC = 40; CALL; } break; \
    case 48: { constexpr int CC = 48; CALL; } break; \
    case 56: { constexpr int CC = 56; CALL; } break; \
    default: { constexpr int CC = 64; CALL; } break; \
  }

}  // namespace

extern "C" {

NQ_API int64_t nq_convnext_block_ws_bytes(int N, int C, int H, int W) {
  CxPlan p;
  return cx_plan(N, C, H, W, p) == NQ_OK ? p.ws_floats * 4 : 0;
}

NQ_API int nq_convnext_block_forward(const float* x, const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b,
                                     const float* w1, const float* b1, const float* w2, const float* b2, const float* gamma,
                                     float* out, float* xhat, float* rstd, int N, int C, int H, int W, nq_stream_t stream) {
  CxPlan p;
  int rc = cx_plan(N, C, H, W, p);
  if (rc != NQ_OK) return rc;
  for (const void* a : {(const void*)x, (const void*)dw_w, (const void*)dw_b, (const void*)ln_w, (const void*)ln_b, (const void*)w1,
                        (const void*)b1, (const void*)w2, (const void*)b2, (const void*)gamma, (const void*)out, (const void*)xhat})
    if (!cx_aligned(a)) return NQ_ERR_INVALID;
  if (!rstd) return NQ_ERR_INVALID;
  CX_DISPATCH(C, rc = cx_forward<CC>(x, dw_w, dw_b, ln_w, ln_b, w1, b1, w2, b2, gamma, out, xhat, rstd, N, H, W, p, nq_s(stream)))
  return rc;
}

NQ_API int nq_convnext_block_backward(const float* dy, const float* x, const float* xhat, const float* rstd, const float* dw_w,
                                      const float* ln_w, const float* ln_b, const float* w1, const float* b1, const float* w2,
                                      const float* b2, const float* gamma, float* dx, float* d_dw_w, float* d_dw_b, float* d_ln_w,
                                      float* d_ln_b, float* d_w1, float* d_b1, float* d_w2, float* d_b2, float* d_gamma, void* ws,
                                      int64_t ws_bytes, int N, int C, int H, int W, nq_stream_t stream) {
  CxPlan p;
  int rc = cx_plan(N, C, H, W, p);
  if (rc != NQ_OK) return rc;
  for (const void* a : {(const void*)dy, (const void*)x, (const void*)xhat, (const void*)dw_w, (const void*)ln_w, (const void*)ln_b,
                        (const void*)w1, (const void*)b1, (const void*)w2, (const void*)b2, (const void*)gamma, (const void*)ws})
    if (!cx_aligned(a)) return NQ_ERR_INVALID;
  for (const void* a : {(const void*)rstd, (const void*)dx, (const void*)d_dw_w, (const void*)d_dw_b, (const void*)d_ln_w,
                        (const void*)d_ln_b, (const void*)d_w1, (const void*)d_b1, (const void*)d_w2, (const void*)d_b2,
                        (const void*)d_gamma})
    if (!a) return NQ_ERR_INVALID;
  if (ws_bytes < p.ws_floats * 4) return NQ_ERR_INVALID;
  float* wsf = static_cast<float*>(ws);
  hipStream_t st = nq_s(stream);
  CX_DISPATCH(C, rc = cx_backward<CC>(dy, xhat, rstd, ln_w, ln_b, w1, b1, w2, b2, gamma, wsf, p, st))
  cx_dw_bwd<<<dim3(p.tiles_x * p.tiles_y, C, N), 256, 0, st>>>(wsf, x, dy, dw_w, dx, wsf + p.off_dw, C, H, W, p.tiles_x);
  const int nout = 8 * C * C + 4 * C + 4 * C + 50 * C;
  cx_finish<<<(nout + 255) / 256, 256, 0, st>>>(wsf + p.off_w, 4 * p.S, wsf + p.off_chan, p.G, wsf + p.off_dw, (int)p.T, C,
                                                CxGrads{d_w1, d_b1, d_w2, d_b2, d_gamma, d_ln_w, d_ln_b, d_dw_w, d_dw_b});
  return nq_launch_status();
}

}  // extern "C"

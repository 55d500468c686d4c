// Activation-side elementwise / reduction kernels around the convolutions (HBM-bound):
// PixelShuffle+GELU backward, OutImg(tanh) backward, L2 reconstruction loss (+gradient),
// per-frame squared error for PSNR, uint8 frame gather.
#include "nq_common.h"

namespace {

constexpr int TPB = 256;

// One workgroup per (b, c, y): reads the r rows Y = y*r+i of da / z (each W*r contiguous floats) and scatters
// to the r*r planes of dconv.  R = 0 -> runtime r.
template <int R>
__global__ __launch_bounds__(TPB) void ps_gelu_bwd_kernel(const float* __restrict__ da, const float* __restrict__ z,
                                                          float* __restrict__ dconv, int C, int H, int W, int r_rt) {
  const int r = R ? R : r_rt;
  const int64_t bcy = blockIdx.x;  // ((b*C + c)*H + y)
  const int y = (int)(bcy % H);
  const int64_t bc = bcy / H;
  const int Wr = W * r;
  const int64_t in_base = (bc * (int64_t)(H * r) + (int64_t)y * r) * Wr;  // row Y = y*r of plane (b,c)
  const int64_t out_plane = (int64_t)H * W;
  const int64_t out_base = (bc * (r * r)) * out_plane + (int64_t)y * W;
  const int total = r * Wr;
  for (int e = threadIdx.x; e < total; e += TPB) {
    int i = e / Wr, X = e - i * Wr;
    int x = X / r, j = X - x * r;
    float g = da[in_base + e] * z[in_base + e];  // z = gelu'(pre-activation), saved by the forward epilogue
    dconv[out_base + (int64_t)(i * r + j) * out_plane + x] = g;
  }
}

__global__ __launch_bounds__(TPB) void tanh_out_bwd_kernel(const float* __restrict__ dimg, const float* __restrict__ img,
                                                           float* __restrict__ dconv, int64_t n) {
  int64_t i = ((int64_t)blockIdx.x * TPB + threadIdx.x) * 4;
  if (i + 3 < n) {
    float4 g = *reinterpret_cast<const float4*>(dimg + i);
    float4 o = *reinterpret_cast<const float4*>(img + i);
    float4 r;
    float t;
    t = 2.f * o.x - 1.f; r.x = g.x * 0.5f * (1.f - t * t);
    t = 2.f * o.y - 1.f; r.y = g.y * 0.5f * (1.f - t * t);
    t = 2.f * o.z - 1.f; r.z = g.z * 0.5f * (1.f - t * t);
    t = 2.f * o.w - 1.f; r.w = g.w * 0.5f * (1.f - t * t);
    *reinterpret_cast<float4*>(dconv + i) = r;
  } else {
    for (; i < n; ++i) {
      float t = 2.f * img[i] - 1.f;
      dconv[i] = dimg[i] * 0.5f * (1.f - t * t);
    }
  }
}

__global__ __launch_bounds__(TPB) void l2_loss_stage1(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                      float* __restrict__ dpred, float* __restrict__ ws, int64_t n,
                                                      float gcoef) {
  __shared__ float red[16];
  int64_t i0 = (int64_t)blockIdx.x * NQ_RED_CHUNK;
  float acc = 0.f;
#pragma unroll 4
  for (int k = 0; k < NQ_RED_CHUNK / TPB; ++k) {
    int64_t i = i0 + k * TPB + threadIdx.x;
    if (i < n) {
      float d = pred[i] - tgt[i];
      acc += d * d;
      if (dpred) dpred[i] = gcoef * d;
    }
  }
  float s = nq_block_sum(acc, red);
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}

// lp_loss (p = 2) of a tanh-headed decoder in ONE pass: the loss partials (same chunks, same per-thread order as
// l2_loss_stage1: the loss is bit-identical), the conv-output gradient of the head dconv = [gcoef*(pred-tgt)] * 0.5 *
// (1 - t^2), t = 2*pred - 1 (the two roundings of l2_loss_stage1 followed by tanh_out_bwd_kernel), and per-chunk sums of
// dconv (the head's bias gradient).  The target comes as float frames or straight from the uint8 frame cache
// (frames[idx[b]] / 255, the arithmetic of gather_u8_kernel).  A chunk never straddles a channel plane (HW % chunk == 0).
template <bool U8>
__global__ __launch_bounds__(TPB) void l2_tanh_head_stage1(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                           const uint8_t* __restrict__ cache, const int64_t* __restrict__ idx,
                                                           float* __restrict__ dconv, float* __restrict__ ws, int64_t parts,
                                                           int cpf /* chunks per frame = C*HW/chunk */, float gcoef) {
  __shared__ float red[16];
  const int64_t i0 = (int64_t)blockIdx.x * NQ_RED_CHUNK;
  const uint8_t* __restrict__ src = nullptr;
  if constexpr (U8) {
    const int64_t f = blockIdx.x / cpf;
    src = cache + idx[f] * ((int64_t)cpf * NQ_RED_CHUNK) + (int64_t)(blockIdx.x - f * cpf) * NQ_RED_CHUNK;
  }
  float acc = 0.f, accg = 0.f;
#pragma unroll 4
  for (int k = 0; k < NQ_RED_CHUNK / TPB; ++k) {
    const int e = k * TPB + threadIdx.x;
    const int64_t i = i0 + e;
    const float p = pred[i];
    const float t = U8 ? (float)src[e] / 255.f : tgt[i];
    const float d = p - t;
    acc += d * d;
    const float g = gcoef * d;
    const float u = 2.f * p - 1.f;
    const float r = g * 0.5f * (1.f - u * u);
    dconv[i] = r;
    accg += r;
  }
  const float s = nq_block_sum(acc, red);
  const float sg = nq_block_sum(accg, red);
  if (threadIdx.x == 0) {
    ws[blockIdx.x] = s;
    ws[parts + blockIdx.x] = sg;
  }
}
// block 0: the loss (as nq_sum_stage2); block 1 + c: db[c] = sum over frames and chunks of channel c, fixed order
__global__ __launch_bounds__(256) void l2_tanh_head_stage2(const float* __restrict__ ws, int64_t parts, float scale,
                                                           float* __restrict__ loss, float* __restrict__ db, int B, int C,
                                                           int cpp /* chunks per plane */) {
  __shared__ float red[16];
  float acc = 0.f;
  if (blockIdx.x == 0) {
    for (int64_t i = threadIdx.x; i < parts; i += 256) acc += ws[i];
    const float s = nq_block_sum(acc, red);
    if (threadIdx.x == 0) loss[0] = 0.f + s * scale;
  } else {
    const int c = blockIdx.x - 1;
    for (int b = 0; b < B; ++b) {
      const float* p = ws + parts + ((int64_t)b * C + c) * cpp;
      for (int j = threadIdx.x; j < cpp; j += 256) acc += p[j];
    }
    const float s = nq_block_sum(acc, red);
    if (threadIdx.x == 0) db[c] = s;
  }
}

__global__ __launch_bounds__(1024) void frame_sse_kernel(const float* __restrict__ out, const float* __restrict__ gt,
                                                         float* __restrict__ sse, int64_t frame_len) {
  __shared__ float red[16];
  const float* a = out + (int64_t)blockIdx.x * frame_len;
  const float* b = gt + (int64_t)blockIdx.x * frame_len;
  float acc = 0.f;
  for (int64_t i = threadIdx.x; i < frame_len; i += 1024) {
    float d = a[i] - b[i];
    acc += d * d;
  }
  float s = nq_block_sum(acc, red);
  if (threadIdx.x == 0) sse[blockIdx.x] = s;
}

// per-channel sums of an NCHW tensor (bias gradient of a conv): stage 1 = (chunk, channel) partials, stage 2 = fixed order
constexpr int CS_CHUNKS = 512;   // (chunk, channel) workgroups: 1536 for a 3-channel image, enough to fill the chip
__global__ __launch_bounds__(TPB) void channel_sum_stage1(const float* __restrict__ x, float* __restrict__ ws, int B, int C,
                                                          int64_t HW) {
  __shared__ float red[16];
  const int c = blockIdx.y, chunk = blockIdx.x;
  const int64_t per = (HW + CS_CHUNKS - 1) / CS_CHUNKS, lo = chunk * per, hi = min(HW, lo + per);
  float acc = 0.f;
  for (int b = 0; b < B; ++b) {
    const float* p = x + ((int64_t)b * C + c) * HW;
    for (int64_t i = lo + threadIdx.x; i < hi; i += TPB) acc += p[i];
  }
  float s = nq_block_sum(acc, red);
  if (threadIdx.x == 0) ws[c * CS_CHUNKS + chunk] = s;
}
__global__ void channel_sum_stage2(const float* __restrict__ ws, float* __restrict__ out, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
#pragma unroll 8
  for (int k = 0; k < CS_CHUNKS; ++k) s += ws[c * CS_CHUNKS + k];
  out[c] = s;
}

__global__ __launch_bounds__(TPB) void gather_u8_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ idx,
                                                        float* __restrict__ dst, int64_t frame_len) {
  const int64_t f = blockIdx.y;
  const uint8_t* s = src + idx[f] * frame_len;
  float* d = dst + f * frame_len;
  int64_t i = ((int64_t)blockIdx.x * TPB + threadIdx.x) * 4;
  // both vector accesses need their alignment: with a frame length that is no multiple of 4 neither s + i nor d + i has it
  if (i + 3 < frame_len && ((reinterpret_cast<uintptr_t>(s + i) & 3) == 0) && ((reinterpret_cast<uintptr_t>(d + i) & 15) == 0)) {
    uchar4 v = *reinterpret_cast<const uchar4*>(s + i);
    float4 o = make_float4((float)v.x / 255.f, (float)v.y / 255.f, (float)v.z / 255.f, (float)v.w / 255.f);
    *reinterpret_cast<float4*>(d + i) = o;
  } else {
    for (int k = 0; k < 4 && i + k < frame_len; ++k) d[i + k] = (float)s[i + k] / 255.f;  // img / 255. (datasets.py:23)
  }
}

// ---- twice-differentiable elementwise pieces of the decoder (Omega bit-allocation criterion: Hessian-vector products by
//      double backward, reference methods/bit_assign.py:57-118 through models/_layers.py:10-36, 104-105) ----
// y = f(x) * g * g2 (g, g2 optional), f = the value / first / second derivative of the exact-erf GELU (nn.GELU()) or of
// OutImg's tanh(x) * 0.5 + 0.5.  erff / expf / tanhf: this is the bit-allocation sweep, not the calibration iteration.
__device__ __forceinline__ float act_dd_eval(float x, int mode) {
  const float kInvSqrt2 = 0.70710678118654752440f, kInvSqrt2Pi = 0.39894228040143267794f;
  if (mode <= 2) {
    const float cdf = 0.5f * (1.0f + erff(x * kInvSqrt2));
    if (mode == 0) return x * cdf;
    const float pdf = kInvSqrt2Pi * expf(-0.5f * x * x);
    if (mode == 1) return cdf + x * pdf;
    return pdf * (2.0f - x * x);          // gelu'' = 2 phi + x phi' = phi (2 - x^2)
  }
  const float t = tanhf(x);
  if (mode == 3) return t * 0.5f + 0.5f;
  const float s = 1.0f - t * t;
  if (mode == 4) return 0.5f * s;
  return -t * s;                          // (0.5 (1 - t^2))' = -t (1 - t^2)
}
__global__ __launch_bounds__(TPB) void act_dd_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                     const float* __restrict__ g2, float* __restrict__ y, int64_t n, int mode) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  float v = act_dd_eval(x[i], mode);
  if (g) v *= g[i];
  if (g2) v *= g2[i];
  y[i] = v;
}
// PixelShuffle(r): (B, C*r*r, H, W) -> (B, C, H*r, W*r), out[b][c][y*r+i][x*r+j] = in[b][c*r*r + i*r + j][y][x]; inverse = the
// un-shuffle.  One thread per element of the SHUFFLED tensor (its side is contiguous across lanes).
__global__ __launch_bounds__(TPB) void pixel_shuffle_kernel(const float* __restrict__ in, float* __restrict__ out, int C, int H,
                                                            int W, int r, int inverse, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (e >= n) return;
  const int Wr = W * r, Hr = H * r;
  const int X = (int)(e % Wr);
  const int64_t t = e / Wr;
  const int Y = (int)(t % Hr);
  const int64_t bc = t / Hr;                       // b*C + c
  const int yy = Y / r, i = Y - yy * r, xx = X / r, j = X - xx * r;
  const int64_t u = ((bc * (r * r) + i * r + j) * H + yy) * (int64_t)W + xx;   // index in the un-shuffled tensor
  if (inverse) out[u] = in[e];
  else out[e] = in[u];
}
// y[b][c][p] = (x ? x[b][c][p] : 0) + bias[c]
__global__ __launch_bounds__(TPB) void bias_add_kernel(const float* __restrict__ x, const float* __restrict__ bias,
                                                       float* __restrict__ y, int C, int64_t HW, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (e >= n) return;
  const int c = (int)((e / HW) % C);
  y[e] = (x ? x[e] : 0.f) + bias[c];
}

// float -> split {hi | lo} word (nq_common.h), elementwise: for callers that hand a bf16x3 kernel a pre-split operand
__global__ __launch_bounds__(256) void split_words_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = nq_split_word_f(x[i]);
}

}  // namespace

extern "C" {

int nq_act_dd(const float* x, const float* g, const float* g2, float* y, int64_t n, int mode, nq_stream_t stream) {
  if (!x || !y || n <= 0 || mode < 0 || mode > 5) return NQ_ERR_INVALID;
  hipLaunchKernelGGL(act_dd_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, nq_s(stream), x, g, g2, y, n, mode);
  return nq_launch_status();
}

int nq_pixel_shuffle(const float* x, float* y, int B, int C, int H, int W, int r, int inverse, nq_stream_t stream) {
  if (!x || !y || x == y || B <= 0 || C <= 0 || H <= 0 || W <= 0 || r <= 0) return NQ_ERR_INVALID;
  const int64_t n = (int64_t)B * C * r * r * H * W;
  hipLaunchKernelGGL(pixel_shuffle_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, nq_s(stream), x, y, C, H, W, r,
                     inverse ? 1 : 0, n);
  return nq_launch_status();
}

int nq_split_words(const float* x, float* y, int64_t n, nq_stream_t stream) {
  if (!x || !y || n < 0) return NQ_ERR_INVALID;
  if (n == 0) return NQ_OK;
  hipLaunchKernelGGL(split_words_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nq_s(stream), x, y, n);
  return nq_launch_status();
}

int nq_bias_add(const float* x, const float* bias, float* y, int B, int C, int64_t HW, nq_stream_t stream) {
  if (!bias || !y || B <= 0 || C <= 0 || HW <= 0) return NQ_ERR_INVALID;
  const int64_t n = (int64_t)B * C * HW;
  hipLaunchKernelGGL(bias_add_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, nq_s(stream), x, bias, y, C, HW, n);
  return nq_launch_status();
}


int nq_ps_gelu_backward(const float* da, const float* z, float* dconv, int B, int C, int H, int W, int r,
                        nq_stream_t stream) {
  if (!da || !z || !dconv || B <= 0 || C <= 0 || H <= 0 || W <= 0 || r <= 0) return NQ_ERR_INVALID;
  int64_t blocks = (int64_t)B * C * H;
  if (blocks > 0x7fffffffLL) return NQ_ERR_UNSUPPORTED;
  dim3 g((unsigned)blocks), b(TPB);
  switch (r) {
    case 1: hipLaunchKernelGGL(ps_gelu_bwd_kernel<1>, g, b, 0, nq_s(stream), da, z, dconv, C, H, W, r); break;
    case 2: hipLaunchKernelGGL(ps_gelu_bwd_kernel<2>, g, b, 0, nq_s(stream), da, z, dconv, C, H, W, r); break;
    case 4: hipLaunchKernelGGL(ps_gelu_bwd_kernel<4>, g, b, 0, nq_s(stream), da, z, dconv, C, H, W, r); break;
    case 5: hipLaunchKernelGGL(ps_gelu_bwd_kernel<5>, g, b, 0, nq_s(stream), da, z, dconv, C, H, W, r); break;
    default: hipLaunchKernelGGL(ps_gelu_bwd_kernel<0>, g, b, 0, nq_s(stream), da, z, dconv, C, H, W, r); break;
  }
  return nq_launch_status();
}

int nq_tanh_out_backward(const float* dimg, const float* img, float* dconv, int64_t n, nq_stream_t stream) {
  if (!dimg || !img || !dconv || n <= 0) return NQ_ERR_INVALID;
  int64_t blocks = (n + TPB * 4 - 1) / (TPB * 4);
  hipLaunchKernelGGL(tanh_out_bwd_kernel, dim3((unsigned)blocks), dim3(TPB), 0, nq_s(stream), dimg, img, dconv, n);
  return nq_launch_status();
}

int nq_l2_loss(const float* pred, const float* tgt, float* loss, float* dpred, float* ws, int64_t n, int64_t mean_count,
               float gscale, nq_stream_t stream) {
  if (!pred || !tgt || !loss || !ws || n <= 0 || mean_count <= 0) return NQ_ERR_INVALID;
  int64_t parts = (n + NQ_RED_CHUNK - 1) / NQ_RED_CHUNK;
  float gcoef = (float)(2.0 / (double)mean_count) * gscale;
  hipLaunchKernelGGL(l2_loss_stage1, dim3((unsigned)parts), dim3(TPB), 0, nq_s(stream), pred, tgt, dpred, ws, n, gcoef);
  hipLaunchKernelGGL(nq_sum_stage2, dim3(1), dim3(256), 0, nq_s(stream), ws, parts, (float)(1.0 / (double)mean_count),
                     loss, 0);
  return nq_launch_status();
}

int nq_l2_loss_tanh_head(const float* pred, const float* tgt, const uint8_t* cache_u8, const int64_t* idx, float* loss,
                         float* dconv, float* db, float* ws, int B, int C, int64_t HW, int64_t mean_count, float gscale,
                         nq_stream_t stream) {
  if (!pred || !loss || !dconv || !db || !ws || B <= 0 || C <= 0 || HW <= 0 || mean_count <= 0) return NQ_ERR_INVALID;
  if ((tgt == nullptr) == (cache_u8 == nullptr) || (cache_u8 && !idx)) return NQ_ERR_INVALID;
  if (HW % NQ_RED_CHUNK != 0 || C > 1024) return NQ_ERR_UNSUPPORTED;   // a chunk must stay inside one channel plane
  const int64_t n = (int64_t)B * C * HW, parts = n / NQ_RED_CHUNK;
  const int cpp = (int)(HW / NQ_RED_CHUNK), cpf = C * cpp;
  if (parts > 0x7fffffffLL) return NQ_ERR_UNSUPPORTED;
  const float gcoef = (float)(2.0 / (double)mean_count) * gscale;
  if (cache_u8)
    hipLaunchKernelGGL(l2_tanh_head_stage1<true>, dim3((unsigned)parts), dim3(TPB), 0, nq_s(stream), pred, tgt, cache_u8, idx,
                       dconv, ws, parts, cpf, gcoef);
  else
    hipLaunchKernelGGL(l2_tanh_head_stage1<false>, dim3((unsigned)parts), dim3(TPB), 0, nq_s(stream), pred, tgt, cache_u8, idx,
                       dconv, ws, parts, cpf, gcoef);
  hipLaunchKernelGGL(l2_tanh_head_stage2, dim3((unsigned)(1 + C)), dim3(256), 0, nq_s(stream), ws, parts,
                     (float)(1.0 / (double)mean_count), loss, db, B, C, cpp);
  return nq_launch_status();
}

int nq_frame_sse(const float* out, const float* gt, float* sse, int64_t frames, int64_t frame_len, nq_stream_t stream) {
  if (!out || !gt || !sse || frames <= 0 || frame_len <= 0) return NQ_ERR_INVALID;
  hipLaunchKernelGGL(frame_sse_kernel, dim3((unsigned)frames), dim3(1024), 0, nq_s(stream), out, gt, sse, frame_len);
  return nq_launch_status();
}

int nq_channel_sum(const float* x, float* out, float* ws, int B, int C, int64_t HW, nq_stream_t stream) {
  if (!x || !out || !ws || B <= 0 || C <= 0 || HW <= 0 || C > 65535) return NQ_ERR_INVALID;
  hipLaunchKernelGGL(channel_sum_stage1, dim3(CS_CHUNKS, (unsigned)C), dim3(TPB), 0, nq_s(stream), x, ws, B, C, HW);
  hipLaunchKernelGGL(channel_sum_stage2, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, nq_s(stream), ws, out, C);
  return nq_launch_status();
}

int nq_gather_frames_u8(const uint8_t* src, const int64_t* idx, float* dst, int64_t n, int64_t frame_len,
                        nq_stream_t stream) {
  if (!src || !idx || !dst || n <= 0 || frame_len <= 0 || n > 65535) return NQ_ERR_INVALID;
  dim3 g((unsigned)((frame_len + TPB * 4 - 1) / (TPB * 4)), (unsigned)n);
  hipLaunchKernelGGL(gather_u8_kernel, g, dim3(TPB), 0, nq_s(stream), src, idx, dst, frame_len);
  return nq_launch_status();
}

}  // extern "C"

// Reconstruction loss in the 8-bit YUV 4:2:0 domain: the weighted plane MSEs of the UNROUNDED codes that
// nq_frames_to_yuv420 would round, their exact gradient and, behind a tanh head, the gradient at the head conv's output with
// the head's bias gradient (the contract of nq_l2_loss_tanh_head).
//
// The colour transform is linear, so it is applied to d = pred - tgt: offsets cancel, nothing is clamped.  Per pixel
//   dy = (Kr d_r + Kg d_g) + Kb d_b,  dcb = (d_b - dy) icb,  dcr = (d_r - dy) icr
// per 2 x 2 block (row 0 first, left before right: the box of yuv.hip)
//   mu = ((dcb00 + dcb01) + (dcb10 + dcb11)) * 0.25,  mv likewise
// and with c_p = gscale * 6 w_p s_p^2 / ((wY + wU + wV) B H W)  (s_Y = 219/255, s_C = 224/255; 1 in full range)
//   tb = (c_U mu) icb,  tr = (c_V mv) icr,  gy = (c_Y dy - tb) - tr
//   g_r = Kr gy + tr,   g_g = Kg gy,        g_b = Kb gy + tb
// In tanh-head mode each g is then multiplied as nq_tanh_out_backward does: g * 0.5 * (1 - (2 pred - 1)^2).  Both modes run
// the same instructions up to that product (contraction is off), so the head-mode gradient equals the image-mode gradient
// passed through nq_tanh_out_backward bit for bit.  Constants as in yuv.hip: formed in double, rounded once to float.
//
// Memory: pred and the target are read once, the gradient is written once; nothing is shared between threads, so the kernels
// are shaped by coalescing alone.  Vector kernel: a thread owns 2 rows x 4 columns (two whole chroma blocks), consecutive
// lanes take consecutive 16-byte pieces of a row (a wave reads 1 KB contiguous per row and plane).  Block kernel: one thread
// per 2 x 2 block, scalar accesses, any even size and any alignment.  LDS holds the workgroup sums only.
//
// Sums: every workgroup leaves six partial sums (dy^2, mu^2, mv^2 and, in head mode, the three channel sums of the gradient)
// in ws[p * parts + workgroup]; one more workgroup adds them in a fixed order.  No atomics: bit-identical from call to call.
#include <cmath>

#include "nq_common.h"

namespace {

constexpr int TPB = 256;

struct LossK {
  float kr, kg, kb, icb, icr;
  float cy, cu, cv;   // gscale * 6 w_p s_p^2 / ((wY + wU + wV) B H W)
};
struct FinK {
  float my, mc;       // plane MSE = sum * s_p^2 / plane samples
  float ly, lu, lv;   // L = (ly MSE_Y + lu MSE_U) + lv MSE_V, l_p = 3 w_p / (wY + wU + wV)
};

// one 2 x 2 block: p / t / g[channel][2 * row + column]; acc = {dy^2, mu^2, mv^2, sum g_r, sum g_g, sum g_b}
template <bool HEAD>
__device__ __forceinline__ void loss_block(const LossK& k, const float (&p)[3][4], const float (&t)[3][4], float (&g)[3][4],
                                           float (&acc)[6]) {
  float dr[4], db[4], dy[4], cb[4], cr[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    dr[j] = p[0][j] - t[0][j];
    const float dg = p[1][j] - t[1][j];
    db[j] = p[2][j] - t[2][j];
    dy[j] = (k.kr * dr[j] + k.kg * dg) + k.kb * db[j];
    cb[j] = (db[j] - dy[j]) * k.icb;
    cr[j] = (dr[j] - dy[j]) * k.icr;
    acc[0] += dy[j] * dy[j];
  }
  const float mu = ((cb[0] + cb[1]) + (cb[2] + cb[3])) * 0.25f;
  const float mv = ((cr[0] + cr[1]) + (cr[2] + cr[3])) * 0.25f;
  acc[1] += mu * mu;
  acc[2] += mv * mv;
  const float tb = (k.cu * mu) * k.icb;
  const float tr = (k.cv * mv) * k.icr;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float gy = (k.cy * dy[j] - tb) - tr;
    g[0][j] = k.kr * gy + tr;
    g[1][j] = k.kg * gy;
    g[2][j] = k.kb * gy + tb;
    if constexpr (HEAD) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float u = 2.f * p[c][j] - 1.f;
        g[c][j] = g[c][j] * 0.5f * (1.f - u * u);   // the expression of tanh_out_bwd_kernel
        acc[3 + c] += g[c][j];
      }
    }
  }
}

// thread t -> frame, block row (2 image rows) and column group of its piece
struct Piece {
  int64_t f;
  int by, bx;
};
__device__ __forceinline__ Piece piece_of(int64_t t, int rows2, int groups) {
  const int64_t per_frame = (int64_t)rows2 * groups;
  Piece p;
  p.f = t / per_frame;
  const int64_t rem = t - p.f * per_frame;
  p.by = (int)(rem / groups);
  p.bx = (int)(rem - (int64_t)p.by * groups);
  return p;
}

// the six workgroup sums -> ws[p * parts + workgroup]; every thread of the workgroup arrives here.  The sums of nq_block_sum
// (wave sum, then the waves in order, starting from 0), all six behind ONE barrier: six calls in a row are twelve barriers and
// six shuffle chains one after the other in a workgroup that has only four waves to hide them (measured: DESIGN.md §19.5).
template <bool HEAD>
__device__ __forceinline__ void store_partials(const float (&acc)[6], float* __restrict__ ws, int64_t parts) {
  constexpr int N = HEAD ? 6 : 3, NW = TPB / 64;
  __shared__ float red[6][NW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int p = 0; p < N; ++p) {
    const float w = nq_wave_sum(acc[p]);
    if (lane == 0) red[p][wave] = w;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    float r = 0.f;
#pragma unroll
    for (int i = 0; i < NW; ++i) r += red[threadIdx.x][i];
    ws[threadIdx.x * parts + blockIdx.x] = r;
  }
}

// W % 4 == 0, pred / tgt / grad 16-byte and the cache 4-byte aligned: 2 rows x 4 columns per thread, six 16-byte loads of pred,
// six of tgt (or six dwords of the cache), six 16-byte stores.  Every address is aligned because W * 4 and H * W * 4 are
// multiples of 16 and 3 * H * W is a multiple of 4.
template <bool U8, bool HEAD>
__global__ __launch_bounds__(TPB) void yuv_loss_vec_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                           const uint8_t* __restrict__ cache, const int64_t* __restrict__ idx,
                                                           float* __restrict__ grad, float* __restrict__ ws, int64_t total,
                                                           int64_t parts, int H, int W, LossK k) {
  const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
  float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (t < total) {
    const Piece pc = piece_of(t, H >> 1, W >> 2);
    const int64_t HW = (int64_t)H * W;
    const int64_t off = (int64_t)(2 * pc.by) * W + pc.bx * 4;     // in a channel plane
    const int64_t base = pc.f * 3 * HW + off;
    const uint8_t* __restrict__ src = nullptr;
    if constexpr (U8) src = cache + idx[pc.f] * 3 * HW + off;
    float pv[3][2][4], tv[3][2][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int row = 0; row < 2; ++row) {
        const int64_t o = c * HW + (int64_t)row * W;
        const float4 a = *reinterpret_cast<const float4*>(pred + base + o);
        pv[c][row][0] = a.x; pv[c][row][1] = a.y; pv[c][row][2] = a.z; pv[c][row][3] = a.w;
        if constexpr (U8) {
          const uchar4 v = *reinterpret_cast<const uchar4*>(src + o);
          tv[c][row][0] = (float)v.x / 255.f; tv[c][row][1] = (float)v.y / 255.f;
          tv[c][row][2] = (float)v.z / 255.f; tv[c][row][3] = (float)v.w / 255.f;
        } else {
          const float4 b = *reinterpret_cast<const float4*>(tgt + base + o);
          tv[c][row][0] = b.x; tv[c][row][1] = b.y; tv[c][row][2] = b.z; tv[c][row][3] = b.w;
        }
      }
    }
    float gv[3][2][4];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      float p[3][4], tt[3][4], g[3][4];
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          p[c][j] = pv[c][j >> 1][2 * blk + (j & 1)];
          tt[c][j] = tv[c][j >> 1][2 * blk + (j & 1)];
        }
      loss_block<HEAD>(k, p, tt, g, acc);
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) gv[c][j >> 1][2 * blk + (j & 1)] = g[c][j];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int row = 0; row < 2; ++row)
        *reinterpret_cast<float4*>(grad + base + c * HW + (int64_t)row * W) =
            make_float4(gv[c][row][0], gv[c][row][1], gv[c][row][2], gv[c][row][3]);
  }
  store_partials<HEAD>(acc, ws, parts);
}

// any even H and W, any alignment: one thread per 2 x 2 block, scalar accesses
template <bool U8, bool HEAD>
__global__ __launch_bounds__(TPB) void yuv_loss_block_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                             const uint8_t* __restrict__ cache, const int64_t* __restrict__ idx,
                                                             float* __restrict__ grad, float* __restrict__ ws, int64_t total,
                                                             int64_t parts, int H, int W, LossK k) {
  const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
  float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (t < total) {
    const Piece pc = piece_of(t, H >> 1, W >> 1);
    const int64_t HW = (int64_t)H * W;
    const int64_t off = (int64_t)(2 * pc.by) * W + pc.bx * 2;
    const int64_t base = pc.f * 3 * HW + off;
    const uint8_t* __restrict__ src = nullptr;
    if constexpr (U8) src = cache + idx[pc.f] * 3 * HW + off;
    float p[3][4], tt[3][4], g[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t o = c * HW + (int64_t)(j >> 1) * W + (j & 1);
        p[c][j] = pred[base + o];
        tt[c][j] = U8 ? (float)src[o] / 255.f : tgt[base + o];
      }
    loss_block<HEAD>(k, p, tt, g, acc);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) grad[base + c * HW + (int64_t)(j >> 1) * W + (j & 1)] = g[c][j];
  }
  store_partials<HEAD>(acc, ws, parts);
}

// one workgroup: the nsum (3 or 6) sums over the workgroups' partials, each in a fixed order, then the plane MSEs, L and db
__global__ __launch_bounds__(256) void yuv_loss_stage2(const float* __restrict__ ws, int64_t parts, int nsum, FinK k,
                                                       float* __restrict__ loss, float* __restrict__ db) {
  __shared__ float red[6][4], fin[6];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  // the columns side by side (independent loads and shuffle chains), each summed in the order of nq_sum_stage2
  for (int64_t i = threadIdx.x; i < parts; i += 256) {
#pragma unroll
    for (int p = 0; p < 6; ++p)
      if (p < nsum) acc[p] += ws[p * parts + i];
  }
#pragma unroll
  for (int p = 0; p < 6; ++p) {
    const float w = nq_wave_sum(acc[p]);
    if (lane == 0) red[p][wave] = w;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    float r = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) r += red[threadIdx.x][i];
    fin[threadIdx.x] = r;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float* tot = fin;
    const float my = tot[0] * k.my, mu = tot[1] * k.mc, mv = tot[2] * k.mc;
    loss[0] = (k.ly * my + k.lu * mu) + k.lv * mv;
    loss[1] = my;
    loss[2] = mu;
    loss[3] = mv;
    if (db) {
      db[0] = tot[3];
      db[1] = tot[4];
      db[2] = tot[5];
    }
  }
}

// workgroups of the block kernel (the larger launch of the two) for a valid call; 0 for sizes the entry rejects, -1 where the
// grid cannot hold them
inline int64_t block_path_parts(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1)) return 0;
  const int64_t HW = (int64_t)H * W;          // < 2^62
  if (B > INT64_MAX / 3 / HW) return 0;       // B * 3 * H * W past int64
  const int64_t parts = ((int64_t)B * (HW / 4) + TPB - 1) / TPB;
  return parts <= 0x7fffffffLL ? parts : -1;
}

template <bool U8, bool HEAD>
void launch_stage1(bool vec, int64_t parts, hipStream_t st, const float* pred, const float* tgt, const uint8_t* cache,
                   const int64_t* idx, float* grad, float* ws, int64_t total, int H, int W, const LossK& k) {
  if (vec)
    hipLaunchKernelGGL((yuv_loss_vec_kernel<U8, HEAD>), dim3((unsigned)parts), dim3(TPB), 0, st, pred, tgt, cache, idx, grad, ws,
                       total, parts, H, W, k);
  else
    hipLaunchKernelGGL((yuv_loss_block_kernel<U8, HEAD>), dim3((unsigned)parts), dim3(TPB), 0, st, pred, tgt, cache, idx, grad,
                       ws, total, parts, H, W, k);
}

}  // namespace

extern "C" {

int64_t nq_yuv420_loss_ws_floats(int B, int H, int W) {
  const int64_t parts = block_path_parts(B, H, W);
  return parts > 0 ? 6 * parts : 0;
}

int nq_yuv420_loss(const float* pred, const float* tgt, const uint8_t* cache_u8, const int64_t* idx, float* loss, float* grad,
                   float* db, float* ws, int B, int H, int W, int matrix, int full_range, float wy, float wu, float wv,
                   float gscale, nq_stream_t stream) {
  if (!pred || !loss || !grad || !ws) return NQ_ERR_INVALID;
  if ((tgt == nullptr) == (cache_u8 == nullptr) || (cache_u8 && !idx)) return NQ_ERR_INVALID;
  if ((matrix != 0 && matrix != 1) || (full_range != 0 && full_range != 1)) return NQ_ERR_INVALID;
  if (!std::isfinite(wy) || !std::isfinite(wu) || !std::isfinite(wv) || wy < 0.f || wu < 0.f || wv < 0.f) return NQ_ERR_INVALID;
  const double wsum = (double)wy + (double)wu + (double)wv;
  if (!(wsum > 0.0)) return NQ_ERR_INVALID;
  const int64_t max_parts = block_path_parts(B, H, W);
  if (max_parts == 0) return NQ_ERR_INVALID;
  if (max_parts < 0) return NQ_ERR_UNSUPPORTED;

  const double kr = matrix == 0 ? 0.299 : 0.2126, kb = matrix == 0 ? 0.114 : 0.0722, kg = 1.0 - kr - kb;
  const double sy = full_range ? 1.0 : 219.0 / 255.0, sc = full_range ? 1.0 : 224.0 / 255.0;
  const double n = (double)B * (double)H * (double)W;
  LossK k;
  k.kr = (float)kr;
  k.kg = (float)kg;
  k.kb = (float)kb;
  k.icb = (float)(1.0 / (2.0 * (1.0 - kb)));
  k.icr = (float)(1.0 / (2.0 * (1.0 - kr)));
  k.cy = (float)((double)gscale * 6.0 * (double)wy * sy * sy / (wsum * n));
  k.cu = (float)((double)gscale * 6.0 * (double)wu * sc * sc / (wsum * n));
  k.cv = (float)((double)gscale * 6.0 * (double)wv * sc * sc / (wsum * n));
  FinK f;
  f.my = (float)(sy * sy / n);
  f.mc = (float)(sc * sc * 4.0 / n);
  f.ly = (float)(3.0 * (double)wy / wsum);
  f.lu = (float)(3.0 * (double)wu / wsum);
  f.lv = (float)(3.0 * (double)wv / wsum);

  const bool aligned = ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(tgt)) & 15) == 0 &&
                       (reinterpret_cast<uintptr_t>(cache_u8) & 3) == 0;
  const bool vec = W % 4 == 0 && aligned;
  const int64_t total = (int64_t)B * (H / 2) * (vec ? W / 4 : W / 2), parts = (total + TPB - 1) / TPB;   // <= max_parts
  hipStream_t st = nq_s(stream);
  if (cache_u8) {
    if (db) launch_stage1<true, true>(vec, parts, st, pred, tgt, cache_u8, idx, grad, ws, total, H, W, k);
    else launch_stage1<true, false>(vec, parts, st, pred, tgt, cache_u8, idx, grad, ws, total, H, W, k);
  } else {
    if (db) launch_stage1<false, true>(vec, parts, st, pred, tgt, cache_u8, idx, grad, ws, total, H, W, k);
    else launch_stage1<false, false>(vec, parts, st, pred, tgt, cache_u8, idx, grad, ws, total, H, W, k);
  }
  hipLaunchKernelGGL(yuv_loss_stage2, dim3(1), dim3(256), 0, st, ws, parts, db ? 6 : 3, f, loss, db);
  return nq_launch_status();
}

}  // extern "C"

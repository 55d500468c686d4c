// Training loss of MSE and single-scale SSIM with its exact gradient: the reference's `ssim` and `Fusion1/3/5` losses
// (reference utils.py:119-130 -> pytorch_msssim.ssim(X, Y, data_range=1, size_average=False)); the definition and the
// gradient are spelled out at nq_ssim_loss in include/nq_hip.h.
//
// Forward launch, tiled as msssim_scale_kernel (msssim.hip): a workgroup owns an 8 x 118 tile of the valid region of one
// (frame, channel) plane, stages the 18 x 128 input tile of both images in LDS, filters the five moments along H into LDS
// and along W in registers, evaluates S per valid pixel and reduces S and (X - Y)^2 to ONE partial sum each (every image
// pixel belongs to exactly one tile: the last tile of a row / column of tiles owns its halo).  With a gradient wanted it
// also writes the three maps P = dS/d mu_x, Q = dS/d Sxx, R = dS/d Sxy.  Moments are taken about a per-workgroup pivot
// with the window-sum correction that msssim.hip derives, so variances cancel at the size of the local contrast.
//
// Backward launch, a gather: a workgroup owns an 8 x 118 tile of INPUT pixels, stages the 18 x 128 tiles of P, Q, R that
// reach it (zero outside the valid region: the adjoint of the valid filter), filters them with the same two passes (the
// window is symmetric) and writes dL/dX with the MSE term folded in.  No atomics: every gradient element has one writer.
//
// Finishing launch: one workgroup adds the partial sums frame by frame in a fixed order in double.
//
// nq_ssim_loss_head (the tail of a calibration iteration) launches the same three kernels with template
// flags: U8 reads the target from the uint8 frame cache through device-side frame indices while the tiles are staged, HEAD
// applies the tanh backward to every gradient element and leaves one partial sum of the results per backward workgroup, which
// further workgroups of the finishing launch add per channel (the head's bias gradient).  The instantiations nq_ssim_loss
// launches run the arithmetic they ran, operation by operation (its results are unchanged); they take the new kernel
// arguments and read the target through SlTarget, so their machine code is not the earlier build's.
//
// X and Y go through the same instructions and P, Q, R are formed so that X == Y gives S = 1, P = 0 and R = -2 Q bit for
// bit: the SSIM is then exactly 1 and the gradient exactly 0.  Window products are explicit fused multiply-adds,
// everything else rounds operation by operation (-ffp-contract=off).
#include <cmath>

#include "nq_common.h"
#include "ssim_tile.h"

namespace {

// The target plane of a workgroup: float frames, or (U8) the plane of frame idx[plane / C] of the uint8 cache, converted as
// gather_u8_kernel does while the tile is staged (elementwise.hip: (float)byte / 255.f).
template <bool U8>
struct SlTarget {
  const float* __restrict__ f;
  const uint8_t* __restrict__ u;
  __device__ __forceinline__ SlTarget(const float* yi, const uint8_t* cache, const int64_t* idx, int64_t plane, int C, int64_t hw)
      : f(nullptr), u(nullptr) {
    if constexpr (U8) {
      const int64_t b = plane / C;
      u = cache + (idx[b] * C + (plane - b * C)) * hw;
    } else {
      f = yi + plane * hw;
    }
  }
  __device__ __forceinline__ float operator[](int64_t o) const {
    if constexpr (U8) return (float)u[o] / 255.f;
    else return f[o];
  }
};

// grid (ntx * nty, planes).  maps: P, Q, R of every plane ((h - 10) x (w - 10) each), map_stride floats apart; MAPS false: unused.
// U8: the target is read from the uint8 frame cache (cache, idx, C; yi unused), else from yi (cache, idx, C unused).
template <bool MAPS, bool U8 = false>
__global__ __launch_bounds__(SL_TPB) void ssim_loss_forward_kernel(const float* __restrict__ xi, const float* __restrict__ yi,
                                                                   const uint8_t* __restrict__ cache,
                                                                   const int64_t* __restrict__ idx, int C,
                                                                   float* __restrict__ part_s, float* __restrict__ part_m,
                                                                   float* __restrict__ maps, int64_t map_stride, int h, int w,
                                                                   int ntx, int nty) {
  __shared__ float sx[SL_IH][SL_IW], sy[SL_IH][SL_IW];
  __shared__ __attribute__((aligned(16))) float sv[5][SL_TH][SL_VS];
  __shared__ double red[SL_TPB / 64][2];
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int64_t plane = blockIdx.y;
  const int R0 = ty * SL_TH, C0 = tx * SL_TW;
  const int vh = h - SL_HALO, vw = w - SL_HALO;
  const float* __restrict__ xp = xi + plane * ((int64_t)h * w);
  const SlTarget<U8> yp(yi, cache, idx, plane, C, (int64_t)h * w);

  // ---- stage the tile + halo of both images (zeros beyond the image); the squared differences of the pixels this tile owns ----
  double sum_m = 0.0;
  {
    const int c = tid & (SL_IW - 1), gx = C0 + c;
    const bool own_c = c < SL_TW || tx == ntx - 1;
#pragma unroll
    for (int k = 0; k < SL_IH / (SL_TPB / SL_IW); ++k) {
      const int r = tid / SL_IW + k * (SL_TPB / SL_IW), gy = R0 + r;
      const bool in = gy < h && gx < w;
      const int64_t o = (int64_t)gy * w + gx;
      const float x = in ? xp[o] : 0.f, y = in ? yp[o] : 0.f;
      sx[r][c] = x;
      sy[r][c] = y;
      const double d = (double)(x - y);
      sum_m += own_c && (r < SL_TH || ty == nty - 1) ? d * d : 0.0;
    }
  }
  __syncthreads();

  // the pivots: the staged tile's centre, moved into the image where the tile hangs over its edge
  const int pr = min(SL_IH / 2, h - 1 - R0), pc = min(SL_IW / 2, w - 1 - C0);
  const float pvx = sx[pr][pc], pvy = sy[pr][pc];

  sl_filter_h<5>(sv, [&](int r, int c, float* m) {
    const float x = sx[r][c] - pvx, y = sy[r][c] - pvy;
    m[0] = x; m[1] = y; m[2] = x * x; m[3] = y * y; m[4] = x * y;
  });
  __syncthreads();

  // ---- along W + the maps: thread = (row, group of 4 columns) ----
  double sum_s = 0.0;
  if (tid < SL_TH * SL_NCG) {
    const int r = tid / SL_NCG, c0 = (tid - r * SL_NCG) * SL_RG;
    float acc[SL_RG][5];
    sl_filter_w<5>(sv, r, c0, acc);
    const float C1c = 0.01f * 0.01f, C2c = 0.03f * 0.03f;
    float* __restrict__ mp = MAPS ? maps + plane * ((int64_t)vh * vw) + (int64_t)(R0 + r) * vw + C0 : nullptr;
#pragma unroll
    for (int j = 0; j < SL_RG; ++j) {
      const int cc = c0 + j;
      // columns past the tile (or the valid region) were filtered from stale LDS: selected away, never added or stored
      const bool ok = cc < SL_TW && C0 + cc < vw && R0 + r < vh;
      const float m1 = acc[j][0], m2 = acc[j][1];
      const float s1 = (acc[j][2] - m1 * m1) + sl_shift_term(pvx, pvx, m1, m1);
      const float s2 = (acc[j][3] - m2 * m2) + sl_shift_term(pvy, pvy, m2, m2);
      const float s12 = (acc[j][4] - m1 * m2) + sl_shift_term(pvx, pvy, m1, m2);
      const float u1 = (m1 - pvx * SL_D2) + pvx, u2 = (m2 - pvy * SL_D2) + pvy;   // g*x = g*x' + p G^2
      const float A1 = 2.f * u1 * u2 + C1c, B1 = u1 * u1 + u2 * u2 + C1c;
      const float A2 = 2.f * s12 + C2c, B2 = s1 + s2 + C2c;
      const float lum = A1 / B1;
      const float S = lum * (A2 / B2);
      sum_s += ok ? (double)S : 0.0;
      if (MAPS && ok) {
        // P = 2 mu_y (A2 - A1) / (B1 B2) + 2 mu_x S (1 / B2 - 1 / B1) over one denominator: both products cancel when X == Y
        mp[cc] = 2.f * (u2 * (A2 - A1) + (u1 * S) * (B1 - B2)) / (B1 * B2);
        mp[map_stride + cc] = -S / B2;
        mp[2 * map_stride + cc] = 2.f * lum / B2;
      }
    }
  }
  sl_block_sum2(sum_s, sum_m, red);
  if (tid == 0) {
    const int64_t o = plane * ((int64_t)ntx * nty) + blockIdx.x;
    part_s[o] = (float)sum_s;
    part_m[o] = (float)sum_m;
  }
}

// grid (ntx * nty, planes), tiles of the h x w image.  grad = k_mse (X - Y) + k_ssim (gT*P + 2 X gT*Q + Y gT*R).
// U8: the target as in the forward kernel.  HEAD (X = tanh(conv) * 0.5 + 0.5): that value times 0.5 (1 - (2 X - 1)^2), the
// expression of tanh_out_bwd_kernel (elementwise.hip) on the very float the other mode stores, and the sum of the tile's
// results -- one (frame, channel) plane, added in double -- rounded once into part_g[plane * tiles + tile].
template <bool U8 = false, bool HEAD = false>
__global__ __launch_bounds__(SL_TPB) void ssim_loss_backward_kernel(const float* __restrict__ xi, const float* __restrict__ yi,
                                                                    const uint8_t* __restrict__ cache,
                                                                    const int64_t* __restrict__ idx, int C,
                                                                    const float* __restrict__ maps, int64_t map_stride,
                                                                    float* __restrict__ grad, float* __restrict__ part_g, int h,
                                                                    int w, int ntx, float k_mse, float k_ssim) {
  __shared__ float sm[3][SL_IH][SL_IW];
  __shared__ __attribute__((aligned(16))) float sv[3][SL_TH][SL_VS];
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int64_t plane = blockIdx.y;
  const int R0 = ty * SL_TH, C0 = tx * SL_TW;
  const int vh = h - SL_HALO, vw = w - SL_HALO;
  const float* __restrict__ mp = maps + plane * ((int64_t)vh * vw);

  // ---- stage the map pixels whose windows reach the tile: rows R0 - 10 .. R0 + 7, zero outside the valid region ----
  {
    const int c = tid & (SL_IW - 1), gx = C0 - SL_HALO + c;
#pragma unroll
    for (int k = 0; k < SL_IH / (SL_TPB / SL_IW); ++k) {
      const int r = tid / SL_IW + k * (SL_TPB / SL_IW), gy = R0 - SL_HALO + r;
      const bool in = gy >= 0 && gy < vh && gx >= 0 && gx < vw;
      const int64_t o = (int64_t)gy * vw + gx;
#pragma unroll
      for (int q = 0; q < 3; ++q) sm[q][r][c] = in ? mp[q * map_stride + o] : 0.f;
    }
  }
  __syncthreads();
  sl_filter_h<3>(sv, [&](int r, int c, float* m) {
    m[0] = sm[0][r][c]; m[1] = sm[1][r][c]; m[2] = sm[2][r][c];
  });
  __syncthreads();

  const SlTarget<U8> yp(yi, cache, idx, plane, C, (int64_t)h * w);
  double sum_g = 0.0;
  if (tid < SL_TH * SL_NCG) {
    const int r = tid / SL_NCG, c0 = (tid - r * SL_NCG) * SL_RG;
    float acc[SL_RG][3];
    sl_filter_w<3>(sv, r, c0, acc);
    const int gy = R0 + r;
#pragma unroll
    for (int j = 0; j < SL_RG; ++j) {
      const int cc = c0 + j, gx = C0 + cc;
      if (cc < SL_TW && gx < w && gy < h) {
        const int64_t po = (int64_t)gy * w + gx, o = plane * ((int64_t)h * w) + po;
        const float x = xi[o], y = yp[po];
        // the three terms cancel to a small part of their size where the image is flat: their products and sum in double
        const double ds = (double)acc[j][0] + ((double)(2.f * x) * (double)acc[j][1] + (double)y * (double)acc[j][2]);
        const float g = k_mse * (x - y) + k_ssim * (float)ds;
        if constexpr (HEAD) {
          const float u = 2.f * x - 1.f;
          const float d = g * 0.5f * (1.f - u * u);
          grad[o] = d;
          sum_g += (double)d;
        } else {
          grad[o] = g;
        }
      }
    }
  }
  if constexpr (HEAD) {
    __shared__ double red[SL_TPB / 64][2];   // in the HEAD instantiations only
    double unused = 0.0;
    sl_block_sum2(sum_g, unused, red);
    if (tid == 0) part_g[plane * (int64_t)gridDim.x + blockIdx.x] = (float)sum_g;
  }
}

// Workgroup 0.  per_frame = C * tiles partial sums of each kind per frame, added lane-strided, then the tree, in double.
// HEAD (nq_ssim_loss_head): loss3[0] is the float L times `scale`; with db, workgroup 1 + c adds the backward launch's partial
// sums of channel c (g_tiles per plane) frame by frame, lane-strided, then the tree, in double: db[c].
template <bool HEAD = false>
__global__ __launch_bounds__(SL_TPB) void ssim_loss_finish_kernel(const float* __restrict__ part_s, const float* __restrict__ part_m,
                                                                  int B, int64_t per_frame, double n_ssim, double n_mse,
                                                                  double w_mse, double w_ssim, float* __restrict__ frame_ssim,
                                                                  float* __restrict__ loss3, float scale,
                                                                  const float* __restrict__ part_g, int64_t g_tiles, int C,
                                                                  float* __restrict__ db) {
  __shared__ double red[SL_TPB / 64][2];
  if constexpr (HEAD) {
    if (blockIdx.x > 0) {
      const int c = blockIdx.x - 1;
      double s = 0.0, unused = 0.0;
      for (int b = 0; b < B; ++b) {
        const float* __restrict__ p = part_g + ((int64_t)b * C + c) * g_tiles;
        for (int64_t i = threadIdx.x; i < g_tiles; i += SL_TPB) s += (double)p[i];
      }
      sl_block_sum2(s, unused, red);
      if (threadIdx.x == 0) db[c] = (float)s;
      return;
    }
  }
  double tot_s = 0.0, tot_m = 0.0;
  for (int b = 0; b < B; ++b) {
    double s = 0.0, m = 0.0;
    for (int64_t i = threadIdx.x; i < per_frame; i += SL_TPB) {
      s += (double)part_s[b * per_frame + i];
      m += (double)part_m[b * per_frame + i];
    }
    sl_block_sum2(s, m, red);
    if (threadIdx.x == 0) {
      const double v = s / n_ssim;                      // divided by the count: a map of ones has mean exactly 1
      frame_ssim[b] = (float)v;
      tot_s += v;
      tot_m += m;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double mse = tot_m / n_mse, ssim = tot_s / (double)B;
    const float l = (float)(w_mse * mse + w_ssim * (1.0 - ssim));
    if constexpr (HEAD) loss3[0] = scale * l;
    else loss3[0] = l;
    loss3[1] = (float)mse;
    loss3[2] = (float)ssim;
  }
}

struct SlPlan {
  int64_t planes, fwd_tiles, bwd_tiles, map_stride;
  int ntx, nty, btx;
  int64_t off_s, off_m, off_maps, total;   // the workspace: B frame values, the two kinds of partial sums, P | Q | R
  int64_t off_g, total_head;               // nq_ssim_loss_head: + one partial sum per backward workgroup
};

inline bool sl_plan(int B, int C, int H, int W, SlPlan& p) {
  if (B <= 0 || C <= 0 || H < SL_WIN || W < SL_WIN) return false;
  p.planes = (int64_t)B * C;
  const int64_t hw = (int64_t)H * W;
  if (p.planes > (INT64_MAX / 8) / hw) return false;
  p.ntx = (W - SL_HALO + SL_TW - 1) / SL_TW;
  p.nty = (H - SL_HALO + SL_TH - 1) / SL_TH;
  p.btx = (W + SL_TW - 1) / SL_TW;
  p.fwd_tiles = (int64_t)p.ntx * p.nty;
  p.bwd_tiles = (int64_t)p.btx * ((H + SL_TH - 1) / SL_TH);
  p.map_stride = p.planes * (H - SL_HALO) * (int64_t)(W - SL_HALO);
  p.off_s = B;
  p.off_m = p.off_s + p.planes * p.fwd_tiles;
  p.off_maps = p.off_m + p.planes * p.fwd_tiles;
  p.total = p.off_maps + 3 * p.map_stride;
  p.off_g = p.total;
  p.total_head = p.off_g + p.planes * p.bwd_tiles;
  return true;
}

// the launches of nq_ssim_loss_head for one kind of target
template <bool U8>
void sl_head_launches(const SlPlan& p, hipStream_t st, const float* pred, const float* tgt, const uint8_t* cache, const int64_t* idx,
                      float* loss3, float* grad, float* db, float* ws, int B, int C, int H, int W, float w_mse, float w_ssim,
                      float scale) {
  float *part_s = ws + p.off_s, *part_m = ws + p.off_m, *maps = ws + p.off_maps, *part_g = ws + p.off_g;
  const dim3 fgrid((unsigned)p.fwd_tiles, (unsigned)p.planes), bgrid((unsigned)p.bwd_tiles, (unsigned)p.planes);
  if (grad)
    hipLaunchKernelGGL((ssim_loss_forward_kernel<true, U8>), fgrid, dim3(SL_TPB), 0, st, pred, tgt, cache, idx, C, part_s, part_m,
                       maps, p.map_stride, H, W, p.ntx, p.nty);
  else
    hipLaunchKernelGGL((ssim_loss_forward_kernel<false, U8>), fgrid, dim3(SL_TPB), 0, st, pred, tgt, cache, idx, C, part_s, part_m,
                       (float*)nullptr, (int64_t)0, H, W, p.ntx, p.nty);
  const double n_mse = (double)p.planes * (double)H * (double)W;
  const double n_map = (double)(H - SL_HALO) * (double)(W - SL_HALO);
  if (grad) {   // the constants of nq_ssim_loss with grad_scale = scale
    const float k_mse = (float)((double)scale * (double)w_mse * 2.0 / n_mse);
    const float k_ssim = (float)(-(double)scale * (double)w_ssim / ((double)p.planes * n_map));
    if (db)
      hipLaunchKernelGGL((ssim_loss_backward_kernel<U8, true>), bgrid, dim3(SL_TPB), 0, st, pred, tgt, cache, idx, C, maps,
                         p.map_stride, grad, part_g, H, W, p.btx, k_mse, k_ssim);
    else
      hipLaunchKernelGGL((ssim_loss_backward_kernel<U8, false>), bgrid, dim3(SL_TPB), 0, st, pred, tgt, cache, idx, C, maps,
                         p.map_stride, grad, (float*)nullptr, H, W, p.btx, k_mse, k_ssim);
  }
  hipLaunchKernelGGL(ssim_loss_finish_kernel<true>, dim3(db ? 1u + (unsigned)C : 1u), dim3(SL_TPB), 0, st, part_s, part_m, B,
                     (int64_t)C * p.fwd_tiles, (double)C * n_map, n_mse, (double)w_mse, (double)w_ssim, ws, loss3, scale, part_g,
                     p.bwd_tiles, C, db);
}

}  // namespace

extern "C" {

int64_t nq_ssim_loss_ws_floats(int B, int C, int H, int W) {
  SlPlan p;
  return sl_plan(B, C, H, W, p) ? p.total : 0;
}

int nq_ssim_loss(const float* pred, const float* tgt, float* loss3, float* grad, float* ws, int B, int C, int H, int W, float w_mse,
                 float w_ssim, float grad_scale, nq_stream_t stream) {
  SlPlan p;
  if (!pred || !tgt || !loss3 || !ws || !sl_plan(B, C, H, W, p)) return NQ_ERR_INVALID;
  if (!std::isfinite(w_mse) || !std::isfinite(w_ssim) || !std::isfinite(grad_scale) || w_mse < 0.f || w_ssim < 0.f)
    return NQ_ERR_INVALID;
  if (p.planes > 65535 || p.bwd_tiles > 0x7fffffffLL) return NQ_ERR_UNSUPPORTED;   // grid.y, grid.x
  const hipStream_t st = nq_s(stream);
  float *part_s = ws + p.off_s, *part_m = ws + p.off_m, *maps = ws + p.off_maps;
  const dim3 fgrid((unsigned)p.fwd_tiles, (unsigned)p.planes);
  const uint8_t* no_cache = nullptr;
  const int64_t* no_idx = nullptr;
  if (grad)
    hipLaunchKernelGGL(ssim_loss_forward_kernel<true>, fgrid, dim3(SL_TPB), 0, st, pred, tgt, no_cache, no_idx, C, part_s, part_m,
                       maps, p.map_stride, H, W, p.ntx, p.nty);
  else
    hipLaunchKernelGGL(ssim_loss_forward_kernel<false>, fgrid, dim3(SL_TPB), 0, st, pred, tgt, no_cache, no_idx, C, part_s, part_m,
                       (float*)nullptr, (int64_t)0, H, W, p.ntx, p.nty);
  const double n_mse = (double)p.planes * (double)H * (double)W;
  const double n_map = (double)(H - SL_HALO) * (double)(W - SL_HALO);
  if (grad) {
    const float k_mse = (float)((double)grad_scale * (double)w_mse * 2.0 / n_mse);
    const float k_ssim = (float)(-(double)grad_scale * (double)w_ssim / ((double)p.planes * n_map));
    hipLaunchKernelGGL(ssim_loss_backward_kernel<>, dim3((unsigned)p.bwd_tiles, (unsigned)p.planes), dim3(SL_TPB), 0, st, pred, tgt,
                       no_cache, no_idx, C, maps, p.map_stride, grad, (float*)nullptr, H, W, p.btx, k_mse, k_ssim);
  }
  hipLaunchKernelGGL(ssim_loss_finish_kernel<>, dim3(1), dim3(SL_TPB), 0, st, part_s, part_m, B, (int64_t)C * p.fwd_tiles,
                     (double)C * n_map, n_mse, (double)w_mse, (double)w_ssim, ws, loss3, 1.f, (const float*)nullptr, (int64_t)0, C,
                     (float*)nullptr);
  return nq_launch_status();
}

int64_t nq_ssim_loss_head_ws_floats(int B, int C, int H, int W) {
  SlPlan p;
  return sl_plan(B, C, H, W, p) ? p.total_head : 0;
}

int nq_ssim_loss_head(const float* pred, const float* tgt, const uint8_t* cache_u8, const int64_t* idx, float* loss3, float* grad,
                      float* db, float* ws, int B, int C, int H, int W, float w_mse, float w_ssim, float scale,
                      nq_stream_t stream) {
  SlPlan p;
  if (!pred || !loss3 || !ws || !sl_plan(B, C, H, W, p)) return NQ_ERR_INVALID;
  if ((tgt == nullptr) == (cache_u8 == nullptr) || (cache_u8 && !idx)) return NQ_ERR_INVALID;
  if (db && !grad) return NQ_ERR_INVALID;   // the bias gradient is the sum of what the backward launch writes
  if (!std::isfinite(w_mse) || !std::isfinite(w_ssim) || !std::isfinite(scale) || w_mse < 0.f || w_ssim < 0.f) return NQ_ERR_INVALID;
  if (p.planes > 65535 || p.bwd_tiles > 0x7fffffffLL) return NQ_ERR_UNSUPPORTED;   // grid.y, grid.x
  const hipStream_t st = nq_s(stream);
  if (cache_u8)
    sl_head_launches<true>(p, st, pred, tgt, cache_u8, idx, loss3, grad, db, ws, B, C, H, W, w_mse, w_ssim, scale);
  else
    sl_head_launches<false>(p, st, pred, tgt, cache_u8, idx, loss3, grad, db, ws, B, C, H, W, w_mse, w_ssim, scale);
  return nq_launch_status();
}

}  // extern "C"

// Training loss of MSE and five-scale MS-SSIM with its exact gradient; the definition, the gradient and the
// clamp rule are spelled out at nq_msssim_loss in include/nq_hip.h.
//
// Forward, one launch per scale, tiled as ssim_loss_forward_kernel (ssim_tile.h): a workgroup owns an 8 x 118 tile of the
// valid region of one (frame, channel) plane of that scale, stages the 18 x 128 tile of both images, filters the five moments
// about a per-workgroup pivot, evaluates the cs map (scales 1 .. 4) or the ssim map (scale 5) and leaves ONE partial sum of it
// (at scale 1 also of (X - Y)^2).  With a gradient wanted it writes the three derivative maps of that scale's map.  From the
// staged tiles it also writes the 2 x 2 averages (divisor 4, padding h % 2 / w % 2 in front) of the next scale whose top-left
// source pixel it owns: every pooled pixel has one writer, and both images go through the same additions.
//
// Finishing launch: one workgroup; a wavefront takes a frame, adds the partial sums of each (channel, scale) lane-strided in
// double, forms v_s, M = prod relu(v_s)^w_s, the frame's MS-SSIM and, per plane and scale, the coefficient
// grad_scale dL/dv_s / N_s that the backward launches multiply their gathers by -- exactly 0 at every scale of a plane where
// some v_s <= 0 (M = 0 there: this project defines that plane's MS-SSIM gradient as zero).
//
// Backward, one launch per scale from 5 down to 1, the gather of ssim_loss_backward_kernel: a workgroup owns an 8 x 118 tile of
// that scale's pixels, filters the three maps with the adjoint of the valid filter, multiplies by the plane's coefficient and
// adds up(G_{s+1}) = G_{s+1}[(i + h % 2) / 2][(j + w % 2) / 2] / 4, the exact adjoint of the pooling.  Scales 5 .. 2 write G_s
// into the workspace, scale 1 adds the MSE term and writes the gradient.  No atomics: every element has one writer.
//
// X and Y go through the same instructions, so X == Y gives every map value 1, P = 0 and R = -2 Q bit for bit: MS-SSIM is then
// exactly 1 and the gradient exactly 0.  Plain C++ stores only.
#include <cmath>

#include "nq_common.h"
#include "ssim_tile.h"

namespace {

constexpr int ML_SCALES = 5;
__constant__ double ml_w[ML_SCALES] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};

// sl_block_sum2 for one value: the same additions in the same order; valid in thread 0.
__device__ __forceinline__ void ml_block_sum1(double& a, double (*red)[2]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  a = sl_wave_sum_d(a);
  if (lane == 0) red[wave][0] = a;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int i = 1; i < nw; ++i) a += red[i][0];
}

// grid (ntx * nty, planes) over the valid region of the h x w images of one scale.  maps: P, Q, R of every plane, map_stride
// floats apart (MAPS false: unused).  LAST (scale 5): the ssim map, nothing pooled; else the cs map and xn, yn = the next scale's
// images.  FIRST (scale 1): also the partial sums of (X - Y)^2 into part_m (else unused: nothing is squared, added or reduced).
template <bool MAPS, bool LAST, bool FIRST>
__global__ __launch_bounds__(SL_TPB) void msl_forward_kernel(const float* __restrict__ xi, const float* __restrict__ yi,
                                                             float* __restrict__ part_v, float* __restrict__ part_m,
                                                             float* __restrict__ maps, int64_t map_stride,
                                                             float* __restrict__ xn, float* __restrict__ yn, int h, int w, int ntx,
                                                             int nty) {
  __shared__ float sx[SL_IH][SL_IW], sy[SL_IH][SL_IW];
  __shared__ __attribute__((aligned(16))) float sv[5][SL_TH][SL_VS];
  __shared__ double red[SL_TPB / 64][2];
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int64_t plane = blockIdx.y;
  const int R0 = ty * SL_TH, C0 = tx * SL_TW;
  const int vh = h - SL_HALO, vw = w - SL_HALO;
  const float* __restrict__ xp = xi + plane * ((int64_t)h * w);
  const float* __restrict__ yp = yi + plane * ((int64_t)h * w);

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
      if constexpr (FIRST) {
        const double d = (double)(x - y);
        sum_m += own_c && (r < SL_TH || ty == nty - 1) ? d * d : 0.0;
      }
    }
  }
  __syncthreads();

  // ---- the next scale: pooled pixel (i, j) averages rows 2 i - ph, 2 i - ph + 1 and columns 2 j - pw, 2 j - pw + 1 (row / column
  //      -1 is the padding: zero).  The tile that owns the top-left source pixel writes it (the first tile owns the padding, the
  //      last its halo); R0 and C0 are even, so the other three pixels are at most one row / column on, inside the staged tile. ----
  if constexpr (!LAST) {
    const int ph = h & 1, pw = w & 1, hn = (h + 1) >> 1, wn = (w + 1) >> 1;
    const int i_lo = ty == 0 ? 0 : R0 / 2 + ph, i_hi = ty == nty - 1 ? hn : R0 / 2 + SL_TH / 2 + ph;
    const int j_lo = tx == 0 ? 0 : C0 / 2 + pw, j_hi = tx == ntx - 1 ? wn : C0 / 2 + SL_TW / 2 + pw;
    const int nj = j_hi - j_lo, n = (i_hi - i_lo) * nj;
    float* __restrict__ xo = xn + plane * ((int64_t)hn * wn);
    float* __restrict__ yo = yn + plane * ((int64_t)hn * wn);
    for (int e = tid; e < n; e += SL_TPB) {
      const int di = e / nj, i = i_lo + di, j = j_lo + (e - di * nj);
      const int r = 2 * i - ph - R0, c = 2 * j - pw - C0;   // >= -1; r + 1 <= 17 and c + 1 <= 127 (the last tile ends with the image)
      const bool r_in = r >= 0, c_in = c >= 0;
      const int ra = r_in ? r : 0, ca = c_in ? c : 0;
      const float x00 = r_in && c_in ? sx[ra][ca] : 0.f, x01 = r_in ? sx[ra][c + 1] : 0.f;
      const float x10 = c_in ? sx[r + 1][ca] : 0.f, x11 = sx[r + 1][c + 1];
      const float y00 = r_in && c_in ? sy[ra][ca] : 0.f, y01 = r_in ? sy[ra][c + 1] : 0.f;
      const float y10 = c_in ? sy[r + 1][ca] : 0.f, y11 = sy[r + 1][c + 1];
      const int64_t o = (int64_t)i * wn + j;
      xo[o] = ((x00 + x01) + (x10 + x11)) * 0.25f;
      yo[o] = ((y00 + y01) + (y10 + y11)) * 0.25f;
    }
  }

  // the pivots: the staged tile's centre, moved into the image where the tile hangs over its edge
  const int pr = min(SL_IH / 2, h - 1 - R0), pc = min(SL_IW / 2, w - 1 - C0);
  const float pvx = sx[pr][pc], pvy = sy[pr][pc];

  sl_filter_h<5>(sv, [&](int r, int c, float* m) {
    const float x = sx[r][c] - pvx, y = sy[r][c] - pvy;
    m[0] = x; m[1] = y; m[2] = x * x; m[3] = y * y; m[4] = x * y;
  });
  __syncthreads();

  // ---- along W + the maps: thread = (row, group of 4 columns) ----
  double sum_v = 0.0;
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
      const float A2 = 2.f * s12 + C2c, B2 = s1 + s2 + C2c;
      const float cs = A2 / B2;
      if constexpr (LAST) {
        const float A1 = 2.f * u1 * u2 + C1c, B1 = u1 * u1 + u2 * u2 + C1c;
        const float lum = A1 / B1;
        const float S = lum * cs;
        sum_v += ok ? (double)S : 0.0;
        if (MAPS && ok) {   // the maps of ssim_loss_forward_kernel
          mp[cc] = 2.f * (u2 * (A2 - A1) + (u1 * S) * (B1 - B2)) / (B1 * B2);
          mp[map_stride + cc] = -S / B2;
          mp[2 * map_stride + cc] = 2.f * lum / B2;
        }
      } else {
        sum_v += ok ? (double)cs : 0.0;
        if (MAPS && ok) {
          // d cs / d mu_x = 2 (mu_x cs - mu_y) / B2, d cs / d Sxx = -cs / B2, d cs / d Sxy = 2 / B2: X == Y gives 0, -1 / B2, 2 / B2
          mp[cc] = 2.f * (u1 * cs - u2) / B2;
          mp[map_stride + cc] = -cs / B2;
          mp[2 * map_stride + cc] = 2.f / B2;
        }
      }
    }
  }
  if constexpr (FIRST) sl_block_sum2(sum_v, sum_m, red);
  else ml_block_sum1(sum_v, red);
  if (tid == 0) {
    const int64_t o = plane * ((int64_t)ntx * nty) + blockIdx.x;
    part_v[o] = (float)sum_v;
    if constexpr (FIRST) part_m[o] = (float)sum_m;
  }
}

// grid (tiles of the h x w image, planes).  gout = coef[plane] (gT*P + 2 X gT*Q + Y gT*R) + up(gnext) [+ k_mse (X - Y), FIRST];
// gnext: G of the next scale, ((h + 1) / 2) x ((w + 1) / 2) per plane, NULL at scale 5.
template <bool FIRST>
__global__ __launch_bounds__(SL_TPB) void msl_backward_kernel(const float* __restrict__ xi, const float* __restrict__ yi,
                                                              const float* __restrict__ maps, int64_t map_stride,
                                                              const float* __restrict__ coef, const float* __restrict__ gnext,
                                                              float* __restrict__ gout, int h, int w, int btx, float k_mse) {
  __shared__ float sm[3][SL_IH][SL_IW];
  __shared__ __attribute__((aligned(16))) float sv[3][SL_TH][SL_VS];
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / btx, tx = blockIdx.x - ty * btx;
  const int64_t plane = blockIdx.y;
  const int R0 = ty * SL_TH, C0 = tx * SL_TW;
  const int vh = h - SL_HALO, vw = w - SL_HALO;
  const float* __restrict__ mp = maps + plane * ((int64_t)vh * vw);
  const float kc = coef[plane];

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

  if (tid < SL_TH * SL_NCG) {
    const int r = tid / SL_NCG, c0 = (tid - r * SL_NCG) * SL_RG;
    float acc[SL_RG][3];
    sl_filter_w<3>(sv, r, c0, acc);
    const int gy = R0 + r;
    const int ph = h & 1, pw = w & 1, wn = (w + 1) >> 1, hn = (h + 1) >> 1;
    const float* __restrict__ gn = gnext ? gnext + plane * ((int64_t)hn * wn) + (int64_t)((gy + ph) >> 1) * wn : nullptr;
#pragma unroll
    for (int j = 0; j < SL_RG; ++j) {
      const int cc = c0 + j, gx = C0 + cc;
      if (cc < SL_TW && gx < w && gy < h) {
        const int64_t o = plane * ((int64_t)h * w) + (int64_t)gy * w + gx;
        const float x = xi[o], y = yi[o];
        // the three terms cancel to a small part of their size where the image is flat: their products and sum in double
        const double ds = (double)acc[j][0] + ((double)(2.f * x) * (double)acc[j][1] + (double)y * (double)acc[j][2]);
        float g = kc == 0.f ? 0.f : kc * (float)ds;   // a clamped plane (or w_ms = 0): exactly zero, whatever the maps hold
        if (gn) g += gn[(gx + pw) >> 1] * 0.25f;
        if constexpr (FIRST) g = k_mse * (x - y) + g;
        gout[o] = g;
      }
    }
  }
}

// Lane `lane` of a wavefront adds p[lane], p[lane + 64], ... in that order in double; eight loads are in flight at a time (the
// finishing launch is one workgroup: what it waits for is the latency of these loads, not their number).
__device__ __forceinline__ double ml_lane_sum(const float* __restrict__ p, int64_t n, int lane) {
  double t = 0.0;
  int64_t i = lane;
  for (; i + 7 * 64 < n; i += 8 * 64) {
    float a[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = p[i + 64 * k];
#pragma unroll
    for (int k = 0; k < 8; ++k) t += (double)a[k];
  }
  for (; i < n; i += 64) t += (double)p[i];
  return t;
}

struct MlFinishArgs {
  const float* part[ML_SCALES];   // the partial sums of each scale's map, planes x tiles[s]
  int64_t tiles[ML_SCALES];
  double n_map[ML_SCALES];        // (h_s - 10) (w_s - 10)
};

// One workgroup; wavefront k takes frames k, k + 4, ...  kms = grad_scale w_ms / (B C).  coef: [scale][plane].
__global__ __launch_bounds__(SL_TPB) void msl_finish_kernel(MlFinishArgs a, const float* __restrict__ part_m, int B, int C,
                                                            double n_mse, double w_mse, double w_ms, double kms,
                                                            float* __restrict__ frame_ms, float* __restrict__ coef,
                                                            float* __restrict__ loss3) {
  __shared__ double red[SL_TPB / 64][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t planes = (int64_t)B * C;
  double tot_ms = 0.0, tot_m = 0.0;
  for (int b = wave; b < B; b += SL_TPB / 64) {
    double ms = 0.0;
    for (int c = 0; c < C; ++c) {
      const int64_t plane = (int64_t)b * C + c;
      double v[ML_SCALES], M = 1.0;
      bool live = true;
#pragma unroll
      for (int s = 0; s < ML_SCALES; ++s) {
        const double t = __shfl(sl_wave_sum_d(ml_lane_sum(a.part[s] + plane * a.tiles[s], a.tiles[s], lane)), 0, 64);
        v[s] = t / a.n_map[s];                          // divided by the count: a map of ones has mean exactly 1
        if (v[s] > 0.0) M *= pow(v[s], ml_w[s]);
        else live = false;                              // relu: M = 0 and, by this project's rule, no gradient (NaN lands here too)
      }
      if (!live) M = 0.0;
      if (lane == 0) {
#pragma unroll
        for (int s = 0; s < ML_SCALES; ++s)
          coef[s * planes + plane] = live ? (float)(-(kms * ml_w[s]) * M / v[s] / a.n_map[s]) : 0.f;
      }
      ms += M;
    }
    ms /= (double)C;
    const int64_t per_frame = (int64_t)C * a.tiles[0];
    const double m = sl_wave_sum_d(ml_lane_sum(part_m + b * per_frame, per_frame, lane));
    if (lane == 0) frame_ms[b] = (float)ms;
    tot_ms += ms;
    tot_m += m;
  }
  if (lane == 0) {
    red[wave][0] = tot_ms;
    red[wave][1] = tot_m;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < SL_TPB / 64; ++i) {
      tot_ms += red[i][0];
      tot_m += red[i][1];
    }
    const double mse = tot_m / n_mse, msv = tot_ms / (double)B;
    loss3[0] = (float)(w_mse * mse + w_ms * (1.0 - msv));
    loss3[1] = (float)mse;
    loss3[2] = (float)msv;
  }
}

struct MlScale {
  int h, w, ntx, nty, btx;
  int64_t fwd_tiles, bwd_tiles, map_stride;          // map_stride = planes (h - 10) (w - 10)
  int64_t off_part, off_maps, off_x, off_y, off_g;   // off_x / off_y / off_g: scales 2 .. 5 only
};
struct MlPlan {
  int64_t planes;
  MlScale s[ML_SCALES];
  // the workspace: B frame values | 5 planes coefficients | the partial sums of (X - Y)^2 | per scale: the map's partial sums |
  // scales 2 .. 5: X_s, Y_s, G_s | per scale: P | Q | R
  int64_t off_coef, off_pm, total;
};

inline bool ml_plan(int B, int C, int H, int W, MlPlan& p) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || (H < W ? H : W) <= SL_HALO * 16) return false;
  p.planes = (int64_t)B * C;
  if (p.planes > (INT64_MAX / 64) / ((int64_t)H * W)) return false;   // the workspace is under 8 x the images: counts fit
  int h = H, w = W;
  for (int s = 0; s < ML_SCALES; ++s) {
    MlScale& q = p.s[s];
    q.h = h;
    q.w = w;
    q.ntx = (w - SL_HALO + SL_TW - 1) / SL_TW;
    q.nty = (h - SL_HALO + SL_TH - 1) / SL_TH;
    q.btx = (w + SL_TW - 1) / SL_TW;
    q.fwd_tiles = (int64_t)q.ntx * q.nty;
    q.bwd_tiles = (int64_t)q.btx * ((h + SL_TH - 1) / SL_TH);
    q.map_stride = p.planes * (h - SL_HALO) * (int64_t)(w - SL_HALO);
    h = (h + 1) / 2;
    w = (w + 1) / 2;
  }
  int64_t o = B;
  p.off_coef = o;
  o += ML_SCALES * p.planes;
  p.off_pm = o;
  o += p.planes * p.s[0].fwd_tiles;
  for (int s = 0; s < ML_SCALES; ++s) {
    p.s[s].off_part = o;
    o += p.planes * p.s[s].fwd_tiles;
  }
  for (int s = 0; s < ML_SCALES; ++s) {
    const int64_t n = s ? p.planes * p.s[s].h * (int64_t)p.s[s].w : 0;
    p.s[s].off_x = o;
    p.s[s].off_y = o + n;
    p.s[s].off_g = o + 2 * n;
    o += 3 * n;
  }
  for (int s = 0; s < ML_SCALES; ++s) {
    p.s[s].off_maps = o;
    o += 3 * p.s[s].map_stride;
  }
  p.total = o;
  return true;
}

// grid.y, grid.x of the largest launch (scale 1, backward): beyond them the entry answers NQ_ERR_UNSUPPORTED
inline bool ml_launchable(const MlPlan& p) { return p.planes <= 65535 && p.s[0].bwd_tiles <= 0x7fffffffLL; }

template <bool MAPS, bool LAST, bool FIRST>
void ml_forward(const MlScale& q, int64_t planes, hipStream_t st, const float* x, const float* y, float* ws, float* part_m,
                float* xn, float* yn) {
  hipLaunchKernelGGL((msl_forward_kernel<MAPS, LAST, FIRST>), dim3((unsigned)q.fwd_tiles, (unsigned)planes), dim3(SL_TPB), 0, st, x, y,
                     ws + q.off_part, part_m, MAPS ? ws + q.off_maps : (float*)nullptr, MAPS ? q.map_stride : (int64_t)0, xn, yn,
                     q.h, q.w, q.ntx, q.nty);
}

}  // namespace

extern "C" {

int64_t nq_msssim_loss_ws_floats(int B, int C, int H, int W) {
  MlPlan p;
  return ml_plan(B, C, H, W, p) && ml_launchable(p) ? p.total : 0;
}

int nq_msssim_loss(const float* pred, const float* tgt, float* loss3, float* grad, float* ws, int B, int C, int H, int W, float w_mse,
                   float w_ms, float grad_scale, nq_stream_t stream) {
  MlPlan p;
  if (!pred || !tgt || !loss3 || !ws || !ml_plan(B, C, H, W, p)) return NQ_ERR_INVALID;
  if (!std::isfinite(w_mse) || !std::isfinite(w_ms) || !std::isfinite(grad_scale) || w_mse < 0.f || w_ms < 0.f ||
      !(w_mse + w_ms > 0.f))
    return NQ_ERR_INVALID;
  if (!ml_launchable(p)) return NQ_ERR_UNSUPPORTED;
  const hipStream_t st = nq_s(stream);

  // ---- forward: scale s reads X_s, Y_s and writes X_{s+1}, Y_{s+1} ----
  const float *x = pred, *y = tgt;
  for (int s = 0; s < ML_SCALES; ++s) {
    const MlScale& q = p.s[s];
    if (s < ML_SCALES - 1) {
      float *xn = ws + p.s[s + 1].off_x, *yn = ws + p.s[s + 1].off_y;
      if (s == 0) {
        if (grad) ml_forward<true, false, true>(q, p.planes, st, x, y, ws, ws + p.off_pm, xn, yn);
        else ml_forward<false, false, true>(q, p.planes, st, x, y, ws, ws + p.off_pm, xn, yn);
      } else {
        if (grad) ml_forward<true, false, false>(q, p.planes, st, x, y, ws, nullptr, xn, yn);
        else ml_forward<false, false, false>(q, p.planes, st, x, y, ws, nullptr, xn, yn);
      }
      x = xn;
      y = yn;
    } else {
      if (grad) ml_forward<true, true, false>(q, p.planes, st, x, y, ws, nullptr, nullptr, nullptr);
      else ml_forward<false, true, false>(q, p.planes, st, x, y, ws, nullptr, nullptr, nullptr);
    }
  }

  // ---- finish: values, coefficients, clamp ----
  MlFinishArgs a;
  for (int s = 0; s < ML_SCALES; ++s) {
    a.part[s] = ws + p.s[s].off_part;
    a.tiles[s] = p.s[s].fwd_tiles;
    a.n_map[s] = (double)(p.s[s].h - SL_HALO) * (double)(p.s[s].w - SL_HALO);
  }
  const double n_mse = (double)p.planes * (double)H * (double)W;
  hipLaunchKernelGGL(msl_finish_kernel, dim3(1), dim3(SL_TPB), 0, st, a, (const float*)(ws + p.off_pm), B, C, n_mse, (double)w_mse,
                     (double)w_ms, (double)grad_scale * (double)w_ms / (double)p.planes, ws, ws + p.off_coef, loss3);

  // ---- backward: scale 5 down to 1 ----
  if (grad) {
    const float k_mse = (float)((double)grad_scale * (double)w_mse * 2.0 / n_mse);
    for (int s = ML_SCALES - 1; s >= 0; --s) {
      const MlScale& q = p.s[s];
      const float* xs = s ? ws + q.off_x : pred;
      const float* ys = s ? ws + q.off_y : tgt;
      const float* gnext = s < ML_SCALES - 1 ? ws + p.s[s + 1].off_g : nullptr;
      const float* coef = ws + p.off_coef + s * p.planes;
      const dim3 grid((unsigned)q.bwd_tiles, (unsigned)p.planes);
      if (s)
        hipLaunchKernelGGL(msl_backward_kernel<false>, grid, dim3(SL_TPB), 0, st, xs, ys, (const float*)(ws + q.off_maps),
                           q.map_stride, coef, gnext, ws + q.off_g, q.h, q.w, q.btx, 0.f);
      else
        hipLaunchKernelGGL(msl_backward_kernel<true>, grid, dim3(SL_TPB), 0, st, xs, ys, (const float*)(ws + q.off_maps),
                           q.map_stride, coef, gnext, grad, q.h, q.w, q.btx, k_mse);
    }
  }
  return nq_launch_status();
}

}  // extern "C"

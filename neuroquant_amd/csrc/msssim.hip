// MS-SSIM (five scales, 11-tap Gaussian window, valid filtering) of image batches: the second quality number of every
// evaluation (reference utils.py:158-164 -> pytorch_msssim.ms_ssim(X, Y, data_range=1, size_average=False)).
//
// One launch per scale.  A workgroup owns an 8 x 118 tile of the valid output region of one (frame, channel) plane: it
// stages the 18 x 128 input tile (the tile + the 10-pixel halo) of both images in LDS, filters the five moments
// (x, y, xx, yy, xy) along H into LDS, filters them along W in registers, evaluates cs_map (scales 1-4) or ssim_map
// (scale 5) and reduces it to ONE partial sum.  The same workgroup writes the 2x2-pooled images of the next scale from
// the staged tile, so a scale's images are read once (plus halo) and the moment maps never exist in memory.  A finishing
// launch adds the partial sums of every (frame, channel, scale) in a fixed order (in double), takes the means, relu, the
// five powers, their product and the channel mean.  No atomics: a frame's result depends on that frame's bytes only.
//
// Moments are taken about a pivot (the value at the centre of the staged tile, one per image and workgroup), so that
// E[x^2] - mu^2 cancels between numbers of the size of the local contrast, not of the size of the image values.  The
// float32 taps of the window do not add up to 1 but to G = 1 - 3.07e-8 (G^2 = 1 - 6.15e-8 in two dimensions), so the
// definition's variances are NOT invariant under a shift: with x = x' + p, y = y' + q,
//   g*(xy) - (g*x)(g*y) = [g*(x'y') - (g*x')(g*y')] + (1 - G^2) (q g*x' + p g*y') + p q G^2 (1 - G^2),
// and the second and third term (a few 1e-9, against C2 = 9e-4: up to 7e-6 of a map value, all of one sign) are added
// back; likewise g*x = g*x' + p G^2 for the luminance term.  X and Y go through the same instructions, so identical
// inputs give cs_map = ssim_map = 1 exactly.  The 2 x 55 window products per output pixel are explicit fused multiply-adds
// (the kernel is bound by them: one instruction per tap instead of two); everything else rounds operation by operation.
#include "nq_common.h"

namespace {

constexpr int MS_WIN = 11, MS_HALO = MS_WIN - 1, MS_SCALES = 5;
constexpr int MS_TH = 8, MS_TW = 118;                    // output tile
constexpr int MS_IH = MS_TH + MS_HALO, MS_IW = MS_TW + MS_HALO;   // staged tile: 18 x 128
constexpr int MS_VS = MS_IW + 4;                         // row stride of the H-filtered moments (16-byte reads run 4 past)
constexpr int MS_TPB = 256;
constexpr int MS_RG = 4;                                 // output rows / columns one thread filters at a time
static_assert(MS_IW * (MS_TH / MS_RG) == MS_TPB, "one (column, row group) per thread in the H pass");
static_assert(MS_IH % (MS_TPB / MS_IW) == 0, "the staging loop covers the tile's rows exactly");
static_assert(MS_TH * ((MS_TW + MS_RG - 1) / MS_RG) <= MS_TPB, "one (row, column group) per thread in the W pass");

// exp(-(i-5)^2 / (2 * 1.5^2)) / sum, evaluated in float32 as the package builds its window
__constant__ float ms_g[MS_WIN] = {0x1.0d957p-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f,
                                   0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d957p-10f};

// the exact sum of the window's float32 taps is G = 0.999999969266355; two dimensions: G^2
constexpr float MS_D2 = 6.146728898e-08f;       // 1 - G^2
constexpr float MS_G2D2 = 6.146728520e-08f;     // G^2 (1 - G^2)

// what the shift by the pivots (p of x, q of y) took from g*(xy) - (g*x)(g*y); a = g*x', b = g*y'
__device__ __forceinline__ float ms_shift_term(float p, float q, float a, float b) {
  return MS_D2 * (q * a + p * b) + (p * q) * MS_G2D2;
}

struct MsPlan {
  int h[MS_SCALES], w[MS_SCALES], nty[MS_SCALES], ntx[MS_SCALES];
  int64_t img_off[MS_SCALES];    // X of scale s (s >= 1) in the workspace; Y follows at + planes * h * w
  int64_t part_off[MS_SCALES];   // partial sums of scale s: planes * nty * ntx floats
  int64_t total;
};

inline MsPlan ms_plan(int64_t planes, int H, int W) {
  MsPlan p;
  int64_t off = 0;
  for (int s = 0; s < MS_SCALES; ++s) {
    p.h[s] = s ? (p.h[s - 1] + 1) / 2 : H;      // floor((n + 2 (n % 2) - 2) / 2) + 1
    p.w[s] = s ? (p.w[s - 1] + 1) / 2 : W;
    p.nty[s] = (p.h[s] - MS_HALO + MS_TH - 1) / MS_TH;
    p.ntx[s] = (p.w[s] - MS_HALO + MS_TW - 1) / MS_TW;
    p.img_off[s] = off;
    if (s) off += 2 * planes * p.h[s] * p.w[s];
  }
  for (int s = 0; s < MS_SCALES; ++s) {
    p.part_off[s] = off;
    off += planes * p.nty[s] * p.ntx[s];
  }
  p.total = off;
  return p;
}

// grid (ntx * nty, planes).  xo / yo: the pooled planes (oh x ow) of the next scale, null at the last scale.
template <bool LAST>
__global__ __launch_bounds__(MS_TPB) void msssim_scale_kernel(const float* __restrict__ xi, const float* __restrict__ yi,
                                                              float* __restrict__ xo, float* __restrict__ yo,
                                                              float* __restrict__ part, int h, int w, int oh, int ow, int ntx,
                                                              int nty) {
  __shared__ float sx[MS_IH][MS_IW], sy[MS_IH][MS_IW];
  __shared__ __attribute__((aligned(16))) float sv[5][MS_TH][MS_VS];
  __shared__ float red[16];
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int64_t plane = blockIdx.y;
  const int R0 = ty * MS_TH, C0 = tx * MS_TW;
  const float* __restrict__ xp = xi + plane * ((int64_t)h * w);
  const float* __restrict__ yp = yi + plane * ((int64_t)h * w);

  // ---- stage the tile + halo of both images (zeros beyond the image) ----
  {
    const int c = tid & (MS_IW - 1), gx = C0 + c;
#pragma unroll
    for (int k = 0; k < MS_IH / (MS_TPB / MS_IW); ++k) {
      const int r = tid / MS_IW + k * (MS_TPB / MS_IW), gy = R0 + r;
      const bool in = gy < h && gx < w;
      const int64_t o = (int64_t)gy * w + gx;
      sx[r][c] = in ? xp[o] : 0.f;
      sy[r][c] = in ? yp[o] : 0.f;
    }
  }
  __syncthreads();

  // ---- the next scale: avg_pool2d(kernel 2, stride 2, padding (h % 2, w % 2)), zeros padded, divisor 4.  A pooled pixel
  //      belongs to the tile that holds its first in-image row and column; its second ones lie at most one further, inside
  //      the halo (the last tile of a row / column of tiles owns everything up to the image's edge). ----
  if (!LAST) {
    const int padh = h & 1, padw = w & 1;
    const int R1 = ty == nty - 1 ? h : R0 + MS_TH, C1 = tx == ntx - 1 ? w : C0 + MS_TW;
    const int py0 = R0 ? (R0 + padh + 1) / 2 : 0, py1 = min(oh, (R1 + padh + 1) / 2);
    const int px0 = C0 ? (C0 + padw + 1) / 2 : 0, px1 = min(ow, (C1 + padw + 1) / 2);
    const int nr = max(py1 - py0, 0), nc = max(px1 - px0, 0);
    float* __restrict__ xq = xo + plane * ((int64_t)oh * ow);
    float* __restrict__ yq = yo + plane * ((int64_t)oh * ow);
    for (int e = tid; e < nr * nc; e += MS_TPB) {
      const int j = e / nc, i = e - j * nc;
      const int py = py0 + j, px = px0 + i;
      const int r = 2 * py - padh - R0, c = 2 * px - padw - C0;   // -1: the padded row / column before the image
      const bool r_in = r >= 0, c_in = c >= 0;
      const int ra = r_in ? r : 0, ca = c_in ? c : 0;
      const float xa = r_in && c_in ? sx[ra][ca] : 0.f, xb = r_in ? sx[ra][c + 1] : 0.f;
      const float xc = c_in ? sx[r + 1][ca] : 0.f, xd = sx[r + 1][c + 1];
      const float ya = r_in && c_in ? sy[ra][ca] : 0.f, yb = r_in ? sy[ra][c + 1] : 0.f;
      const float yc = c_in ? sy[r + 1][ca] : 0.f, yd = sy[r + 1][c + 1];
      const int64_t o = (int64_t)py * ow + px;
      xq[o] = ((xa + xb) + (xc + xd)) * 0.25f;
      yq[o] = ((ya + yb) + (yc + yd)) * 0.25f;
    }
  }

  // the pivots: the staged tile's centre, moved into the image where the tile hangs over its edge
  const int pr = min(MS_IH / 2, h - 1 - R0), pc = min(MS_IW / 2, w - 1 - C0);
  const float pvx = sx[pr][pc], pvy = sy[pr][pc];

  // ---- along H: thread = (column, group of 4 output rows); 14 staged rows feed 4 x 5 sums, taps in rising order ----
  {
    const int c = tid & (MS_IW - 1), r0 = (tid / MS_IW) * MS_RG;
    float acc[MS_RG][5];
#pragma unroll
    for (int j = 0; j < MS_RG; ++j)
#pragma unroll
      for (int q = 0; q < 5; ++q) acc[j][q] = 0.f;
#pragma unroll
    for (int r = 0; r < MS_RG + MS_HALO; ++r) {
      const float x = sx[r0 + r][c] - pvx, y = sy[r0 + r][c] - pvy;
      const float m[5] = {x, y, x * x, y * y, x * y};
#pragma unroll
      for (int j = 0; j < MS_RG; ++j) {
        const int t = r - j;
        if (t >= 0 && t < MS_WIN) {
#pragma unroll
          for (int q = 0; q < 5; ++q) acc[j][q] = __builtin_fmaf(ms_g[t], m[q], acc[j][q]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < MS_RG; ++j)
#pragma unroll
      for (int q = 0; q < 5; ++q) sv[q][r0 + j][c] = acc[j][q];
  }
  __syncthreads();

  // ---- along W + the maps: thread = (row, group of 4 output columns) ----
  constexpr int NCG = (MS_TW + MS_RG - 1) / MS_RG;   // 30
  float sum = 0.f;
  if (tid < MS_TH * NCG) {
    const int r = tid / NCG, c0 = (tid - r * NCG) * MS_RG;
    float acc[MS_RG][5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      float v[MS_RG + MS_HALO + 2];
#pragma unroll
      for (int k = 0; k < (MS_RG + MS_HALO + 2) / 4; ++k) {
        const float4 t = *reinterpret_cast<const float4*>(&sv[q][r][c0 + 4 * k]);
        v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w;
      }
#pragma unroll
      for (int j = 0; j < MS_RG; ++j) {
        float a = 0.f;
#pragma unroll
        for (int t = 0; t < MS_WIN; ++t) a = __builtin_fmaf(ms_g[t], v[j + t], a);
        acc[j][q] = a;
      }
    }
    const float C1c = 0.01f * 0.01f, C2c = 0.03f * 0.03f;
#pragma unroll
    for (int j = 0; j < MS_RG; ++j) {
      const int cc = c0 + j;
      // columns past the tile (or the valid region) were filtered from stale LDS: selected away, never added
      const bool ok = cc < MS_TW && C0 + cc < w - MS_HALO && R0 + r < h - MS_HALO;
      const float m1 = acc[j][0], m2 = acc[j][1];
      const float s1 = (acc[j][2] - m1 * m1) + ms_shift_term(pvx, pvx, m1, m1);
      const float s2 = (acc[j][3] - m2 * m2) + ms_shift_term(pvy, pvy, m2, m2);
      const float s12 = (acc[j][4] - m1 * m2) + ms_shift_term(pvx, pvy, m1, m2);
      float v = (2.f * s12 + C2c) / (s1 + s2 + C2c);
      if (LAST) {
        const float u1 = (m1 - pvx * MS_D2) + pvx, u2 = (m2 - pvy * MS_D2) + pvy;   // g*x = g*x' + p G^2
        v = (2.f * u1 * u2 + C1c) / (u1 * u1 + u2 * u2 + C1c) * v;
      }
      sum += ok ? v : 0.f;
    }
  }
  const float s = nq_block_sum(sum, red);
  if (tid == 0) part[plane * ((int64_t)ntx * nty) + blockIdx.x] = s;
}

struct MsFinish {
  int64_t part_off[MS_SCALES];
  int ntiles[MS_SCALES];
  double count[MS_SCALES];
};

__device__ __forceinline__ double ms_wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// grid (frames), 5 waves: wave s adds the partial sums of scale s of one channel in lane-strided order, then the tree.
__global__ __launch_bounds__(64 * MS_SCALES) void msssim_finish_kernel(const float* __restrict__ ws, MsFinish fin, int C,
                                                                       float* __restrict__ out) {
  __shared__ double val[MS_SCALES];
  const int s = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double wgt[MS_SCALES] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
  const int64_t f = blockIdx.x;
  double acc = 0.0;
  for (int c = 0; c < C; ++c) {
    const float* __restrict__ p = ws + fin.part_off[s] + (f * C + c) * (int64_t)fin.ntiles[s];
    double a = 0.0;
    for (int i = lane; i < fin.ntiles[s]; i += 64) a += (double)p[i];
    a = ms_wave_sum_d(a);
    if (lane == 0) {
      const double m = a / fin.count[s];                 // divided by the count: a map of ones has mean exactly 1
      val[s] = m > 0.0 ? pow(m, wgt[s]) : 0.0;           // relu, 0^w = 0
    }
    __syncthreads();
    if (threadIdx.x == 0) acc += val[0] * val[1] * val[2] * val[3] * val[4];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[f] = (float)(acc / (double)C);
}

inline bool ms_args_ok(int64_t frames, int C, int H, int W) {
  return frames > 0 && C > 0 && H > 0 && W > 0 && (H < W ? H : W) > MS_HALO * (1 << (MS_SCALES - 1));
}

}  // namespace

extern "C" {

int64_t nq_ms_ssim_ws_floats(int64_t frames, int C, int H, int W) {
  if (!ms_args_ok(frames, C, H, W)) return 0;
  return ms_plan(frames * C, H, W).total;
}

int nq_ms_ssim(const float* out, const float* gt, float* msssim, float* ws, int64_t frames, int C, int H, int W,
               nq_stream_t stream) {
  if (!out || !gt || !msssim || !ws || !ms_args_ok(frames, C, H, W)) return NQ_ERR_INVALID;
  const int64_t planes = frames * C;
  if (planes > 65535 || frames > 0x7fffffffLL) return NQ_ERR_UNSUPPORTED;   // grid.y
  const MsPlan p = ms_plan(planes, H, W);
  MsFinish fin;
  const float *xi = out, *yi = gt;
  for (int s = 0; s < MS_SCALES; ++s) {
    const bool last = s == MS_SCALES - 1;
    float* xo = last ? nullptr : ws + p.img_off[s + 1];
    float* yo = last ? nullptr : xo + planes * p.h[s + 1] * p.w[s + 1];
    const dim3 grid((unsigned)(p.ntx[s] * p.nty[s]), (unsigned)planes);
    if (last)
      hipLaunchKernelGGL(msssim_scale_kernel<true>, grid, dim3(MS_TPB), 0, nq_s(stream), xi, yi, xo, yo, ws + p.part_off[s],
                         p.h[s], p.w[s], 0, 0, p.ntx[s], p.nty[s]);
    else
      hipLaunchKernelGGL(msssim_scale_kernel<false>, grid, dim3(MS_TPB), 0, nq_s(stream), xi, yi, xo, yo, ws + p.part_off[s],
                         p.h[s], p.w[s], p.h[s + 1], p.w[s + 1], p.ntx[s], p.nty[s]);
    xi = xo;
    yi = yo;
    fin.part_off[s] = p.part_off[s];
    fin.ntiles[s] = p.ntx[s] * p.nty[s];
    fin.count[s] = (double)(p.h[s] - MS_HALO) * (double)(p.w[s] - MS_HALO);
  }
  hipLaunchKernelGGL(msssim_finish_kernel, dim3((unsigned)frames), dim3(64 * MS_SCALES), 0, nq_s(stream), ws, fin, C, msssim);
  return nq_launch_status();
}

}  // extern "C"

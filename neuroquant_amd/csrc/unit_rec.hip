// Unit-wise reconstruction (the layer-wise / block-wise calibration baselines): the tail of one unit's iteration
// and the QDrop input mix.  The definitions are spelled out at nq_unit_rec_loss / nq_qdrop_mix in include/nq_hip.h.
//
// nq_unit_rec_loss: a loss on the unit's OUTPUT activation pred (B, C, H r, W r) against the cached FP output, and its gradient
// carried back through GELU' (the z a NQ_EPI_PS_GELU forward saved) and PixelUnshuffle into dconv (B, C r^2, H, W), the layout
// the weight-gradient kernels read -- one pass over pred / tgt / z (/ fisher) and one write of dconv.
//
// Work split.  A workgroup of 256 lanes owns one BAND: the r rows Y = y r .. y r + r - 1 of one (b, c) plane of pred, which are
// exactly the sources of row y of the r^2 planes c r^2 + i r + j of dconv.  The band is walked in tiles of 256 conv columns
// (256 r floats of each of the r rows):
//   load    16-byte loads along the W r row (lane l takes floats 4 l .. 4 l + 3 of a row segment: every load instruction of a
//           wave covers 1 KB of one row), the gradient of the four elements is formed in registers,
//   stage   and written to LDS in the INPUT order, row i at i * RS, float X of the segment at word pad(X) = X + (X >> 5) for even r
//           (one pad word per 32 floats) and X + (X >> 2) for odd r (one per 4).  A lane's component t goes to 4 l + t + (l >> 3)
//           resp. 5 l + t: over 32 lanes all banks differ.
//   store   lane l of the store side owns columns x = 4 l .. 4 l + 3 of ONE output plane (i, j) and reads floats (x + t) r + j
//           of row i, a lane stride of 4 r floats: 8 l + (l >> 2), 16 l + (l >> 1) for r = 2, 4 and 15 l, 25 l (+ a constant)
//           for r = 3, 5 -- odd strides and the two folded ones walk the 32 banks once (enumerated for every r, t, j).  Each
//           lane stores one 16-byte piece; a wave writes 1 KB of one output row.
// r = 1 (a bare layer, or a layer-wise unit at its convolution output) has nothing to transpose: a band is a run of whole rows
// (about 4096 floats) of one plane and every gradient goes from registers straight to dconv; no LDS is touched.
// Any H, W >= 1: the 16-byte forms need W r % 4 == 0 (loads) resp. W % 4 == 0 (stores) and 16-byte aligned tensors; otherwise
// the same lanes run one float each (consecutive lanes on consecutive floats), decided once per launch on the host.
//
// Sums: per lane in double, waves by __shfl_down, the four waves through LDS in wave order, ONE double per workgroup; the
// finishing workgroup adds them lane-strided in index order, then the same tree.  fisher_full needs s_b = sum_{c,h,w} |d| g
// of the whole sample before any gradient: a first launch of G <= 256 workgroups per sample (workgroup g takes the 4096-float
// chunks g, g + G, ... of the sample) leaves G doubles; every workgroup of the gradient launch adds its sample's G doubles in
// that fixed order (2 KB from L2), and workgroup 0 also forms the loss sum_b s_b^2 / (100 n).  No atomics, nothing allocated, no
// host read: bit-identical from call to call and capturable.  -ffp-contract=off: for lp, p = 2 the float k d and the product
// with z are the two roundings of nq_lp_loss (image mode) followed by nq_ps_gelu_backward.
//
// nq_qdrop_mix: x[b] = u < prob ? xq_cache[idx[b]] : xfp_cache[idx[b]], one launch that gathers and mixes; u from Philox-4x32-10
// (nq_common.h) on counter {i >> 2 low, i >> 2 high, b, *step}, so a lane's four elements cost one generator call.
#include <cmath>

#include "nq_common.h"

namespace {

constexpr int UR_TPB = 256;
constexpr int UR_TW = 256;         // conv columns per tile, r >= 2
constexpr int UR_TW1 = 1024;       // floats per tile, r == 1
constexpr int UR_RUN1 = 4096;      // r == 1: floats of a band (whole rows; one row where W is longer)
constexpr int UR_DOT_G = 256;      // fisher_full: at most this many workgroups per sample in the dots launch
constexpr int UR_DOT_CHUNK = 4096;

enum UrMode { UR_LP2 = 0, UR_LP1 = 1, UR_LPGEN = 2, UR_FDIAG = 3, UR_FFULL = 4 };

struct UrArgs {
  const float *pred, *tgt, *fisher, *z;
  const int64_t* idx;
  float *dconv, *loss;
  double* part;          // one per workgroup
  const double* dots;    // fisher_full: G per sample
  int B, C, H, W, nb, bands, G, vec_ld, vec_st;
  float k, pm1;          // gradient coefficient, p - 1
  double ffs, inv;       // fisher_full: 2 / (100 n); the loss: 1 / count
};

// staged float X of a row -> its LDS word: one pad word per 32 floats for even r, per 4 floats for odd r
template <int R>
__host__ __device__ constexpr int ur_pad(int X) { return X + (X >> ((R & 1) ? 2 : 5)); }

__device__ __forceinline__ double ur_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
// sum over the workgroup, waves in wave order; the same double in EVERY thread
__device__ __forceinline__ double ur_block_sum(double v, double* red) {
  v = ur_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int i = 1; i < UR_TPB / 64; ++i) s += red[i];
  return s;
}

// one element: adds its loss term to the lane's sum -> dL/dpred of that element.  f: the Fisher weight (fisher modes only)
template <int MODE>
__device__ __forceinline__ float ur_elem(float x, float y, float f, float k, float pm1, double& s) {
  const float d = x - y;
  if constexpr (MODE == UR_LP2) {
    const double dd = (double)d;
    s += dd * dd;
    return k * d;
  } else if constexpr (MODE == UR_LP1) {
    s += (double)fabsf(d);
    return d > 0.f ? k : (d < 0.f ? -k : 0.f);
  } else if constexpr (MODE == UR_LPGEN) {
    const float a = fabsf(d);
    const float q = powf(a, pm1);              // |d|^(p-1): 0 at d == 0 (p > 1)
    s += (double)(q * a);
    const float ga = k * q;
    return d > 0.f ? ga : (d < 0.f ? -ga : 0.f);
  } else if constexpr (MODE == UR_FDIAG) {
    const float g2 = f * f;
    const double dd = (double)d;
    s += dd * dd * (double)g2;
    return (k * d) * g2;
  } else {
    const float kg = k * fabsf(f);             // k = 2 s_b / (100 n)
    return d > 0.f ? kg : (d < 0.f ? -kg : 0.f);
  }
}

__device__ __forceinline__ float4 ur_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// grid B * C * bands.  R == 1: a band is the run of rows [y nb, y nb + nb) of the plane, handled as one long row.
template <int R, int MODE>
__global__ __launch_bounds__(UR_TPB) void unit_rec_kernel(UrArgs a) {
  constexpr int TW = R == 1 ? UR_TW1 : UR_TW;
  constexpr int RS = R == 1 ? 1 : ur_pad<R>(R * TW);     // floats of one staged row
  __shared__ float tile[R * RS];
  __shared__ double red[UR_TPB / 64];
  const int tid = threadIdx.x;
  const int64_t bid = blockIdx.x;
  const int y = (int)(bid % a.bands);
  const int64_t bc = bid / a.bands;
  const int b = (int)(bc / a.C), c = (int)(bc - (int64_t)b * a.C);
  const int64_t tb = a.idx ? a.idx[b] : (int64_t)b;

  const int Wout = R == 1 ? min(a.nb, a.H - y * a.nb) * a.W : a.W;   // output floats of the band per plane
  const int Wr = Wout * R;                                          // floats of one band row of pred
  const int64_t plane_out = (int64_t)a.H * a.W, plane_in = plane_out * (R * R);
  const int64_t row0 = R == 1 ? (int64_t)y * a.nb * a.W : (int64_t)y * R * Wr;
  const int64_t toff = (tb * a.C + c) * plane_in + row0;
  const float* __restrict__ xp = a.pred + bc * plane_in + row0;
  const float* __restrict__ yp = a.tgt + toff;
  const float* __restrict__ fp = MODE >= UR_FDIAG ? a.fisher + toff : nullptr;
  const float* __restrict__ zp = a.z ? a.z + bc * plane_in + row0 : nullptr;
  float* __restrict__ op = a.dconv + bc * (R * R) * plane_out + (R == 1 ? row0 : (int64_t)y * a.W);

  float k = a.k;
  if constexpr (MODE == UR_FFULL) {
    const double sb = ur_block_sum(tid < a.G ? a.dots[(int64_t)b * a.G + tid] : 0.0, red);
    k = (float)(sb * a.ffs);
    if (bid == 0) {   // the loss: mean of s_b a g / 100 = sum_b s_b^2 / (100 n)
      double acc = 0.0;
      for (int bb = 0; bb < a.B; ++bb) {
        const double s = ur_block_sum(tid < a.G ? a.dots[(int64_t)bb * a.G + tid] : 0.0, red);
        acc += s * s;
      }
      if (tid == 0) a.loss[0] = (float)(acc * a.inv);
    }
  }

  double s = 0.0;
  for (int x0 = 0; x0 < Wout; x0 += TW) {
    const int tw = min(TW, Wout - x0), seg = tw * R, X0 = x0 * R;
    if (a.vec_ld) {
      const int ng = seg >> 2, total = R * ng;
      for (int q = tid; q < total; q += UR_TPB) {
        const int i = R == 1 ? 0 : q / ng, X = 4 * (q - i * ng);
        const int64_t e = (int64_t)i * Wr + X0 + X;
        const float4 xv = ur_ld4(xp + e), yv = ur_ld4(yp + e);
        float4 fv = make_float4(0.f, 0.f, 0.f, 0.f), zv = make_float4(1.f, 1.f, 1.f, 1.f), g;
        if constexpr (MODE >= UR_FDIAG) fv = ur_ld4(fp + e);
        if (zp) zv = ur_ld4(zp + e);
        g.x = ur_elem<MODE>(xv.x, yv.x, fv.x, k, a.pm1, s) * zv.x;
        g.y = ur_elem<MODE>(xv.y, yv.y, fv.y, k, a.pm1, s) * zv.y;
        g.z = ur_elem<MODE>(xv.z, yv.z, fv.z, k, a.pm1, s) * zv.z;
        g.w = ur_elem<MODE>(xv.w, yv.w, fv.w, k, a.pm1, s) * zv.w;
        if constexpr (R == 1) {
          if (a.vec_st) {
            *reinterpret_cast<float4*>(op + X0 + X) = g;
          } else {
            op[X0 + X] = g.x; op[X0 + X + 1] = g.y; op[X0 + X + 2] = g.z; op[X0 + X + 3] = g.w;
          }
        } else {
          float* t = tile + i * RS;
          t[ur_pad<R>(X)] = g.x; t[ur_pad<R>(X + 1)] = g.y; t[ur_pad<R>(X + 2)] = g.z; t[ur_pad<R>(X + 3)] = g.w;
        }
      }
    } else {
      const int total = R * seg;
      for (int q = tid; q < total; q += UR_TPB) {
        const int i = R == 1 ? 0 : q / seg, X = q - i * seg;
        const int64_t e = (int64_t)i * Wr + X0 + X;
        const float g = ur_elem<MODE>(xp[e], yp[e], MODE >= UR_FDIAG ? fp[e] : 0.f, k, a.pm1, s) * (zp ? zp[e] : 1.f);
        if constexpr (R == 1) op[X0 + X] = g;
        else tile[i * RS + ur_pad<R>(X)] = g;
      }
    }
    if constexpr (R > 1) {
      __syncthreads();
      if (a.vec_st) {
        const int ng = tw >> 2, total = R * R * ng;
        for (int q = tid; q < total; q += UR_TPB) {
          const int pl = q / ng, x = 4 * (q - pl * ng);
          const int i = pl / R, j = pl - i * R;
          const float* t = tile + i * RS;
          float4 v;
          v.x = t[ur_pad<R>(x * R + j)];
          v.y = t[ur_pad<R>((x + 1) * R + j)];
          v.z = t[ur_pad<R>((x + 2) * R + j)];
          v.w = t[ur_pad<R>((x + 3) * R + j)];
          *reinterpret_cast<float4*>(op + pl * plane_out + x0 + x) = v;
        }
      } else {
        const int total = R * R * tw;
        for (int q = tid; q < total; q += UR_TPB) {
          const int pl = q / tw, x = q - pl * tw;
          const int i = pl / R, j = pl - i * R;
          op[pl * plane_out + x0 + x] = tile[i * RS + ur_pad<R>(x * R + j)];
        }
      }
      __syncthreads();
    }
  }
  if constexpr (MODE != UR_FFULL) {
    s = ur_block_sum(s, red);
    if (tid == 0) a.part[bid] = s;
  }
}

__global__ __launch_bounds__(UR_TPB) void unit_rec_finish_kernel(const double* __restrict__ part, int64_t n, double inv,
                                                                 float* __restrict__ loss) {
  __shared__ double red[UR_TPB / 64];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += UR_TPB) s += part[i];
  s = ur_block_sum(s, red);
  if (threadIdx.x == 0) loss[0] = (float)(s * inv);
}

// fisher_full, launch 1.  grid B * G; workgroup (b, g) takes the chunks g, g + G, ... of sample b -> dots[b G + g]
__global__ __launch_bounds__(UR_TPB) void unit_rec_dots_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                               const float* __restrict__ fisher, const int64_t* __restrict__ idx,
                                                               double* __restrict__ dots, int64_t n, int G, int vec) {
  __shared__ double red[UR_TPB / 64];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / G, g = blockIdx.x - b * G;
  const int64_t tb = idx ? idx[b] : (int64_t)b;
  const float* __restrict__ xp = pred + (int64_t)b * n;
  const float* __restrict__ yp = tgt + tb * n;
  const float* __restrict__ fp = fisher + tb * n;
  const int64_t chunks = (n + UR_DOT_CHUNK - 1) / UR_DOT_CHUNK;
  double s = 0.0;
  for (int64_t ch = g; ch < chunks; ch += G) {
    const int64_t start = ch * UR_DOT_CHUNK;
    const int len = (int)(n - start < (int64_t)UR_DOT_CHUNK ? n - start : (int64_t)UR_DOT_CHUNK);
    if (vec) {
      float4 xv[4], yv[4], fv[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int e = 4 * (tid + v * UR_TPB);
        xv[v] = yv[v] = fv[v] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (e < len) {
          xv[v] = ur_ld4(xp + start + e);
          yv[v] = ur_ld4(yp + start + e);
          fv[v] = ur_ld4(fp + start + e);
        }
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) {   // an absent group adds |0 - 0| * 0
        s += (double)fabsf(xv[v].x - yv[v].x) * (double)fabsf(fv[v].x);
        s += (double)fabsf(xv[v].y - yv[v].y) * (double)fabsf(fv[v].y);
        s += (double)fabsf(xv[v].z - yv[v].z) * (double)fabsf(fv[v].z);
        s += (double)fabsf(xv[v].w - yv[v].w) * (double)fabsf(fv[v].w);
      }
    } else {
      for (int e = tid; e < len; e += UR_TPB) s += (double)fabsf(xp[start + e] - yp[start + e]) * (double)fabsf(fp[start + e]);
    }
  }
  s = ur_block_sum(s, red);
  if (tid == 0) dots[blockIdx.x] = s;
}

// grid (ceil(n / 1024), B): a lane owns elements 4 q .. 4 q + 3 of sample blockIdx.y
template <bool MIX>
__global__ __launch_bounds__(UR_TPB) void qdrop_mix_kernel(const float* __restrict__ xq, const float* __restrict__ xfp,
                                                           const int64_t* __restrict__ idx, float* __restrict__ x, int64_t n,
                                                           float prob, unsigned k0, unsigned k1, const int* __restrict__ step,
                                                           int vec) {
  const int b = blockIdx.y;
  const int64_t q = (int64_t)blockIdx.x * UR_TPB + threadIdx.x, i = 4 * q;
  if (i >= n) return;
  const int64_t src = idx[b] * n + i;
  float* out = x + (int64_t)b * n + i;
  bool take[4] = {true, true, true, true};
  if constexpr (MIX) {
    unsigned r[4];
    nq_philox4x32_10((unsigned)q, (unsigned)((uint64_t)q >> 32), (unsigned)b, (unsigned)*step, k0, k1, r);
#pragma unroll
    for (int t = 0; t < 4; ++t) take[t] = (float)(r[t] >> 8) * 5.9604644775390625e-8f < prob;
  }
  if (vec) {   // n % 4 == 0: the four elements exist
    float4 v = ur_ld4(xq + src);
    if constexpr (MIX) {
      const float4 f = ur_ld4(xfp + src);
      v.x = take[0] ? v.x : f.x;
      v.y = take[1] ? v.y : f.y;
      v.z = take[2] ? v.z : f.z;
      v.w = take[3] ? v.w : f.w;
    }
    *reinterpret_cast<float4*>(out) = v;
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (i + t < n) {
        float v = xq[src + t];
        if constexpr (MIX) v = take[t] ? v : xfp[src + t];
        out[t] = v;
      }
  }
}

struct UrPlan {
  int nb, bands, G;
  int64_t parts, per_sample;   // workgroups of the main launch; C H r W r
};

inline bool ur_plan(int B, int C, int H, int W, int r, UrPlan& p) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || r < 1 || r > 5) return false;
  const int64_t plane = (int64_t)H * W * r * r;
  if ((int64_t)B * C > (INT64_MAX / 16) / plane) return false;
  if ((int64_t)W * r > 0x7fffffffLL / 8) return false;   // a band row and its tile arithmetic stay in int
  p.nb = r == 1 ? (UR_RUN1 / W < 1 ? 1 : (UR_RUN1 / W > H ? H : UR_RUN1 / W)) : 1;
  p.bands = r == 1 ? (H + p.nb - 1) / p.nb : H;
  p.parts = (int64_t)B * C * p.bands;
  p.per_sample = (int64_t)C * plane;
  const int64_t chunks = (p.per_sample + UR_DOT_CHUNK - 1) / UR_DOT_CHUNK;
  p.G = (int)(chunks < UR_DOT_G ? chunks : UR_DOT_G);
  return true;
}

inline bool ur_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int R>
void ur_launch(int mode, const UrArgs& a, unsigned grid, hipStream_t st) {
  switch (mode) {
    case UR_LP2: hipLaunchKernelGGL((unit_rec_kernel<R, UR_LP2>), dim3(grid), dim3(UR_TPB), 0, st, a); break;
    case UR_LP1: hipLaunchKernelGGL((unit_rec_kernel<R, UR_LP1>), dim3(grid), dim3(UR_TPB), 0, st, a); break;
    case UR_LPGEN: hipLaunchKernelGGL((unit_rec_kernel<R, UR_LPGEN>), dim3(grid), dim3(UR_TPB), 0, st, a); break;
    case UR_FDIAG: hipLaunchKernelGGL((unit_rec_kernel<R, UR_FDIAG>), dim3(grid), dim3(UR_TPB), 0, st, a); break;
    default: hipLaunchKernelGGL((unit_rec_kernel<R, UR_FFULL>), dim3(grid), dim3(UR_TPB), 0, st, a); break;
  }
}

}  // namespace

extern "C" {

int64_t nq_unit_rec_loss_ws_floats(int B, int C, int H, int W, int r) {
  UrPlan p;
  return ur_plan(B, C, H, W, r, p) ? 2 * (p.parts + (int64_t)B * p.G) : 0;
}

int nq_unit_rec_loss(const float* pred, const float* tgt, const float* fisher, const int64_t* idx, const float* z, float* loss,
                     float* dconv, float* ws, int B, int C, int H, int W, int r, int mode, float p, nq_stream_t stream) {
  UrPlan pl;
  if (!pred || !tgt || !loss || !dconv || !ws || !ur_plan(B, C, H, W, r, pl)) return NQ_ERR_INVALID;
  if (mode != NQ_UNIT_LP && mode != NQ_UNIT_FISHER_DIAG && mode != NQ_UNIT_FISHER_FULL) return NQ_ERR_INVALID;
  if (mode == NQ_UNIT_LP ? (!std::isfinite(p) || p < 1.f) : !fisher) return NQ_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(ws) & 7) != 0 || dconv == pred || dconv == z) return NQ_ERR_INVALID;
  if (pl.parts > 0x7fffffffLL || (int64_t)B * pl.G > 0x7fffffffLL) return NQ_ERR_UNSUPPORTED;   // grid.x
  hipStream_t st = nq_s(stream);
  UrArgs a;
  a.pred = pred; a.tgt = tgt; a.fisher = mode == NQ_UNIT_LP ? nullptr : fisher; a.z = z; a.idx = idx;
  a.dconv = dconv; a.loss = loss;
  a.part = reinterpret_cast<double*>(ws);
  a.dots = a.part + pl.parts;
  a.B = B; a.C = C; a.H = H; a.W = W; a.nb = pl.nb; a.bands = pl.bands; a.G = pl.G;
  const bool in16 = ur_al16(pred) && ur_al16(tgt) && (!a.fisher || ur_al16(fisher)) && (!z || ur_al16(z));
  a.vec_ld = in16 && ((int64_t)W * r) % 4 == 0;
  a.vec_st = ur_al16(dconv) && W % 4 == 0 && (r > 1 || a.vec_ld);
  const double count = (double)B * (double)H * r * (double)W * r;   // the mean of the lp / fisher_diag losses: over (B, H r, W r)
  const double n = count * (double)C;
  int km = UR_FFULL;
  a.pm1 = p - 1.f;
  a.ffs = 2.0 / (100.0 * n);
  a.inv = 1.0 / count;
  if (mode == NQ_UNIT_LP) {
    km = p == 2.f ? UR_LP2 : (p == 1.f ? UR_LP1 : UR_LPGEN);
    a.k = (float)((double)C * (double)p / n);   // p / count, in the operation order of nq_lp_loss at scale C
  } else if (mode == NQ_UNIT_FISHER_DIAG) {
    km = UR_FDIAG;
    a.k = (float)(2.0 / count);
  } else {
    a.k = 0.f;
    a.inv = 1.0 / (100.0 * n);
    hipLaunchKernelGGL(unit_rec_dots_kernel, dim3((unsigned)(B * pl.G)), dim3(UR_TPB), 0, st, pred, tgt, fisher, idx,
                       const_cast<double*>(a.dots), pl.per_sample, pl.G,
                       (int)(ur_al16(pred) && ur_al16(tgt) && ur_al16(fisher) && pl.per_sample % 4 == 0));
  }
  const unsigned grid = (unsigned)pl.parts;
  switch (r) {
    case 1: ur_launch<1>(km, a, grid, st); break;
    case 2: ur_launch<2>(km, a, grid, st); break;
    case 3: ur_launch<3>(km, a, grid, st); break;
    case 4: ur_launch<4>(km, a, grid, st); break;
    default: ur_launch<5>(km, a, grid, st); break;
  }
  if (km != UR_FFULL)
    hipLaunchKernelGGL(unit_rec_finish_kernel, dim3(1), dim3(UR_TPB), 0, st, a.part, pl.parts, a.inv, loss);
  return nq_launch_status();
}

int nq_qdrop_mix(const float* xq_cache, const float* xfp_cache, const int64_t* idx, float* x, int B, int64_t n, float prob,
                 uint64_t seed, const int* step, nq_stream_t stream) {
  if (!xq_cache || !idx || !x || B <= 0 || n <= 0 || !(prob >= 0.f)) return NQ_ERR_INVALID;
  const bool mix = prob < 1.f;
  if (mix && (!xfp_cache || !step)) return NQ_ERR_INVALID;
  if (n > INT64_MAX / 8 / B) return NQ_ERR_INVALID;
  const int64_t gx = (n + 4 * UR_TPB - 1) / (4 * UR_TPB);
  if (B > 65535 || gx > 0x7fffffffLL) return NQ_ERR_UNSUPPORTED;
  const int vec = ur_al16(xq_cache) && ur_al16(x) && (!mix || ur_al16(xfp_cache)) && n % 4 == 0;
  const dim3 grid((unsigned)gx, (unsigned)B);
  if (mix)
    hipLaunchKernelGGL(qdrop_mix_kernel<true>, grid, dim3(UR_TPB), 0, nq_s(stream), xq_cache, xfp_cache, idx, x, n, prob,
                       (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), step, vec);
  else
    hipLaunchKernelGGL(qdrop_mix_kernel<false>, grid, dim3(UR_TPB), 0, nq_s(stream), xq_cache, xfp_cache, idx, x, n, prob, 0u, 0u,
                       step, vec);
  return nq_launch_status();
}

}  // extern "C"

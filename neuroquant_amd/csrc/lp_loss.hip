// Absolute-error objectives: the streaming loss w_abs * mean |d|^p + w_mse * mean d^2 (d = pred - tgt) with its gradient; the
// reference's `l1`, `Fusion7`, `Fusion8` losses and lp_loss(p) of its calibration, and -- in accumulate mode, launched behind
// nq_ssim_loss / nq_ssim_loss_head / nq_msssim_loss -- the L1 term of `Fusion2/4/6/9/10/11/12`.  The definition and the modes
// are spelled out at nq_lp_loss in include/nq_hip.h; the choices below are DESIGN.md §32.
//
// Streaming launch.  A workgroup of 256 lanes owns one CHUNK of LP_CHUNK = 4096 consecutive elements that lies inside ONE
// (frame, channel) plane (a plane of H*W elements is ceil(H*W / 4096) chunks, the last one short), so its partial sum of head
// gradients belongs to one channel and a uint8 target plane is one contiguous run of the cache.  At (2, 3, 640, 1280) that is
// 1200 workgroups of 4 waves: all of them are resident at once on 256 CUs (8 such workgroups fit a CU), and every lane has
// four independent 16-byte loads per array in flight.  A (1, 1, 1, 1) image is one workgroup with one live lane.
//
// Inside a chunk: the address of the chunk's first pred element decides a scalar HEAD of 0..3 elements up to the next 16-byte
// boundary, then comes the vector BODY (lane l takes the float4 groups l, l + 256, l + 512, l + 768: all loads of a lane are
// issued before the first is used), then a scalar TAIL of 0..3 elements.  H*W need not be a multiple of 4: every plane after
// the first may start misaligned, and the head absorbs that.  pred, a float target and grad share one element offset; where
// their base addresses do not share the phase mod 16 too (a caller's odd view) the whole chunk runs on the scalar lanes.  The
// uint8 target is read 4 bytes per lane where that address is 4-byte aligned -- its phase is the cache frame's, not pred's --
// and byte by byte otherwise; both convert as gather_u8_kernel does, (float)byte / 255.f.
//
// p and the absent terms are template cases (LpTerm x MSE), not branches of the inner loop: p == 1 is a compare and a
// select, no transcendental; p == 2 and w_abs == 0 run the squared-error instantiation (the host folds w_abs into the
// coefficient of d); general p calls the accurate library powf ONCE per element for |d|^(p-1) and gets |d|^p by one
// multiply; w_mse == 0 instantiations hold no squared-error arithmetic.  sign(0) = 0: an element with pred == tgt gets a
// gradient of exactly 0 in every case (powf(0, p - 1) = 0 for p > 1).
//
// Sums: per lane in double, wave reduction by __shfl_down, the four waves through LDS in wave order, ONE float partial per
// workgroup for each of A = sum |d|^p, M = sum d^2 and (head mode) the sum of the head gradients it wrote.  The finishing
// launch adds the partials lane-strided in index order, then the same tree, in double: workgroup 0 the loss, workgroup 1 + c
// the bias gradient of channel c (frame by frame).  No atomics, nothing allocated, no host read: bit-identical from call to
// call and capturable.  Everything rounds operation by operation (-ffp-contract=off), so the gradient float that the head mode
// multiplies by tanh' is the very float the image mode stores.
#include <cmath>

#include "nq_common.h"

namespace {

constexpr int LP_TPB = 256;
constexpr int LP_CHUNK = 4096;                       // ops.LP_LOSS_CHUNK
constexpr int LP_VPL = LP_CHUNK / (4 * LP_TPB);      // float4 groups per lane

enum LpTerm { LP_NONE = 0, LP_P1 = 1, LP_PGEN = 2 };   // the |d|^p term: absent (or folded into the squared error), p == 1, general p
enum LpGrad { LP_FWD = 0, LP_IMG = 1, LP_HEAD = 2 };   // no gradient, dL/dpred, the gradient at the head conv's output + db partials

struct LpCoef {
  float kA, kM, pm1;   // scale w_abs p / N, scale 2 w_mse / N (p == 2: + the folded absolute term), p - 1
};

// one element: adds its |d|^p and d^2 to the lane's sums -> scale dL/dpred of that element
template <int TERM, bool MSE>
__device__ __forceinline__ float lp_elem(float x, float y, const LpCoef& k, double& sa, double& sm) {
  static_assert(TERM != LP_NONE || MSE, "a loss with no term");
  const float d = x - y;
  float g = 0.f;
  if constexpr (TERM == LP_P1) {
    sa += (double)fabsf(d);
    g = d > 0.f ? k.kA : (d < 0.f ? -k.kA : 0.f);
  } else if constexpr (TERM == LP_PGEN) {
    const float a = fabsf(d);
    const float q = powf(a, k.pm1);            // |d|^(p-1): 0 at d == 0 (p > 1)
    sa += (double)(q * a);
    const float ga = k.kA * q;
    g = d > 0.f ? ga : (d < 0.f ? -ga : 0.f);
  }
  if constexpr (MSE) {
    const double dd = (double)d;
    sm += dd * dd;
    if constexpr (TERM == LP_NONE) g = k.kM * d;
    else g = g + k.kM * d;
  }
  return g;
}

// what is stored for an element whose image gradient is g: g, or (HEAD) g * tanh' as tanh_out_bwd_kernel forms it; `old` is added
// in accumulate mode.  The head value (without `old`) goes into the lane's db sum.
template <int GM>
__device__ __forceinline__ float lp_out(float g, float x, float old, bool acc, double& sg) {
  float r = g;
  if constexpr (GM == LP_HEAD) {
    const float t = 2.f * x - 1.f;
    r = g * 0.5f * (1.f - t * t);
    sg += (double)r;
  }
  return acc ? old + r : r;
}

__device__ __forceinline__ double lp_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// sums of three doubles over the workgroup, valid in thread 0; waves are added in wave order
__device__ __forceinline__ void lp_block_sum3(double& a, double& b, double& c, double (*red)[3]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  a = lp_wave_sum(a);
  b = lp_wave_sum(b);
  c = lp_wave_sum(c);
  __syncthreads();
  if (lane == 0) {
    red[wave][0] = a;
    red[wave][1] = b;
    red[wave][2] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int i = 1; i < LP_TPB / 64; ++i) {
      a += red[i][0];
      b += red[i][1];
      c += red[i][2];
    }
}

// grid planes * cpp (cpp = chunks per plane).  part_a / part_m / part_g: one float per workgroup (part_g: LP_HEAD only).
template <int TERM, bool MSE, bool U8, int GM>
__global__ __launch_bounds__(LP_TPB) void lp_loss_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                         const uint8_t* __restrict__ cache, const int64_t* __restrict__ idx, int C,
                                                         int64_t hw, int64_t cpp, float* grad, float* __restrict__ part_a,
                                                         float* __restrict__ part_m, float* __restrict__ part_g, LpCoef k,
                                                         int accumulate) {
  __shared__ double red[LP_TPB / 64][3];
  const int tid = threadIdx.x;
  const int64_t bid = blockIdx.x;
  const int64_t plane = bid / cpp;
  const int64_t start = (bid - plane * cpp) * LP_CHUNK;
  const int len = (int)(hw - start < (int64_t)LP_CHUNK ? hw - start : (int64_t)LP_CHUNK);
  const int64_t off = plane * hw + start;
  const float* __restrict__ xp = pred + off;
  float* gp = GM != LP_FWD ? grad + off : nullptr;
  const float* __restrict__ yf = nullptr;
  const uint8_t* __restrict__ yu = nullptr;
  if constexpr (U8) {
    const int64_t b = plane / C;
    yu = cache + (idx[b] * C + (plane - b * C)) * hw + start;
  } else {
    yf = tgt + off;
  }
  const bool acc = GM != LP_FWD && accumulate != 0;

  // head | body | tail of the chunk (uniform over the workgroup)
  const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(xp) & 15);
  bool vec = (mis & 3) == 0;
  if constexpr (!U8) vec = vec && (reinterpret_cast<uintptr_t>(yf) & 15) == mis;
  if constexpr (GM != LP_FWD) vec = vec && (reinterpret_cast<uintptr_t>(gp) & 15) == mis;
  const int head = vec ? min(len, (int)(((16u - mis) & 15u) >> 2)) : 0;
  const int nvec = vec ? (len - head) >> 2 : 0;
  const bool u8vec = U8 && (reinterpret_cast<uintptr_t>(yu + head) & 3) == 0;

  double sa = 0.0, sm = 0.0, sg = 0.0;

  // ---- body: every load of the lane first, then the arithmetic and the stores ----
  float4 x[LP_VPL], y[LP_VPL], o[LP_VPL];
#pragma unroll
  for (int v = 0; v < LP_VPL; ++v) {
    const int g4 = tid + v * LP_TPB;
    x[v] = y[v] = o[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (g4 < nvec) {
      const int e = head + 4 * g4;
      x[v] = *reinterpret_cast<const float4*>(xp + e);
      if constexpr (U8) {
        uchar4 q;
        if (u8vec) {
          q = *reinterpret_cast<const uchar4*>(yu + e);
        } else {
          q.x = yu[e]; q.y = yu[e + 1]; q.z = yu[e + 2]; q.w = yu[e + 3];
        }
        y[v] = make_float4((float)q.x / 255.f, (float)q.y / 255.f, (float)q.z / 255.f, (float)q.w / 255.f);
      } else {
        y[v] = *reinterpret_cast<const float4*>(yf + e);
      }
      if constexpr (GM != LP_FWD)
        if (acc) o[v] = *reinterpret_cast<const float4*>(gp + e);
    }
  }
#pragma unroll
  for (int v = 0; v < LP_VPL; ++v) {
    const int g4 = tid + v * LP_TPB;
    if (g4 < nvec) {
      float4 r;
      r.x = lp_out<GM>(lp_elem<TERM, MSE>(x[v].x, y[v].x, k, sa, sm), x[v].x, o[v].x, acc, sg);
      r.y = lp_out<GM>(lp_elem<TERM, MSE>(x[v].y, y[v].y, k, sa, sm), x[v].y, o[v].y, acc, sg);
      r.z = lp_out<GM>(lp_elem<TERM, MSE>(x[v].z, y[v].z, k, sa, sm), x[v].z, o[v].z, acc, sg);
      r.w = lp_out<GM>(lp_elem<TERM, MSE>(x[v].w, y[v].w, k, sa, sm), x[v].w, o[v].w, acc, sg);
      if constexpr (GM != LP_FWD) *reinterpret_cast<float4*>(gp + head + 4 * g4) = r;
    }
  }

  // ---- head and tail: the elements [0, head) and [head + 4 nvec, len), one per lane (all of the chunk when nothing is vector) ----
  const int nscalar = len - 4 * nvec;
  for (int i = tid; i < nscalar; i += LP_TPB) {
    const int e = i < head ? i : i + 4 * nvec;
    const float xs = xp[e];
    float ys;
    if constexpr (U8) ys = (float)yu[e] / 255.f;
    else ys = yf[e];
    const float g = lp_elem<TERM, MSE>(xs, ys, k, sa, sm);
    if constexpr (GM != LP_FWD) gp[e] = lp_out<GM>(g, xs, acc ? gp[e] : 0.f, acc, sg);
  }

  lp_block_sum3(sa, sm, sg, red);
  if (tid == 0) {
    if constexpr (TERM != LP_NONE) part_a[bid] = (float)sa;
    if constexpr (MSE) part_m[bid] = (float)sm;
    if constexpr (GM == LP_HEAD) part_g[bid] = (float)sg;
  }
}

// Workgroup 0: the loss from the n partial sums of each present term, lane-strided in index order, then the tree, in double.
//   a_from_m: p == 2, A is M.  Workgroup 1 + c (launched with db): db[c] from the partial sums of channel c, frame by frame.
__global__ __launch_bounds__(LP_TPB) void lp_loss_finish_kernel(const float* __restrict__ part_a, const float* __restrict__ part_m,
                                                                const float* __restrict__ part_g, int64_t n, double count,
                                                                double w_abs, double w_mse, int has_a, int has_m, int a_from_m,
                                                                float scale, int accumulate, float* __restrict__ loss3, int B,
                                                                int C, int64_t cpp, float* __restrict__ db) {
  __shared__ double red[LP_TPB / 64][3];
  double a = 0.0, m = 0.0, g = 0.0;
  if (blockIdx.x > 0) {
    const int c = blockIdx.x - 1;
    for (int b = 0; b < B; ++b) {
      const float* __restrict__ p = part_g + ((int64_t)b * C + c) * cpp;
      for (int64_t i = threadIdx.x; i < cpp; i += LP_TPB) g += (double)p[i];
    }
    lp_block_sum3(g, a, m, red);
    if (threadIdx.x == 0) db[c] = accumulate ? db[c] + (float)g : (float)g;
    return;
  }
  for (int64_t i = threadIdx.x; i < n; i += LP_TPB) {
    if (has_a) a += (double)part_a[i];
    if (has_m) m += (double)part_m[i];
  }
  lp_block_sum3(a, m, g, red);
  if (threadIdx.x == 0) {
    const double M = m / count, A = a_from_m ? M : a / count;
    const float l = (float)(w_abs * A + w_mse * M);
    if (accumulate) {
      loss3[0] = loss3[0] + scale * l;
    } else {
      loss3[0] = scale * l;
      loss3[1] = (float)A;     // 0 where the term is absent (w_abs == 0, p != 2: not computed)
      loss3[2] = (float)M;     // 0 where the term is absent (w_mse == 0, p != 2: not computed)
    }
  }
}

struct LpPlan {
  int64_t planes, hw, cpp, parts;
};

inline bool lp_plan(int B, int C, int H, int W, LpPlan& p) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return false;
  p.planes = (int64_t)B * C;
  p.hw = (int64_t)H * W;
  if (p.planes > (INT64_MAX / 8) / p.hw) return false;
  p.cpp = (p.hw + LP_CHUNK - 1) / LP_CHUNK;
  p.parts = p.planes * p.cpp;
  return true;
}

struct LpCall {
  const float *pred, *tgt;
  const uint8_t* cache;
  const int64_t* idx;
  float *grad, *ws;
  int C, accumulate;
  LpPlan plan;
  LpCoef k;
  hipStream_t st;
};

template <int TERM, bool MSE, bool U8, int GM>
void lp_launch(const LpCall& c) {
  const LpPlan& p = c.plan;
  hipLaunchKernelGGL((lp_loss_kernel<TERM, MSE, U8, GM>), dim3((unsigned)p.parts), dim3(LP_TPB), 0, c.st, c.pred, c.tgt, c.cache,
                     c.idx, c.C, p.hw, p.cpp, c.grad, c.ws, c.ws + p.parts, c.ws + 2 * p.parts, c.k, c.accumulate);
}

template <int TERM, bool MSE, bool U8>
void lp_launch_grad(const LpCall& c, int gm) {
  if (gm == LP_HEAD) lp_launch<TERM, MSE, U8, LP_HEAD>(c);
  else if (gm == LP_IMG) lp_launch<TERM, MSE, U8, LP_IMG>(c);
  else lp_launch<TERM, MSE, U8, LP_FWD>(c);
}

template <int TERM, bool MSE>
void lp_launch_target(const LpCall& c, int gm) {
  if (c.cache) lp_launch_grad<TERM, MSE, true>(c, gm);
  else lp_launch_grad<TERM, MSE, false>(c, gm);
}

}  // namespace

extern "C" {

int64_t nq_lp_loss_ws_floats(int B, int C, int H, int W) {
  LpPlan p;
  return lp_plan(B, C, H, W, p) ? 3 * p.parts : 0;
}

int nq_lp_loss(const float* pred, const float* tgt, const uint8_t* cache_u8, const int64_t* idx, float* loss3, float* grad, float* db,
               float* ws, int B, int C, int H, int W, float p, float w_abs, float w_mse, float scale, int accumulate,
               nq_stream_t stream) {
  LpCall c;
  if (!pred || !loss3 || !ws || !lp_plan(B, C, H, W, c.plan)) return NQ_ERR_INVALID;
  if ((tgt == nullptr) == (cache_u8 == nullptr) || (cache_u8 && !idx)) return NQ_ERR_INVALID;
  if (db && !grad) return NQ_ERR_INVALID;   // the bias gradient is the sum of what the launch writes (accumulate mode included)
  if (!std::isfinite(p) || p < 1.f) return NQ_ERR_INVALID;   // below 1 the gradient is singular at d == 0
  if (!std::isfinite(w_abs) || !std::isfinite(w_mse) || !std::isfinite(scale) || w_abs < 0.f || w_mse < 0.f) return NQ_ERR_INVALID;
  if (w_abs == 0.f && w_mse == 0.f) return NQ_ERR_INVALID;
  if (c.plan.parts > 0x7fffffffLL) return NQ_ERR_UNSUPPORTED;   // grid.x
  c.pred = pred; c.tgt = tgt; c.cache = cache_u8; c.idx = idx; c.grad = grad; c.ws = ws; c.C = C;
  c.accumulate = accumulate != 0;
  c.st = nq_s(stream);
  const double n = (double)c.plan.planes * (double)c.plan.hw;
  const bool p2 = p == 2.f;
  const bool has_a = w_abs > 0.f && !p2, has_m = w_mse > 0.f || (p2 && w_abs > 0.f);
  c.k.kA = (float)((double)scale * (double)w_abs * (double)p / n);
  c.k.kM = (float)((double)scale * ((double)w_mse + (p2 ? (double)w_abs : 0.0)) * 2.0 / n);
  c.k.pm1 = p - 1.f;
  const int gm = db ? LP_HEAD : (grad ? LP_IMG : LP_FWD);
  if (!has_a) lp_launch_target<LP_NONE, true>(c, gm);
  else if (p == 1.f) has_m ? lp_launch_target<LP_P1, true>(c, gm) : lp_launch_target<LP_P1, false>(c, gm);
  else has_m ? lp_launch_target<LP_PGEN, true>(c, gm) : lp_launch_target<LP_PGEN, false>(c, gm);
  hipLaunchKernelGGL(lp_loss_finish_kernel, dim3(db ? 1u + (unsigned)C : 1u), dim3(LP_TPB), 0, c.st, ws, ws + c.plan.parts,
                     ws + 2 * c.plan.parts, c.plan.parts, n, (double)w_abs, (double)w_mse, (int)has_a, (int)has_m, (int)p2, scale,
                     c.accumulate, loss3, B, C, c.plan.cpp, db);
  return nq_launch_status();
}

}  // extern "C"

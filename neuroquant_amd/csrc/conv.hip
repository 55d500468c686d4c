// C-ABI entry points of the convolution side: tile selection + dispatch to the per-kernel-size
// implicit-GEMM / weight-gradient kernels, weight re-layout, split-K slab reduction.
#include <algorithm>

#include "nq_common.h"
#include "seg_table.h"

extern "C" {
int nq_tiny_pw_supported(int B, int Cin, int H, int W, int Cout, int k);
int nq_tiny_pw_ksl(int Cin);
int nq_tiny_pw_forward(const float* x, const float* wt, const float* bias, float* y, float* z, const float* zprev, int B,
                       int Cin, int H, int W, int Cout, int ld, int r, int epi, hipStream_t st);
int nq_tiny_pw_wgrad(const float* x, const float* dy, float* dw, float* db, int B, int Cin, int H, int W, int Cout,
                     hipStream_t st);
}

extern "C" {
int nq_conv_igemm_k1(const float*, const float*, const float*, float*, float*, int, int, int, int, int, int, int, int, int,
                     int, float*, const float*, hipStream_t);
int nq_conv_igemm_k3(const float*, const float*, const float*, float*, float*, int, int, int, int, int, int, int, int, int,
                     int, float*, const float*, hipStream_t);
int nq_conv_igemm_k5(const float*, const float*, const float*, float*, float*, int, int, int, int, int, int, int, int, int,
                     int, float*, const float*, hipStream_t);
int nq_conv_splitk_finish(const float*, const float*, float*, float*, const float*, int, int, int, int, int, int, int,
                          hipStream_t);
int nq_conv_splitk_finish_sg(int64_t, int);
int nq_head_supported(int, int);
int nq_head_forward_route(int, int, int, int, int, int, int, int*);
int nq_head_dgrad_route(int, int, int, int, int, int, int, int, int*, int*, int*, int*);
int nq_head_forward(const float*, const float*, int, const float*, float*, int, int, int, int, int, int, int, hipStream_t);
int nq_head_dgrad(const float*, const float*, int, const float*, float*, int, int, int, int, int, int, int, int, hipStream_t);
int nq_conv_wgrad_k1(const float*, const float*, float*, float*, int, int, int, int, int, int, int, int, int, int,
                     hipStream_t);
int nq_conv_wgrad_k3(const float*, const float*, float*, float*, int, int, int, int, int, int, int, int, int, int,
                     hipStream_t);
int nq_conv_wgrad_k5(const float*, const float*, float*, float*, int, int, int, int, int, int, int, int, int, int,
                     hipStream_t);
}

namespace {

constexpr int kMiOptions[] = {11, 10, 9, 8, 6, 5, 4, 3, 2, 1};

inline int ci_per_slice(int k) { return k == 5 ? 4 : (k == 3 ? 8 : 16); }
inline bool ks_ok(int k) { return k == 1 || k == 3 || k == 5; }

// forward / data-gradient: fewest padded output channels, then the widest tile
inline int pick_mi_fwd(int Cout) {
  int best = 1, best_pad = 1 << 30;
  for (int mi : kMiOptions) {
    int mt = 16 * mi, pad = (Cout + mt - 1) / mt * mt;
    if (pad < best_pad) {
      best_pad = pad;
      best = mi;
    }
  }
  return best;
}

// split-K factor of the implicit-GEMM kernel: layers with few pixel tiles (dec0..dec3 and their data gradients)
// would otherwise occupy a handful of the 256 CUs with a very long K loop
inline int pick_nsplit(int B, int Cin, int H, int W, int Cout, int k) {
  const int mi = pick_mi_fwd(Cout);
  const int64_t base = (int64_t)((W + 31) / 32) * ((H + 3) / 4) * ((Cout + 16 * mi - 1) / (16 * mi)) * B;
  if (base >= 384) return 1;
  const int ncg = (Cin + ci_per_slice(k) - 1) / ci_per_slice(k);
  int ns = (int)((512 + base - 1) / base);
  if (ns > ncg) ns = ncg;
  if (ns > 32) ns = 32;
  return ns < 1 ? 1 : ns;
}

inline bool use_head_fwd(int Cout, int k, int epi) {
  return nq_head_supported(Cout, k) && (epi == NQ_EPI_PLAIN || epi == NQ_EPI_TANH);
}
inline bool use_head_dgrad(int Cin, int k, int epi, bool has_bias) {
  return nq_head_supported(Cin, k) && (epi == NQ_EPI_PLAIN || epi == NQ_EPI_DGRAD_GELU) && !has_bias;
}

inline int wgrad_ni(int mi, int k) { return k == 1 ? 2 : (mi <= 3 ? 6 : (mi <= 6 ? 4 : 3)); }

// ONE resolution of a weight-gradient shape: nq_conv_wgrad, nq_conv_wgrad_ws_floats and nq_conv_wgrad_plan read it.  The slab
// dimensions are resolved for the tiny shapes too: their workspace keeps its size although tiny_pw_wgrad never writes it.
inline nq_conv_wgrad_plan_t route_wgrad(int B, int Cin, int H, int W, int Cout, int k) {
  nq_conv_wgrad_plan_t p{};
  int64_t best_cost = INT64_MAX;
  const int N = Cin * k * k;
  for (int mi : kMiOptions) {
    int ni = wgrad_ni(mi, k);
    int mt = 16 * mi, nt = 64 * ni;
    int co_pad = (Cout + mt - 1) / mt * mt, n_pad = (N + nt - 1) / nt * nt;
    int64_t cost = (int64_t)co_pad * n_pad;
    if (cost < best_cost) {
      best_cost = cost;
      p.mi = mi;
      p.ni = ni;
      p.co_pad = co_pad;
      p.n_pad = n_pad;
    }
  }
  int tiles = (p.co_pad / (16 * p.mi)) * (p.n_pad / (64 * p.ni));
  int nseg = ((W + 31) / 32) * H * B;
  // one full wave of workgroups: 256 CUs x 2 resident workgroups (the kernels sit at 170-230 VGPRs), no ragged tail
  int ns = 512 / tiles;
  if (ns > nseg) ns = nseg;
  // (fewer, longer splits for problems with few segments -- HNeRV-3M dec2: 20 segments, 16 splits x 3.1 MB of slab -- were
  // tried: the reduction got 5 us shorter and the kernel 8 us longer)
  if (ns > 256) ns = 256;
  if (ns < 1) ns = 1;
  p.nsplit = ns;
  p.nseg = nseg;
  p.ws_floats = (int64_t)p.nsplit * p.co_pad * ((int64_t)p.n_pad + 1);
  p.kernel = NQ_CONV_WGRAD_MFMA;
  if (nq_tiny_pw_supported(B, Cin, H, W, Cout, k)) {
    p.kernel = NQ_CONV_WGRAD_TINY;
    p.mi = p.ni = p.co_pad = p.n_pad = p.nsplit = p.nseg = 0;
    p.tiny_px8 = ((int64_t)H * W) % 8 == 0;
  }
  return p;
}

// The implicit-GEMM side of a forward shape, whatever the epilogue: tile, K-loop groups, split, workspace.  A shape the tiny kernel
// owns never reaches the implicit-GEMM kernel (the head kernels come before it, nothing after): no workspace.
struct FwdShape {
  int tiny, mi, ncg, nsplit;
  int64_t ws_floats;
};
inline FwdShape route_fwd_shape(int B, int Cin, int H, int W, int Cout, int k) {
  FwdShape s{};
  s.tiny = nq_tiny_pw_supported(B, Cin, H, W, Cout, k);
  s.mi = pick_mi_fwd(Cout);
  s.ncg = (Cin + ci_per_slice(k) - 1) / ci_per_slice(k);
  s.nsplit = pick_nsplit(B, Cin, H, W, Cout, k);
  s.ws_floats = (!s.tiny && s.nsplit > 1) ? (int64_t)s.nsplit * B * Cout * H * W : 0;
  return s;
}

// ONE resolution of a forward call (sizes and epilogue already validated): nq_conv_forward, nq_conv_forward_plan and
// nq_conv_split_out read it.  NQ_ERR_UNSUPPORTED where a head knob names a build that is not compiled.
inline int route_fwd(int B, int Cin, int H, int W, int Cout, int k, int ld, int r, int epi, bool has_bias, nq_conv_plan& p) {
  p = nq_conv_plan{};
  const FwdShape s = route_fwd_shape(B, Cin, H, W, Cout, k);
  p.ws_floats = s.ws_floats;
  // <= 4 output channels (the decoder head) / <= 4 input channels (its data gradient): HBM-bound vector kernels
  if (use_head_fwd(Cout, k, epi)) {
    const int route = nq_head_forward_route(B, Cin, H, W, Cout, k, ld, &p.rows);
    if (route < 0) return NQ_ERR_UNSUPPORTED;
    p.kernel = route ? NQ_CONV_HEAD_FWD : NQ_CONV_HEAD_FWD_LDS;
    if (!route) p.hd_ks = k;
    return NQ_OK;
  }
  if (use_head_dgrad(Cin, k, epi, has_bias)) {
    const bool gelu = epi == NQ_EPI_DGRAD_GELU;
    const int route = nq_head_dgrad_route(B, Cout, H, W, Cin, k, gelu ? r : 1, gelu, &p.rows, &p.hd_r2, &p.hd_co, &p.hd_px);
    if (route < 0) return NQ_ERR_UNSUPPORTED;
    p.kernel = route ? NQ_CONV_HEAD_DGRAD : NQ_CONV_HEAD_DGRAD_LDS;
    p.split_out = route;
    if (!route) p.hd_ks = k;
    return NQ_OK;
  }
  // 1x1 convolutions over a handful of pixels (decoder stem / first block): compact thread-per-output kernel
  if (s.tiny) {
    p.kernel = NQ_CONV_TINY;
    p.ksl = nq_tiny_pw_ksl(Cin);
    return NQ_OK;
  }
  p.kernel = NQ_CONV_IGEMM;
  p.mi = s.mi;
  p.ncg = s.ncg;
  p.nsplit = s.nsplit;
  p.finish = s.nsplit > 1 ? nq_conv_splitk_finish_sg((int64_t)B * Cout * H * W, s.nsplit) : 0;
  if ((int64_t)B * s.nsplit > 65535) return NQ_ERR_UNSUPPORTED;
  return NQ_OK;
}

// the argument checks of nq_conv_forward that depend on values alone (no pointers); epilogue without the split-word bits
inline int check_fwd_args(int B, int Cin, int H, int W, int Cout, int k, int r, int epilogue) {
  if (B <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0) return NQ_ERR_INVALID;
  if (!ks_ok(k)) return NQ_ERR_UNSUPPORTED;
  if (epilogue < 0 || epilogue > NQ_EPI_DGRAD_GELU) return NQ_ERR_INVALID;
  if ((epilogue == NQ_EPI_PS_GELU || epilogue == NQ_EPI_PS) && (r <= 0 || Cout % (r * r) != 0)) return NQ_ERR_INVALID;
  if (epilogue == NQ_EPI_DGRAD_GELU && (r <= 0 || H % r != 0 || W % r != 0)) return NQ_ERR_INVALID;
  if (B > 65535) return NQ_ERR_UNSUPPORTED;
  return NQ_OK;
}

__global__ __launch_bounds__(256) void weight_fwd_layout_kernel(const float* __restrict__ w, float* __restrict__ wt,
                                                                int Cout, int K, int krows, int ld) {
  // wt[k][co] = w[co][k]  (k = (ci*KS+kh)*KS+kw is the OIHW inner index); 32x32 LDS transpose tile
  __shared__ float tile[32][33];
  const int k0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int j = ty; j < 32; j += 8) {
    int co = c0 + j, k = k0 + tx;
    tile[j][tx] = (co < Cout && k < K) ? w[(int64_t)co * K + k] : 0.f;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    int k = k0 + j, co = c0 + tx;
    if (k < krows && co < ld) wt[(int64_t)k * ld + co] = tile[tx][j];
  }
}

__global__ __launch_bounds__(256) void weight_bwd_layout_kernel(const float* __restrict__ w, float* __restrict__ wt,
                                                                int Cout, int Cin, int KK, int krows, int ld) {
  // wt[(co*KK + tap')][ci] = w[co][ci][KK-1-tap']   (both spatial taps flipped)
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)krows * ld) return;
  int row = (int)(i / ld), ci = (int)(i - (int64_t)row * ld);
  int co = row / KK, tap = row - co * KK;
  float v = 0.f;
  if (co < Cout && ci < Cin) v = w[((int64_t)co * Cin + ci) * KK + (KK - 1 - tap)];
  wt[i] = v;
}

// Both fp32 operands of several layers in ONE launch (the per-layer kernels above are launch-bound: five ~5 us launches per
// iteration for the layers that stay on the fp32 kernels).  Flat element index per segment; same values as the two
// kernels above.
__global__ __launch_bounds__(256) void weight_layouts_multi_kernel(NqSegTable<NqWLSeg> t) {
  int blk;
  const int k = t.find((int)blockIdx.x, blk);
  nq_wl_elem(t.s[k], (int64_t)blk * 256 + threadIdx.x);
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slab, const float* __restrict__ slab_db,
                                                           float* __restrict__ dw, float* __restrict__ db, int Cout, int N,
                                                           int co_pad, int n_pad, int nsplit) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = (int64_t)Cout * N;
  if (i < total) {
    int co = (int)(i / N), n = (int)(i - (int64_t)co * N);
    const float* p = slab + (int64_t)co * n_pad + n;
    const int64_t stride = (int64_t)co_pad * n_pad;
    float s = 0.f;
    for (int k = 0; k < nsplit; ++k) s += p[k * stride];
    dw[i] = s;
  } else if (db && i < total + Cout) {
    int co = (int)(i - total);
    float s = 0.f;
    for (int k = 0; k < nsplit; ++k) s += slab_db[(int64_t)k * co_pad + co];
    db[co] = s;
  }
}

}  // namespace

extern "C" {

int nq_conv_operand_dims(int Cin, int Cout, int k, int* krows, int* ld) {
  if (!ks_ok(k) || Cin <= 0 || Cout <= 0 || !krows || !ld) return NQ_ERR_INVALID;
  int ci = ci_per_slice(k);
  *krows = (Cin + ci - 1) / ci * ci * k * k;
  int mt = 16 * pick_mi_fwd(Cout);
  *ld = (Cout + mt - 1) / mt * mt;
  return NQ_OK;
}

int nq_weight_layouts(const float* w, float* wt_fwd, float* wt_bwd, int Cout, int Cin, int k, int krows_fwd, int ld_fwd,
                      int krows_bwd, int ld_bwd, nq_stream_t stream) {
  if (!w || Cout <= 0 || Cin <= 0 || k <= 0) return NQ_ERR_INVALID;
  const int KK = k * k;
  if (wt_fwd) {
    if (krows_fwd < Cin * KK || ld_fwd < Cout) return NQ_ERR_INVALID;
    dim3 g((unsigned)((krows_fwd + 31) / 32), (unsigned)((ld_fwd + 31) / 32));
    hipLaunchKernelGGL(weight_fwd_layout_kernel, g, dim3(256), 0, nq_s(stream), w, wt_fwd, Cout, Cin * KK, krows_fwd,
                       ld_fwd);
  }
  if (wt_bwd) {
    if (krows_bwd < Cout * KK || ld_bwd < Cin) return NQ_ERR_INVALID;
    int64_t total = (int64_t)krows_bwd * ld_bwd;
    hipLaunchKernelGGL(weight_bwd_layout_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, nq_s(stream), w,
                       wt_bwd, Cout, Cin, KK, krows_bwd, ld_bwd);
  }
  return nq_launch_status();
}

int nq_weight_layouts_multi(const nq_wl_seg* segs, int nseg, nq_stream_t stream) {
  return NqSegTable<NqWLSeg>::launch_all(
      segs, 2 * nseg, [&](int i, NqWLSeg& d) { return nq_wl_fill(segs, i, d); },
      [&](const NqSegTable<NqWLSeg>& t, unsigned blocks) {
        hipLaunchKernelGGL(weight_layouts_multi_kernel, dim3(blocks), dim3(256), 0, nq_s(stream), t);
      });
}

int64_t nq_conv_forward_ws_floats(int B, int Cin, int H, int W, int Cout, int k) {
  if (!ks_ok(k) || B <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0) return 0;
  return route_fwd_shape(B, Cin, H, W, Cout, k).ws_floats;
}

// 1 when nq_conv_forward can write its output y as split {hi | lo} words for this call (include/nq_hip.h)
int nq_conv_split_out(int B, int Cin, int H, int W, int Cout, int k, int r, int epilogue, int has_bias) {
  nq_conv_plan p;
  if (check_fwd_args(B, Cin, H, W, Cout, k, r, epilogue) != NQ_OK) return 0;
  if (route_fwd(B, Cin, H, W, Cout, k, 0, r, epilogue, has_bias != 0, p) != NQ_OK) return 0;
  return p.split_out;
}

int nq_conv_forward_plan(int B, int Cin, int H, int W, int Cout, int k, int r, int epilogue, int has_bias, nq_conv_plan* out) {
  if (!out) return NQ_ERR_INVALID;
  if (int rc = check_fwd_args(B, Cin, H, W, Cout, k, r, epilogue)) return rc;
  return route_fwd(B, Cin, H, W, Cout, k, 0, r, epilogue, has_bias != 0, *out);
}

int nq_conv_forward(const float* x, const float* wt, const float* bias, float* y, float* z, float* ws, int B, int Cin, int H,
                    int W, int Cout, int k, int krows, int ld, int r, int epilogue, const float* zprev, nq_stream_t stream) {
  if (!x || !wt || (!y && epilogue != NQ_EPI_PS) || B <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0)
    return NQ_ERR_INVALID;
  if (!ks_ok(k)) return NQ_ERR_UNSUPPORTED;
  // NQ_EPI_Y_SPLIT: the output as split {hi | lo} words -- only the streaming head data gradient offers it (nq_conv_split_out)
  const int y_split = (epilogue & NQ_EPI_Y_SPLIT) ? 1 : 0;
  if (epilogue & NQ_EPI_X_SPLIT) return NQ_ERR_UNSUPPORTED;
  epilogue &= ~NQ_EPI_Y_SPLIT;
  if (y_split && !nq_conv_split_out(B, Cin, H, W, Cout, k, r, epilogue, bias != nullptr)) return NQ_ERR_UNSUPPORTED;
  if (epilogue < 0 || epilogue > NQ_EPI_DGRAD_GELU) return NQ_ERR_INVALID;
  if ((epilogue == NQ_EPI_PS_GELU || epilogue == NQ_EPI_PS) && !z) return NQ_ERR_INVALID;
  if (epilogue == NQ_EPI_DGRAD_GELU && !zprev) return NQ_ERR_INVALID;
  int need_rows, need_ld;
  nq_conv_operand_dims(Cin, Cout, k, &need_rows, &need_ld);
  if (krows < need_rows || ld < need_ld || (ld & 3)) return NQ_ERR_INVALID;
  if (int rc = check_fwd_args(B, Cin, H, W, Cout, k, r, epilogue)) return rc;
  nq_conv_plan p;
  if (int rc = route_fwd(B, Cin, H, W, Cout, k, ld, r, epilogue, bias != nullptr, p)) return rc;
  hipStream_t st = nq_s(stream);
  switch (p.kernel) {
    case NQ_CONV_HEAD_FWD:
    case NQ_CONV_HEAD_FWD_LDS: return nq_head_forward(x, wt, ld, bias, y, B, Cin, H, W, Cout, k, epilogue, st);
    case NQ_CONV_HEAD_DGRAD:
    case NQ_CONV_HEAD_DGRAD_LDS:
      return nq_head_dgrad(x, wt, ld, epilogue == NQ_EPI_DGRAD_GELU ? zprev : nullptr, y, B, Cout, H, W, Cin, k,
                           epilogue == NQ_EPI_DGRAD_GELU ? r : 1, y_split, st);
    case NQ_CONV_TINY: return nq_tiny_pw_forward(x, wt, bias, y, z, zprev, B, Cin, H, W, Cout, ld, r, epilogue, st);
    default: break;
  }
  const int mi = p.mi, ns = p.nsplit;
  if (ns > 1 && !ws) return NQ_ERR_INVALID;
  int rc;
  switch (k) {
    case 1: rc = nq_conv_igemm_k1(x, wt, bias, y, z, B, Cin, H, W, Cout, ld, r, epilogue, mi, ns, ws, zprev, st); break;
    case 3: rc = nq_conv_igemm_k3(x, wt, bias, y, z, B, Cin, H, W, Cout, ld, r, epilogue, mi, ns, ws, zprev, st); break;
    default: rc = nq_conv_igemm_k5(x, wt, bias, y, z, B, Cin, H, W, Cout, ld, r, epilogue, mi, ns, ws, zprev, st); break;
  }
  if (rc != NQ_OK || ns == 1) return rc;
  return nq_conv_splitk_finish(ws, bias, y, z, zprev, B, H, W, Cout, r, epilogue, ns, st);
}

int64_t nq_conv_wgrad_ws_floats(int B, int Cin, int H, int W, int Cout, int k) {
  if (!ks_ok(k) || B <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0) return 0;
  return route_wgrad(B, Cin, H, W, Cout, k).ws_floats;
}

int nq_conv_wgrad_plan(int B, int Cin, int H, int W, int Cout, int k, nq_conv_wgrad_plan_t* out) {
  if (!out || B <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0) return NQ_ERR_INVALID;
  if (!ks_ok(k)) return NQ_ERR_UNSUPPORTED;
  *out = route_wgrad(B, Cin, H, W, Cout, k);
  return NQ_OK;
}

// seg == NULL: split kernel + reduction; seg != NULL: the split kernel only, *seg describes the pending reduction
int nq_conv_wgrad(const float* x, const float* dy, float* dw, float* db, float* ws, int B, int Cin, int H, int W, int Cout,
                  int k, nq_wgr_seg* seg, nq_stream_t stream) {
  if (!x || !dy || !dw || !ws || B <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0) return NQ_ERR_INVALID;
  if (!ks_ok(k)) return NQ_ERR_UNSUPPORTED;
  if (seg) *seg = nq_wgr_seg{nullptr, nullptr, dw, db, Cout, Cin * k * k, 0, 0, 0, 0, 1};
  const nq_conv_wgrad_plan_t p = route_wgrad(B, Cin, H, W, Cout, k);
  if (p.kernel == NQ_CONV_WGRAD_TINY) return nq_tiny_pw_wgrad(x, dy, dw, db, B, Cin, H, W, Cout, nq_s(stream));
  float* slab = ws;
  float* slab_db = ws + (int64_t)p.nsplit * p.co_pad * p.n_pad;
  hipStream_t st = nq_s(stream);
  int rc;
  switch (k) {
    case 1: rc = nq_conv_wgrad_k1(x, dy, slab, slab_db, B, Cin, H, W, Cout, p.co_pad, p.n_pad, p.nsplit, p.mi, p.ni, st); break;
    case 3: rc = nq_conv_wgrad_k3(x, dy, slab, slab_db, B, Cin, H, W, Cout, p.co_pad, p.n_pad, p.nsplit, p.mi, p.ni, st); break;
    default: rc = nq_conv_wgrad_k5(x, dy, slab, slab_db, B, Cin, H, W, Cout, p.co_pad, p.n_pad, p.nsplit, p.mi, p.ni, st); break;
  }
  if (rc != NQ_OK) return rc;
  const int N = Cin * k * k;
  if (seg) {   // deferred: the sequential fixed-order sum over the splits (sg = 1) runs in nq_wgrad_reduce_multi
    *seg = nq_wgr_seg{slab, db ? slab_db : nullptr, dw, db, Cout, N, p.co_pad, p.n_pad, p.nsplit, 0, 1};
    return NQ_OK;
  }
  int64_t total = (int64_t)Cout * N + Cout;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, slab, slab_db, dw, db, Cout,
                     N, p.co_pad, p.n_pad, p.nsplit);
  return nq_launch_status();
}

}  // extern "C"

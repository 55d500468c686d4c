// C-ABI entry points of the bf16x3 convolution path (conv_igemm3_impl.h): weight pre-split/re-order + dispatch.
#include <cstdlib>
#include "nq_common.h"
#include "conv3_layout.h"
#include "seg_table.h"

extern "C" {
int nq_conv_igemm3_k3(const float*, const void*, const float*, float*, float*, const float*, int, int, int, int, int, int, int,
                      int, int, int, float*, hipStream_t);
int nq_conv_igemm3_k5(const float*, const void*, const float*, float*, float*, const float*, int, int, int, int, int, int, int,
                      int, int, int, float*, hipStream_t);
// levels (l) and half (h) units: one signature; the unsigned* is the half builds' flag word and null for the levels builds
typedef int nq_igemm3_levels_fn(const float*, const void*, const float*, const float*, float*, float*, unsigned*, int, int, int, int,
                                int, int, int, int, hipStream_t);
nq_igemm3_levels_fn nq_conv_igemm3l_k3, nq_conv_igemm3l_k5, nq_conv_igemm3h_k3, nq_conv_igemm3h_k5;
int nq_conv_splitk_finish(const float*, const float*, float*, float*, const float*, int, int, int, int, int, int, int, hipStream_t);
int nq_conv_flat3_plan(int, int, int, int, int, int, NqFlat3Plan*);
int nq_conv3_waves_k3(int, int, int, int, int);
int nq_conv3_waves_k5(int, int, int, int, int);
int nq_conv3_lds_k3(int, int, int);
int nq_conv3_lds_k5(int, int, int);
int nq_conv_flat3(const float*, const void*, const float*, float*, float*, const float*, float*, int, int, int, int, int, int, int, int,
                  int, const NqFlat3Plan*, hipStream_t);
int nq_conv_wgrad_flat3_ok(int, int, int, int, int, int);
int nq_conv_wgrad_flat3(const float*, const float*, float*, float*, int, int, int, int, int, int, hipStream_t);
int nq_conv_wgrad3_k3(const float*, const float*, float*, float*, int, int, int, int, int, int, int, int, int, int, int, int, hipStream_t);
int nq_conv_wgrad3_k5(const float*, const float*, float*, float*, int, int, int, int, int, int, int, int, int, int, int, int, hipStream_t);
}

namespace {

constexpr int CC = 16;

// channel blocks (of 16) per workgroup: fewest padded channels among the wide tiles (narrow tiles re-read the
// activation patch once per tile and run too few MFMAs per barrier), narrow tiles only for narrow layers
inline int pick_mi3(int Cout) {
  if (Cout <= 16) return 1;
  if (Cout <= 32) return 2;
  int best = 3, best_pad = 1 << 30;
  for (int mi = 5; mi >= 3; --mi) {
    int mt = 16 * mi, pad = (Cout + mt - 1) / mt * mt;
    if (pad < best_pad) {
      best_pad = pad;
      best = mi;
    }
  }
  // many-channel layers are the low-resolution ones (few pixel tiles): 64-channel tiles give a workgroup count that fills
  // the chip in one round where 48 needs a second, nearly empty one and 80 leaves a third of the slots idle (dec3
  // 64->848 at 40x80: forward 0.093 -> 0.075 ms, weight gradient 0.126 -> 0.108 ms), at <= 6 % more padding
  if (Cout > 256 && (Cout + 63) / 64 * 64 <= best_pad + best_pad * 6 / 100) return 4;
  return best;
}
// what every entry point of this path asks of a shape before anything is planned for it
inline bool shape_ok3(int B, int Cin, int H, int W, int Cout, int k) {
  return (k == 3 || k == 5) && B > 0 && Cin > 0 && H > 0 && W > 0 && Cout > 0;
}

// Operand of the bf16x3 kernels: 16-byte fragment slots [global k-step][plane hi/lo][co tile][kq][MT] of 8 bf16 k-values.
// transposed = 0: logical conv == the stored conv, src(co, ch, tap) = w[co][ch][tap]
// transposed = 1: data gradient, logical (Cin=Cout_w -> Cout=Cin_w): src(co, ch, tap) = w[ch][co][KK-1-tap]
struct WL3 {
  const float* w;
  uint4* out;
  int Cin, Cout, KK, NST, NSTT, nchunk, tail, co_tiles, MT, transposed;   // tail: kind of the last chunk, NSTT its k-steps
  int co16;        // 16-channel groups of output channels: ceil(co_tiles*MT / 16)
  int64_t slots;
};
// (k-value e of lane group kq at k-step s -> (channel, tap): wl3_elem, conv3_layout.h)

// One workgroup per (16-channel chunk c of the logical input channels, group of 16 logical output channels): the 16 x 16 x KK
// weights it needs are 16 CONTIGUOUS runs of 16*KK floats in the stored tensor (rows = co for the forward operand, = ch
// for the transposed one), loaded coalesced into LDS; the fragment slots are then assembled from LDS and stored 16 bytes
// per thread, 256 contiguous bytes per 16 lanes.  (Round 2's kernel gathered the 8 values of a slot straight from global
// memory at a stride of KK or Cout*KK floats: 22.6 us for the layers of HNeRV-3M, most of it uncoalesced reads.)
constexpr int WL3_KKMAX = 25;
// (KK is a template parameter: the index arithmetic -- e / (16*KK), rem / KK per loaded float, eight (channel, tap) pairs per
// slot -- was most of the kernel's time with a run-time divisor)
// F16 (nq_weight_layout3_f16, the half build of the tiled forward): the hi plane holds the values as IEEE halves, the lo plane zeros
template <int KK, bool F16 = false>
__device__ __forceinline__ void wl3_tile(const WL3& p, int c, int g16, float* __restrict__ T /* [16][16*KK (+1)] */) {
  constexpr int RS = 16 * KK + 1;   // row stride: odd -> the 16 rows of a column land in different banks
  const int tid = threadIdx.x;
  const int nfull = p.nchunk - (p.tail ? 1 : 0);
  const int kind = (c == nfull) ? p.tail : 0;
  const int nst = kind ? p.NSTT : p.NST;
  const int64_t gs0 = (int64_t)c * p.NST;   // every chunk in front of c is a full one
  // rows a = 0..15, columns (b, tap): forward a = co (g16*16 + a), b = ch (c*16 + b); transposed a = ch, b = co
  const int Ra = p.transposed ? p.Cin : p.Cout;            // valid extent of the row index (stored tensor's dim 0)
  const int Cb = p.transposed ? p.Cout : p.Cin;            // stored tensor's dim 1
  const int a0 = p.transposed ? c * 16 : g16 * 16, b0 = p.transposed ? g16 * 16 : c * 16;
  // all KK loads of a thread in flight together (branch-free: an out-of-range element reads element 0 and is zeroed
  // afterwards) -- with a conditional load the compiler waited for each group of five before issuing the next
  {
    float v[KK];
#pragma unroll
    for (int j = 0; j < KK; ++j) {
      const int e = tid + j * 256;
      const int a = e / (16 * KK), rem = e - a * (16 * KK);
      const int bb = rem / KK;
      const bool ok = a0 + a < Ra && b0 + bb < Cb;
      const float t = p.w[ok ? ((int64_t)(a0 + a) * Cb + b0) * KK + rem : 0];
      v[j] = ok ? t : 0.f;
    }
#pragma unroll
    for (int j = 0; j < KK; ++j) {
      const int e = tid + j * 256;
      const int a = e / (16 * KK), rem = e - a * (16 * KK);
      T[a * RS + rem] = v[j];
    }
  }
  __syncthreads();
  const int MT = p.MT;
  const int64_t plane_stride = (int64_t)p.co_tiles * 4 * MT;
  for (int sl = tid; sl < nst * 4 * 16; sl += 256) {
    const int col = sl & 15, kq = (sl >> 4) & 3, st = sl >> 6;
    const int co = g16 * 16 + col;
    if (co >= p.co_tiles * MT) continue;
    unsigned hi[4], lo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        int ch, tap;
        wl3_elem(kind, KK, st, kq, 2 * j + t, ch, tap);
        float x = 0.f;
        if (tap < KK) x = p.transposed ? T[ch * RS + col * KK + (KK - 1 - tap)] : T[col * RS + ch * KK + tap];
        v[t] = x;
      }
      if constexpr (F16) {
        const _Float16 h0 = (_Float16)v[0], h1 = (_Float16)v[1];
        hi[j] = (unsigned)__builtin_bit_cast(unsigned short, h0) | ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16);
        lo[j] = 0u;
        continue;
      }
      __bf16 h0 = (__bf16)v[0], h1 = (__bf16)v[1];
      __bf16 l0 = (__bf16)(v[0] - (float)h0), l1 = (__bf16)(v[1] - (float)h1);
      hi[j] = (unsigned)__builtin_bit_cast(unsigned short, h0) | ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16);
      lo[j] = (unsigned)__builtin_bit_cast(unsigned short, l0) | ((unsigned)__builtin_bit_cast(unsigned short, l1) << 16);
    }
    const int tile = co / MT, co_l = co - tile * MT;
    const int64_t base = (gs0 + st) * 2 * plane_stride + (int64_t)tile * 4 * MT + kq * MT + co_l;
    p.out[base] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    p.out[base + plane_stride] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
  }
}

template <bool F16 = false>
__device__ __forceinline__ void wl3_seg_tile(const WL3& p, int blk, float* T) {
  if (p.KK == 25) wl3_tile<25, F16>(p, blk / p.co16, blk % p.co16, T);
  else wl3_tile<9, F16>(p, blk / p.co16, blk % p.co16, T);
}
__global__ __launch_bounds__(256) void weight_layout3_kernel(WL3 p) {
  __shared__ float T[16 * (16 * WL3_KKMAX + 1)];
  wl3_seg_tile(p, (int)blockIdx.x, T);
}

__global__ __launch_bounds__(256) void weight_layout3_f16_kernel(WL3 p) {
  __shared__ float T[16 * (16 * WL3_KKMAX + 1)];
  wl3_seg_tile<true>(p, (int)blockIdx.x, T);
}

// all layers' operands (forward and data-gradient) in ONE launch: the table travels as a kernel argument
__global__ __launch_bounds__(256) void weight_layout3_multi_kernel(NqSegTable<WL3> t) {
  __shared__ float T[16 * (16 * WL3_KKMAX + 1)];
  int blk;
  const int k = t.find((int)blockIdx.x, blk);
  wl3_seg_tile(t.s[k], blk, T);
}

// Round 4: the fp32 operands of the layers that stay on the fp32 / vector kernels (the 1 x 1 stem, the head) in the SAME launch
// as the bf16x3 operands: blocks past the bf16x3 tiles run the element code of weight_layouts_multi_kernel (conv.hip) -- the
// same values, one launch (~5 us of launch floor) less per iteration.
struct WLAll {
  NqSegTable<WL3> t3;
  NqSegTable<NqWLSeg> tf;
};
__global__ __launch_bounds__(256) void weight_layouts_all_kernel(WLAll t) {
  __shared__ float T[16 * (16 * WL3_KKMAX + 1)];
  const int nb3 = t.t3.blocks();
  if ((int)blockIdx.x < nb3) {
    int blk;
    const int k = t.t3.find((int)blockIdx.x, blk);
    wl3_seg_tile(t.t3.s[k], blk, T);
    return;
  }
  int blk;
  const int k = t.tf.find((int)blockIdx.x - nb3, blk);
  nq_wl_elem(t.tf.s[k], (int64_t)blk * 256 + threadIdx.x);
}

// split-K of the forward / data-gradient kernel over 16-channel chunks when the pixel x channel grid alone cannot fill
// the chip (deep, low-resolution layers): ~512 workgroups, every split non-empty
struct Fwd3Plan {
  int mi, nsplit, per;
  int64_t wgs;
};
inline Fwd3Plan plan_fwd3(int B, int Cin, int H, int W, int Cout) {
  Fwd3Plan p;
  p.mi = pick_mi3(Cout);
  p.wgs = (int64_t)((W + 31) / 32) * ((H + 7) / 8) * ((Cout + 16 * p.mi - 1) / (16 * p.mi)) * B;
  const int nchunk = (Cin + CC - 1) / CC;
  p.nsplit = 1;
  p.per = nchunk;
  // (a K loop of <= 4 chunks is not worth splitting: the slabs and the finish launch cost more than the half-empty round --
  // NeRV's 36 -> 384 layer at 40 x 80: 180 workgroups, 20.0 + 23.2 us split in two vs one launch without slabs)
  static const int min_chunks = [] { const char* e = getenv("NQ_SPLITK_MIN_CHUNKS"); return e ? atoi(e) : 5; }();
  if (p.wgs < 256 && nchunk >= min_chunks) {
    int want = (int)(512 / p.wgs);   // floor: stay within ONE round of 512 resident workgroups (a second, nearly empty
                                     // round costs as much as the first)
    if (want > nchunk) want = nchunk;
    p.per = (nchunk + want - 1) / want;
    p.nsplit = (nchunk + p.per - 1) / p.per;
  }
  return p;
}

// Few-pixel layers (conv_flat3.hip): taken when the flat kernel needs no slabs (forward convolutions of the deep layers: no
// finish launch), or when the tiled kernel's grid would not fill the chip even with split-K (it would fall back to the fp32
// kernels).  Long K loops that the tiled split-K path already handles stay there: measured (us, kernel + finish) HNeRV dec2
// data gradient 21.0 flat vs 21.7 tiled, NeRV dec1 data gradient 22.4 vs 18.7, NeRV dec2 data gradient 19.3 vs 25.6 (fp32).
//
// Everything nq_conv_forward3 decides from the shape, resolved ONCE per call (shape_ok3 holds): the queries below read it and
// the launch runs it, so they cannot disagree.  The only caller of nq_conv_flat3_plan and of plan_fwd3.
struct Fwd3Route {
  bool flat;               // the few-pixel kernel (conv_flat3.hip) has the shape, else the tiled one (conv_igemm3_impl.h)
  int mi, tail;            // the operand's layout: 16*mi-channel tiles, kind of the last chunk; the tiled kernel's tile
  int nsplit, per_split;   // K split of the kernel that has the shape
  NqFlat3Plan fp;          // few-pixel launch plan (flat only)
  int supported;           // nq_conv3_supported
  int split_io;            // nq_conv3_split_io
  int64_t ws_floats;       // nq_conv_forward3_ws_floats
};
inline Fwd3Route route_fwd3(int B, int Cin, int H, int W, int Cout, int k) {
  Fwd3Route r{};
  const bool fits = nq_conv_flat3_plan(B, Cin, H, W, Cout, k, &r.fp) != 0;
  const Fwd3Plan p = plan_fwd3(B, Cin, H, W, Cout);
  const bool tiled_fills = p.wgs * p.nsplit >= 128;   // still smaller grids stay on the fp32 split-K kernel
  r.flat = fits && (r.fp.nsplit == 1 || !tiled_fills);
  r.mi = p.mi;
  r.tail = wl3_tail_kind(Cin);
  r.nsplit = r.flat ? r.fp.nsplit : p.nsplit;
  r.per_split = r.flat ? r.fp.per_split : p.per;
  r.ws_floats = r.nsplit > 1 ? (int64_t)r.nsplit * B * Cout * H * W : 0;
  // <= 4 channels on either side (the image head): the streaming VALU kernels of conv_head.hip are faster than a
  // >80 %-padded MFMA tile (measured 0.17 / 0.23 ms vs 0.21 / 0.38 ms, forward / data gradient of 37->3 at 640x1280).
  // The kernel addresses the input with 32-bit buffer offsets (conv_igemm3_impl.h): tensors of 4 GiB and more stay on the
  // fp32 kernels.
  if (Cout <= 4 || Cin <= 4 || (int64_t)B * Cin * H * W * 4 >= 0xFFFFFF00ll) return r;   // supported = split_io = 0
  // few-pixel kernel -- offered for layers whose weight tensor is worth streaming; a toy convolution (a few hundred weights)
  // stays on the exact-fp32 kernels: nothing to gain, and its callers keep fp32-level results
  r.supported = (r.flat && (int64_t)Cin * k * k * Cout >= 65536) || tiled_fills;
  // Which sides may travel as split {hi | lo} words: the input where the tiled kernel with >= 32-channel tiles stages it (the
  // few-pixel kernel reads floats only), the output where the kernel's own epilogue writes it (no slabs)
  if (r.supported) r.split_io = (!r.flat && r.mi >= 2 ? NQ_EPI_X_SPLIT : 0) | (r.nsplit == 1 ? NQ_EPI_Y_SPLIT : 0);
  return r;
}

struct Wg3Plan {
  int mi, ni, co_pad, n_pad, nsplit, pc;
};
// NQ_WGRAD3_PC=0 keeps every layer on the 4-wave kernel (A/B runs of the two structures in one build)
inline bool wgrad3_ss1() {   // NQ_WGRAD3_SS=1: 32-pixel segments only (A/B runs)
  const char* e = std::getenv("NQ_WGRAD3_SS");
  return e && e[0] == '1';
}
inline bool wgrad3_pc_enabled() {   // read per call: tools/bench_kernels.py flips it between launches of one process
  const char* e = std::getenv("NQ_WGRAD3_PC");
  return !(e && e[0] == '0');
}
inline Wg3Plan plan_wgrad3(int B, int Cin, int H, int W, int Cout, int k) {
  Wg3Plan p;
  p.mi = pick_mi3(Cout);
  const int N = Cin * k * k;
  if (N <= 64) {
    p.ni = 1;
  } else {   // n-tile of 64*ni columns: the ni in {5,6,7} that pads C_in*k*k least (7 only with <= 4 channel blocks);
             // ties go to the wider tile (fewer tiles re-staging dY)
    int best = 6, best_pad = 1 << 30;
    for (int ni = 5; ni <= (p.mi <= 4 ? 7 : 6); ++ni) {
      const int nt = 64 * ni, pad = (N + nt - 1) / nt * nt;
      if (pad <= best_pad) {
        best_pad = pad;
        best = ni;
      }
    }
    p.ni = best;
  }
  int mt = 16 * p.mi, nt = 64 * p.ni;
  p.co_pad = (Cout + mt - 1) / mt * mt;
  p.n_pad = (N + nt - 1) / nt * nt;
  int tiles = (p.co_pad / mt) * (p.n_pad / nt);
  // Very wide layers (more than 256 output tiles: the UVG-12M shape's 128 -> 1712) fell off the producer/consumer kernel, which
  // wants one workgroup per CU in ONE round: the 80-channel tile gets them back under 256 when its extra padding is small
  // (preferring them wherever they pad no more -- HNeRV-3M's 64 -> 848: 880 instead of 896 rows -- measured 66-68 -> 65 us with one
  // more slab to reduce: not kept)
  if (tiles > 256 && p.mi < 5 && p.ni >= 5 && p.ni <= 6 /* (no 80 x 448 tile) */) {
    const int co5 = (Cout + 79) / 80 * 80, tiles5 = (co5 / 80) * (p.n_pad / nt);
    if (tiles5 <= 256 && co5 * 100 <= p.co_pad * 105) {
      p.mi = 5;
      mt = 80;
      p.co_pad = co5;
      tiles = tiles5;
    }
  }
  const int nseg = ((W + 31) / 32) * H * B;
  int ns = 512 / tiles;  // one full wave of workgroups (2 resident per CU)
  if (ns > nseg) ns = nseg;
  if (ns < 1) ns = 1;
  p.nsplit = ns;
  p.pc = 0;
  // the producer/consumer kernel addresses x through SIGNED and dy through unsigned 32-bit byte offsets (raw buffer loads):
  // operands of 2 GiB and more stay on the 4-wave kernel (64-bit pointers)
  const bool pc_ok = wgrad3_pc_enabled() && (int64_t)B * Cin * H * W * 4 < (1ll << 31) && (int64_t)B * Cout * H * W * 4 < (1ll << 31);
  // producer/consumer kernel (8 waves, ONE workgroup per CU): wide tiles with a long K loop per workgroup
  if (pc_ok && p.ni >= 5 && p.mi >= 3 && tiles <= 256) {
    // rows per staged segment: 4 (2) where H divides and every workgroup still gets >= 16 segments; NQ_WGRAD3_SS=1 -> 1
    int sy = 1;
    int ns_pc = 256 / tiles;
    const int segs_x = (W + 31) / 32;
    // segments per workgroup a taller segment must leave (NQ_WGRAD3_MINSEG; 16 until late round 4: NeRV-3M's 24 -> 96 at
    // 160 x 320 stayed on one-row segments for it, 44.2 us; 12 -> two rows 42.3; 6 -> four rows 41.3; HNeRV dec3 84.0 -> 80.9)
    static const int minseg = [] { const char* e = std::getenv("NQ_WGRAD3_MINSEG"); return e ? atoi(e) : 6; }();
    if (!wgrad3_ss1() && ns_pc >= 1) {
      // (k = 3, 80 x 384 tile: the four-row image is 2 x 82032 bytes of LDS, 224 more than a workgroup can have; two rows
      // fit.  launch_wgrad3p in conv_wgrad3_impl.h does not build that kernel and static_asserts that it is the only one)
      const bool sy4_fits = !(k == 3 && p.mi == 5 && p.ni == 6);
      if (sy4_fits && H % 4 == 0 && segs_x * (H / 4) * B / ns_pc >= minseg) sy = 4;
      else if (H % 2 == 0 && segs_x * (H / 2) * B / ns_pc >= minseg) sy = 2;
    }
    const int nseg_pc = segs_x * (H / sy) * B;
    const int need = minseg < 16 ? minseg : 16;
    // a little short of segments for one workgroup per CU (NeRV-3M's 36 -> 384 at 40 x 80: 240 one-row segments for 42 splits):
    // fewer splits, as long as three quarters of the CUs still get a workgroup (NQ_WGRAD3_SHRINK=0: the 4-wave kernel as before)
    static const int shrink = [] { const char* e = std::getenv("NQ_WGRAD3_SHRINK"); return e ? atoi(e) : 1; }();
    if (shrink && ns_pc >= 1 && nseg_pc / ns_pc < need && (nseg_pc / need) * tiles >= 192) ns_pc = nseg_pc / need;
    if (ns_pc >= 1 && nseg_pc / ns_pc >= need) {
      p.pc = sy == 1 ? 1 : 10 + sy;
      p.nsplit = ns_pc;
    }
  }
  // narrow problems streaming a big tensor (the role-swapped head gradient: 3 x 9 n-values, K = all pixels): the 4-wave
  // kernel runs 18 MFMAs per barrier with one 6 KB segment in flight per workgroup (latency-bound, 2.1 TB/s); the
  // producer/consumer kernel with 128-pixel segments keeps 2 x 24 KB in flight per CU
  if (pc_ok && p.ni == 1 && p.mi >= 2 && p.mi <= 5 && tiles == 1 && W % 128 == 0) {
    const int nseg_pc = (W / 128) * H * B;
    if (nseg_pc / 256 >= 8) {
      p.pc = 4;
      // NQ_WGRAD3_HEAD_SPLITS (timing runs): 256 = one 8-wave workgroup per CU (round 2), 512 = two
      static const int hs = [] { const char* e = std::getenv("NQ_WGRAD3_HEAD_SPLITS"); return e ? atoi(e) : 512; }();
      p.nsplit = (p.mi <= 3 && nseg_pc / hs >= 8) ? hs : 256;   // (64- / 80-channel tiles: one workgroup per CU)
    }
  }
  return p;
}

// Everything the weight-gradient entries decide from the shape, resolved ONCE per call (shape_ok3 holds); the role-swapped
// entries resolve the EXCHANGED problem (Cin <-> Cout).  The only caller of nq_conv_wgrad_flat3_ok and of plan_wgrad3.
struct Wg3Route {
  bool flat;           // the few-pixel kernel (conv_wgrad_flat3.hip: no slabs, no reduction) has the shape
  Wg3Plan p;           // plan of the tiled kernels (what nq_conv_wgrad3_plan reports, also for few-pixel shapes)
  int supported;       // nq_conv_wgrad3_supported
  int split_io;        // nq_conv_wgrad3_split_io
  int sg;              // split groups of the slab reduction (wgrad3_reduce_kernel<sg>, nq_wgr_seg::sg)
  int64_t ws_floats;   // nq_conv_wgrad3_ws_floats
};
inline Wg3Route route_wgrad3(int B, int Cin, int H, int W, int Cout, int k) {
  Wg3Route r{};
  r.flat = nq_conv_wgrad_flat3_ok(B, Cin, H, W, Cout, k) != 0;
  r.p = plan_wgrad3(B, Cin, H, W, Cout, k);
  // few-pixel layers leave no slabs (a token workspace keeps the pointer non-NULL)
  r.ws_floats = r.flat ? 4 : (int64_t)r.p.nsplit * r.p.co_pad * ((int64_t)r.p.n_pad + 1);
  // tiled kernels: enough 32-pixel segments to split over
  r.supported = Cout > 4 && (r.flat || (int64_t)((W + 31) / 32) * H * B >= 128);
  r.split_io = (r.supported && !r.flat && nq_wgrad3_pc_takes_split(r.p.pc)) ? 3 : 0;
  r.sg = ((int64_t)Cout * Cin * k * k + Cout < 65536 && r.p.nsplit >= 16) ? 16 : 4;
  return r;
}

// Fixed-order reduction of the split slabs: a workgroup owns 256/SG consecutive outputs, split group g adds slabs
// g, g+SG, g+2SG, ... in order, and the SG partial sums are combined in LDS in index order -> run-to-run identical.
// swap_kk > 0: the slabs hold R[co'][ci'][tap] of the ROLE-SWAPPED problem (x and dy exchanged); the result is written as
// dW[ci'][co'][KK-1-tap], KK = swap_kk -- the weight gradient of the original convolution (ops.conv_wgrad_swapped3).
template <int SG>
__global__ __launch_bounds__(256) void wgrad3_reduce_kernel(const float* __restrict__ slab, const float* __restrict__ slab_db,
                                                            float* __restrict__ dw, float* __restrict__ db, int Cout, int N,
                                                            int co_pad, int n_pad, int nsplit, int swap_kk) {
  constexpr int OG = 256 / SG;
  __shared__ float part[SG][OG];
  const int o = threadIdx.x % OG, g = threadIdx.x / OG;
  const int64_t i = (int64_t)blockIdx.x * OG + o;
  const int64_t total = (int64_t)Cout * N;
  float s = 0.f;
  if (i < total) {
    const int co = (int)(i / N), n = (int)(i - (int64_t)co * N);
    const float* p = slab + (int64_t)co * n_pad + n;
    const int64_t stride = (int64_t)co_pad * n_pad;
#pragma unroll 4
    for (int k = g; k < nsplit; k += SG) s += p[k * stride];
  } else if (db && i < total + Cout) {
    const int co = (int)(i - total);
#pragma unroll 4
    for (int k = g; k < nsplit; k += SG) s += slab_db[(int64_t)k * co_pad + co];
  }
  part[g][o] = s;
  __syncthreads();
  if (g == 0) {
    float t = part[0][o];
#pragma unroll
    for (int j = 1; j < SG; ++j) t += part[j][o];
    if (i < total) {
      if (swap_kk > 0) {
        const int co = (int)(i / N), n = (int)(i - (int64_t)co * N);
        const int ci = n / swap_kk, tap = n - ci * swap_kk;
        dw[((int64_t)ci * Cout + co) * swap_kk + (swap_kk - 1 - tap)] = t;
      } else {
        dw[i] = t;
      }
    } else if (db && i < total + Cout) {
      db[(int)(i - total)] = t;
    }
  }
}

// Several pending reductions in ONE launch (nq_wgrad_reduce_multi): per segment the arithmetic of wgrad3_reduce_kernel<sg>
// (sg = 4 / 16) or of the sequential fp32 reduction (sg = 1), so results are bit-identical to the single-tensor launches.
// (round 3: a thread owns FOUR consecutive n of one channel -- one 16-byte load per slab instead of four 4-byte ones; the
// launch read 115 MB of slabs at 2.8 TB/s with scalar loads.  Per output the slabs are still added in the order
// j = g, g + SG, ... and the SG partial sums in the order 0 .. SG-1: bit-identical to the scalar form.)
__global__ __launch_bounds__(256) void wgrad_reduce_multi_kernel(NqSegTable<nq_wgr_seg> t) {
  __shared__ float4 part[256];
  int blk;
  const nq_wgr_seg& q = t.s[t.find((int)blockIdx.x, blk)];
  const int SG = q.sg, OG = 256 / SG;
  const int o = threadIdx.x % OG, g = threadIdx.x / OG;
  const int N = q.N, Cout = q.Cout, nsplit = q.nsplit;
  const int NQ = (N + 3) >> 2;                                   // quads per channel (n_pad is a multiple of 16)
  const int64_t i = (int64_t)blk * OG + o;   // quad index, then the bias entries
  const int64_t total = (int64_t)Cout * NQ;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  int co = 0, n = 0;
  if (i < total) {
    co = (int)(i / NQ);
    n = 4 * (int)(i - (int64_t)co * NQ);
    const float* p = q.slab + (int64_t)co * q.n_pad + n;
    const int64_t stride = (int64_t)q.co_pad * q.n_pad;
#pragma unroll 8
    for (int j = g; j < nsplit; j += SG) {
      const float4 v = *reinterpret_cast<const float4*>(p + j * stride);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  } else if (q.db && i < total + Cout) {
    const int cb = (int)(i - total);
#pragma unroll 8
    for (int j = g; j < nsplit; j += SG) s.x += q.slab_db[(int64_t)j * q.co_pad + cb];
  }
  if (SG > 1) {   // block-uniform
    part[g * OG + o] = s;
    __syncthreads();
    if (g != 0) return;
    s = part[o];
    for (int j = 1; j < SG; ++j) {
      const float4 v = part[j * OG + o];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  if (i < total) {
    const float sv[4] = {s.x, s.y, s.z, s.w};
    if (q.swap_kk > 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (n + e >= N) break;
        const int ci = (n + e) / q.swap_kk, tap = (n + e) - ci * q.swap_kk;
        q.dw[((int64_t)ci * Cout + co) * q.swap_kk + (q.swap_kk - 1 - tap)] = sv[e];
      }
    } else if ((N & 3) == 0) {
      *reinterpret_cast<float4*>(q.dw + (int64_t)co * N + n) = s;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (n + e < N) q.dw[(int64_t)co * N + n + e] = sv[e];
    }
  } else if (q.db && i < total + Cout) {
    q.db[(int)(i - total)] = s.x;
  }
}

}  // namespace

extern "C" {

int nq_conv3_supported(int B, int Cin, int H, int W, int Cout, int k) {
  return shape_ok3(B, Cin, H, W, Cout, k) ? route_fwd3(B, Cin, H, W, Cout, k).supported : 0;
}

int64_t nq_conv_forward3_ws_floats(int B, int Cin, int H, int W, int Cout, int k) {
  return shape_ok3(B, Cin, H, W, Cout, k) ? route_fwd3(B, Cin, H, W, Cout, k).ws_floats : 0;
}

int64_t nq_conv3_weight_bytes(int Cin, int Cout, int k) {
  if (!(k == 3 || k == 5)) return 0;
  const int mt = 16 * pick_mi3(Cout);
  return wl3_bytes(Cin, k * k, (Cout + mt - 1) / mt, mt);
}

// w: OIHW weight tensor of the STORED conv (Cout_w, Cin_w, k, k).  transposed = 0 -> operand of the forward conv
// (Cin = Cin_w, Cout = Cout_w); transposed = 1 -> operand of its data gradient (Cin = Cout_w, Cout = Cin_w).
static bool wl3_fill(WL3& p, const float* w, void* wt3, int Cin, int Cout, int k, int transposed) {
  if (!w || !wt3 || !(k == 3 || k == 5) || Cin <= 0 || Cout <= 0) return false;
  const int mi = pick_mi3(Cout);
  p.w = w; p.out = reinterpret_cast<uint4*>(wt3);
  p.Cin = Cin; p.Cout = Cout; p.KK = k * k; p.NST = wl3_steps(p.KK, 0); p.tail = wl3_tail_kind(Cin); p.NSTT = wl3_steps(p.KK, p.tail);
  p.MT = 16 * mi; p.co_tiles = (Cout + p.MT - 1) / p.MT; p.nchunk = (Cin + CC - 1) / CC; p.transposed = transposed;
  p.slots = wl3_plane_slots(Cin, p.KK, p.co_tiles, p.MT);
  p.co16 = (p.co_tiles * p.MT + 15) / 16;
  return true;
}

int nq_weight_layout3(const float* w, void* wt3, int Cin, int Cout, int k, int transposed, nq_stream_t stream) {
  WL3 p;
  if (!wl3_fill(p, w, wt3, Cin, Cout, k, transposed)) return NQ_ERR_INVALID;
  hipLaunchKernelGGL(weight_layout3_kernel, dim3((unsigned)(p.nchunk * p.co16)), dim3(256), 0, nq_s(stream), p);
  return nq_launch_status();
}

// Same byte layout, size and slots; the hi plane as IEEE halves, the lo plane zero (forward operand only: transposed = 0)
int nq_weight_layout3_f16(const float* w, void* wt, int Cin, int Cout, int k, nq_stream_t stream) {
  WL3 p;
  if (!wl3_fill(p, w, wt, Cin, Cout, k, 0)) return NQ_ERR_INVALID;
  hipLaunchKernelGGL(weight_layout3_f16_kernel, dim3((unsigned)(p.nchunk * p.co16)), dim3(256), 0, nq_s(stream), p);
  return nq_launch_status();
}

// table segment of one bf16x3 operand: its workgroups or NQ_ERR_INVALID
static int64_t wl3_seg_fill(const nq_wl3_seg& h, WL3& d) {
  return wl3_fill(d, h.w, h.wt3, h.Cin, h.Cout, h.k, h.transposed) ? d.nchunk * d.co16 : NQ_ERR_INVALID;
}

int nq_weight_layout3_multi(const nq_wl3_seg* segs, int nseg, nq_stream_t stream) {
  return NqSegTable<WL3>::launch_all(
      segs, nseg, [&](int i, WL3& d) { return wl3_seg_fill(segs[i], d); },
      [&](const NqSegTable<WL3>& t, unsigned blocks) {
        hipLaunchKernelGGL(weight_layout3_multi_kernel, dim3(blocks), dim3(256), 0, nq_s(stream), t);
      });
}

int nq_weight_layouts_all(const nq_wl3_seg* segs3, int n3, const nq_wl_seg* segsf, int nf, nq_stream_t stream) {
  if ((n3 > 0 && !segs3) || (nf > 0 && !segsf) || n3 < 0 || nf < 0 || n3 + nf == 0) return NQ_ERR_INVALID;
  // count the fp32 operands (one per direction)
  int nfo = 0;
  for (int i = 0; i < nf; ++i) nfo += (segsf[i].wt_fwd ? 1 : 0) + (segsf[i].wt_bwd ? 1 : 0);
  if (n3 > 16 || nfo > 16 || n3 == 0 || nfo == 0) {   // does not fit one argument block: the two launches
    if (n3 > 0)
      if (int rc = nq_weight_layout3_multi(segs3, n3, stream)) return rc;
    if (nf > 0) return nq_weight_layouts_multi(segsf, nf, stream);
    return NQ_OK;
  }
  WLAll t;
  t.t3.clear();
  t.tf.clear();
  const auto fits = [] {};   // counted above: neither table runs full
  if (int rc = t.t3.fill_all(n3, [&](int i, WL3& d) { return wl3_seg_fill(segs3[i], d); }, fits)) return rc;
  if (int rc = t.tf.fill_all(2 * nf, [&](int i, NqWLSeg& d) { return nq_wl_fill(segsf, i, d); }, fits)) return rc;
  const int64_t blocks = (int64_t)t.t3.blocks() + t.tf.blocks();
  if (blocks > 0x7fffffffLL) return NQ_ERR_INVALID;
  hipLaunchKernelGGL(weight_layouts_all_kernel, dim3((unsigned)blocks), dim3(256), 0, nq_s(stream), t);
  return nq_launch_status();
}

// Which sides of nq_conv_forward3 may travel as split {hi | lo} words for this shape: bit NQ_EPI_X_SPLIT -- the input (the tiled
// kernel with >= 32-channel tiles stages it), bit NQ_EPI_Y_SPLIT -- the output y (the tiled kernel's own epilogue writes it: no
// split-K; the few-pixel kernel when it leaves no slabs).  0 for shapes this path does not serve.
int nq_conv3_split_io(int B, int Cin, int H, int W, int Cout, int k) {
  return shape_ok3(B, Cin, H, W, Cout, k) ? route_fwd3(B, Cin, H, W, Cout, k).split_io : 0;
}

// the route nq_conv_forward3 resolves for the shape, written out; of the tiled kernel also which build of the tile and how much
// LDS its launch takes (the per-kernel-size rules of conv_igemm3_impl.h)
int nq_conv_forward3_plan(int B, int Cin, int H, int W, int Cout, int k, nq_conv3_plan* out) {
  if (!shape_ok3(B, Cin, H, W, Cout, k) || !out) return NQ_ERR_INVALID;
  const Fwd3Route rt = route_fwd3(B, Cin, H, W, Cout, k);
  nq_conv3_plan q{};
  q.supported = rt.supported;
  q.split_io = rt.split_io;
  q.mi = rt.mi;
  q.tail = rt.tail;
  q.nsplit = rt.nsplit; q.per_split = rt.per_split;
  if (rt.flat) {
    q.kernel = NQ_CONV3_FLAT;
    q.flat_nw = rt.fp.nw; q.flat_nb = rt.fp.nb; q.flat_mi = rt.fp.mi;
    q.lds_bytes = q.lds_bytes_dgrad = rt.fp.lds_bytes;
  } else {
    const int nchunk = (Cin + CC - 1) / CC;
    const auto waves = k == 3 ? nq_conv3_waves_k3 : nq_conv3_waves_k5;
    const auto lds = k == 3 ? nq_conv3_lds_k3 : nq_conv3_lds_k5;
    q.kernel = NQ_CONV3_TILED;
    q.waves = waves(rt.mi, nchunk, rt.tail, rt.nsplit, rt.per_split);
    q.lds_bytes = lds(rt.mi, NQ_EPI_PLAIN, rt.nsplit);
    q.lds_bytes_dgrad = lds(rt.mi, NQ_EPI_DGRAD_GELU, rt.nsplit);
  }
  *out = q;
  return NQ_OK;
}

int nq_conv_forward3(const float* x, const void* wt3, const float* bias, float* y, float* z, const float* zprev, float* ws, int B,
                     int Cin, int H, int W, int Cout, int k, int r, int epilogue, nq_stream_t stream) {
  // split {hi | lo} word interchange (include/nq_hip.h: NQ_EPI_X_SPLIT / NQ_EPI_Y_SPLIT): only where nq_conv3_split_io says so
  // (taken off before the epilogue is looked at: NQ_EPI_PS | NQ_EPI_X_SPLIT with y == NULL was refused as invalid)
  const int fmt = epilogue & (NQ_EPI_X_SPLIT | NQ_EPI_Y_SPLIT);
  epilogue &= ~(NQ_EPI_X_SPLIT | NQ_EPI_Y_SPLIT);
  if (!x || !wt3 || (!y && epilogue != NQ_EPI_PS) || B <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0) return NQ_ERR_INVALID;
  if (!(k == 3 || k == 5)) return NQ_ERR_UNSUPPORTED;
  // the one resolution of this call; here, because the split-word check is the next of the argument checks
  const Fwd3Route rt = route_fwd3(B, Cin, H, W, Cout, k);
  if (fmt & ~rt.split_io) return NQ_ERR_UNSUPPORTED;
  if (epilogue < 0 || epilogue > NQ_EPI_DGRAD_GELU) return NQ_ERR_INVALID;
  if ((epilogue == NQ_EPI_PS_GELU || epilogue == NQ_EPI_PS) && (!z || r <= 0 || Cout % (r * r) != 0)) return NQ_ERR_INVALID;
  if (epilogue == NQ_EPI_DGRAD_GELU && (!zprev || r <= 0 || H % r != 0 || W % r != 0)) return NQ_ERR_INVALID;
  if (B > 65535) return NQ_ERR_UNSUPPORTED;
  hipStream_t st = nq_s(stream);
  if (rt.nsplit > 1 && !ws) return NQ_ERR_INVALID;
  int rc;
  if (rt.flat)   // few-pixel layers: pixels of all frames as one flat GEMM dimension, waves split the K loop (conv_flat3.hip)
    rc = nq_conv_flat3(x, wt3, bias, y, z, zprev, ws, B, Cin, H, W, Cout, k, r, epilogue | fmt, 16 * rt.mi, &rt.fp, st);
  else
    rc = (k == 3 ? nq_conv_igemm3_k3 : nq_conv_igemm3_k5)(x, wt3, bias, y, z, zprev, B, Cin, H, W, Cout, r, epilogue | fmt, rt.mi,
                                                          rt.nsplit, rt.per_split, ws, st);
  if (rc != NQ_OK || rt.nsplit == 1) return rc;
  return nq_conv_splitk_finish(ws, bias, y, z, zprev, B, H, W, Cout, r, epilogue, rt.nsplit, st);
}

// Levels build of the tiled forward (conv_igemm3_impl.h, template parameter WX): offered exactly where the one resolution of the
// shape gives the UNSPLIT tiled kernel to a shape this path serves -- the few-pixel and the split-K kernels have no such build.
static inline bool levels_route_ok(const Fwd3Route& rt) { return !rt.flat && rt.supported && rt.nsplit == 1; }

int nq_conv3_levels_supported(int B, int Cin, int H, int W, int Cout, int k) {
  return shape_ok3(B, Cin, H, W, Cout, k) && levels_route_ok(route_fwd3(B, Cin, H, W, Cout, k)) ? 1 : 0;
}

// the argument checks of both levels launches, made before any device call: NQ_OK and the route, or the code to return
static int levels_args(const float* x, const void* wt, const float* scale, float* y, float* z, int B, int Cin, int H, int W, int Cout,
                       int k, int r, int& epilogue, Fwd3Route& rt) {
  const int fmt = epilogue & (NQ_EPI_X_SPLIT | NQ_EPI_Y_SPLIT);
  epilogue &= ~(NQ_EPI_X_SPLIT | NQ_EPI_Y_SPLIT);
  if (!x || !wt || !scale || (!y && epilogue != NQ_EPI_PS) || B <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0) return NQ_ERR_INVALID;
  if (epilogue < 0 || epilogue >= NQ_EPI_DGRAD_GELU) return NQ_ERR_INVALID;   // forward epilogues only
  if ((epilogue == NQ_EPI_PS_GELU || epilogue == NQ_EPI_PS) && (!z || r <= 0 || Cout % (r * r) != 0)) return NQ_ERR_INVALID;
  if (!(k == 3 || k == 5)) return NQ_ERR_UNSUPPORTED;
  if (fmt) return NQ_ERR_UNSUPPORTED;        // floats in, floats out: the player passes no split words
  if (B > 65535) return NQ_ERR_UNSUPPORTED;
  // the one resolution of this call: the same the plan query and nq_conv3_levels_supported read
  rt = route_fwd3(B, Cin, H, W, Cout, k);
  return levels_route_ok(rt) ? NQ_OK : NQ_ERR_UNSUPPORTED;
}

// Both public entries: f16 selects the half build (template parameter XH), which takes the same checks and the same shapes
// (nq_conv3_levels_supported) and, in front of them, asks for its flag word
static int forward3_levels(bool f16, const float* x, const void* wt, const float* scale, const float* bias, float* y, float* z,
                           unsigned* sat_flag, int B, int Cin, int H, int W, int Cout, int k, int r, int epilogue, nq_stream_t stream) {
  static nq_igemm3_levels_fn* const entry[2][2] = {{nq_conv_igemm3l_k3, nq_conv_igemm3l_k5}, {nq_conv_igemm3h_k3, nq_conv_igemm3h_k5}};
  if (f16 && !sat_flag) return NQ_ERR_INVALID;
  Fwd3Route rt;
  if (int rc = levels_args(x, wt, scale, y, z, B, Cin, H, W, Cout, k, r, epilogue, rt)) return rc;
  return entry[f16][k == 5](x, wt, scale, bias, y, z, sat_flag, B, Cin, H, W, Cout, r, epilogue, rt.mi, nq_s(stream));
}

int nq_conv_forward3_levels(const float* x, const void* wt, const float* scale, const float* bias, float* y, float* z, int B, int Cin,
                            int H, int W, int Cout, int k, int r, int epilogue, nq_stream_t stream) {
  return forward3_levels(false, x, wt, scale, bias, y, z, nullptr, B, Cin, H, W, Cout, k, r, epilogue, stream);
}

int nq_conv_forward3_levels_f16(const float* x, const void* wt, const float* scale, const float* bias, float* y, float* z,
                                unsigned* sat_flag, int B, int Cin, int H, int W, int Cout, int k, int r, int epilogue,
                                nq_stream_t stream) {
  return forward3_levels(true, x, wt, scale, bias, y, z, sat_flag, B, Cin, H, W, Cout, k, r, epilogue, stream);
}

int nq_conv_wgrad3_supported(int B, int Cin, int H, int W, int Cout, int k) {
  return shape_ok3(B, Cin, H, W, Cout, k) ? route_wgrad3(B, Cin, H, W, Cout, k).supported : 0;
}

int nq_conv_wgrad3_plan(int B, int Cin, int H, int W, int Cout, int k, int* mi, int* ni, int* nsplit, int* pc) {
  if (!shape_ok3(B, Cin, H, W, Cout, k) || !mi || !ni || !nsplit || !pc) return NQ_ERR_INVALID;
  const Wg3Plan p = route_wgrad3(B, Cin, H, W, Cout, k).p;
  *mi = p.mi; *ni = p.ni; *nsplit = p.nsplit; *pc = p.pc;
  return NQ_OK;
}

int64_t nq_conv_wgrad3_ws_floats(int B, int Cin, int H, int W, int Cout, int k) {
  return shape_ok3(B, Cin, H, W, Cout, k) ? route_wgrad3(B, Cin, H, W, Cout, k).ws_floats : 0;
}

static int conv_wgrad3_impl(const float* x, const float* dy, float* dw, float* db, float* ws, int B, int Cin, int H, int W,
                            int Cout, int k, int swap_kk, nq_wgr_seg* seg, nq_stream_t stream, int fmt);

// Operands as split {hi | lo} words (include/nq_hip.h): fmt bit 0 -- x, bit 1 -- dy; where nq_conv_wgrad3_split_io says so
int nq_conv_wgrad3_split_io(int B, int Cin, int H, int W, int Cout, int k) {
  return shape_ok3(B, Cin, H, W, Cout, k) ? route_wgrad3(B, Cin, H, W, Cout, k).split_io : 0;
}

// seg == NULL: split kernel + reduction; seg != NULL: the split kernel only, *seg describes the pending reduction
int nq_conv_wgrad3(const float* x, const float* dy, float* dw, float* db, float* ws, int B, int Cin, int H, int W, int Cout,
                   int k, int fmt, nq_wgr_seg* seg, nq_stream_t stream) {
  return conv_wgrad3_impl(x, dy, dw, db, ws, B, Cin, H, W, Cout, k, 0, seg, stream, fmt);
}

// Role-swapped form, arguments of the ORIGINAL layer: 0 where the few-pixel kernel owns the exchanged shape (it has no
// transposing store, so nq_conv_wgrad3_swapped refuses it), else the slab size of the exchanged problem's plan
int64_t nq_conv_wgrad3_swapped_ws_floats(int B, int Cin, int H, int W, int Cout, int k) {
  if (!shape_ok3(B, Cin, H, W, Cout, k)) return 0;
  const Wg3Route rt = route_wgrad3(B, Cout, H, W, Cin, k);
  return rt.flat ? 0 : rt.ws_floats;
}

// where callers should route a weight gradient to the role-swapped form (narrower than what the launch accepts)
int nq_conv_wgrad3_swapped_supported(int B, int Cin, int H, int W, int Cout, int k) {
  if (!shape_ok3(B, Cin, H, W, Cout, k) || !(Cout <= 4 && Cin > 4 && Cout * k * k <= 64)) return 0;
  const Wg3Route rt = route_wgrad3(B, Cout, H, W, Cin, k);
  return rt.supported && !rt.flat;   // (a tiled plan always has slabs: its workspace is never 0)
}

int nq_conv_wgrad3_swapped(const float* x, const float* dy, float* dw, float* ws, int B, int Cin, int H, int W, int Cout, int k,
                           nq_wgr_seg* seg, nq_stream_t stream) {
  // the kernel sees the exchanged problem: "x" = dy (Cout channels), "dy" = x (Cin channels)
  return conv_wgrad3_impl(dy, x, dw, nullptr, ws, B, Cout, H, W, Cin, k, k * k, seg, stream, 0);
}

int nq_wgrad_reduce_multi(const nq_wgr_seg* segs, int nseg, nq_stream_t stream) {
  if (segs && nseg == 0) return nq_launch_status();   // an empty list is no error here
  return NqSegTable<nq_wgr_seg>::launch_all(
      segs, nseg,
      [&](int i, nq_wgr_seg& d) -> int64_t {
        const nq_wgr_seg& h = segs[i];
        if (h.nsplit == 0) return 0;   // nothing pending (the kernel wrote dw itself)
        if (!h.slab || !h.dw || h.Cout <= 0 || h.N <= 0 || h.nsplit < 0 || !(h.sg == 1 || h.sg == 4 || h.sg == 16) ||
            (h.db && !h.slab_db))
          return NQ_ERR_INVALID;
        d = h;
        const int og = 256 / h.sg;
        return ((int64_t)h.Cout * ((h.N + 3) / 4) + h.Cout + og - 1) / og;   // quads of n, then the bias entries
      },
      [&](const NqSegTable<nq_wgr_seg>& t, unsigned blocks) {
        hipLaunchKernelGGL(wgrad_reduce_multi_kernel, dim3(blocks), dim3(256), 0, nq_s(stream), t);
      });
}

static int conv_wgrad3_impl(const float* x, const float* dy, float* dw, float* db, float* ws, int B, int Cin, int H, int W,
                            int Cout, int k, int swap_kk, nq_wgr_seg* seg, nq_stream_t stream, int fmt) {
  // the one resolution of this call (a shape that fails the checks below has no route: no split words either)
  const Wg3Route rt = shape_ok3(B, Cin, H, W, Cout, k) ? route_wgrad3(B, Cin, H, W, Cout, k) : Wg3Route{};
  if (fmt & ~rt.split_io) return NQ_ERR_UNSUPPORTED;
  if (!x || !dy || !dw || !ws || B <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0) return NQ_ERR_INVALID;
  if (!(k == 3 || k == 5)) return NQ_ERR_UNSUPPORTED;
  if ((int64_t)Cout * H * W >= (1ll << 31) || (int64_t)Cin * H * W >= (1ll << 31)) return NQ_ERR_UNSUPPORTED;
  if (rt.flat) {
    // Role-swapped entry (here Cin / Cout are those of the EXCHANGED problem): the few-pixel kernel has no transposing
    // store and no slabs (nq_conv_wgrad3_swapped_ws_floats answers 0).  Refused.
    if (swap_kk != 0) return NQ_ERR_UNSUPPORTED;
    // few-pixel layer: every output block is owned by one wave for the whole K range -- dw / db are final, nothing pending
    if (seg) *seg = nq_wgr_seg{nullptr, nullptr, dw, db, Cout, Cin * k * k, 0, 0, 0, 0, 1};
    return nq_conv_wgrad_flat3(x, dy, dw, db, B, Cin, H, W, Cout, k, nq_s(stream));
  }
  const Wg3Plan& p = rt.p;
  float* slab = ws;
  float* slab_db = ws + (int64_t)p.nsplit * p.co_pad * p.n_pad;
  hipStream_t st = nq_s(stream);
  int rc = (k == 3) ? nq_conv_wgrad3_k3(x, dy, slab, slab_db, B, Cin, H, W, Cout, p.co_pad, p.n_pad, p.nsplit, p.mi, p.ni, p.pc, fmt, st)
                    : nq_conv_wgrad3_k5(x, dy, slab, slab_db, B, Cin, H, W, Cout, p.co_pad, p.n_pad, p.nsplit, p.mi, p.ni, p.pc, fmt, st);
  if (rc != NQ_OK) return rc;
  const int N = Cin * k * k;
  int64_t total = (int64_t)Cout * N + Cout;
  if (seg) {   // deferred: describe the reduction, nq_wgrad_reduce_multi runs it (same split groups as below)
    *seg = nq_wgr_seg{slab, db ? slab_db : nullptr, dw, db, Cout, N, p.co_pad, p.n_pad, p.nsplit, swap_kk, rt.sg};
    return NQ_OK;
  }
  if (rt.sg == 16) {
    hipLaunchKernelGGL(wgrad3_reduce_kernel<16>, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, st, slab, slab_db, dw, db,
                       Cout, N, p.co_pad, p.n_pad, p.nsplit, swap_kk);
  } else {
    hipLaunchKernelGGL(wgrad3_reduce_kernel<4>, dim3((unsigned)((total + 63) / 64)), dim3(256), 0, st, slab, slab_db, dw, db,
                       Cout, N, p.co_pad, p.n_pad, p.nsplit, swap_kk);
  }
  return nq_launch_status();
}

}  // extern "C"

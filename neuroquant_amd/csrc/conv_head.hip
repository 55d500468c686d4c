// Vector (VALU) kernels for the decoder's head convolution: C_in -> C_out <= 4 channels, 3x3 or 5x5 or 1x1, over the
// full-resolution image (HNeRV/NeRV head_layer: 37|24 -> 3, k=3, 640x1280; reference models/HNeRV.py:42, :63-64).
//
// With 3 output channels a GEMM tile is >80 % padding, and the op is HBM-bound anyway (arithmetic intensity
// 2*3*9 = 54 flop per 4-byte input element, ~13 flop/B << the 19.7 flop/B fp32 ridge): forward and data gradient
// each read or write the 242 MB activation tensor once.  So these are streaming kernels:
//   head_fwd   : thread = 4 consecutive pixels, input patch staged in LDS per 4-channel chunk, weights via
//                scalar loads, fused bias + tanh*0.5+0.5 (OutImg, models/_layers.py:10-16)
//   head_dgrad : thread = 4 pixels, the C_out x k x (4+k-1) neighbourhood of dY lives in registers, loop over C_in,
//                fused multiply by the saved gelu'(z) and PixelUnshuffle store (same contract as NQ_EPI_DGRAD_GELU)
// (The weight gradient of the head stays on the MFMA split-K kernel of conv_wgrad_impl.h: a VALU variant with one
//  thread per (ci,kh,kw) was measured slower, 0.66-0.80 ms vs 0.56 ms.)
// Roofline: HBM (8 TB/s spec / 6.3 TB/s achievable); algorithmic bytes = 4*B*H*W*(C_in + C_out) per launch
// (+ the same again for z in head_dgrad).
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "nq_common.h"

namespace {

constexpr int MAXCO = 4;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

template <int I0, int N, class F>
__device__ __forceinline__ void hf2_rows(F&& f) {
  if constexpr (I0 < N) {
    f(std::integral_constant<int, I0>{});
    hf2_rows<I0 + 1, N>(f);
  }
}

// ------------------------------------------------------------------------------------------------ forward
template <int KS>
__global__ __launch_bounds__(256) void head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wt, int ld,
                                                       const float* __restrict__ bias, float* __restrict__ y, int Cin,
                                                       int H, int W, int CO, int epi, int tiles_x) {
  constexpr int KK = KS * KS, PAD = KS / 2;
#ifndef NQ_HEAD_CCH
#define NQ_HEAD_CCH 4
#endif
  constexpr int TH = 16, TW = 64, CCH = NQ_HEAD_CCH;
  constexpr int PH = TH + KS - 1;
  // LDS rows: [OFF-PAD, OFF) left halo | [OFF, OFF+64) interior (16-byte aligned) | [OFF+64, OFF+64+PAD) right halo.
  // The interior is staged with 16-byte global loads / ds_write_b128 (4.5 per thread per chunk instead of 18 scalar
  // loads: the kernel is bound by the number of memory instructions), only the 2*PAD halo columns are scalar.
  constexpr int OFF = 4, PWS = 72;
  constexpr int NQUAD = CCH * PH * (TW / 4), NHALO = CCH * PH * 2 * PAD;
  __shared__ __attribute__((aligned(16))) float patch[CCH * PH * PWS];

  const int tid = threadIdx.x;
  const int row = tid >> 4, c4 = (tid & 15) * 4;
  // 1-D grid over (image, tile), XCD-chunked (nq_xcd_chunk): neighbouring tiles share halo rows / lines behind one L2
  const int lid = nq_xcd_chunk((int)blockIdx.x, (int)gridDim.x);
  const int tiles = tiles_x * ((H + TH - 1) / TH), tile = lid % tiles;
  const int tile_x = tile % tiles_x, tile_y = tile / tiles_x;
  const int x0 = tile_x * TW, y0 = tile_y * TH, b = lid / tiles;
  const int64_t HW = (int64_t)H * W;
  const float* __restrict__ xb = x + (int64_t)b * Cin * HW;
  const bool w4 = (W & 3) == 0;

  f32x2 acc2[MAXCO][2];
#pragma unroll
  for (int co = 0; co < MAXCO; ++co) acc2[co][0] = acc2[co][1] = f32x2{0.f, 0.f};

  for (int c0 = 0; c0 < Cin; c0 += CCH) {
    __syncthreads();
    for (int e = tid; e < NQUAD; e += 256) {
      const int ci = e / (PH * (TW / 4)), rem = e - ci * (PH * (TW / 4));
      const int r = rem / (TW / 4), q = rem - r * (TW / 4);
      const int gy = y0 - PAD + r, gx = x0 + 4 * q, cig = c0 + ci;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (cig < Cin && gy >= 0 && gy < H && gx < W) {
        const float* p = xb + (int64_t)cig * HW + (int64_t)gy * W + gx;
        if (w4) {
          v = *reinterpret_cast<const float4*>(p);
        } else {
          v.x = p[0];
          if (gx + 1 < W) v.y = p[1];
          if (gx + 2 < W) v.z = p[2];
          if (gx + 3 < W) v.w = p[3];
        }
      }
      *reinterpret_cast<float4*>(patch + (ci * PH + r) * PWS + OFF + 4 * q) = v;
    }
    if constexpr (PAD > 0) {
      for (int e = tid; e < NHALO; e += 256) {
        const int ci = e / (PH * 2 * PAD), rem = e - ci * (PH * 2 * PAD);
        const int r = rem / (2 * PAD), h = rem - r * (2 * PAD);
        const int c = (h < PAD) ? h - PAD : TW + (h - PAD);   // column relative to x0: [-PAD, 0) or [TW, TW+PAD)
        const int gy = y0 - PAD + r, gx = x0 + c, cig = c0 + ci;
        float v = 0.f;
        if (cig < Cin && gy >= 0 && gy < H && gx >= 0 && gx < W) v = xb[(int64_t)cig * HW + (int64_t)gy * W + gx];
        patch[(ci * PH + r) * PWS + OFF + c] = v;
      }
    }
    __syncthreads();
    const int cmax = min(CCH, Cin - c0);
    for (int ci = 0; ci < cmax; ++ci) {
      const float* __restrict__ wc = wt + (int64_t)(c0 + ci) * KK * ld;  // wt[(ci*KK + tap)*ld + co]
#pragma unroll
      for (int kh = 0; kh < KS; ++kh) {
        float in[4 + KS - 1];
        const float* pr = patch + (ci * PH + row + kh) * PWS + (OFF - PAD) + c4;
#pragma unroll
        for (int j = 0; j < 4 + KS - 1; ++j) in[j] = pr[j];
#pragma unroll
        for (int co = 0; co < MAXCO; ++co) {
          if (co < CO) {
#pragma unroll
            for (int kw = 0; kw < KS; ++kw) {
              const float wv = wc[(kh * KS + kw) * ld + co];  // wave-uniform -> scalar load
              // two pixels per instruction (v_pk_fma_f32: the fp32 vector peak assumes packed math); per element the
              // same fused multiply-add as fmaf
              const f32x2 w2 = {wv, wv};
              acc2[co][0] = __builtin_elementwise_fma(w2, f32x2{in[kw], in[kw + 1]}, acc2[co][0]);
              acc2[co][1] = __builtin_elementwise_fma(w2, f32x2{in[kw + 2], in[kw + 3]}, acc2[co][1]);
            }
          }
        }
      }
    }
  }
  const int gy = y0 + row;
  if (gy >= H) return;
#pragma unroll
  for (int co = 0; co < MAXCO; ++co) {
    if (co >= CO) break;
    const float bv = bias ? bias[co] : 0.f;
    float* __restrict__ yo = y + ((int64_t)b * CO + co) * HW + (int64_t)gy * W + x0 + c4;
    float o[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const float v = acc2[co][p >> 1][p & 1] + bv;
      o[p] = (epi == NQ_EPI_TANH) ? tanhf(v) * 0.5f + 0.5f : v;
    }
    if (w4 && x0 + c4 + 3 < W) {
      *reinterpret_cast<float4*>(yo) = make_float4(o[0], o[1], o[2], o[3]);   // one 16-byte store per channel
    } else {
#pragma unroll
      for (int p = 0; p < 4; ++p)
        if (x0 + c4 + p < W) yo[p] = o[p];
    }
  }
}

// ------------------------------------------------------------------------------------------------ forward, streaming
// Round 3.  The LDS-staged kernel above runs at 2.3-2.5 TB/s (wait_any 0.64: 4-channel staging rounds between two
// barriers, nothing in flight while a workgroup computes).  This one has no barrier in its loop: a WAVE owns a strip of
// 256 columns x R output rows and walks the input channels ONCE; per channel it loads the R + 2 input rows (one 16-byte
// load per lane and row: 1 KiB per wave-instruction, bounds-checked buffer loads at per-row offsets computed once per
// wave -- rows / columns outside the image read as zero, no branch, no address arithmetic in the loop) one channel ahead
// into the other register set, and keeps the R x CO x 4 partial sums of all its output rows in registers, so every
// activation is fetched once per R + 2 rows (R = 5: 1.4 x the tensor through L2; the halo rows are shared with the row
// blocks above / below, which the XCD-chunked order runs behind the same L2).  The horizontal halo comes from the
// neighbouring lanes by DPP wave shifts whose "old" operand is the one dword per row that lane 0 / lane 63 fetch from
// outside the strip.  The weights are wave-uniform: 9 scalar 16-byte loads {co0..co3} per channel, one channel ahead,
// used as the SGPR operand of v_pk_fma_f32.  A first version (input rows outermost, three accumulator rows, a load queue) was
// bound by instruction ISSUE at ~1.25 waves per SIMD: 66 bookkeeping instructions per 54 v_pk_fma; this order has ~13.
// Per output the fp32 fused multiply-adds run in (ci, kh, kw) order, as in head_fwd_kernel.
// cache-hot-first wave order of head_fwd2_kernel (see there): needs 8 whole bands of row blocks and whole workgroups per XCD
// chunk; NQ_HEAD_HOT=0 restores the top-down order (A/B runs)
static inline int head_hot_first(int B, int strips, int rblocks) {
  static const int on = [] { const char* e = getenv("NQ_HEAD_HOT"); return e ? atoi(e) : 1; }();
  return (on && B >= 1 && B <= 8 && 8 % B == 0 && rblocks % (8 / B) == 0 && (B * strips * rblocks) % 32 == 0) ? 1 : 0;
}
struct HeadFwd2Args {
  int B, Cin, H, W, ld, strips, rblocks;
  unsigned x_bytes;
  int hot_first;
};
// Round 4: the loss tail fused behind the head (LOSS = true).  The wave that owns a strip of the image has every output pixel of
// it in registers: lp_loss (quantizer.py:66-71), the tanh backward of OutImg (_layers.py:10-16) and the head's bias gradient
// are computed there -- the arithmetic of l2_tanh_head_stage1 per element -- and the image is still written (evaluation and
// the autograd node keep their tensor).  Per wave: {sum (p-t)^2, sum dconv[c0], [c1], [c2]} -> ws[4*wave id ..]; head_loss_stage2
// adds them in wave-id order (deterministic; another summation order than l2_tanh_head_stage1's 4096-element chunks).
struct HeadLossArgs {
  const float* tgt;          // float target (B,3,H,W) ...
  const uint8_t* cache;      // ... or the uint8 frame cache (N,3,H,W) with
  const int64_t* idx;        //     the batch's frame indices
  float* dconv;              // gradient at the head conv's output (B,3,H,W)
  float* ws;                 // 4 floats per wave
  float gcoef;               // 2 / (B*H*W) * gscale
};

// (the pointers are kernel PARAMETERS with __restrict__: the compiler then knows that the stores to y cannot change x / wt)
// wt[(ci*9 + tap)*ld + co], zero for co >= CO (nq_weight_layouts)
template <int R, int NCO, bool TANH, bool LOSS = false>
__global__ __launch_bounds__(256) void head_fwd2_kernel(const float* __restrict__ x_, const float* __restrict__ wt,
                                                        const float* __restrict__ bias, float* __restrict__ y_,
                                                        HeadFwd2Args a, HeadLossArgs la = HeadLossArgs{}) {
  constexpr int KS = 3, KK = 9, NR = R + 2;
  constexpr unsigned OOB = 0xFFFFFF00u;
  // (the wave index through readfirstlane: everything derived from it -- frame, strip, row block, the scalar offsets of the
  // loads -- is then wave-uniform for the compiler too; as a function of threadIdx it put every load into a waterfall loop)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int total = a.B * a.strips * a.rblocks;
  const int wid = nq_xcd_chunk((int)blockIdx.x, (int)gridDim.x) * 4 + wave;
  if (wid >= total) return;   // whole wave
  int by = wid % a.rblocks, t0 = wid / a.rblocks;
  int sx = t0 % a.strips, b = t0 / a.strips;
  if (a.hot_first) {
    // Round 4: the producer (the last block's forward convolution, XCD-chunked) wrote this tensor as 8 row bands, one per XCD,
    // each from its top row down, so the END of every band is what the 256 MB memory-side cache still holds when this kernel
    // starts.  XCD k walks band k from its last rows upwards (strips fastest) instead of top-down: the same waves on the same
    // operands (identical results), 85 -> 78 us inside an HNeRV-3M iteration, 65 -> 60 us for NeRV-3M (same-box A/B, twice).
    const int q = total >> 3, k = wid / q, i = wid - k * q;
    const int bands = 8 / a.B, rows_per_band = a.rblocks / bands;
    b = k / bands;
    by = (k - b * bands) * rows_per_band + (rows_per_band - 1 - i / a.strips);
    sx = i % a.strips;
  }
  const int H = a.H, W = a.W, Cin = a.Cin;
  const int y0 = by * R, x0 = sx * 256, gx = x0 + 4 * lane;
  const unsigned HWb = (unsigned)H * (unsigned)W * 4u, Wb = (unsigned)W * 4u;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x_), 0, (int)a.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_y = __builtin_amdgcn_make_buffer_rsrc(y_, 0, (int)((unsigned)a.B * NCO * HWb), 0x00020000);
  // per-lane byte offsets of the quad and of the one pixel outside the strip (lane 0: left, lane 63: right) in each of the
  // NR input rows, relative to (frame b, channel 0); out-of-range where the row / column does not exist
  const int ex = (lane == 0) ? x0 - 1 : x0 + 256;
  const bool e_ok = (lane == 0 || lane == 63) && ex >= 0 && ex < W;
  unsigned oq[NR], oe[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int iy = y0 - 1 + r;
    const bool rok = iy >= 0 && iy < H;
    oq[r] = (rok && gx < W) ? (unsigned)iy * Wb + (unsigned)gx * 4u : OOB;
    oe[r] = (rok && e_ok) ? (unsigned)iy * Wb + (unsigned)ex * 4u : OOB;
  }
  const unsigned base_b = (unsigned)b * (unsigned)Cin * HWb;

  auto load_x = [&](int ci, f32x4 (&v)[NR], float (&e)[NR]) {
    const unsigned so = base_b + (unsigned)min(ci, Cin - 1) * HWb;   // scalar offset of the channel (past the end: the last again)
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      v[r] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, oq[r], so, 0));
      e[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, oe[r], so, 0));
    }
  };
  // the 9 x {co0..co3} weights of a channel: wave-uniform 16-byte loads = scalar loads into SGPRs (v_pk_fma_f32 takes the
  // pair as its scalar operand: no vector registers, no LDS)
  const int ld = a.ld;
  auto load_w = [&](int ci, float4 (&w)[KK]) {
    const float* __restrict__ wr = wt + (int64_t)min(ci, Cin - 1) * KK * ld;
#pragma unroll
    for (int t = 0; t < KK; ++t) w[t] = *reinterpret_cast<const float4*>(wr + t * ld);
  };

  f32x2 acc[R][NCO][2];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int co = 0; co < NCO; ++co) acc[r][co][0] = acc[r][co][1] = f32x2{0.f, 0.f};

  auto compute = [&](const f32x4 (&v)[NR], const float (&e)[NR], const float4 (&w)[KK]) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {   // input row y0 - 1 + r feeds output rows r - kh, kh = 0..2
      // halo pixels from the neighbouring lanes; lane 0 / lane 63 have no neighbour and keep `old` = the edge dword.
      // (NB: __builtin_bit_cast applied DIRECTLY to a vector element, `__builtin_bit_cast(int, v[3])`, reads element 0 with
      // hipcc 7.2 -- checked on a four-line kernel; the elements go through named floats first)
      const float v3f = v[r][3], v0f = v[r][0], ef = e[r];
      const int ei = __builtin_bit_cast(int, ef);
      const float lf = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(ei, __builtin_bit_cast(int, v3f), 0x138, 0xF, 0xF, false));
      const float rt = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(ei, __builtin_bit_cast(int, v0f), 0x130, 0xF, 0xF, false));
      const float in[6] = {lf, v[r][0], v[r][1], v[r][2], v[r][3], rt};
#pragma unroll
      for (int kh = 0; kh < KS; ++kh) {
        const int rel = r - kh;               // output row relative to y0
        if (rel < 0 || rel >= R) continue;    // compile-time after unrolling
#pragma unroll
        for (int kw = 0; kw < KS; ++kw) {
#pragma unroll
          for (int co = 0; co < NCO; ++co) {
            const float4 w4 = w[kh * KS + kw];
            const float wv = co == 0 ? w4.x : (co == 1 ? w4.y : (co == 2 ? w4.z : w4.w));
            const f32x2 w2 = {wv, wv};
            acc[rel][co][0] = __builtin_elementwise_fma(w2, f32x2{in[kw], in[kw + 1]}, acc[rel][co][0]);
            acc[rel][co][1] = __builtin_elementwise_fma(w2, f32x2{in[kw + 2], in[kw + 3]}, acc[rel][co][1]);
          }
        }
      }
    }
  };

  // two register sets: while channel ci is consumed from one, the loads of channel ci + 1 (14 per wave: 7 KiB) fill the
  // other; same for the weights in SGPRs.  Scalar loads return out of order, so a wait for them is always "all of them":
  // it is placed at the END of each compute block, where the next channel's weights (requested a whole block earlier) have
  // long arrived, instead of in front of the first use, where it would also wait for the requests just issued.
  f32x4 vA[NR], vB[NR];
  float eA[NR], eB[NR];
  float4 wA[KK], wB[KK];
  load_x(0, vA, eA);
  load_w(0, wA);
#pragma unroll 1
  for (int ci = 0; ci + 1 < Cin; ci += 2) {
    load_x(ci + 1, vB, eB);
    load_w(ci + 1, wB);
    __builtin_amdgcn_sched_barrier(0);   // the prefetch is issued HERE, not sunk towards its uses one channel later
    compute(vA, eA, wA);
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
    __builtin_amdgcn_sched_barrier(0);
    load_x(ci + 2, vA, eA);              // (past the last channel: the last one again, not used)
    load_w(ci + 2, wA);
    __builtin_amdgcn_sched_barrier(0);
    compute(vB, eB, wB);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_sched_barrier(0);
  }
  if (Cin & 1) compute(vA, eA, wA);      // set A holds the last channel

  float bv[NCO];
#pragma unroll
  for (int co = 0; co < NCO; ++co) bv[co] = bias ? bias[co] : 0.f;
  float lsum = 0.f, gsum[NCO];
#pragma unroll
  for (int co = 0; co < NCO; ++co) gsum[co] = 0.f;
  __amdgpu_buffer_rsrc_t rs_d = rs_y;
  int64_t tbase = 0;   // element offset of (frame, channel 0) in the target
  if constexpr (LOSS) {
    rs_d = __builtin_amdgcn_make_buffer_rsrc(la.dconv, 0, (int)((unsigned)a.B * NCO * HWb), 0x00020000);
    tbase = (la.cache ? la.idx[b] : (int64_t)b) * NCO * (int64_t)H * W;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int oy = y0 + r;
    const bool in = oy < H && gx < W;   // (W % 4 == 0: a quad is inside or outside as a whole)
    // bounds-checked buffer stores (an out-of-range offset for rows / columns outside the image): no branch
    const unsigned so = in ? ((unsigned)b * NCO * (unsigned)H + (unsigned)oy) * Wb + (unsigned)gx * 4u : OOB;
#pragma unroll
    for (int co = 0; co < NCO; ++co) {
      f32x4 o;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const float v = acc[r][co][p >> 1][p & 1] + bv[co];
        o[p] = TANH ? tanhf(v) * 0.5f + 0.5f : v;
      }
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, o), rs_y,
                                             so == OOB ? OOB : so + (unsigned)co * HWb, 0, 0);
      if constexpr (LOSS) {
        f32x4 t4 = {0.f, 0.f, 0.f, 0.f};
        if (in) {
          const int64_t te = tbase + ((int64_t)co * H + oy) * W + gx;
          if (la.cache) {
            const uchar4 u = *reinterpret_cast<const uchar4*>(la.cache + te);   // gx % 4 == 0: aligned
            t4 = f32x4{(float)u.x / 255.f, (float)u.y / 255.f, (float)u.z / 255.f, (float)u.w / 255.f};
          } else {
            t4 = *reinterpret_cast<const f32x4*>(la.tgt + te);
          }
        }
        f32x4 dc;
#pragma unroll
        for (int p = 0; p < 4; ++p) {   // l2_tanh_head_stage1, element by element
          const float d = o[p] - t4[p];
          const float g = la.gcoef * d;
          const float u = 2.f * o[p] - 1.f;
          const float rr = g * 0.5f * (1.f - u * u);
          dc[p] = rr;
          if (in) {
            lsum += d * d;
            gsum[co] += rr;
          }
        }
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, dc), rs_d,
                                               so == OOB ? OOB : so + (unsigned)co * HWb, 0, 0);
      }
    }
  }
  if constexpr (LOSS) {
    lsum = nq_wave_sum(lsum);
#pragma unroll
    for (int co = 0; co < NCO; ++co) gsum[co] = nq_wave_sum(gsum[co]);
    if (lane == 0) {
      float* w4 = la.ws + (int64_t)wid * 4;
      w4[0] = lsum;
#pragma unroll
      for (int co = 0; co < NCO && co < 3; ++co) w4[1 + co] = gsum[co];
    }
  }
}

// block 0: loss = scale * sum over waves; block 1 + c: db[c] -- fixed order (thread-strided partial sums, then the block sum)
__global__ __launch_bounds__(256) void head_loss_stage2(const float* __restrict__ ws, int waves, float scale,
                                                        float* __restrict__ loss, float* __restrict__ db) {
  __shared__ float red[16];
  float acc = 0.f;
  for (int i = threadIdx.x; i < waves; i += 256) acc += ws[(int64_t)i * 4 + blockIdx.x];
  const float s = nq_block_sum(acc, red);
  if (threadIdx.x == 0) {
    if (blockIdx.x == 0) loss[0] = 0.f + s * scale;
    else db[blockIdx.x - 1] = s;
  }
}

// ------------------------------------------------------------------------------------------------ data gradient
// R2 = 1: r == 2 with W % 4 == 0 and H % 2 == 0 checked by the host -> only the 8-byte un-shuffle stores are compiled
// (the generic path's 64-bit per-element addressing otherwise sets the kernel's VGPR count and halves the occupancy).
template <int KS, int R2, int NCO, int PX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((KS <= 3 && NCO <= 3 && R2 && PX == 4) ? 4 : 1, 8))) void head_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ wt, int ld,
                                                         const float* __restrict__ zprev, float* __restrict__ out,
                                                         int Cin, int H, int W, int CO, int r, int tiles_x) {
  // NB naming follows the data-gradient use: "CO" (<= 4) = channels of the INPUT dy, "Cin" = channels of the OUTPUT;
  // wt[(co*KK + tap)*ld + ci] is the (already tap-flipped) wt_bwd operand of nq_weight_layouts.
  constexpr int KK = KS * KS, PAD = KS / 2;
  // PX pixels per thread (4, or 8 for the r == 2 fast path: un-shuffled stores become 16 bytes, 2 loads + 2 stores per
  // 8 pixels and channel instead of 2 + 4 -- the kernel is bound by the number of global memory instructions)
  constexpr int TW = 64, TPR = TW / PX, TH = 256 / TPR;
  constexpr int PH = TH + KS - 1, PW = TW + KS - 1;
  constexpr int PWS = (PW + 3) / 4 * 4;
  __shared__ __attribute__((aligned(16))) float patch[NCO * PH * PWS];
  // weights of one output channel ci, contiguous: wl[ci][co*KK + tap] (row padded to a multiple of 4 floats).  The
  // operand arrives k-major ([co*KK + tap][ld]): reading it per ci would be NCO*KK separate scalar loads; from LDS it is
  // NCO*KK/4 broadcast ds_read_b128.
  constexpr int KKP = (KK + 3) / 4 * 4;        // taps of one input channel, padded to whole 16-byte vectors
  constexpr int WROW = NCO * KKP;
  constexpr int WL_MAX = 64;   // output channels cached per pass (64 * 112 * 4 B = 28 KB for k = 5)
  __shared__ __attribute__((aligned(16))) float wl[WL_MAX * WROW];

  const int tid = threadIdx.x;
  const int row = tid / TPR, c4 = (tid % TPR) * PX;
  // 1-D grid over (image, tile), XCD-chunked (nq_xcd_chunk): neighbouring tiles share halo rows / lines behind one L2
  const int lid = nq_xcd_chunk((int)blockIdx.x, (int)gridDim.x);
  const int tiles = tiles_x * ((H + TH - 1) / TH), tile = lid % tiles;
  const int tile_x = tile % tiles_x, tile_y = tile / tiles_x;
  const int x0 = tile_x * TW, y0 = tile_y * TH, b = lid / tiles;
  const int64_t HW = (int64_t)H * W;
  const float* __restrict__ dyb = dy + (int64_t)b * CO * HW;

  for (int e = tid; e < CO * PH * PW; e += 256) {
    int co = e / (PH * PW), rem = e - co * (PH * PW);
    int rr = rem / PW, c = rem - rr * PW;
    int gy = y0 - PAD + rr, gx = x0 - PAD + c;
    float v = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = dyb[(int64_t)co * HW + (int64_t)gy * W + gx];
    patch[(co * PH + rr) * PWS + c] = v;
  }
  __syncthreads();
  // the thread's dY neighbourhood: CO x KS rows x (4+KS-1) columns, kept in registers for the whole C_in loop
  float nb[NCO][KS][PX + KS - 1];
#pragma unroll
  for (int co = 0; co < NCO; ++co)
#pragma unroll
    for (int kh = 0; kh < KS; ++kh)
#pragma unroll
      for (int j = 0; j < PX + KS - 1; ++j) nb[co][kh][j] = (co < CO) ? patch[(co * PH + row + kh) * PWS + c4 + j] : 0.f;

  const int gy = y0 + row, gx0 = x0 + c4;
  const bool active = (gy < H && gx0 < W);   // inactive threads still help staging the weights and join the barriers
  const bool full = (gx0 + PX - 1 < W);
#pragma unroll 1
  for (int ci = 0; ci < Cin; ++ci) {
    if (ci % WL_MAX == 0) {   // (re)fill the weight cache for output channels [ci, ci + WL_MAX)
      __syncthreads();
      const int nci = min(WL_MAX, Cin - ci);
      for (int e = tid; e < nci * WROW; e += 256) {
        const int cl = e / WROW, j = e - cl * WROW;
        const int co = j / KKP, tap = j - co * KKP;
        wl[e] = (co < CO && tap < KK) ? wt[(int64_t)(co * KK + tap) * ld + ci + cl] : 0.f;
      }
      __syncthreads();
    }
    if (!active) continue;
    float acc[PX];
#pragma unroll
    for (int p = 0; p < PX; ++p) acc[p] = 0.f;
    const float* __restrict__ wrow = wl + (ci % WL_MAX) * WROW;
#pragma unroll
    for (int co = 0; co < NCO; ++co) {
      if (co < CO) {
        // the KK weights of (ci, co): KKP/4 broadcast 16-byte LDS reads (same address in every lane), consumed before the
        // next input channel's are requested -- keeps ~28 weight registers live instead of all NCO*KK
        float wv[KKP];
#pragma unroll
        for (int q = 0; q < KKP / 4; ++q) {
          const float4 t = *reinterpret_cast<const float4*>(wrow + co * KKP + 4 * q);
          wv[4 * q] = t.x; wv[4 * q + 1] = t.y; wv[4 * q + 2] = t.z; wv[4 * q + 3] = t.w;
        }
#pragma unroll
        for (int kh = 0; kh < KS; ++kh)
#pragma unroll
          for (int kw = 0; kw < KS; ++kw) {
#pragma unroll
            for (int p = 0; p < PX; ++p) acc[p] = fmaf(wv[kh * KS + kw], nb[co][kh][p + kw], acc[p]);
          }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    const int64_t zi = ((int64_t)b * Cin + ci) * HW + (int64_t)gy * W + gx0;
    if (zprev) {
      if (full && (W & 3) == 0) {
#pragma unroll
        for (int q = 0; q < PX / 4; ++q) {
          const float4 zv = *reinterpret_cast<const float4*>(zprev + zi + 4 * q);
          acc[4 * q] *= zv.x; acc[4 * q + 1] *= zv.y; acc[4 * q + 2] *= zv.z; acc[4 * q + 3] *= zv.w;
        }
      } else {
#pragma unroll
        for (int p = 0; p < PX; ++p)
          if (gx0 + p < W) acc[p] *= zprev[zi + p];
      }
    }
    if constexpr (R2) {
      // un-shuffle: channel ci*4 + (y%2)*2 + x%2 at (y/2, x/2): even pixels -> plane j=0, odd pixels -> plane j=1
      const int Ho = H >> 1, Wo = W >> 1;
      const int64_t base = ((((int64_t)b * Cin + ci) * 4 + (gy & 1) * 2) * Ho + (gy >> 1)) * (int64_t)Wo + (gx0 >> 1);
      if constexpr (PX == 8) {
        *reinterpret_cast<float4*>(out + base) = make_float4(acc[0], acc[2], acc[4], acc[6]);
        *reinterpret_cast<float4*>(out + base + (int64_t)Ho * Wo) = make_float4(acc[1], acc[3], acc[5], acc[7]);
      } else {
        *reinterpret_cast<float2*>(out + base) = make_float2(acc[0], acc[2]);
        *reinterpret_cast<float2*>(out + base + (int64_t)Ho * Wo) = make_float2(acc[1], acc[3]);
      }
    } else if (r == 1) {
#pragma unroll
      for (int p = 0; p < PX; ++p)
        if (gx0 + p < W) out[zi + p] = acc[p];
    } else if (PX == 4 && r == 2 && full && (W & 3) == 0 && (H & 1) == 0) {
      // un-shuffle: channel ci*4 + (y%2)*2 + x%2 at (y/2, x/2): pixels {0,2} -> plane j=0, {1,3} -> plane j=1
      const int Ho = H >> 1, Wo = W >> 1;
      const int64_t base = ((((int64_t)b * Cin + ci) * 4 + (gy & 1) * 2) * Ho + (gy >> 1)) * (int64_t)Wo + (gx0 >> 1);
      *reinterpret_cast<float2*>(out + base) = make_float2(acc[0], acc[2]);
      *reinterpret_cast<float2*>(out + base + (int64_t)Ho * Wo) = make_float2(acc[1], acc[3]);
    } else {
      const int Ho = H / r, Wo = W / r, rr2 = r * r;
#pragma unroll
      for (int p = 0; p < PX; ++p) {
        const int gx = gx0 + p;
        if (gx < W) {
          const int yq = gy / r, xq = gx / r;
          const int ch = ci * rr2 + (gy - yq * r) * r + (gx - xq * r);
          out[(((int64_t)b * Cin * rr2 + ch) * Ho + yq) * (int64_t)Wo + xq] = acc[p];
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ data gradient, streaming
// Round 3, same idea as head_fwd2: a WAVE owns a strip of 256 columns x R rows, no barrier in the loop.  The 3-channel dY
// neighbourhood of the whole block ((R + 2) rows x CO x (4 + 2) columns; halo by DPP wave shifts, the strip's outer columns
// by one dword per row and channel) is loaded ONCE into registers; the loop then walks the C_in output channels: 27 x 4
// fused multiply-adds per row from the register neighbourhood (weights: [ci][co*9 + tap] in LDS, filled once per
// workgroup, read one channel ahead by 7 broadcast 16-byte reads), times gelu'(z) -- one 16-byte load per row, one channel
// ahead through bounds-checked buffer loads at per-row offsets computed once -- and two 8-byte PixelUnshuffle(2) stores
// per row (even / odd pixels; 512 contiguous bytes per wave-instruction).  Per output the fp32 fused multiply-adds run
// in (co, kh, kw) order, as in head_dgrad_kernel.
struct HeadDg2Args {
  int B, Cin, H, W, ld, strips, rblocks;   // Cin = channels of the OUTPUT (naming of head_dgrad_kernel)
  unsigned dy_bytes, z_bytes;
  int out_split;                           // the output is written as split {hi | lo} words (nq_common.h)
};

template <int R, int NCO>
__global__ __launch_bounds__(256) void head_dgrad2_kernel(const float* __restrict__ dy_, const float* __restrict__ wt,
                                                          const float* __restrict__ z_, float* __restrict__ out_,
                                                          HeadDg2Args a) {
  constexpr int KS = 3, KK = 9, NR = R + 2, WROW = 28;   // 27 weights per output channel, padded to 7 x 16 bytes
  constexpr unsigned OOB = 0xFFFFFF00u;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int H = a.H, W = a.W, Cin = a.Cin;
  // wl[ci][co*9 + tap] = wt[(co*9 + tap)*ld + ci]   (wt_bwd operand: k-major, already tap-flipped); the only barrier
  extern __shared__ __attribute__((aligned(16))) float wl_f[];
  for (int e = threadIdx.x; e < Cin * WROW; e += 256) {
    const int ci = e / WROW, j = e - ci * WROW;
    wl_f[e] = (j < NCO * KK) ? wt[(int64_t)j * a.ld + ci] : 0.f;
  }
  __syncthreads();
  const int total = a.B * a.strips * a.rblocks;
  const int wid = nq_xcd_chunk((int)blockIdx.x, (int)gridDim.x) * 4 + wave;
  if (wid >= total) return;   // whole wave
  const int by = wid % a.rblocks, t0 = wid / a.rblocks;
  const int sx = t0 % a.strips, b = t0 / a.strips;
  const int y0 = by * R, x0 = sx * 256, gx = x0 + 4 * lane;
  const unsigned HWb = (unsigned)H * (unsigned)W * 4u, Wb = (unsigned)W * 4u;
  const __amdgpu_buffer_rsrc_t rs_dy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dy_), 0, (int)a.dy_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_z = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(z_), 0, (int)a.z_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc(out_, 0, (int)a.z_bytes, 0x00020000);

  // ---- the dY neighbourhood: nb[row][co] = {left, 4 pixels, right}
  float nb[NR][NCO][6];
  {
    const int ex = (lane == 0) ? x0 - 1 : x0 + 256;
    const bool e_ok = (lane == 0 || lane == 63) && ex >= 0 && ex < W;
    f32x4 q[NR][NCO];
    float ed[NR][NCO];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int iy = y0 - 1 + r;
      const bool rok = iy >= 0 && iy < H;
#pragma unroll
      for (int co = 0; co < NCO; ++co) {
        const unsigned ro = ((unsigned)(b * NCO + co) * (unsigned)H + (unsigned)iy) * Wb;
        q[r][co] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_dy, (rok && gx < W) ? ro + (unsigned)gx * 4u : OOB, 0, 0));
        ed[r][co] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_dy, (rok && e_ok) ? ro + (unsigned)ex * 4u : OOB, 0, 0));
      }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int co = 0; co < NCO; ++co) {
        // (named floats: __builtin_bit_cast applied directly to a vector element reads element 0 with hipcc 7.2)
        const float v3f = q[r][co][3], v0f = q[r][co][0], ef = ed[r][co];
        const int ei = __builtin_bit_cast(int, ef);
        nb[r][co][0] = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(ei, __builtin_bit_cast(int, v3f), 0x138, 0xF, 0xF, false));
        nb[r][co][5] = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(ei, __builtin_bit_cast(int, v0f), 0x130, 0xF, 0xF, false));
#pragma unroll
        for (int p = 0; p < 4; ++p) nb[r][co][1 + p] = q[r][co][p];
      }
  }

  // per-row byte offsets (relative to (frame b, channel ci)) of the gelu' quad and of the two un-shuffled 8-byte stores:
  // output row y0 + r, channel ci -> planes ci*4 + (y%2)*2 + {0: even pixels, 1: odd pixels} at (y/2, x/2); the plane of
  // channel ci*4 starts at the same offset as channel ci of the full-resolution tensor ((b*Cin + ci)*H*W)
  const unsigned Ho = (unsigned)H >> 1, Wo = (unsigned)W >> 1;
  unsigned oz[R], oo[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int gy = y0 + r;
    const bool ok = gy < H && gx < W;
    oz[r] = ok ? (unsigned)gy * Wb + (unsigned)gx * 4u : OOB;
    oo[r] = ok ? ((((unsigned)gy & 1u) * 2u * Ho + ((unsigned)gy >> 1)) * Wo + ((unsigned)gx >> 1)) * 4u : OOB;
  }
  const unsigned plane_b = Ho * Wo * 4u;
  const unsigned base_b = (unsigned)b * (unsigned)Cin * HWb;

  auto load_z = [&](int ci, f32x4 (&z)[R]) {
    const unsigned so = base_b + (unsigned)min(ci, Cin - 1) * HWb;
#pragma unroll
    for (int r = 0; r < R; ++r) z[r] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_z, oz[r], so, 0));
  };
  auto load_w = [&](int ci, f32x4 (&w)[WROW / 4]) {
    const f32x4* __restrict__ wr = reinterpret_cast<const f32x4*>(wl_f) + min(ci, Cin - 1) * (WROW / 4);
#pragma unroll
    for (int t = 0; t < WROW / 4; ++t) w[t] = wr[t];
  };
  auto compute = [&](int ci, const f32x4 (&z)[R], const f32x4 (&w)[WROW / 4]) {
    const unsigned so = base_b + (unsigned)ci * HWb;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      f32x2 acc0 = {0.f, 0.f}, acc1 = {0.f, 0.f};   // pixels (0,1) and (2,3)
#pragma unroll
      for (int co = 0; co < NCO; ++co)
#pragma unroll
        for (int kh = 0; kh < KS; ++kh)
#pragma unroll
          for (int kw = 0; kw < KS; ++kw) {
            const int j = co * KK + kh * KS + kw;
            const float wv = w[j >> 2][j & 3];
            const f32x2 w2 = {wv, wv};
            const float* in = nb[r + kh][co];
            acc0 = __builtin_elementwise_fma(w2, f32x2{in[kw], in[kw + 1]}, acc0);
            acc1 = __builtin_elementwise_fma(w2, f32x2{in[kw + 2], in[kw + 3]}, acc1);
          }
      const f32x4 zz = z[r];
      f32x2 ev = {acc0[0] * zz[0], acc1[0] * zz[2]}, od = {acc0[1] * zz[1], acc1[1] * zz[3]};
      if (a.out_split) {
        ev = f32x2{nq_split_word_f(ev[0]), nq_split_word_f(ev[1])};
        od = f32x2{nq_split_word_f(od[0]), nq_split_word_f(od[1])};
      }
      const unsigned vo = oo[r];
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(__attribute__((ext_vector_type(2))) unsigned, ev), rs_o, vo, so, 0);
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(__attribute__((ext_vector_type(2))) unsigned, od), rs_o,
                                            vo == OOB ? OOB : vo + plane_b, so, 0);
    }
  };

  f32x4 zA[R], zB[R], wA[WROW / 4], wB[WROW / 4];
  load_z(0, zA);
  load_w(0, wA);
#pragma unroll 1
  for (int ci = 0; ci + 1 < Cin; ci += 2) {
    load_z(ci + 1, zB);
    load_w(ci + 1, wB);
    __builtin_amdgcn_sched_barrier(0);
    compute(ci, zA, wA);
    __builtin_amdgcn_sched_barrier(0);
    load_z(ci + 2, zA);
    load_w(ci + 2, wA);
    __builtin_amdgcn_sched_barrier(0);
    compute(ci + 1, zB, wB);
    __builtin_amdgcn_sched_barrier(0);
  }
  if (Cin & 1) compute(Cin - 1, zA, wA);
}

}  // namespace

extern "C" {

// Selection rule shared with conv.hip: the vector path serves C_out <= 4.
int nq_head_supported(int Cout, int k) { return Cout <= MAXCO && (k == 1 || k == 3 || k == 5); }

// ONE resolution of a head forward call, read by the launch below and by nq_conv_forward_plan (conv.hip): 1 the streaming kernel
// with *rows output rows per wave, 0 the LDS-staged kernel, -1 NQ_HEAD_RD names a value that is not compiled.
// 3x3 heads with whole 16-byte quads per row and a tensor below 4 GiB (32-bit buffer offsets) stream.
int nq_head_forward_route(int B, int Cin, int H, int W, int Cout, int k, int ld, int* rows) {
  const char* hv = getenv("NQ_HEAD_FWD");   // NQ_HEAD_FWD=1: the LDS-staged kernel (A/B runs; read per call)
  const bool v1 = hv && hv[0] == '1';
  *rows = 0;
  if (!(k == 3 && Cout == 3 && (W & 3) == 0 && (ld & 3) == 0 && (int64_t)B * Cin * H * W * 4 < 0xFFFFFF00ll && !v1)) return 0;
  // R output rows per wave; NQ_HEAD_RD=r picks another compiled value (timing runs)
  int R = 4;
  if (const char* rd = getenv("NQ_HEAD_RD")) R = atoi(rd);
  *rows = R;
  return (R == 4 || R == 5) ? 1 : -1;
}

int nq_head_forward(const float* x, const float* wt, int ld, const float* bias, float* y, int B, int Cin, int H, int W,
                    int Cout, int k, int epi, hipStream_t st) {
  int R;
  const int route = nq_head_forward_route(B, Cin, H, W, Cout, k, ld, &R);
  if (route < 0) return NQ_ERR_UNSUPPORTED;
  if (route == 1) {
    HeadFwd2Args a;
    a.B = B; a.Cin = Cin; a.H = H; a.W = W; a.ld = ld;
    a.strips = (W + 255) / 256; a.rblocks = (H + R - 1) / R;
    a.x_bytes = (unsigned)((int64_t)B * Cin * H * W * 4);
    a.hot_first = head_hot_first(B, a.strips, a.rblocks);
    const int waves = B * a.strips * a.rblocks;
    dim3 g2((unsigned)((waves + 3) / 4)), blk2(256);
    const size_t lds = 0;
    const bool th = epi == NQ_EPI_TANH;
#define NQ_HF2(R_)                                                                                              \
  if (R == R_) {                                                                                                \
    if (th) hipLaunchKernelGGL((head_fwd2_kernel<R_, 3, true>), g2, blk2, lds, st, x, wt, bias, y, a);          \
    else hipLaunchKernelGGL((head_fwd2_kernel<R_, 3, false>), g2, blk2, lds, st, x, wt, bias, y, a);            \
    return nq_launch_status();                                                                                  \
  }
    NQ_HF2(4)
    NQ_HF2(5)
#undef NQ_HF2
    return NQ_ERR_UNSUPPORTED;
  }
  const int tiles_x = (W + 63) / 64, tiles = tiles_x * ((H + 15) / 16);
  dim3 g((unsigned)(tiles * B)), blk(256);
  switch (k) {
    case 1: hipLaunchKernelGGL(head_fwd_kernel<1>, g, blk, 0, st, x, wt, ld, bias, y, Cin, H, W, Cout, epi, tiles_x); break;
    case 3: hipLaunchKernelGGL(head_fwd_kernel<3>, g, blk, 0, st, x, wt, ld, bias, y, Cin, H, W, Cout, epi, tiles_x); break;
    default: hipLaunchKernelGGL(head_fwd_kernel<5>, g, blk, 0, st, x, wt, ld, bias, y, Cin, H, W, Cout, epi, tiles_x); break;
  }
  return nq_launch_status();
}

// The 3-channel tanh head and the loss tail in ONE pass (include/nq_hip.h: nq_head_forward_loss).
int64_t nq_head_forward_loss_ws_floats(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (int64_t)B * ((W + 255) / 256) * ((H + 3) / 4) * 4;
}

int nq_head_forward_loss(const float* x, const float* wt, int ld, const float* bias, float* y, const float* tgt,
                         const uint8_t* cache_u8, const int64_t* idx, float* loss, float* dconv, float* db, float* ws, int B,
                         int Cin, int H, int W, int64_t mean_count, float gscale, nq_stream_t stream) {
  if (!x || !wt || !y || !loss || !dconv || !db || !ws || B <= 0 || Cin <= 0 || H <= 0 || W <= 0 || mean_count <= 0) return NQ_ERR_INVALID;
  if ((tgt == nullptr) == (cache_u8 == nullptr) || (cache_u8 && !idx)) return NQ_ERR_INVALID;
  if ((W & 3) != 0 || (ld & 3) != 0 || (int64_t)B * Cin * H * W * 4 >= 0xFFFFFF00ll) return NQ_ERR_UNSUPPORTED;
  constexpr int R = 4;
  HeadFwd2Args a;
  a.B = B; a.Cin = Cin; a.H = H; a.W = W; a.ld = ld;
  a.strips = (W + 255) / 256; a.rblocks = (H + R - 1) / R;
  a.x_bytes = (unsigned)((int64_t)B * Cin * H * W * 4);
  a.hot_first = head_hot_first(B, a.strips, a.rblocks);
  HeadLossArgs la;
  la.tgt = tgt; la.cache = cache_u8; la.idx = idx; la.dconv = dconv; la.ws = ws;
  la.gcoef = (float)(2.0 / (double)mean_count) * gscale;
  const int waves = B * a.strips * a.rblocks;
  hipStream_t st = nq_s(stream);
  hipLaunchKernelGGL((head_fwd2_kernel<R, 3, true, true>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, x, wt, bias, y, a, la);
  hipLaunchKernelGGL(head_loss_stage2, dim3(4), dim3(256), 0, st, ws, waves, (float)(1.0 / (double)mean_count), loss, db);
  return nq_launch_status();
}

// dy (B,Cout,H,W) -> out = d/dx (B,Cin,H,W) [* gelu'(zprev)] stored PixelUnshuffle(r)-ed
// ONE resolution of a head data-gradient call, read by the launch below, nq_conv_split_out and nq_conv_forward_plan (conv.hip):
// 1 the streaming kernel with *rows rows per wave, -1 NQ_HEAD_DG_R names a value that is not compiled, 0 the LDS-staged kernel
// head_dgrad_kernel<k, *r2, *co, *px>.  The shipped head (3x3, 3 image channels, GELU + PixelShuffle(2) below it) streams; 32-bit
// buffer offsets; its weights (Cin x 28 floats) must fit 64 KiB of LDS.
int nq_head_dgrad_route(int B, int Cin, int H, int W, int Cout, int k, int r, int has_z, int* rows, int* r2, int* co, int* px) {
  const char* hv = getenv("NQ_HEAD_DGRAD");   // NQ_HEAD_DGRAD=1: the LDS-staged kernel (A/B runs; read per call)
  *rows = *r2 = *co = *px = 0;
  if (k == 3 && Cout == 3 && r == 2 && has_z && (W % 4 == 0) && (H % 2 == 0) && (int64_t)B * Cin * H * W * 4 < 0xFFFFFF00ll &&
      !(hv && hv[0] == '1') && (size_t)Cin * 28 * 4 <= 64 * 1024) {
    int R = 4;
    if (const char* rd = getenv("NQ_HEAD_DG_R")) R = atoi(rd);
    *rows = R;
    return (R == 2 || R == 4) ? 1 : -1;
  }
  // r == 2 fast path: 8 pixels per thread (tile 32 x 64) when W % 8 == 0 and k <= 3, else 4 (tile 16 x 64)
  *r2 = (r == 2) && (W % 4 == 0) && (H % 2 == 0);
  *px = (*r2 && (W % 8 == 0) && k <= 3) ? 8 : 4;
  *co = Cout <= 3 ? 3 : 4;
  return 0;
}

// 1 when nq_head_dgrad runs the streaming kernel for this call (the only one that can write split {hi | lo} words)
int nq_head_dgrad_streams(int B, int Cin, int H, int W, int Cout, int k, int r, int has_z) {
  int rows, r2, co, px;
  return nq_head_dgrad_route(B, Cin, H, W, Cout, k, r, has_z, &rows, &r2, &co, &px) == 1;
}

int nq_head_dgrad(const float* dy, const float* wt, int ld, const float* zprev, float* out, int B, int Cin, int H, int W,
                  int Cout, int k, int r, int out_split, hipStream_t st) {
  int R, r2_, co_, px_;
  const int route = nq_head_dgrad_route(B, Cin, H, W, Cout, k, r, zprev != nullptr, &R, &r2_, &co_, &px_);
  if (route < 0 || (out_split && route != 1)) return NQ_ERR_UNSUPPORTED;
  if (route == 1) {
    HeadDg2Args a;
    a.B = B; a.Cin = Cin; a.H = H; a.W = W; a.ld = ld;
    a.strips = (W + 255) / 256; a.rblocks = (H + R - 1) / R;
    a.dy_bytes = (unsigned)((int64_t)B * Cout * H * W * 4);
    a.z_bytes = (unsigned)((int64_t)B * Cin * H * W * 4);
    a.out_split = out_split;
    const int waves = B * a.strips * a.rblocks;
    dim3 g2((unsigned)((waves + 3) / 4)), blk2(256);
    const size_t lds = (size_t)Cin * 28 * 4;
    if (R == 2) hipLaunchKernelGGL((head_dgrad2_kernel<2, 3>), g2, blk2, lds, st, dy, wt, zprev, out, a);
    else hipLaunchKernelGGL((head_dgrad2_kernel<4, 3>), g2, blk2, lds, st, dy, wt, zprev, out, a);
    return nq_launch_status();
  }
  const bool r2 = r2_ != 0, px8 = px_ == 8;
  const int th = px8 ? 32 : 16;
  const int tiles_x = (W + 63) / 64, tiles = tiles_x * ((H + th - 1) / th);
  dim3 g((unsigned)(tiles * B)), blk(256);
#define NQ_HD(KS_, R2_, PX_)                                                                                          \
  do {                                                                                                                \
    if (co_ == 3)                                                                                                     \
      hipLaunchKernelGGL((head_dgrad_kernel<KS_, R2_, 3, PX_>), g, blk, 0, st, dy, wt, ld, zprev, out, Cin, H, W, Cout, r, \
                         tiles_x);                                                                                    \
    else                                                                                                              \
      hipLaunchKernelGGL((head_dgrad_kernel<KS_, R2_, 4, PX_>), g, blk, 0, st, dy, wt, ld, zprev, out, Cin, H, W, Cout, r, \
                         tiles_x);                                                                                    \
  } while (0)
  switch (k) {
    case 1: if (px8) NQ_HD(1, 1, 8); else if (r2) NQ_HD(1, 1, 4); else NQ_HD(1, 0, 4); break;
    case 3: if (px8) NQ_HD(3, 1, 8); else if (r2) NQ_HD(3, 1, 4); else NQ_HD(3, 0, 4); break;
    default: if (r2) NQ_HD(5, 1, 4); else NQ_HD(5, 0, 4); break;
  }
#undef NQ_HD
  return nq_launch_status();
}

}  // extern "C"

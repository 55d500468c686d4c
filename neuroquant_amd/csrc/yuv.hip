// 8-bit YUV 4:2:0 (I420) frames, the payload of a .y4m / .yuv file: float RGB -> I420 for the player's output,
// I420 -> 8-bit RGB for ground truth read from a clip, and the exact per-plane squared error of two I420 frames.
//
// All arithmetic is fp32 in the order written in include/nq_hip.h, uncontracted (-ffp-contract=off), so the numpy float32
// restatement (tests/yuv_ref.py) is bit-exact.  Every constant is formed in double and rounded once to float:
//
//                                 BT.601 (matrix 0)            BT.709 (matrix 1)
//   Kr                            0.299      0x1.322d0ep-2     0.2126     0x1.b367a0p-3
//   Kg = 1 - Kr - Kb              0.587      0x1.2c8b44p-1     0.7152     0x1.6e2eb2p-1
//   Kb                            0.114      0x1.d2f1aap-4     0.0722     0x1.27bb30p-4
//   icb  = 1 / (2 (1 - Kb))       0.5643341  0x1.20f066p-1     0.53890926 0x1.13ebeap-1
//   icr  = 1 / (2 (1 - Kr))       0.7132668  0x1.6d314ep-1     0.63500124 0x1.451ee2p-1
//   c_r  = 2 (1 - Kr)             1.402      0x1.66e978p+0     1.5748     0x1.932618p+0
//   c_b  = 2 (1 - Kb)             1.772      0x1.c5a1cap+0     1.8556     0x1.db089ap+0
//   c_gb = Kb (2 (1 - Kb)) / Kg   0.3441363  0x1.606544p-2     0.18732427 0x1.7fa3dep-3
//   c_gr = Kr (2 (1 - Kr)) / Kg   0.7141363  0x1.6da346p-1     0.46812427 0x1.df5bf8p-2
//   1/219 = 0x1.2b404ap-8    1/224 = 0x1.24924ap-8    1/255 = 0x1.010102p-8
// (16, 128, 219, 224, 255 and 0.25 are exact.)
//
// Chroma: the forward conversion takes the mean of each 2 x 2 block, the inverse gives each chroma sample to its 2 x 2 block
// (box down / nearest up, sited at the block centre as y4m's C420jpeg).
//
// Memory: a frame is a few MB that is read once and written once, so the kernels are shaped by coalescing alone.  In the
// vector kernels a thread owns 2 rows x 8 columns: consecutive lanes take consecutive 32-byte (float) or 8-byte (code) pieces
// of a row, so a wave reads 2 KB contiguous per row and plane.  No LDS, no atomics, one writer per byte.
#include "nq_common.h"

namespace {

constexpr int TPB = 256;

struct FwdK {   // forward: luma weights, chroma scales, code scales / offset
  float kr, kg, kb, icb, icr, ysc, yoff, csc;
};
struct InvK {   // inverse: code scales / offset, chroma -> colour weights
  float iy, yoff, ic, c_r, c_b, c_gb, c_gr;
};

struct Coef {
  double kr, kb;
};
inline Coef coef(int matrix) { return matrix == 0 ? Coef{0.299, 0.114} : Coef{0.2126, 0.0722}; }

inline FwdK fwd_consts(int matrix, int full_range) {
  const Coef c = coef(matrix);
  const double kg = 1.0 - c.kr - c.kb;
  FwdK k;
  k.kr = (float)c.kr;
  k.kg = (float)kg;
  k.kb = (float)c.kb;
  k.icb = (float)(1.0 / (2.0 * (1.0 - c.kb)));
  k.icr = (float)(1.0 / (2.0 * (1.0 - c.kr)));
  k.ysc = full_range ? 255.0f : 219.0f;
  k.yoff = full_range ? 0.0f : 16.0f;
  k.csc = full_range ? 255.0f : 224.0f;
  return k;
}

inline InvK inv_consts(int matrix, int full_range) {
  const Coef c = coef(matrix);
  const double kg = 1.0 - c.kr - c.kb;
  InvK k;
  k.iy = full_range ? (float)(1.0 / 255.0) : (float)(1.0 / 219.0);
  k.yoff = full_range ? 0.0f : 16.0f;
  k.ic = full_range ? (float)(1.0 / 255.0) : (float)(1.0 / 224.0);
  k.c_r = (float)(2.0 * (1.0 - c.kr));
  k.c_b = (float)(2.0 * (1.0 - c.kb));
  k.c_gb = (float)(c.kb * (2.0 * (1.0 - c.kb)) / kg);
  k.c_gr = (float)(c.kr * (2.0 * (1.0 - c.kr)) / kg);
  return k;
}

// NaN fails `x > 0` and maps to 0: the rule of nq_frames_to_u8
__device__ __forceinline__ float clamp01(float x) {
  const float c = x > 0.f ? x : 0.f;
  return c < 1.f ? c : 1.f;
}
// round half even, then clamp to a byte
__device__ __forceinline__ uint32_t code255(float v) {
  v = rintf(v);
  v = v > 0.f ? v : 0.f;
  v = v < 255.f ? v : 255.f;
  return (uint32_t)v;
}
__device__ __forceinline__ uint32_t pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return a | (b << 8) | (c << 16) | (d << 24);
}

// one pixel: clamped RGB -> luma code, cb, cr
__device__ __forceinline__ uint32_t fwd_px(const FwdK& k, float r, float g, float b, float& cb, float& cr) {
  r = clamp01(r);
  g = clamp01(g);
  b = clamp01(b);
  const float y = (k.kr * r + k.kg * g) + k.kb * b;
  cb = (b - y) * k.icb;
  cr = (r - y) * k.icr;
  return code255(k.yoff + k.ysc * y);
}
// the mean of a 2 x 2 block of one chroma component (row 0 first, left before right) -> code
__device__ __forceinline__ uint32_t chroma_code(const FwdK& k, float c00, float c01, float c10, float c11) {
  const float m = ((c00 + c01) + (c10 + c11)) * 0.25f;
  return code255(128.0f + k.csc * m);
}

// thread t -> frame, block row (2 image rows) and column group (G columns) of its piece
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

// W % 8 == 0, src 16-byte and dst 8-byte aligned: 2 rows x 8 columns per thread, twelve 16-byte loads, two 8-byte Y stores,
// one dword each of U and V.  Every address below is aligned because W * 4, H * W and H * W / 4 are multiples of 32, 16 and 4.
__global__ __launch_bounds__(TPB) void yuv_fwd_vec_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst, int64_t total,
                                                          int H, int W, FwdK k) {
  const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= total) return;
  const Piece p = piece_of(t, H >> 1, W >> 3);
  const int64_t HW = (int64_t)H * W;
  const float* s = src + p.f * 3 * HW + (int64_t)(2 * p.by) * W + p.bx * 8;
  uint8_t* d = dst + p.f * (HW + HW / 2);
  float cb[2][8], cr[2][8];
#pragma unroll
  for (int row = 0; row < 2; ++row) {
    const float* sr = s + (int64_t)row * W;
    float r[8], g[8], b[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float4 vr = *reinterpret_cast<const float4*>(sr + 4 * h);
      const float4 vg = *reinterpret_cast<const float4*>(sr + HW + 4 * h);
      const float4 vb = *reinterpret_cast<const float4*>(sr + 2 * HW + 4 * h);
      r[4 * h] = vr.x; r[4 * h + 1] = vr.y; r[4 * h + 2] = vr.z; r[4 * h + 3] = vr.w;
      g[4 * h] = vg.x; g[4 * h + 1] = vg.y; g[4 * h + 2] = vg.z; g[4 * h + 3] = vg.w;
      b[4 * h] = vb.x; b[4 * h + 1] = vb.y; b[4 * h + 2] = vb.z; b[4 * h + 3] = vb.w;
    }
    uint32_t yc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) yc[j] = fwd_px(k, r[j], g[j], b[j], cb[row][j], cr[row][j]);
    uint2 o;
    o.x = pack4(yc[0], yc[1], yc[2], yc[3]);
    o.y = pack4(yc[4], yc[5], yc[6], yc[7]);
    *reinterpret_cast<uint2*>(d + (int64_t)(2 * p.by + row) * W + p.bx * 8) = o;
  }
  uint32_t u[4], v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    u[j] = chroma_code(k, cb[0][2 * j], cb[0][2 * j + 1], cb[1][2 * j], cb[1][2 * j + 1]);
    v[j] = chroma_code(k, cr[0][2 * j], cr[0][2 * j + 1], cr[1][2 * j], cr[1][2 * j + 1]);
  }
  const int64_t co = (int64_t)p.by * (W >> 1) + p.bx * 4;
  *reinterpret_cast<uint32_t*>(d + HW + co) = pack4(u[0], u[1], u[2], u[3]);
  *reinterpret_cast<uint32_t*>(d + HW + HW / 4 + co) = pack4(v[0], v[1], v[2], v[3]);
}

// any even H and W, any alignment: one thread per 2 x 2 block, scalar loads, byte stores
__global__ __launch_bounds__(TPB) void yuv_fwd_block_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst, int64_t total,
                                                            int H, int W, FwdK k) {
  const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= total) return;
  const Piece p = piece_of(t, H >> 1, W >> 1);
  const int64_t HW = (int64_t)H * W;
  const float* s = src + p.f * 3 * HW + (int64_t)(2 * p.by) * W + p.bx * 2;
  uint8_t* d = dst + p.f * (HW + HW / 2);
  float cb[2][2], cr[2][2];
#pragma unroll
  for (int row = 0; row < 2; ++row) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t o = (int64_t)row * W + j;
      d[(int64_t)(2 * p.by + row) * W + p.bx * 2 + j] = (uint8_t)fwd_px(k, s[o], s[HW + o], s[2 * HW + o], cb[row][j], cr[row][j]);
    }
  }
  const int64_t co = (int64_t)p.by * (W >> 1) + p.bx;
  d[HW + co] = (uint8_t)chroma_code(k, cb[0][0], cb[0][1], cb[1][0], cb[1][1]);
  d[HW + HW / 4 + co] = (uint8_t)chroma_code(k, cr[0][0], cr[0][1], cr[1][0], cr[1][1]);
}

// (uint8) rint(min(max(x, 0), 1) * 255)
__device__ __forceinline__ uint32_t rgb_code(float x) { return (uint32_t)rintf(clamp01(x) * 255.0f); }

struct Chroma {   // what one chroma sample adds to its four pixels
  float r, b, gb, gr;
};
__device__ __forceinline__ Chroma chroma_of(const InvK& k, uint32_t U, uint32_t V) {
  const float cb = ((float)U - 128.0f) * k.ic;
  const float cr = ((float)V - 128.0f) * k.ic;
  return Chroma{k.c_r * cr, k.c_b * cb, k.c_gb * cb, k.c_gr * cr};
}
__device__ __forceinline__ void inv_px(const InvK& k, uint32_t Y, const Chroma& c, uint32_t& r, uint32_t& g, uint32_t& b) {
  const float y = ((float)Y - k.yoff) * k.iy;
  r = rgb_code(y + c.r);
  b = rgb_code(y + c.b);
  g = rgb_code((y - c.gb) - c.gr);
}

// W % 8 == 0, src and dst 8-byte aligned: 2 rows x 8 columns per thread, two 8-byte Y loads, one dword each of U and V,
// six 8-byte stores
__global__ __launch_bounds__(TPB) void yuv_inv_vec_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t total,
                                                          int H, int W, InvK k) {
  const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= total) return;
  const Piece p = piece_of(t, H >> 1, W >> 3);
  const int64_t HW = (int64_t)H * W;
  const uint8_t* s = src + p.f * (HW + HW / 2);
  uint8_t* d = dst + p.f * 3 * HW;
  const int64_t co = (int64_t)p.by * (W >> 1) + p.bx * 4;
  const uint32_t u4 = *reinterpret_cast<const uint32_t*>(s + HW + co);
  const uint32_t v4 = *reinterpret_cast<const uint32_t*>(s + HW + HW / 4 + co);
  Chroma c[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) c[j] = chroma_of(k, (u4 >> (8 * j)) & 255u, (v4 >> (8 * j)) & 255u);
#pragma unroll
  for (int row = 0; row < 2; ++row) {
    const int64_t o = (int64_t)(2 * p.by + row) * W + p.bx * 8;
    const uint2 y8 = *reinterpret_cast<const uint2*>(s + o);
    uint32_t r[8], g[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t Y = ((j < 4 ? y8.x : y8.y) >> (8 * (j & 3))) & 255u;
      inv_px(k, Y, c[j >> 1], r[j], g[j], b[j]);
    }
    *reinterpret_cast<uint2*>(d + o) = make_uint2(pack4(r[0], r[1], r[2], r[3]), pack4(r[4], r[5], r[6], r[7]));
    *reinterpret_cast<uint2*>(d + HW + o) = make_uint2(pack4(g[0], g[1], g[2], g[3]), pack4(g[4], g[5], g[6], g[7]));
    *reinterpret_cast<uint2*>(d + 2 * HW + o) = make_uint2(pack4(b[0], b[1], b[2], b[3]), pack4(b[4], b[5], b[6], b[7]));
  }
}

__global__ __launch_bounds__(TPB) void yuv_inv_block_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t total,
                                                            int H, int W, InvK k) {
  const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= total) return;
  const Piece p = piece_of(t, H >> 1, W >> 1);
  const int64_t HW = (int64_t)H * W;
  const uint8_t* s = src + p.f * (HW + HW / 2);
  uint8_t* d = dst + p.f * 3 * HW;
  const int64_t co = (int64_t)p.by * (W >> 1) + p.bx;
  const Chroma c = chroma_of(k, s[HW + co], s[HW + HW / 4 + co]);
#pragma unroll
  for (int row = 0; row < 2; ++row) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t o = (int64_t)(2 * p.by + row) * W + p.bx * 2 + j;
      uint32_t r, g, b;
      inv_px(k, s[o], c, r, g, b);
      d[o] = (uint8_t)r;
      d[HW + o] = (uint8_t)g;
      d[2 * HW + o] = (uint8_t)b;
    }
  }
}

// Squared code differences of two I420 frames, per frame and plane.  A workgroup takes SSE_CHUNK consecutive bytes of ONE
// frame, 16 per thread; a byte's plane follows from its offset in the frame.  A thread's three sums stay below 16 * 255^2 and a
// wave's below 2^26, so 32-bit registers hold them; the four wave sums meet in LDS as 64-bit values and thread 0 adds the
// workgroup's partial of each plane it touched to sse[frame][plane].  Integer addition is associative: the result does not
// depend on the order in which workgroups arrive.
constexpr int SSE_PER_THREAD = 16;
constexpr int SSE_CHUNK = TPB * SSE_PER_THREAD;

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__global__ __launch_bounds__(TPB) void yuv_sse_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                      unsigned long long* __restrict__ sse, int64_t chunks_per_frame, int64_t HW,
                                                      int vec_ok) {
  __shared__ unsigned long long part[3][TPB / 64];
  const int64_t f = blockIdx.x / chunks_per_frame;
  const int64_t chunk = blockIdx.x - f * chunks_per_frame;
  const int64_t FB = HW + HW / 2, u0 = HW, v0 = HW + HW / 4;
  const int64_t first = chunk * SSE_CHUNK + (int64_t)threadIdx.x * SSE_PER_THREAD;   // offset in the frame
  const uint8_t* pa = a + f * FB + first;
  const uint8_t* pb = b + f * FB + first;
  uint32_t s[3] = {0u, 0u, 0u};
  if (first < FB) {
    uint32_t wa[4] = {0u, 0u, 0u, 0u}, wb[4] = {0u, 0u, 0u, 0u};
    const int cnt = first + SSE_PER_THREAD <= FB ? SSE_PER_THREAD : (int)(FB - first);
    if (vec_ok && cnt == SSE_PER_THREAD) {
      const uint4 va = *reinterpret_cast<const uint4*>(pa);
      const uint4 vb = *reinterpret_cast<const uint4*>(pb);
      wa[0] = va.x; wa[1] = va.y; wa[2] = va.z; wa[3] = va.w;
      wb[0] = vb.x; wb[1] = vb.y; wb[2] = vb.z; wb[3] = vb.w;
    } else {
      for (int j = 0; j < cnt; ++j) {
        wa[j >> 2] |= (uint32_t)pa[j] << (8 * (j & 3));
        wb[j >> 2] |= (uint32_t)pb[j] << (8 * (j & 3));
      }
    }
#pragma unroll
    for (int j = 0; j < SSE_PER_THREAD; ++j) {   // bytes past cnt are zero in both: they add nothing
      const int da = (int)((wa[j >> 2] >> (8 * (j & 3))) & 255u) - (int)((wb[j >> 2] >> (8 * (j & 3))) & 255u);
      const uint32_t sq = (uint32_t)(da * da);
      const int64_t off = first + j;
      s[0] += off < u0 ? sq : 0u;
      s[1] += (off >= u0 && off < v0) ? sq : 0u;
      s[2] += off >= v0 ? sq : 0u;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    const uint32_t w = wave_sum_u32(s[p]);
    if (lane == 0) part[p][wave] = w;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long tot = 0;
#pragma unroll
    for (int w = 0; w < TPB / 64; ++w) tot += part[threadIdx.x][w];
    if (tot) atomicAdd(sse + f * 3 + threadIdx.x, tot);
  }
}

inline bool grid_ok(int64_t blocks) { return blocks > 0 && blocks <= 0x7fffffffLL; }

// what every launch entry checks of its sizes; the element count n * H * W * 3 must fit int64
inline bool sizes_ok(int64_t n, int H, int W) {
  if (n <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1)) return false;
  const int64_t HW = (int64_t)H * W;
  return n <= INT64_MAX / 3 / HW;
}

}  // namespace

extern "C" {

int64_t nq_yuv420_frame_bytes(int64_t H, int64_t W) {
  if (H <= 0 || W <= 0 || (H & 1) || (W & 1)) return 0;
  if (H > INT64_MAX / 3 / W) return 0;
  return H * W / 2 * 3;
}

int nq_frames_to_yuv420(const float* src, uint8_t* dst, int64_t n, int H, int W, int matrix, int full_range, nq_stream_t stream) {
  if (!src || !dst || !sizes_ok(n, H, W) || (matrix != 0 && matrix != 1) || (full_range != 0 && full_range != 1))
    return NQ_ERR_INVALID;
  const FwdK k = fwd_consts(matrix, full_range);
  const bool vec = W % 8 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 7) == 0;
  const int64_t total = n * (H / 2) * (vec ? W / 8 : W / 2), blocks = (total + TPB - 1) / TPB;
  if (!grid_ok(blocks)) return NQ_ERR_UNSUPPORTED;
  if (vec)
    hipLaunchKernelGGL(yuv_fwd_vec_kernel, dim3((unsigned)blocks), dim3(TPB), 0, nq_s(stream), src, dst, total, H, W, k);
  else
    hipLaunchKernelGGL(yuv_fwd_block_kernel, dim3((unsigned)blocks), dim3(TPB), 0, nq_s(stream), src, dst, total, H, W, k);
  return nq_launch_status();
}

int nq_yuv420_to_rgb_u8(const uint8_t* src, uint8_t* dst, int64_t n, int H, int W, int matrix, int full_range, nq_stream_t stream) {
  if (!src || !dst || !sizes_ok(n, H, W) || (matrix != 0 && matrix != 1) || (full_range != 0 && full_range != 1))
    return NQ_ERR_INVALID;
  const InvK k = inv_consts(matrix, full_range);
  const bool vec = W % 8 == 0 && (reinterpret_cast<uintptr_t>(src) & 7) == 0 && (reinterpret_cast<uintptr_t>(dst) & 7) == 0;
  const int64_t total = n * (H / 2) * (vec ? W / 8 : W / 2), blocks = (total + TPB - 1) / TPB;
  if (!grid_ok(blocks)) return NQ_ERR_UNSUPPORTED;
  if (vec)
    hipLaunchKernelGGL(yuv_inv_vec_kernel, dim3((unsigned)blocks), dim3(TPB), 0, nq_s(stream), src, dst, total, H, W, k);
  else
    hipLaunchKernelGGL(yuv_inv_block_kernel, dim3((unsigned)blocks), dim3(TPB), 0, nq_s(stream), src, dst, total, H, W, k);
  return nq_launch_status();
}

int nq_yuv420_sse(const uint8_t* a, const uint8_t* b, uint64_t* sse, int64_t n, int H, int W, nq_stream_t stream) {
  if (!a || !b || !sse || !sizes_ok(n, H, W)) return NQ_ERR_INVALID;
  const int64_t HW = (int64_t)H * W, FB = HW + HW / 2;
  const int64_t chunks = (FB + SSE_CHUNK - 1) / SSE_CHUNK;
  if (n > 0x7fffffffLL / chunks) return NQ_ERR_UNSUPPORTED;
  const int64_t blocks = n * chunks;
  if (!grid_ok(blocks)) return NQ_ERR_UNSUPPORTED;
  // 16-byte loads need every frame's first byte aligned as the buffers are
  const int vec_ok = FB % 16 == 0 && (reinterpret_cast<uintptr_t>(a) & 15) == 0 && (reinterpret_cast<uintptr_t>(b) & 15) == 0;
  if (hipMemsetAsync(sse, 0, (size_t)n * 3 * sizeof(uint64_t), nq_s(stream)) != hipSuccess) return NQ_ERR_LAUNCH;
  hipLaunchKernelGGL(yuv_sse_kernel, dim3((unsigned)blocks), dim3(TPB), 0, nq_s(stream), a, b,
                     reinterpret_cast<unsigned long long*>(sse), chunks, HW, vec_ok);
  return nq_launch_status();
}

}  // extern "C"

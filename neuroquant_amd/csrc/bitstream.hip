// Packed bit-stream kernels: b-bit quantisation levels <-> 32-bit words, the dequantising unpack a player
// runs once per file, and the float -> 8-bit frame conversion it runs on every decoded frame.
//
// Bit order (the file format): level i occupies bits [i*b, (i+1)*b) of the stream, bit j of the stream is bit j % 32 of
// word j / 32.  32 consecutive levels make exactly b words, so a "group" of 32 levels is the unit of work of the packer:
// one thread owns a group and is the only writer of its b words (no atomics, no shared words).
#include "nq_common.h"

namespace {

constexpr int TPB = 256;

// One thread per group of 32 levels -> n_bits words.  Levels past n read as 0 (zero tail bits); words at or past nwords are
// never written (they would hold only zeros).
__global__ __launch_bounds__(TPB) void pack_levels_kernel(const uint8_t* __restrict__ levels, uint32_t* __restrict__ words,
                                                          int64_t n, int64_t nwords, int n_bits, int vec_ok) {
  const int64_t g = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int64_t first = g * 32;
  if (first >= n) return;
  uint32_t lv[8];   // 32 levels, 4 per dword, little-endian like the byte array
  if (vec_ok && first + 32 <= n) {
    const uint4 a = *reinterpret_cast<const uint4*>(levels + first);
    const uint4 b = *reinterpret_cast<const uint4*>(levels + first + 16);
    lv[0] = a.x; lv[1] = a.y; lv[2] = a.z; lv[3] = a.w;
    lv[4] = b.x; lv[5] = b.y; lv[6] = b.z; lv[7] = b.w;
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      uint32_t d = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t i = first + q * 4 + e;
        if (i < n) d |= (uint32_t)levels[i] << (8 * e);
      }
      lv[q] = d;
    }
  }
  const uint32_t mask = (1u << n_bits) - 1u;
  const int64_t w0 = g * n_bits;
  uint64_t acc = 0;   // pending bits, low `fill` bits valid; fill < 32 before each insert, so fill + n_bits <= 39
  int fill = 0, out = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc |= (uint64_t)((lv[q] >> (8 * e)) & mask) << fill;
      fill += n_bits;
      if (fill >= 32) {
        if (w0 + out < nwords) words[w0 + out] = (uint32_t)acc;
        ++out;
        acc >>= 32;
        fill -= 32;
      }
    }
  }
  // 32 * n_bits bits are a whole number of words: nothing is left in acc here
}

// One thread per element.  A level that straddles a word boundary (shift + n_bits > 32) reads the next word, which then
// holds some of its bits and therefore exists; a level that ends exactly on a boundary does not.
__global__ __launch_bounds__(TPB) void unpack_dequant_kernel(const uint32_t* __restrict__ words, const float* __restrict__ delta,
                                                             const float* __restrict__ zp, float* __restrict__ w, int64_t n,
                                                             int64_t row_len, int n_bits) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const int64_t bit = i * n_bits;
  const int64_t wi = bit >> 5;
  const int sh = (int)(bit & 31);
  uint32_t v = words[wi] >> sh;
  if (sh + n_bits > 32) v |= words[wi + 1] << (32 - sh);
  const float level = (float)(v & ((1u << n_bits) - 1u));
  const int64_t r = i / row_len;
  w[i] = (level - zp[r]) * delta[r];
}

// (uint8) rint(min(max(x, 0), 1) * 255); NaN fails `x > 0` and maps to 0.  rintf rounds to nearest even.
__device__ __forceinline__ uint32_t to_u8(float x) {
  float c = x > 0.f ? x : 0.f;
  c = c < 1.f ? c : 1.f;
  return (uint32_t)rintf(c * 255.0f);
}
__device__ __forceinline__ uint32_t pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return a | (b << 8) | (c << 16) | (d << 24);
}

// Planar layout keeps the element order, so the whole tensor is one flat array: a 16-byte load and a dword store per thread,
// whatever H * W is; the last n % 4 elements go one by one.
__global__ __launch_bounds__(TPB) void frames_u8_flat_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst, int64_t n) {
  const int64_t i = ((int64_t)blockIdx.x * TPB + threadIdx.x) * 4;
  if (i + 4 <= n) {
    const float4 v = *reinterpret_cast<const float4*>(src + i);
    *reinterpret_cast<uint32_t*>(dst + i) = pack4(to_u8(v.x), to_u8(v.y), to_u8(v.z), to_u8(v.w));
  } else {
    for (int64_t j = i; j < n; ++j) dst[j] = (uint8_t)to_u8(src[j]);
  }
}

// Interleaved layout, three channels, H * W a multiple of 4: a thread takes 4 pixels of one frame, one 16-byte load per plane,
// and stores their 12 bytes as 3 dwords (byte offset (f * HW + p) * 3 is then a multiple of 4).
__global__ __launch_bounds__(TPB) void frames_u8_hwc3_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst,
                                                             int64_t quads, int64_t HW) {
  const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= quads) return;
  const int64_t q_per_frame = HW >> 2;
  const int64_t f = t / q_per_frame, p = (t - f * q_per_frame) * 4;
  const float* s = src + f * 3 * HW + p;
  const float4 r = *reinterpret_cast<const float4*>(s);
  const float4 g = *reinterpret_cast<const float4*>(s + HW);
  const float4 b = *reinterpret_cast<const float4*>(s + 2 * HW);
  uint32_t* d = reinterpret_cast<uint32_t*>(dst + (f * HW + p) * 3);
  d[0] = pack4(to_u8(r.x), to_u8(g.x), to_u8(b.x), to_u8(r.y));
  d[1] = pack4(to_u8(g.y), to_u8(b.y), to_u8(r.z), to_u8(g.z));
  d[2] = pack4(to_u8(b.z), to_u8(r.w), to_u8(g.w), to_u8(b.w));
}

// Interleaved layout, any channel count and any H * W (planes and pixels not dword-aligned): one thread per output byte.
__global__ __launch_bounds__(TPB) void frames_u8_hwc_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst, int64_t total,
                                                            int C, int64_t HW) {
  const int64_t o = (int64_t)blockIdx.x * TPB + threadIdx.x;   // o = (f * HW + p) * C + c
  if (o >= total) return;
  const int64_t fp = o / C;
  const int c = (int)(o - fp * C);
  const int64_t f = fp / HW, p = fp - f * HW;
  dst[o] = (uint8_t)to_u8(src[(f * C + c) * HW + p]);
}

inline bool grid_ok(int64_t blocks) { return blocks > 0 && blocks <= 0x7fffffffLL; }

}  // namespace

extern "C" {

int64_t nq_packed_words(int64_t n, int n_bits) {
  if (n <= 0 || n_bits < 1 || n_bits > 8) return 0;
  if (n > (INT64_MAX - 31) / n_bits) return 0;
  return (n * n_bits + 31) / 32;
}

int nq_pack_levels(const uint8_t* levels, uint32_t* words, int64_t n, int n_bits, nq_stream_t stream) {
  if (!levels || !words || n <= 0 || n_bits < 1 || n_bits > 8) return NQ_ERR_INVALID;
  const int64_t nwords = nq_packed_words(n, n_bits);
  if (nwords <= 0) return NQ_ERR_INVALID;
  const int64_t groups = (n + 31) / 32, blocks = (groups + TPB - 1) / TPB;
  if (!grid_ok(blocks)) return NQ_ERR_UNSUPPORTED;
  const int vec_ok = (reinterpret_cast<uintptr_t>(levels) & 15) == 0;
  hipLaunchKernelGGL(pack_levels_kernel, dim3((unsigned)blocks), dim3(TPB), 0, nq_s(stream), levels, words, n, nwords, n_bits,
                     vec_ok);
  return nq_launch_status();
}

int nq_unpack_dequant(const uint32_t* words, const float* delta, const float* zp, float* w, int64_t rows, int64_t row_len,
                      int n_bits, nq_stream_t stream) {
  if (!words || !delta || !zp || !w || rows <= 0 || row_len <= 0 || n_bits < 1 || n_bits > 8) return NQ_ERR_INVALID;
  if (rows > INT64_MAX / row_len) return NQ_ERR_INVALID;
  const int64_t n = rows * row_len;
  if (nq_packed_words(n, n_bits) <= 0) return NQ_ERR_INVALID;
  const int64_t blocks = (n + TPB - 1) / TPB;
  if (!grid_ok(blocks)) return NQ_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(unpack_dequant_kernel, dim3((unsigned)blocks), dim3(TPB), 0, nq_s(stream), words, delta, zp, w, n, row_len,
                     n_bits);
  return nq_launch_status();
}

int nq_frames_to_u8(const float* src, uint8_t* dst, int64_t n, int C, int64_t HW, int layout, nq_stream_t stream) {
  if (!src || !dst || n <= 0 || C <= 0 || HW <= 0 || (layout != 0 && layout != 1)) return NQ_ERR_INVALID;
  if (n > INT64_MAX / C || n * C > INT64_MAX / HW) return NQ_ERR_INVALID;
  const int64_t total = n * C * HW;
  const bool aligned = (reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0;
  if ((layout == 0 || C == 1) && aligned) {   // one channel: interleaved is planar
    const int64_t blocks = ((total + 3) / 4 + TPB - 1) / TPB;
    if (!grid_ok(blocks)) return NQ_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(frames_u8_flat_kernel, dim3((unsigned)blocks), dim3(TPB), 0, nq_s(stream), src, dst, total);
  } else if (layout == 1 && C == 3 && HW % 4 == 0 && aligned) {
    const int64_t quads = total / 12, blocks = (quads + TPB - 1) / TPB;
    if (!grid_ok(blocks)) return NQ_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(frames_u8_hwc3_kernel, dim3((unsigned)blocks), dim3(TPB), 0, nq_s(stream), src, dst, quads, HW);
  } else {
    // per-byte kernel; with C = 1 its index map is the identity, so it also serves unaligned planar buffers
    const int Ce = layout == 0 ? 1 : C;
    const int64_t HWe = layout == 0 ? C * HW : HW;
    const int64_t blocks = (total + TPB - 1) / TPB;
    if (!grid_ok(blocks)) return NQ_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(frames_u8_hwc_kernel, dim3((unsigned)blocks), dim3(TPB), 0, nq_s(stream), src, dst, total, Ce, HWe);
  }
  return nq_launch_status();
}

}  // extern "C"

// The QAT baselines to the bit stream (the quantisers are defined in include/nq_hip.h above nq_qat_forward and
// not restated here): latent fp32 weights -> the unsigned b-bit symbols a file stores, and stored symbols -> the weight the
// decoder reads, for ALL weight tensors of a decoder in one call.
//
//   nq_qat_levels    w -> symbols, as the 32-bit words of the packed layout (§11.1, what nq_pack_levels writes) straight from w
//                    -- no symbol tensor in between -- or as one byte per symbol (for the rANS coders); hinerv: + s_c, fp32
//   nq_qat_restore   packed words or byte symbols (+ s_c) -> fp32 weights, equal to nq_qat_forward's noise-off output
//
// Split of the work, the same in both directions.  Symbol i occupies bits [i b, (i + 1) b) of the stream, so the stream falls
// into RUNS of lcm(b, 32) bits that start and end on a symbol boundary AND on a word boundary: 32 / g symbols in b / g words,
// g = gcd(b, 32) (b = 2, 4, 8: one word of 16, 8, 4 symbols; b = 6: 16 symbols in 3 words; b = 3, 5, 7: 32 symbols in b
// words).  One thread owns one run: it is the only reader / writer of its words and of its 16 or 32 (b = 4, 8: 8 or 4)
// weights, which lie side by side: 16-byte accesses where the tensor is 16-byte aligned (a run is 16, 32, 64 or 128 bytes of
// weights and starts at a multiple of that), scalar ones otherwise and in the last, partial run of a tensor, whose missing
// symbols are zero bits, as the existing packer pads them.  The bit width is a template argument under a switch on the
// segment's, so the shift-and-merge of a run is straight-line code on registers.
//   hinerv: the column of element e is e mod K.  A workgroup's 256 runs are consecutive elements, so its columns are one
// cyclic window of min(elements, K) <= 8192 scales: staged ONCE in LDS (32 KB), read from there per element with an index
// that is incremented and wrapped, never divided.  nq_qat_levels first runs the column-statistics launch of the forward
// itself (nq_qat_column_stats of qat.hip: one copy of that arithmetic) into the caller's workspace; the workgroup whose
// window holds an element of row 0 writes that column's s_c out, so every s_c has one writer.
// No atomics, nothing allocated on the device, no host read, bit-identical from call to call.  Compiled like qat.hip.
#include "qat_elem.h"
#include "seg_table.h"

#include <vector>

namespace {

constexpr int TPB = 256;
constexpr int MAX_RUN = 32;                    // symbols of the longest run
constexpr int WINDOW = TPB * MAX_RUN;          // scales a workgroup stages at most

struct SSeg {
  float* w;              // levels: read; restore: written
  uint32_t* words;       // FORM packed
  uint8_t* bytes;        // FORM symbols
  float* scale;          // hinerv: the file's s_c (levels: written; restore: read)
  const float* s_c;      // hinerv levels: s_c of the column launch (workspace)
  unsigned n, nwords;    // Cout K < 2^31 and its packed words
  int K, bits;
  int vec, al4;          // w 16-byte aligned; bytes 4-byte aligned
};
using Table = NqSegTable<SSeg, 16>;

__host__ __device__ __forceinline__ int run_symbols(int bits) { return 32 / (bits & -bits); }   // bits <= 8: gcd(bits, 32) = its lowest set bit

// the workgroup's cyclic window of column scales -> LDS; `src` has K entries.  -> the window's length
__device__ __forceinline__ unsigned stage_scales(const SSeg& s, const float* src, unsigned first, float* lds, bool write_out) {
  const unsigned span = s.n - first < (unsigned)(TPB * run_symbols(s.bits)) ? s.n - first : (unsigned)(TPB * run_symbols(s.bits));
  const unsigned K = (unsigned)s.K, len = span < K ? span : K;
  unsigned c = (first + threadIdx.x) % K;
  const unsigned hop = TPB % K;
  for (unsigned j = threadIdx.x; j < len; j += TPB) {
    const float v = src[c];
    lds[j] = v;
    if (write_out && first + j < K) s.scale[c] = v;    // element first + j lies in row 0: the column's one writer
    c += hop;
    if (c >= K) c -= K;
  }
  __syncthreads();
  return len;
}

template <int B>
struct Run {
  static constexpr int G = B & -B, S = 32 / G, W = B / G;   // symbols and words of a run
};

enum Form { PACKED = 0, SYMBOLS = 1 };

// ------------------------------------------------------------------------------------------------------------ w -> symbols
template <int MODE, int FORM, int B>
__device__ __forceinline__ void levels_run(const SSeg& s, unsigned run, unsigned first, const float* lds, unsigned len) {
  constexpr int S = Run<B>::S, W = Run<B>::W;
  const unsigned e0 = run * S;                     // < n + TPB * 32 <= 2^31 + 8192
  if (e0 >= s.n) return;
  const int cnt = s.n - e0 < (unsigned)S ? (int)(s.n - e0) : S;
  float w[S];
  if (s.vec && cnt == S) {
#pragma unroll
    for (int i = 0; i < S; i += 4) {
      const float4 v = *reinterpret_cast<const float4*>(s.w + e0 + i);
      w[i] = v.x, w[i + 1] = v.y, w[i + 2] = v.z, w[i + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < S; ++i) w[i] = i < cnt ? s.w[e0 + i] : 0.f;
  }
  uint32_t sym[S];
  if (MODE == NQ_QAT_FFNERV) {
    constexpr int n = (1 << (B - 1)) - 1;
#pragma unroll
    for (int i = 0; i < S; ++i) {
      const float th = tanhf(w[i]);
      const int q = (int)nq_qat_ff_floor(th, (float)n) * (int)nq_qat_sign(th);   // |q| <= n: |tanh| <= 1
      sym[i] = (uint32_t)(q + n);
    }
  } else {
    unsigned j = (e0 - first) % len;
#pragma unroll
    for (int i = 0; i < S; ++i) {
      sym[i] = (uint32_t)((int)nq_qat_level(w[i], lds[j], B) + (1 << (B - 1)));
      if (++j == len) j = 0;
    }
  }
#pragma unroll
  for (int i = 0; i < S; ++i)
    if (i >= cnt) sym[i] = 0;                      // the zero tail bits of a tensor's last run
  if (FORM == PACKED) {
    const unsigned w0 = run * W;
    uint64_t acc = 0;                              // pending bits, low `fill` valid; fill < 32 before an insert: fill + B <= 39
    int fill = 0, out = 0;
#pragma unroll
    for (int i = 0; i < S; ++i) {
      acc |= (uint64_t)(sym[i] & ((1u << B) - 1u)) << fill;   // a symbol of finite w fits B bits; a NaN's must not reach its neighbours
      fill += B;
      if (fill >= 32) {
        if (w0 + out < s.nwords) s.words[w0 + out] = (uint32_t)acc;   // words past the last hold only tail zeros: not stored
        ++out;
        acc >>= 32;
        fill -= 32;
      }
    }
  } else if (s.al4 && cnt == S) {
#pragma unroll
    for (int i = 0; i < S; i += 4)
      *reinterpret_cast<uint32_t*>(s.bytes + e0 + i) = sym[i] | (sym[i + 1] << 8) | (sym[i + 2] << 16) | (sym[i + 3] << 24);
  } else {
#pragma unroll
    for (int i = 0; i < S; ++i)
      if (i < cnt) s.bytes[e0 + i] = (uint8_t)sym[i];
  }
}

// ------------------------------------------------------------------------------------------------------------ symbols -> w
template <int MODE, int FORM, int B>
__device__ __forceinline__ void restore_run(const SSeg& s, unsigned run, unsigned first, const float* lds, unsigned len) {
  constexpr int S = Run<B>::S, W = Run<B>::W;
  const unsigned e0 = run * S;
  if (e0 >= s.n) return;
  const int cnt = s.n - e0 < (unsigned)S ? (int)(s.n - e0) : S;
  uint32_t sym[S];
  if (FORM == PACKED) {
    const unsigned w0 = run * W;
    uint32_t word[W];
#pragma unroll
    for (int i = 0; i < W; ++i) word[i] = w0 + i < s.nwords ? s.words[w0 + i] : 0u;
    uint64_t acc = 0;                              // low `fill` bits valid; refilled below B bits: fill + 32 <= 39
    int fill = 0, in = 0;
#pragma unroll
    for (int i = 0; i < S; ++i) {
      if (fill < B) {
        acc |= (uint64_t)word[in < W ? in : W - 1] << fill;   // in < W whenever this runs: S B = 32 W bits in all
        ++in;
        fill += 32;
      }
      sym[i] = (uint32_t)acc & ((1u << B) - 1u);
      acc >>= B;
      fill -= B;
    }
  } else if (s.al4 && cnt == S) {
#pragma unroll
    for (int i = 0; i < S; i += 4) {
      const uint32_t d = *reinterpret_cast<const uint32_t*>(s.bytes + e0 + i);
      sym[i] = d & 255u, sym[i + 1] = (d >> 8) & 255u, sym[i + 2] = (d >> 16) & 255u, sym[i + 3] = d >> 24;
    }
  } else {
#pragma unroll
    for (int i = 0; i < S; ++i) sym[i] = i < cnt ? s.bytes[e0 + i] : 0u;
  }
  float y[S];
  if (MODE == NQ_QAT_FFNERV) {
    constexpr int n = (1 << (B - 1)) - 1;
#pragma unroll
    for (int i = 0; i < S; ++i) y[i] = (float)((int)sym[i] - n) / (float)n;
  } else {
    unsigned j = (e0 - first) % len;
#pragma unroll
    for (int i = 0; i < S; ++i) {
      y[i] = (float)((int)sym[i] - (1 << (B - 1))) * lds[j];
      if (++j == len) j = 0;
    }
  }
  if (s.vec && cnt == S) {
#pragma unroll
    for (int i = 0; i < S; i += 4) *reinterpret_cast<float4*>(s.w + e0 + i) = make_float4(y[i], y[i + 1], y[i + 2], y[i + 3]);
  } else {
#pragma unroll
    for (int i = 0; i < S; ++i)
      if (i < cnt) s.w[e0 + i] = y[i];
  }
}

template <int MODE, int FORM, bool RESTORE>
__global__ __launch_bounds__(TPB) void qat_stream_kernel(Table t) {
  __shared__ float lds[MODE == NQ_QAT_HINERV ? WINDOW : 1];
  int local;
  const SSeg& s = t.s[t.find(blockIdx.x, local)];
  const unsigned run = (unsigned)local * TPB + threadIdx.x;
  const unsigned first = (unsigned)local * TPB * run_symbols(s.bits);   // the workgroup's first element, < n
  unsigned len = 1;
  if (MODE == NQ_QAT_HINERV) len = stage_scales(s, RESTORE ? s.scale : s.s_c, first, lds, !RESTORE);
#define NQ_QAT_RUN(B)                                             \
  case B:                                                         \
    if (RESTORE)                                                  \
      restore_run<MODE, FORM, B>(s, run, first, lds, len);        \
    else                                                          \
      levels_run<MODE, FORM, B>(s, run, first, lds, len);         \
    break;
  switch (s.bits) {
    NQ_QAT_RUN(2) NQ_QAT_RUN(3) NQ_QAT_RUN(4) NQ_QAT_RUN(5) NQ_QAT_RUN(6) NQ_QAT_RUN(7) NQ_QAT_RUN(8)
  }
#undef NQ_QAT_RUN
}

inline bool misaligned(const void* p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// everything the entries refuse, before the device is touched: what nq_qat_forward refuses, for this segment type
bool segs_ok(const nq_qat_stream_seg* segs, int nseg, int mode, int form) {
  if (!segs || nseg <= 0 || (mode != NQ_QAT_FFNERV && mode != NQ_QAT_HINERV) || (form != NQ_QAT_PACKED && form != NQ_QAT_SYMBOLS))
    return false;
  for (int i = 0; i < nseg; ++i) {
    const nq_qat_stream_seg& h = segs[i];
    if (!h.w || !h.stored || h.bits < 2 || h.bits > 8 || h.Cout <= 0 || h.K <= 0) return false;
    if ((int64_t)h.Cout * h.K > 0x7fffffffLL) return false;
    if (misaligned(h.w, 3u) || (form == NQ_QAT_PACKED && misaligned(h.stored, 3u))) return false;
    if (mode == NQ_QAT_HINERV && (!h.scale || misaligned(h.scale, 3u))) return false;
  }
  return true;
}

template <bool RESTORE>
int run(const nq_qat_stream_seg* segs, int nseg, int mode, int form, float* ws, hipStream_t st) {
  if (!segs_ok(segs, nseg, mode, form)) return NQ_ERR_INVALID;
  const bool hi = mode == NQ_QAT_HINERV;
  if (hi && !RESTORE) {   // s_c by the forward's own column launch, into the forward's workspace layout
    if (!ws || misaligned(ws, 15u)) return NQ_ERR_INVALID;
    std::vector<nq_qat_seg> fwd(nseg);
    for (int i = 0; i < nseg; ++i) fwd[i] = nq_qat_seg{segs[i].w, nullptr, segs[i].w, segs[i].Cout, segs[i].K, segs[i].bits, i};
    if (int rc = nq_qat_column_stats(fwd.data(), nseg, ws, st)) return rc;
  }
  return Table::launch_all(
      segs, nseg,
      [&](int i, SSeg& d) {
        int64_t k0 = 0;
        for (int j = 0; j < i; ++j) k0 += segs[j].K;
        const nq_qat_stream_seg& h = segs[i];
        const int64_t n = (int64_t)h.Cout * h.K;
        d = SSeg{h.w, static_cast<uint32_t*>(h.stored), static_cast<uint8_t*>(h.stored), hi ? h.scale : nullptr,
                 hi && !RESTORE ? ws + 4 * k0 : nullptr, (unsigned)n, (unsigned)nq_packed_words(n, h.bits), h.K, h.bits,
                 !misaligned(h.w, 15u), !misaligned(h.stored, 3u)};
        const int64_t runs = (n + run_symbols(h.bits) - 1) / run_symbols(h.bits);
        return (runs + TPB - 1) / TPB;
      },
      [&](const Table& t, unsigned blocks) {
        const dim3 grid(blocks), block(TPB);
#define NQ_QAT_LAUNCH(M, F) hipLaunchKernelGGL((qat_stream_kernel<M, F, RESTORE>), grid, block, 0, st, t)
        if (!hi && form == NQ_QAT_PACKED) NQ_QAT_LAUNCH(NQ_QAT_FFNERV, PACKED);
        if (!hi && form == NQ_QAT_SYMBOLS) NQ_QAT_LAUNCH(NQ_QAT_FFNERV, SYMBOLS);
        if (hi && form == NQ_QAT_PACKED) NQ_QAT_LAUNCH(NQ_QAT_HINERV, PACKED);
        if (hi && form == NQ_QAT_SYMBOLS) NQ_QAT_LAUNCH(NQ_QAT_HINERV, SYMBOLS);
#undef NQ_QAT_LAUNCH
      });
}

}  // namespace

extern "C" {

int nq_qat_levels(const nq_qat_stream_seg* segs, int nseg, int mode, int form, float* ws, nq_stream_t stream) {
  return run<false>(segs, nseg, mode, form, ws, nq_s(stream));
}

int nq_qat_restore(const nq_qat_stream_seg* segs, int nseg, int mode, int form, nq_stream_t stream) {
  return run<true>(segs, nseg, mode, form, nullptr, nq_s(stream));
}

}  // extern "C"

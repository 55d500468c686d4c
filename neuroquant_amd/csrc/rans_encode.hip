// Entropy-coded levels: the ENCODER of the 64-lane interleaved rANS code rans.hip decodes.  The code is
// §12.1's and nothing else: probabilities f[s] in units of 1 / 4096, 32-bit states that start at 2^16, 16-bit words; a symbol
// s first emits x & 0xffff (x >>= 16) when x >= f[s] << 20, then x = ((x / f[s]) << 12) + x % f[s] + cum[s].  The bytes equal
// bitstream.rans_encode's.
//
// Five launches, nothing allocated, no global atomics, every count an integer:
//   (1) rans_hist_kernel    levels -> one partial histogram per workgroup (LDS counters, 8 copies per wavefront);
//   (2) rans_table_kernel   one workgroup: the partials added in a fixed order, then the three integer steps of the
//                           normalisation rule -> freq;
//   (3) rans_encode_kernel  ONE wavefront per chunk, four chunks per workgroup -> 64 final states, the word count, and the
//                           chunk's words at the TAIL of its own scratch region;
//   (4) rans_offsets_kernel one workgroup: offsets = exclusive scan of the counts;
//   (5) rans_compact_kernel every chunk's tail -> words[offsets[c] ...).
//
// (3) is one dependent chain of chunk / 64 steps per wavefront, so it is bound by the latency of a step, not by bandwidth and
// not by arithmetic; everything in it serves to keep memory off that chain:
//   * per symbol ONE 16-byte LDS read {m_lo, m_hi, f, cum}: m = ceil(2^64 / f) turns x / f into a multiply-high (proof at
//     `divide`), built once per workgroup;
//   * the chunk's symbols are staged through LDS in blocks of 1024 (16 steps), one 16-byte load per lane, walking backwards;
//     the block before is requested BEFORE the 16 steps of the current one and waited for after them, so no step waits for
//     a load (one counter, vmcnt, covers loads and stores alike on this architecture: §12.3);
//   * the encoder runs its steps from last to first while the decoder reads words forwards, so the words of a chunk grow
//     DOWNWARDS from the end of its region: a step's emitting lanes take the slots below the cursor in ascending lane order
//     (ballot + mbcnt), the cursor drops by the ballot's population count.  The words go to a ring of 1024 in LDS; whenever
//     512 finished words lie above the cursor they leave as 64 stores of 16 bytes.
// A lane whose symbol does not exist (short last chunk) neither emits nor updates and stores 2^16.  Levels are masked to
// n_bits bits, as in nq_pack_levels.  No index depends on a level or a frequency beyond its masked width: whatever the
// inputs hold, every access stays inside the buffers the caller passed (a symbol costs at most one word whatever f is).
#include "nq_common.h"

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / NQ_WAVE;               // four wavefronts = four chunks per workgroup
constexpr int MAXK = 256;
constexpr uint32_t PROB_BITS = 12;
constexpr uint32_t PROB_SCALE = 1u << PROB_BITS;
constexpr uint32_t STATE_LOW = 1u << 16;
constexpr uint32_t RING = 1024, HALF = RING / 2;   // words; a step adds at most 64 below the cursor
constexpr int BLOCK = 1024, BLOCK_STEPS = BLOCK / 64;   // symbols staged at once: 16 bytes per lane
constexpr int COPIES = 8, NCOPY = WAVES * COPIES;  // histogram copies: lane & 7 picks one of its wavefront's eight
constexpr int TILE = TPB * 16;                     // levels a histogram workgroup takes per round
constexpr int MAX_HIST_BLOCKS = 1024;
constexpr int64_t SLICE = 8192;                    // words a compaction workgroup moves

typedef uint32_t U4 __attribute__((ext_vector_type(4)));
typedef U4 U4A __attribute__((may_alias));           // a 16-byte piece of memory written or read as 16-bit words elsewhere

__device__ __forceinline__ void settle(uint32_t& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void settle(U4& v) {
  uint32_t a = v.x, b = v.y, c = v.z, d = v.w;
  settle(a); settle(b); settle(c); settle(d);
  v = U4{a, b, c, d};
}
// other lanes of the wavefront read what this one wrote to LDS (and the reverse): LDS serves a wavefront's accesses in order,
// the compiler is told to keep that order
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint32_t wave_sum_all(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_max_all(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}

// 16 levels from i0 as four words, a level past the end reads as 0
__device__ __forceinline__ U4 load16(const uint8_t* __restrict__ lv, int64_t i0, int64_t n, bool vec) {
  if (vec && i0 + 16 <= n) return *reinterpret_cast<const U4A*>(lv + i0);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if (i0 + j < n) w[j >> 2] |= (uint32_t)lv[i0 + j] << (8 * (j & 3));
  return U4{w[0], w[1], w[2], w[3]};
}

// ---- (1) partial histograms.  LDS: NCOPY copies of the table with a stride of K + 1 words, so that one level in the eight
// copies of a wavefront falls on eight banks; integer adds, so the order inside a workgroup does not matter ----
__global__ __launch_bounds__(TPB) void rans_hist_kernel(const uint8_t* __restrict__ lv, int64_t n, int K, int vec, int64_t tiles,
                                                        uint32_t* __restrict__ part) {
  __shared__ uint32_t hist[NCOPY * (MAXK + 1)];
  const int tid = threadIdx.x, stride = K + 1;
  for (int i = tid; i < NCOPY * stride; i += TPB) hist[i] = 0u;
  __syncthreads();
  uint32_t* mine = hist + ((tid >> 6) * COPIES + (tid & (COPIES - 1))) * stride;
  const uint32_t mask = (uint32_t)(K - 1);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t i0 = tile * TILE + 16 * tid;
    if (i0 >= n) continue;
    const int64_t left = n - i0;
    const U4 v = load16(lv, i0, n, vec != 0);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (j < left) atomicAdd(mine + ((w[j >> 2] >> (8 * (j & 3))) & mask), 1u);
  }
  __syncthreads();
  for (int s = tid; s < K; s += TPB) {
    uint32_t c = 0u;
#pragma unroll 4
    for (int cp = 0; cp < NCOPY; ++cp) c += hist[cp * stride + s];
    part[(int64_t)blockIdx.x * K + s] = c;
  }
}

// ---- (2) counts and the normalisation rule of §12.1, exactly.  Thread s adds symbol s's partials in workgroup order; then the
// first wavefront holds the table in registers, lane l the symbols l, l + 64, l + 128, l + 192, and runs the two serial parts
// as wave-wide arg-max steps.  "Largest, lowest symbol on ties" is the maximum of the key value << 8 | (255 - s). ----
__global__ __launch_bounds__(TPB) void rans_table_kernel(const uint32_t* __restrict__ part, int nblk, int K, int64_t n,
                                                         uint16_t* __restrict__ freq) {
  __shared__ uint32_t s_c[MAXK], s_f[MAXK];
  const int tid = threadIdx.x;
  uint32_t c = 0u;
  if (tid < K)
    for (int b = 0; b < nblk; ++b) c += part[(int64_t)b * K + tid];
  uint32_t f = 0u;
  if (c > 0u) {
    f = (uint32_t)(((uint64_t)c * PROB_SCALE) / (uint64_t)n);   // c * 4096 < 2^44: formed in 64-bit
    f = f < 1u ? 1u : f;
  }
  s_c[tid] = c;
  s_f[tid] = f;
  __syncthreads();
  if (tid >= NQ_WAVE) return;
  const int lane = tid;
  uint32_t fv[4], cv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    fv[j] = s_f[lane + 64 * j];
    cv[j] = s_c[lane + 64 * j];
  }
  uint32_t sum = wave_sum_all((fv[0] + fv[1]) + (fv[2] + fv[3]));
  // step 2: only the lifts to 1 push the sum past 4096, at most 255 of them
  for (int it = 0; it < MAXK - 1 && sum > PROB_SCALE; ++it) {
    uint32_t key = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t k = (fv[j] << 8) | (uint32_t)(255 - (lane + 64 * j));
      if (fv[j] > 1u && k > key) key = k;
    }
    const uint32_t best = wave_max_all(key);
    if (best == 0u) break;
    const int sb = 255 - (int)(best & 0xffu);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (lane + 64 * j == sb) fv[j] -= 1u;
    sum -= 1u;
  }
  // step 3: the deficit goes to the first largest COUNT (two-word key: the count, then 255 - s)
  uint32_t kc = 0u, ks = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t s2 = (uint32_t)(255 - (lane + 64 * j));
    if (cv[j] > kc || (cv[j] == kc && s2 > ks)) {
      kc = cv[j];
      ks = s2;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t oc = __shfl_xor(kc, o, 64), os = __shfl_xor(ks, o, 64);
    if (oc > kc || (oc == kc && os > ks)) {
      kc = oc;
      ks = os;
    }
  }
  const int sd = 255 - (int)ks;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (lane + 64 * j == sd && sum < PROB_SCALE) fv[j] += PROB_SCALE - sum;
    if (lane + 64 * j < K) freq[lane + 64 * j] = (uint16_t)fv[j];
  }
}

// x / f for every 32-bit x and 2 <= f <= 4096 as floor(x m / 2^64), m = ceil(2^64 / f) (m < 2^64 since f >= 2).
// Proof: m f = 2^64 + e with 0 <= e < f, so x m / 2^64 = x / f + x e / (f 2^64).  Write x = q f + r, 0 <= r < f: the value is
// q + (r + x e / 2^64) / f, and x e < 2^32 * 2^12 = 2^44 makes x e / 2^64 < 2^-20 < 1, so r + x e / 2^64 < (f - 1) + 1 = f
// and the floor is q.  With x < 2^32 the high 64 bits of x m are (x m_hi + hi32(x m_lo)) >> 32: the sum is below 2^64
// ((2^32 - 1)^2 + 2^32 - 1), so this is one 32-bit multiply-high and one 64-bit multiply-add.  f = 1: q = x.
__device__ __forceinline__ uint32_t divide(uint32_t x, uint32_t m_lo, uint32_t m_hi, uint32_t f) {
  const uint64_t t = (uint64_t)x * (uint64_t)m_hi + (uint64_t)__umulhi(x, m_lo);
  return f == 1u ? x : (uint32_t)(t >> 32);
}

// ---- (3) the encoder ----
__global__ __launch_bounds__(TPB) void rans_encode_kernel(const uint8_t* __restrict__ lv, const uint16_t* __restrict__ freq,
                                                          uint32_t* __restrict__ states, uint32_t* __restrict__ counts,
                                                          uint16_t* __restrict__ scratch, int64_t n, int64_t chunks, int64_t chunk,
                                                          int64_t region, int n_sym, int vec) {
  __shared__ U4 s_tab[MAXK];                 // symbol -> {m_lo, m_hi, f, cum}
  __shared__ U4 s_stage[WAVES][64];          // per wavefront: the 1024 symbols of the block it is encoding
  __shared__ U4 s_ring[WAVES][RING / 8];     // per wavefront: the word at region position p sits at p % RING
  __shared__ uint32_t s_wave_total[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // ---- tables: thread s owns symbol s; inclusive prefix sum of the frequencies over the workgroup ----
  const uint32_t f = tid < n_sym ? (uint32_t)freq[tid] : 0u;
  uint32_t inc = f;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  if (lane == 63) s_wave_total[wave] = inc;
  __syncthreads();
  uint32_t before = 0;
  for (int k = 0; k < wave; ++k) before += s_wave_total[k];
  const uint64_t m = f >= 2u ? ~0ull / (uint64_t)f + 1ull : 0ull;   // ceil(2^64 / f): floor((2^64 - 1) / f) + 1 for every f >= 2
  s_tab[tid] = U4{(uint32_t)m, (uint32_t)(m >> 32), f, before + inc - f};
  __syncthreads();

  // ---- one wavefront per chunk (everything below is wave-uniform except the lane's state, symbol and rank) ----
  const int64_t c = (int64_t)blockIdx.x * WAVES + wave;
  if (c >= chunks) return;
  const int64_t base = c * chunk;
  const int64_t cnt = n - base < chunk ? n - base : chunk;
  const int64_t steps = (cnt + 63) >> 6;
  const int64_t nblocks = (steps + BLOCK_STEPS - 1) / BLOCK_STEPS;
  uint16_t* out = scratch + c * region;                        // 16-byte aligned: the region is a multiple of 64 words
  const uint8_t* stage = reinterpret_cast<const uint8_t*>(s_stage[wave]);
  uint16_t* ring = reinterpret_cast<uint16_t*>(s_ring[wave]);
  const uint32_t sym_mask = (uint32_t)(n_sym - 1);
  const uint32_t top = (uint32_t)region;                       // positions count down from the region's end; only their low
                                                               // bits index the ring, so 32 bits of them do
  uint32_t x = STATE_LOW;
  uint32_t emitted = 0u, flushed = 0u;                         // words below the region's end: written / stored (x HALF)

  // 16 bytes per lane of block b; levels past the tensor's end read as 0 (their steps never run)
  auto load_block = [&](int64_t b) { return load16(lv, base + b * BLOCK + 16 * lane, n, vec != 0); };
  // words [region - flushed - HALF, region - flushed) are final: 64 stores of 16 bytes
  auto flush_half = [&]() {
    wave_lds_order();
    const int64_t p = region - (int64_t)flushed - (int64_t)HALF + 8 * lane;
    *reinterpret_cast<U4A*>(out + p) = *reinterpret_cast<const U4A*>(ring + (p & (int64_t)(RING - 1u)));
    flushed += HALF;
    wave_lds_order();
  };

  U4 next = load_block(nblocks - 1);
  settle(next);
  for (int64_t b = nblocks - 1; b >= 0; --b) {
    wave_lds_order();                                          // the steps of the block before have read their symbols
    s_stage[wave][lane] = next;
    wave_lds_order();
    if (b > 0) next = load_block(b - 1);                       // in flight during the steps below
    const int64_t t0 = b * BLOCK_STEPS;
    const int k1 = (int)(steps - t0 < BLOCK_STEPS ? steps - t0 : BLOCK_STEPS);
    for (int k = k1 - 1; k >= 0; --k) {
      const bool active = (t0 + k) * 64 + lane < cnt;
      const U4 e = s_tab[(uint32_t)stage[k * 64 + lane] & sym_mask];
      const uint32_t fs = e.z;
      // f = 4096 (a constant tensor): f << 20 = 2^32, never reached -- hence 64 bits
      const bool emit = active && (uint64_t)x >= ((uint64_t)fs << 20);
      const unsigned long long ballot = __ballot(emit);
      const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
      emitted += (uint32_t)__popcll(ballot);
      if (emit) {
        ring[(top - emitted + rank) & (RING - 1u)] = (uint16_t)x;
        x >>= 16;
      }
      if (active) {
        const uint32_t q = divide(x, e.x, e.y, fs);
        x = (q << PROB_BITS) + (x - q * fs) + e.w;
      }
      if (emitted - flushed >= HALF) flush_half();             // wave-uniform
    }
    if (b > 0) settle(next);
  }
  // what is left in the ring: whole 16-byte pieces from the one that holds the lowest word (the words below it in that
  // piece are inside the region and never read)
  wave_lds_order();
  const int64_t low = (region - (int64_t)emitted) & ~(int64_t)7, end = region - (int64_t)flushed;
  for (int64_t p = low + 8 * lane; p < end; p += 8 * 64)
    *reinterpret_cast<U4A*>(out + p) = *reinterpret_cast<const U4A*>(ring + (p & (int64_t)(RING - 1u)));
  states[c * 64 + lane] = x;
  if (lane == 0) counts[c] = emitted;
}

// ---- (4) offsets[c] = counts[0] + ... + counts[c - 1], offsets[chunks] = the total: one workgroup, 256 chunks per round ----
__global__ __launch_bounds__(TPB) void rans_offsets_kernel(const uint32_t* __restrict__ counts, int64_t chunks,
                                                           uint32_t* __restrict__ offsets) {
  __shared__ uint32_t s_wave_total[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t carry = 0u;
  for (int64_t b0 = 0; b0 < chunks; b0 += TPB) {
    const int64_t i = b0 + tid;
    const uint32_t v = i < chunks ? counts[i] : 0u;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t up = __shfl_up(inc, o, 64);
      if (lane >= o) inc += up;
    }
    if (lane == 63) s_wave_total[wave] = inc;
    __syncthreads();
    uint32_t before = 0u, total = 0u;
    for (int k = 0; k < WAVES; ++k) {
      if (k < wave) before += s_wave_total[k];
      total += s_wave_total[k];
    }
    if (i < chunks) offsets[i] = carry + before + inc - v;
    carry += total;
    __syncthreads();
  }
  if (tid == 0) offsets[chunks] = carry;
}

// ---- (5) chunk c's words, the last offsets[c + 1] - offsets[c] of its region, to their place; one slice per workgroup ----
__global__ __launch_bounds__(TPB) void rans_compact_kernel(const uint16_t* __restrict__ scratch, const uint32_t* __restrict__ offsets,
                                                           uint16_t* __restrict__ words, int64_t region, int64_t slices) {
  const int64_t c = (int64_t)blockIdx.x / slices, sl = (int64_t)blockIdx.x % slices;
  const uint32_t w0 = offsets[c];
  const int64_t cnt = (int64_t)(offsets[c + 1] - w0);
  const uint16_t* src = scratch + c * region + (region - cnt);
  const int64_t i1 = (sl + 1) * SLICE < cnt ? (sl + 1) * SLICE : cnt;
  for (int64_t i = sl * SLICE + threadIdx.x; i < i1; i += TPB) words[(int64_t)w0 + i] = src[i];
}

inline bool grid_ok(int64_t blocks) { return blocks > 0 && blocks <= 0x7fffffffLL; }
inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// where the three parts of the workspace lie; ok = 0 for arguments the entries refuse
struct EncPlan {
  int ok;
  int K, hist_blocks;
  int64_t tiles, chunks, region, counts_off, scratch_off, bytes;
};
inline EncPlan enc_plan(int64_t n, int n_bits, int64_t chunk) {
  EncPlan p{};
  if (n <= 0 || n > 0xffffffffLL || n_bits < 1 || n_bits > 8 || chunk <= 0 || chunk % 64 != 0) return p;
  p.K = 1 << n_bits;
  p.tiles = (n + TILE - 1) / TILE;
  p.hist_blocks = (int)(p.tiles < MAX_HIST_BLOCKS ? p.tiles : MAX_HIST_BLOCKS);
  p.chunks = n / chunk + (n % chunk != 0);
  const int64_t n64 = (n + 63) & ~(int64_t)63;
  p.region = chunk < n64 ? chunk : n64;            // a single chunk longer than the tensor needs no more than the tensor
  p.counts_off = align16((int64_t)p.hist_blocks * p.K * 4);
  p.scratch_off = p.counts_off + align16(p.chunks * 4);
  p.bytes = p.scratch_off + p.chunks * p.region * 2;   // <= 2 (n + region) + the two small parts: far inside int64
  p.ok = 1;
  return p;
}

}  // namespace

extern "C" {

int64_t nq_rans_encode_ws_bytes(int64_t n, int n_bits, int64_t chunk) {
  const EncPlan p = enc_plan(n, n_bits, chunk);
  return p.ok ? p.bytes : 0;
}

int nq_rans_table(const uint8_t* levels, int64_t n, int n_bits, uint16_t* freq, void* ws, int64_t ws_bytes, nq_stream_t stream) {
  if (!levels || !freq || !ws || n <= 0 || n_bits < 1 || n_bits > 8) return NQ_ERR_INVALID;
  if (n > 0xffffffffLL) return NQ_ERR_UNSUPPORTED;   // the counts are 32-bit
  const EncPlan p = enc_plan(n, n_bits, 64);
  if (ws_bytes < p.counts_off || ((uintptr_t)ws & 15) != 0) return NQ_ERR_INVALID;
  uint32_t* part = static_cast<uint32_t*>(ws);
  const int vec = ((uintptr_t)levels & 15) == 0;
  hipLaunchKernelGGL(rans_hist_kernel, dim3((unsigned)p.hist_blocks), dim3(TPB), 0, nq_s(stream), levels, n, p.K, vec, p.tiles, part);
  hipLaunchKernelGGL(rans_table_kernel, dim3(1), dim3(TPB), 0, nq_s(stream), part, p.hist_blocks, p.K, n, freq);
  return nq_launch_status();
}

int nq_rans_encode(const uint8_t* levels, int64_t n, int n_bits, int64_t chunk, const uint16_t* freq, uint32_t* states,
                   uint32_t* offsets, uint16_t* words, void* ws, int64_t ws_bytes, nq_stream_t stream) {
  if (!levels || !freq || !states || !offsets || !words || !ws || n <= 0 || n_bits < 1 || n_bits > 8) return NQ_ERR_INVALID;
  if (chunk <= 0 || chunk % 64 != 0) return NQ_ERR_INVALID;
  if (n > 0xffffffffLL) return NQ_ERR_UNSUPPORTED;   // word offsets are 32-bit and a symbol may cost a word
  const EncPlan p = enc_plan(n, n_bits, chunk);
  if (!p.ok || ws_bytes < p.bytes || ((uintptr_t)ws & 15) != 0) return NQ_ERR_INVALID;
  const int64_t blocks = (p.chunks + WAVES - 1) / WAVES;
  const int64_t slices = (p.region + SLICE - 1) / SLICE;
  if (!grid_ok(blocks) || p.chunks > 0x7fffffffLL / slices) return NQ_ERR_UNSUPPORTED;
  char* base = static_cast<char*>(ws);
  uint32_t* counts = reinterpret_cast<uint32_t*>(base + p.counts_off);
  uint16_t* scratch = reinterpret_cast<uint16_t*>(base + p.scratch_off);
  const int vec = ((uintptr_t)levels & 15) == 0;
  hipLaunchKernelGGL(rans_encode_kernel, dim3((unsigned)blocks), dim3(TPB), 0, nq_s(stream), levels, freq, states, counts, scratch,
                     n, p.chunks, chunk, p.region, p.K, vec);
  hipLaunchKernelGGL(rans_offsets_kernel, dim3(1), dim3(TPB), 0, nq_s(stream), counts, p.chunks, offsets);
  hipLaunchKernelGGL(rans_compact_kernel, dim3((unsigned)(p.chunks * slices)), dim3(TPB), 0, nq_s(stream), scratch, offsets, words,
                     p.region, slices);
  return nq_launch_status();
}

}  // extern "C"

// Entropy-coded levels: the decoder of the 64-lane interleaved rANS code a `.nqv` file may carry in place of
// packed words.  Static model per tensor (one frequency table over its 2^n_bits levels, probabilities in units of 1 / 4096),
// 32-bit states with lower bound 2^16, 16-bit renormalisation words: a symbol moves at most one word per lane.
//
// A tensor of n levels is cut into chunks of `chunk` symbols (a multiple of 64; the last may be short).  ONE wavefront
// decodes one chunk: lane l owns symbols l, l + 64, l + 128, ... of the chunk and carries one state.  Step t:
//     slot = x & 4095;  s = symbol(slot);  x = f[s] * (x >> 12) + slot - cum[s]
// on every lane whose symbol 64 t + l exists, then the lanes left with x < 2^16 take one word each from the chunk's single word
// stream, in ascending lane order from the chunk's cursor: x = (x << 16) | word.  A lane's rank among the lanes that need a
// word is the number of set ballot bits below it (v_mbcnt), the cursor advances by the ballot's population count.  Each step
// stores 64 consecutive outputs.
//
// A chunk is one long dependent chain, so the step is kept free of memory latency (measured: DESIGN.md §12.4):
//   * the three tables of the step are ONE 4096-entry LDS table indexed by the slot, {s, f[s] - 1, slot - cum[s]} in 8 + 12 + 12
//     bits (f = 4096 only when a single symbol owns every slot, hence f - 1): one LDS read, not two dependent ones;
//   * the words come from a ring of 1024 words in LDS that each wavefront keeps for its own stream and refills half by half
//     (512 words, 8 per lane) whenever the cursor has passed a half: a lane reads ring[(cursor + rank) % 1024];
//   * no load from memory is left pending across a step.  On this architecture one counter (vmcnt) covers loads AND stores, and
//     a wait the compiler places at the use of a loaded value inside the loop would also wait for the stores of the step
//     before, every step.  So the values that are loaded rarely (the ring's refill, the scales of a new row) are waited for
//     where they are loaded (`settle`), and the steady-state step waits for LDS only.
//
// Nothing a file holds can make the kernel leave its buffers, PROVIDED the offsets are what the callers check them to be
// (non-decreasing, ending at the word count; ops.rans_decode and the player check before they launch): a word index at or
// past the chunk's own word count reads as 0, the slot table is filled for all 4096 slots whatever the frequencies sum to, and
// every field of an entry is masked to its width.  A damaged stream decodes to garbage, never to a fault.
#include "nq_common.h"

namespace {

constexpr int TPB = 256;            // four wavefronts = four chunks per workgroup; the tables are built once for all four
constexpr int WAVES = TPB / NQ_WAVE;
constexpr int PROB_BITS = 12;
constexpr uint32_t PROB_SCALE = 1u << PROB_BITS;
constexpr uint32_t STATE_LOW = 1u << 16;
constexpr uint32_t RING = 1024, HALF = RING / 2;   // words; a step reads at most 64 past the cursor

// Makes the compiler wait for a loaded value HERE (an empty statement that reads and writes the register) instead of at its
// first use in a later step.
__device__ __forceinline__ void settle(uint32_t& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void settle(float& v) { asm volatile("" : "+v"(v)); }

__global__ __launch_bounds__(TPB) void rans_decode_kernel(const uint16_t* __restrict__ words, const uint32_t* __restrict__ states,
                                                          const uint32_t* __restrict__ offsets, const uint16_t* __restrict__ freq,
                                                          const float* __restrict__ delta, const float* __restrict__ zp,
                                                          uint8_t* __restrict__ levels, float* __restrict__ w, int64_t n,
                                                          int64_t chunks, int64_t chunk, int64_t row_len, int n_sym) {
  __shared__ uint16_t s_ring[WAVES][RING];    // per wavefront: words [wbase, wbase + RING) of its stream at index i % RING
  __shared__ uint32_t s_f[256];               // f[s]
  __shared__ uint32_t s_end[256];             // cum[s] + f[s]: non-decreasing in s
  __shared__ uint32_t s_wave_total[WAVES];
  __shared__ uint32_t s_slot[PROB_SCALE];     // slot -> s | (f[s] - 1) << 8 | (slot - cum[s]) << 20
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
  s_f[tid] = f;
  s_end[tid] = before + inc;
  __syncthreads();
  // slot -> symbol: the first symbol whose end lies above the slot (symbols of frequency 0 share their end with the symbol
  // before them and are never first).  16 slots per thread; slots past the sum of a damaged table map to symbol 0.
#pragma unroll 1
  for (int q = 0; q < (int)PROB_SCALE / TPB; ++q) {
    const uint32_t slot = (uint32_t)(q * TPB + tid);
    int lo = 0, hi = 256;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_end[mid] > slot) hi = mid; else lo = mid + 1;
    }
    const int sym = lo < 256 ? lo : 0;
    const uint32_t fs = s_f[sym], cum = s_end[sym] - fs;
    s_slot[slot] = (uint32_t)sym | (((fs - 1u) & 0xfffu) << 8) | (((slot - cum) & 0xfffu) << 20);
  }
  __syncthreads();

  // ---- one wavefront per chunk (everything below is wave-uniform except the lane's own state) ----
  const int64_t c = (int64_t)blockIdx.x * WAVES + wave;
  if (c >= chunks) return;
  const int64_t base = c * chunk;
  const int64_t cnt = n - base < chunk ? n - base : chunk;
  const uint32_t w0 = offsets[c], w1 = offsets[c + 1];
  const uint64_t nw = w1 > w0 ? w1 - w0 : 0u;
  const uint16_t* cw = words + w0;
  uint16_t* ring = s_ring[wave];
  // words [first, first + HALF) -> their ring slots; 8 words per lane, lanes side by side; past the chunk's own words: 0
  auto fill_half = [&](uint32_t first) {
    uint32_t v[HALF / 64];
#pragma unroll
    for (int k = 0; k < (int)HALF / 64; ++k) {
      const uint64_t i = (uint64_t)first + (uint32_t)(k * 64 + lane);
      v[k] = i < nw ? (uint32_t)cw[i] : 0u;
    }
#pragma unroll
    for (int k = 0; k < (int)HALF / 64; ++k) {
      settle(v[k]);
      ring[(first + (uint32_t)(k * 64 + lane)) & (RING - 1u)] = (uint16_t)v[k];
    }
    // other lanes read these words: LDS serves a wavefront's accesses in order, the compiler is told to keep that order
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  uint32_t x = states[c * 64 + lane];
  settle(x);
  uint32_t cursor = 0, wbase = 0;             // words consumed; first word the ring holds
  fill_half(0u);
  fill_half(HALF);
  // this lane's current element: its row, its column and the row's scales, re-read only when the row changes (a load
  // inside the step would put its latency on the chain)
  int64_t row = 0, col = 0;
  float z = 0.f, d = 0.f;
  if (w) {
    row = (base + lane) / row_len;
    col = (base + lane) - row * row_len;
    if (lane < cnt) {
      z = zp[row];
      d = delta[row];
      settle(z);
      settle(d);
    }
  }
  const int64_t steps = (cnt + 63) >> 6;
  for (int64_t t = 0; t < steps; ++t) {
    const int64_t i = t * 64 + lane;
    const bool active = i < cnt;
    uint32_t s = 0;
    if (active) {
      const uint32_t e = s_slot[x & (PROB_SCALE - 1u)];
      s = e & 0xffu;
      x = (((e >> 8) & 0xfffu) + 1u) * (x >> PROB_BITS) + (e >> 20);
    }
    const bool need = active && x < STATE_LOW;
    const unsigned long long mask = __ballot(need);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    if (need) x = (x << 16) | (uint32_t)ring[(cursor + rank) & (RING - 1u)];
    cursor += (uint32_t)__popcll(mask);
    if (cursor - wbase >= HALF) {                                   // wave-uniform: the first half is spent
      fill_half(wbase + RING);
      wbase += HALF;
    }
    if (active) {
      if (levels) levels[base + i] = (uint8_t)s;
      if (w) w[base + i] = ((float)s - z) * d;
    }
    if (w) {
      col += 64;
      if (col >= row_len) {
        const int64_t q = col / row_len;
        row += q;
        col -= q * row_len;
        if (i + 64 < cnt) {                   // the element this lane decodes next exists, so its row does
          z = zp[row];
          d = delta[row];
          settle(z);
          settle(d);
        }
      }
    }
  }
}

inline bool grid_ok(int64_t blocks) { return blocks > 0 && blocks <= 0x7fffffffLL; }

}  // namespace

extern "C" {

int64_t nq_rans_chunks(int64_t n, int64_t chunk) {
  if (n <= 0 || chunk <= 0 || chunk % 64 != 0) return 0;
  return n / chunk + (n % chunk != 0);
}

int nq_rans_decode(const uint16_t* words, const uint32_t* states, const uint32_t* offsets, const uint16_t* freq, int64_t n,
                   int n_bits, int64_t chunk, const float* delta, const float* zp, int64_t row_len, uint8_t* levels, float* w,
                   nq_stream_t stream) {
  if (!words || !states || !offsets || !freq || n <= 0 || n_bits < 1 || n_bits > 8) return NQ_ERR_INVALID;
  if (chunk <= 0 || chunk % 64 != 0 || row_len <= 0 || (!levels && !w)) return NQ_ERR_INVALID;
  if (w && (!delta || !zp)) return NQ_ERR_INVALID;
  const int64_t chunks = nq_rans_chunks(n, chunk);
  if (chunks <= 0) return NQ_ERR_INVALID;
  if (n > 0xffffffffLL) return NQ_ERR_UNSUPPORTED;   // word offsets are 32-bit and a symbol may cost a word
  const int64_t blocks = (chunks + WAVES - 1) / WAVES;
  if (!grid_ok(blocks)) return NQ_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(rans_decode_kernel, dim3((unsigned)blocks), dim3(TPB), 0, nq_s(stream), words, states, offsets, freq, delta, zp,
                     levels, w, n, chunks, chunk, row_len, 1 << n_bits);
  return nq_launch_status();
}

}  // extern "C"

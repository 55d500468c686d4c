// Global unstructured magnitude pruning (the definition is in include/nq_hip.h above nq_magnitude_select): an
// exact radix select of the k-th smallest magnitude over a LIST of tensors, the keep-mask with ties broken in the stable order
// (magnitude, segment, index), and the masked write of +0 into weights, gradients and Adam moments.  No global atomics, no
// host read, nothing allocated, every count an integer: bit-identical from call to call and capturable in a hipGraph.
//
// NaN: the order is on the pattern bits(w) & 0x7fffffff, so a NaN (pattern above 0x7f800000) sorts behind every finite value and
// behind the infinities; it still takes a rank, but nq_prune_mask keeps it whatever k says -- a NaN is never pruned.
//
// The index space.  The segments are laid end to end with every segment starting on a multiple of 64 slots: slot v of the
// "virtual" space is element v - 64 word0[s] of the segment s that owns mask word v / 64; the slots behind a segment's last
// element are padding (pattern PAD: counted nowhere, mask bit 0).  The order of the slots IS the order (segment, index).  The
// segment table is seg_table.h's, with a "block" read as one 64-slot wave block = one mask word: blk0[s] is the segment's first
// word, find() gives a slot its segment.  A workgroup owns RUN consecutive slots whatever lies in them (a run crosses segment
// boundaries); wave w of it owns the w-th quarter, as CHUNKS chunks of 256 slots: lane l holds slots 4 l .. 4 l + 3 of a chunk
// (one 16-byte load where the tensor is aligned and the four elements exist; scalar loads at a tail and in unaligned tensors).
#include "nq_common.h"
#include "seg_table.h"

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int RUN = 4096;                 // slots per workgroup (nq_prune_run() tells the tests)
constexpr int WRUN = RUN / WAVES;         // slots per wave
constexpr int CHUNKS = WRUN / 256;        // 16-byte loads per lane
constexpr int COPIES = 8;                 // histogram copies per wave: lane & 7 picks one
constexpr int NCOPY = WAVES * COPIES;
constexpr int HSTRIDE = 257;              // words between copies: one bin of a wave's 8 copies lies in 8 different banks
constexpr int ONE_TPB = 1024;             // the one-workgroup launches
constexpr uint32_t PAD = 0xffffffffu;     // a padding slot; no magnitude pattern has bit 31
constexpr uint32_t INF = 0x7f800000u;
constexpr int MAX_WORDS = 1 << 25;        // 2^31 slots

struct PruneSegD {
  float* w;
  float* c[3];     // companions (nq_prune_apply only)
  int64_t n;
  int vec;         // bit 0: w is 16-byte aligned; bits 1..3: the companions
};
using PruneTable = NqSegTable<PruneSegD>;

typedef uint32_t U4 __attribute__((ext_vector_type(4)));
typedef float V4 __attribute__((ext_vector_type(4)));

// segment and first element of the 4 slots from v0 (a multiple of 4); false behind the last word
__device__ __forceinline__ bool locate(const PruneTable& t, int64_t v0, int& k, int64_t& i0) {
  const int word = (int)(v0 >> 6);
  if (word >= t.blocks()) return false;
  int local;
  k = t.find(word, local);
  i0 = (int64_t)local * 64 + (int)(v0 & 63);
  return true;
}

// magnitude patterns of the 4 slots from v0, PAD where there is no element
__device__ __forceinline__ void load_mags(const PruneTable& t, int64_t v0, uint32_t (&m)[4]) {
  m[0] = m[1] = m[2] = m[3] = PAD;
  int k;
  int64_t i0;
  if (!locate(t, v0, k, i0)) return;
  const int64_t n = t.s[k].n;
  const uint32_t* __restrict__ p = reinterpret_cast<const uint32_t*>(t.s[k].w);
  if ((t.s[k].vec & 1) && i0 + 3 < n) {
    const U4 q = *reinterpret_cast<const U4*>(p + i0);
    m[0] = q.x & 0x7fffffffu; m[1] = q.y & 0x7fffffffu; m[2] = q.z & 0x7fffffffu; m[3] = q.w & 0x7fffffffu;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i0 + j < n) m[j] = p[i0 + j] & 0x7fffffffu;
  }
}

// first slot of this lane in chunk 0 of its wave
__device__ __forceinline__ int64_t lane_slot0() {
  return (int64_t)blockIdx.x * RUN + (threadIdx.x >> 6) * WRUN + 4 * (threadIdx.x & 63);
}

__device__ __forceinline__ int popc64(uint64_t b) { return __builtin_popcountll(b); }
// bits of b below this lane
__device__ __forceinline__ uint32_t below_lane(uint64_t b) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}
// bit i of the low 16 bits of x -> bit 4 i
__device__ __forceinline__ uint64_t spread16(uint64_t x) {
  x &= 0xffffull;
  x = (x | (x << 24)) & 0x000000ff000000ffull;
  x = (x | (x << 12)) & 0x000f000f000f000full;
  x = (x | (x << 6)) & 0x0303030303030303ull;
  x = (x | (x << 3)) & 0x1111111111111111ull;
  return x;
}

// ---- select, pass `pass` of 4: (a) one 256-bin row per workgroup: digit (m >> shift) & 255 of the elements whose higher digits
// equal the prefix.  A lane merges equal digits that follow each other in its 16 elements into one LDS add: where one bin holds
// nearly everything (the exponent digit of trained weights, magnitude 0 after a first pruning) a lane issues 1 add, not 16.
__global__ __launch_bounds__(TPB) void prune_count_kernel(PruneTable t, int pass, const int64_t* __restrict__ sel,
                                                          uint32_t* __restrict__ rows) {
  __shared__ uint32_t hist[NCOPY * HSTRIDE];
  for (int i = threadIdx.x; i < NCOPY * HSTRIDE; i += TPB) hist[i] = 0;
  __syncthreads();
  uint32_t* mine = hist + ((threadIdx.x >> 6) * COPIES + (threadIdx.x & (COPIES - 1))) * HSTRIDE;
  const int shift = 24 - 8 * pass;
  const uint32_t prefix = pass ? (uint32_t)sel[0] : 0u;
  const uint32_t himask = pass ? (0xffffffffu << (shift + 8)) : 0u;
  const int64_t v0 = lane_slot0();
  uint32_t cur = 0, cnt = 0;
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    uint32_t m[4];
    load_mags(t, v0 + c * 256, m);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (m[j] != PAD && ((m[j] ^ prefix) & himask) == 0) {
        const uint32_t d = (m[j] >> shift) & 255u;
        if (cnt && d != cur) {
          atomicAdd(mine + cur, cnt);
          cnt = 0;
        }
        cur = d;
        ++cnt;
      }
    }
  }
  if (cnt) atomicAdd(mine + cur, cnt);
  __syncthreads();
  if (threadIdx.x < 256) {
    uint32_t c = 0;
#pragma unroll 4
    for (int cp = 0; cp < NCOPY; ++cp) c += hist[cp * HSTRIDE + threadIdx.x];
    rows[(int64_t)blockIdx.x * 256 + threadIdx.x] = c;
  }
}

// (b) one workgroup: the rows summed in workgroup order, the 256 bins scanned, the digit that holds the remaining rank chosen.
// sel[0] prefix, sel[1] remaining rank (after pass 3: r), sel[2] elements below the prefix, sel[3] k clamped to [0, N].
// The element looked for is the one of rank min(k, N - 1): it exists for every k, and r = k - below falls out.
__global__ __launch_bounds__(ONE_TPB) void prune_pick_kernel(const uint32_t* __restrict__ rows, int nblk, int pass, int64_t N,
                                                             const int64_t* __restrict__ k_dev, int64_t* __restrict__ sel) {
  __shared__ int64_t part[ONE_TPB / 256][256];
  __shared__ int64_t scan[2][256];
  const int bin = threadIdx.x & 255, g = threadIdx.x >> 8;
  int64_t prefix = 0, rem, below = 0, kc;
  if (pass == 0) {
    const int64_t k = k_dev[0];
    kc = k < 0 ? 0 : (k > N ? N : k);
    rem = kc < N - 1 ? kc : N - 1;
  } else {   // every thread reads the state before the one write below (behind the barriers)
    prefix = sel[0]; rem = sel[1]; below = sel[2]; kc = sel[3];
  }
  int64_t acc = 0;
  for (int b = g; b < nblk; b += ONE_TPB / 256) acc += rows[(int64_t)b * 256 + bin];
  part[g][bin] = acc;
  __syncthreads();
  int64_t c = 0;
  if (threadIdx.x < 256) {
#pragma unroll
    for (int i = 0; i < ONE_TPB / 256; ++i) c += part[i][bin];
    scan[0][bin] = c;
  }
  __syncthreads();
  int src = 0;
  for (int o = 1; o < 256; o <<= 1) {
    if (threadIdx.x < 256) {
      int64_t v = scan[src][bin];
      if (bin >= o) v += scan[src][bin - o];
      scan[src ^ 1][bin] = v;
    }
    __syncthreads();
    src ^= 1;
  }
  if (threadIdx.x < 256) {
    const int64_t incl = scan[src][bin], excl = incl - c;
    if (excl <= rem && rem < incl) {   // exactly one bin: rem is below the count of the elements under the prefix
      const int64_t nb = below + excl;
      sel[0] = prefix | ((int64_t)bin << (24 - 8 * pass));
      sel[1] = pass == 3 ? kc - nb : rem - excl;
      sel[2] = nb;
      sel[3] = kc;
    }
  }
}

// ---- mask: (a) ties (m == T) per workgroup, in the runs of the select
__global__ __launch_bounds__(TPB) void prune_ties_kernel(PruneTable t, const int64_t* __restrict__ sel, uint32_t* __restrict__ ties) {
  __shared__ uint32_t wc[WAVES];
  const uint32_t T = (uint32_t)sel[0];
  const int64_t v0 = lane_slot0();
  uint32_t cnt = 0;
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    uint32_t m[4];
    load_mags(t, v0 + c * 256, m);
#pragma unroll
    for (int j = 0; j < 4; ++j) cnt += popc64(__ballot(m[j] == T));
  }
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) s += wc[w];
    ties[blockIdx.x] = s;
  }
}

// (b) one workgroup: ties[b] -> ties of the workgroups before b (in place: a thread owns a contiguous stretch)
__global__ __launch_bounds__(ONE_TPB) void prune_scan_kernel(uint32_t* __restrict__ ties, int nblk) {
  __shared__ uint32_t scan[2][ONE_TPB];
  const int per = (nblk + ONE_TPB - 1) / ONE_TPB;
  const int b0 = min(threadIdx.x * per, (unsigned)nblk), b1 = min(b0 + per, nblk);
  uint32_t s = 0;
  for (int b = b0; b < b1; ++b) s += ties[b];
  scan[0][threadIdx.x] = s;
  __syncthreads();
  int src = 0;
  for (int o = 1; o < ONE_TPB; o <<= 1) {
    uint32_t v = scan[src][threadIdx.x];
    if ((int)threadIdx.x >= o) v += scan[src][threadIdx.x - o];
    scan[src ^ 1][threadIdx.x] = v;
    __syncthreads();
    src ^= 1;
  }
  uint32_t run = scan[src][threadIdx.x] - s;
  for (int b = b0; b < b1; ++b) {
    const uint32_t c = ties[b];
    ties[b] = run;
    run += c;
  }
}

// (c) the keep bits.  Tie rank of an element = ties of the workgroups before (base) + of the waves before (LDS) + of the chunks
// before in the wave + of the lanes before in the chunk (mbcnt of the four ballots) + of the lane's own earlier elements.  The
// four keep ballots of a chunk hold slot 4 l + j in bit l of ballot j: spread to every fourth bit they interleave into the four
// mask words of the chunk, which lanes 0..3 store.
__global__ __launch_bounds__(TPB) void prune_mask_kernel(PruneTable t, const int64_t* __restrict__ sel, const uint32_t* __restrict__ base,
                                                         uint64_t* __restrict__ mask) {
  __shared__ uint32_t wc[WAVES];
  const uint32_t T = (uint32_t)sel[0], r = (uint32_t)sel[1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t v0 = lane_slot0();
  uint32_t m[CHUNKS][4];
  uint32_t cnt = 0;
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    load_mags(t, v0 + c * 256, m[c]);
#pragma unroll
    for (int j = 0; j < 4; ++j) cnt += popc64(__ballot(m[c][j] == T));
  }
  if (lane == 0) wc[wave] = cnt;
  __syncthreads();
  uint32_t tb = base[blockIdx.x];
  for (int w = 0; w < wave; ++w) tb += wc[w];
  const int nwords = t.blocks();
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    uint64_t tie[4], keep[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) tie[j] = __ballot(m[c][j] == T);
    uint32_t rank = tb + below_lane(tie[0]) + below_lane(tie[1]) + below_lane(tie[2]) + below_lane(tie[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t v = m[c][j];
      const bool is_tie = v == T;
      const bool kp = v != PAD && (v > T || v > INF || (is_tie && rank >= r));
      rank += is_tie ? 1u : 0u;
      keep[j] = __ballot(kp);
      tb += popc64(tie[j]);
    }
    uint64_t word = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint64_t wq = spread16(keep[0] >> (16 * q)) | (spread16(keep[1] >> (16 * q)) << 1) | (spread16(keep[2] >> (16 * q)) << 2) |
                          (spread16(keep[3] >> (16 * q)) << 3);
      if (lane == q) word = wq;
    }
    const int64_t wi = ((int64_t)blockIdx.x * RUN + wave * WRUN + c * 256) / 64 + lane;
    if (lane < 4 && wi < nwords) mask[wi] = word;
  }
}

// ---- apply: +0 into w and its companions where the mask bit is 0
__device__ __forceinline__ void zero4(float* __restrict__ p, bool vec, int64_t i0, uint32_t kill) {
  if (!p) return;
  if (vec && kill >= 16u) {   // bit 4: all four elements exist
    V4 q = *reinterpret_cast<const V4*>(p + i0);
    if (kill & 1u) q.x = 0.f;
    if (kill & 2u) q.y = 0.f;
    if (kill & 4u) q.z = 0.f;
    if (kill & 8u) q.w = 0.f;
    *reinterpret_cast<V4*>(p + i0) = q;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (kill & (1u << j)) p[i0 + j] = 0.f;
  }
}

__global__ __launch_bounds__(TPB) void prune_apply_kernel(PruneTable t, const uint64_t* __restrict__ mask) {
#pragma unroll
  for (int c = 0; c < RUN / (TPB * 4); ++c) {
    const int64_t v0 = (int64_t)blockIdx.x * RUN + c * (TPB * 4) + 4 * threadIdx.x;
    int k;
    int64_t i0;
    if (!locate(t, v0, k, i0)) continue;
    const int64_t n = t.s[k].n;
    if (i0 >= n) continue;
    const uint32_t exist = n - i0 >= 4 ? 31u : ((1u << (int)(n - i0)) - 1u);   // bit 4 marks "all four"
    const uint32_t keep = (uint32_t)(mask[v0 >> 6] >> (v0 & 63)) & 15u;
    const uint32_t kill = exist & ~keep;
    if (!(kill & 15u)) continue;
    const int vec = t.s[k].vec;
    zero4(t.s[k].w, vec & 1, i0, kill);
    zero4(t.s[k].c[0], vec & 2, i0, kill);
    zero4(t.s[k].c[1], vec & 4, i0, kill);
    zero4(t.s[k].c[2], vec & 8, i0, kill);
  }
}

// the table of a segment list -> NQ_OK, or the code the entries return; N: elements in all
int prune_table(const nq_prune_seg* segs, int nseg, bool companions, PruneTable& t, int64_t& N) {
  if (!segs || nseg <= 0) return NQ_ERR_INVALID;
  if (nseg > 16) return NQ_ERR_UNSUPPORTED;
  t.clear();
  N = 0;
  const int rc = t.fill_all(
      nseg,
      [&](int i, PruneSegD& d) -> int64_t {
        const nq_prune_seg& h = segs[i];
        if (!h.w || ((uintptr_t)h.w & 3) || h.n <= 0 || h.n > (int64_t)MAX_WORDS * 64) return NQ_ERR_INVALID;
        d.w = h.w;
        d.n = h.n;
        d.vec = ((uintptr_t)h.w & 15) == 0 ? 1 : 0;
        for (int j = 0; j < 3; ++j) {
          d.c[j] = companions ? h.c[j] : nullptr;
          if ((uintptr_t)d.c[j] & 3) return NQ_ERR_INVALID;
          if (d.c[j] && ((uintptr_t)d.c[j] & 15) == 0) d.vec |= 2 << j;
        }
        N += h.n;
        return (h.n + 63) / 64;
      },
      [] {});
  if (rc) return rc;
  return t.blocks() > MAX_WORDS ? NQ_ERR_INVALID : NQ_OK;
}

inline int prune_blocks(const PruneTable& t) { return (t.blocks() + RUN / 64 - 1) / (RUN / 64); }

}  // namespace

extern "C" {

int nq_prune_run(void) { return RUN; }

int64_t nq_prune_ws_bytes(const nq_prune_seg* segs, int nseg) {
  PruneTable t;
  int64_t N;
  if (prune_table(segs, nseg, false, t, N)) return 0;
  return (int64_t)prune_blocks(t) * 257 * 4;   // a 256-bin row and one tie count per workgroup
}

int nq_magnitude_select(const nq_prune_seg* segs, int nseg, const int64_t* k_dev, int64_t* sel, void* ws, nq_stream_t stream) {
  PruneTable t;
  int64_t N;
  if (int rc = prune_table(segs, nseg, false, t, N)) return rc;
  if (!k_dev || !sel || !ws || ((uintptr_t)k_dev & 7) || ((uintptr_t)sel & 7) || ((uintptr_t)ws & 3)) return NQ_ERR_INVALID;
  const int nblk = prune_blocks(t);
  uint32_t* rows = static_cast<uint32_t*>(ws);
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(prune_count_kernel, dim3((unsigned)nblk), dim3(TPB), 0, nq_s(stream), t, pass, sel, rows);
    hipLaunchKernelGGL(prune_pick_kernel, dim3(1), dim3(ONE_TPB), 0, nq_s(stream), rows, nblk, pass, N, k_dev, sel);
  }
  return nq_launch_status();
}

int nq_prune_mask(const nq_prune_seg* segs, int nseg, const int64_t* sel, uint64_t* mask, void* ws, nq_stream_t stream) {
  PruneTable t;
  int64_t N;
  if (int rc = prune_table(segs, nseg, false, t, N)) return rc;
  if (!sel || !mask || !ws || ((uintptr_t)sel & 7) || ((uintptr_t)mask & 7) || ((uintptr_t)ws & 3)) return NQ_ERR_INVALID;
  const int nblk = prune_blocks(t);
  uint32_t* ties = static_cast<uint32_t*>(ws) + (int64_t)nblk * 256;
  hipLaunchKernelGGL(prune_ties_kernel, dim3((unsigned)nblk), dim3(TPB), 0, nq_s(stream), t, sel, ties);
  hipLaunchKernelGGL(prune_scan_kernel, dim3(1), dim3(ONE_TPB), 0, nq_s(stream), ties, nblk);
  hipLaunchKernelGGL(prune_mask_kernel, dim3((unsigned)nblk), dim3(TPB), 0, nq_s(stream), t, sel, ties, mask);
  return nq_launch_status();
}

int nq_prune_apply(const nq_prune_seg* segs, int nseg, const uint64_t* mask, nq_stream_t stream) {
  PruneTable t;
  int64_t N;
  if (int rc = prune_table(segs, nseg, true, t, N)) return rc;
  if (!mask || ((uintptr_t)mask & 7)) return NQ_ERR_INVALID;
  hipLaunchKernelGGL(prune_apply_kernel, dim3((unsigned)prune_blocks(t)), dim3(TPB), 0, nq_s(stream), t, mask);
  return nq_launch_status();
}

}  // extern "C"

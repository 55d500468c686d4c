// Quantisation-aware-training weight quantisers (the definition is in include/nq_hip.h above nq_qat_forward):
// QATQuantizer of the reference (quantization/quantizer.py:326-375), round modes 'ffnerv' and 'hinerv', forward and backward
// for ALL weight tensors of a decoder in one call.  The reference runs a dozen small torch ops per tensor and direction
// (tanh / abs / max over axis 0 / div / round / clamp / rand_like / compare ... and their autograd twins).
//
// Launch plan -- a function of the segment list only, so two calls give the same bits:
//   ffnerv  forward   1 launch   elementwise over the concatenated segments
//           backward  1 launch   elementwise, tanh recomputed
//   hinerv  forward   2 launches column statistics {s_c, a(c)} -> workspace; elementwise quantise and mix
//           backward  2 launches column sums of g (1 - m) q [double] -> workspace; elementwise g m + the scale term at a(c)
// A weight (Cout, Cin, k, k) is Cout rows of K = Cin k k columns; elements of a column lie K floats apart.  The column
// kernels put the 64 lanes of a wave along 64 neighbouring columns (every row read is one coalesced 256-byte line) and the
// sixteen waves of a workgroup on sixteen row chunks of that tile; the per-wave results meet in LDS and are combined by wave 0
// in wave order, rows ascending, so a tie goes to the lowest row and a sum has one order whatever the geometry.  The
// elementwise kernels give a thread four neighbouring elements: one 16-byte load and store where the segment's pointers
// allow, scalar accesses otherwise and for the last 1-3 elements.  No atomics, nothing allocated, no host read; `step` is
// read on the device.  Compiled with -ffp-contract=off and IEEE division: the fp32 element arithmetic is the definition's,
// op by op.
//
// The noise mask is Philox-4x32-10 (Salmon et al., SC'11) on counter {e >> 2 low, e >> 2 high, tensor index, step} and key
// {seed low, seed high}; element e takes output word e & 3, so a thread's four elements cost one generator call.
#include "qat_elem.h"
#include "seg_table.h"

#include <cmath>

namespace {

constexpr int TPB = 256;                 // elementwise kernels
constexpr int CTPB = 1024;               // column kernels
constexpr int WAVES = CTPB / 64;         // row chunks of a column tile
constexpr int TILE = 64;                 // columns per workgroup of the column kernels
constexpr int VEC = 4;                   // elements per thread of the elementwise kernels
constexpr int ELEMS = TPB * VEC;

struct QSeg {
  const float* w;
  const float* g;      // backward only
  float* out;          // forward: y, backward: dw
  float* scale;        // workspace of the segment's K columns: s_c
  int* arg;            //                                       a(c)
  double* sum;         //                                       sum_j g_jc (1 - m_jc) q_jc
  unsigned n;          // Cout * K < 2^31
  int Cout, K, bits;
  unsigned index;      // the tensor's word of the generator's counter
  int vec;             // w, g and out are 16-byte aligned
};
using Table = NqSegTable<QSeg, 16>;

struct Rng {
  unsigned k0, k1;     // seed
  const int* step;     // device scalar
  int noise;
};

// m = 1 iff the top 24 bits of the word, as a fraction of 2^24, exceed 0.9f (torch.rand_like(x) > 0.9, quantizer.py:362)
__device__ __forceinline__ float mask_of(unsigned word) { return ((float)(word >> 8) * 5.9604644775390625e-8f > 0.9f) ? 1.f : 0.f; }

// the four masks of elements 4 e4 .. 4 e4 + 3 of tensor `index`
__device__ __forceinline__ void mask4(unsigned e4, unsigned index, const Rng& rng, unsigned step, float (&m)[4]) {
  unsigned r[4];
  nq_philox4x32_10(e4, 0u, index, step, rng.k0, rng.k1, r);
#pragma unroll
  for (int i = 0; i < 4; ++i) m[i] = mask_of(r[i]);
}
__device__ __forceinline__ float mask1(unsigned e, unsigned index, const Rng& rng, unsigned step) {
  unsigned r[4];
  nq_philox4x32_10(e >> 2, 0u, index, step, rng.k0, rng.k1, r);
  const unsigned k = e & 3u;
  return mask_of(k == 0 ? r[0] : k == 1 ? r[1] : k == 2 ? r[2] : r[3]);
}

// the element arithmetic shared with qat_stream.hip (qat_elem.h)
__device__ __forceinline__ float level_of(float w, float s, int bits) { return nq_qat_level(w, s, bits); }
__device__ __forceinline__ float sign_of(float v) { return nq_qat_sign(v); }

// ------------------------------------------------------------------------------------------------------ column kernels
// workgroup `local` of a segment: columns [64 local, 64 local + 64); wave v: rows [v chunk, (v + 1) chunk)
struct Tile {
  int c, r0, r1;
  bool live;
  __device__ __forceinline__ Tile(const QSeg& s, int local) {
    const int chunk = (s.Cout + WAVES - 1) / WAVES, wave = threadIdx.x >> 6;
    c = local * TILE + (threadIdx.x & 63);
    r0 = wave * chunk < s.Cout ? wave * chunk : s.Cout;
    r1 = r0 + chunk < s.Cout ? r0 + chunk : s.Cout;
    live = c < s.K;
  }
};

// hinerv forward, launch 1: s_c = 2 max_i |w_ic| / R + 1e-6 and a(c), the lowest row of the maximum
__global__ __launch_bounds__(CTPB) void qat_colmax_kernel(Table t) {
  __shared__ float smax[WAVES][TILE];
  __shared__ int sarg[WAVES][TILE];
  int local;
  const QSeg& s = t.s[t.find(blockIdx.x, local)];
  const Tile tl(s, local);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float mx = -1.f;   // below every |w|: the first row read is taken; an empty chunk never wins
  int am = 0;
  if (tl.live) {
    const float* p = s.w + (size_t)tl.r0 * s.K + tl.c;
    for (int r = tl.r0; r < tl.r1; ++r, p += s.K) {
      const float v = fabsf(*p);
      if (v > mx) {
        mx = v;
        am = r;
      }
    }
  }
  smax[wave][lane] = mx;
  sarg[wave][lane] = am;
  __syncthreads();
  if (wave == 0 && tl.live) {
#pragma unroll
    for (int v = 1; v < WAVES; ++v) {
      if (smax[v][lane] > mx) {
        mx = smax[v][lane];
        am = sarg[v][lane];
      }
    }
    const float R = (float)((1 << s.bits) - 1);
    s.scale[tl.c] = (2.f * mx) / R + 1e-6f;
    s.arg[tl.c] = am;
  }
}

// hinerv backward, launch 1: sum_j g_jc (1 - m_jc) q_jc in double, rows ascending
__global__ __launch_bounds__(CTPB) void qat_colsum_kernel(Table t, Rng rng) {
  __shared__ double ssum[WAVES][TILE];
  int local;
  const QSeg& s = t.s[t.find(blockIdx.x, local)];
  const Tile tl(s, local);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc = 0.0;
  if (tl.live) {
    const unsigned step = rng.noise ? (unsigned)*rng.step : 0u;
    const float sc = s.scale[tl.c];
    unsigned e = (unsigned)tl.r0 * (unsigned)s.K + (unsigned)tl.c;
    for (int r = tl.r0; r < tl.r1; ++r, e += (unsigned)s.K) {
      const float q = level_of(s.w[e], sc, s.bits);
      const float keep = rng.noise ? 1.f - mask1(e, s.index, rng, step) : 1.f;
      acc += (double)s.g[e] * (double)(keep * q);
    }
  }
  ssum[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && tl.live) {
#pragma unroll
    for (int v = 1; v < WAVES; ++v) acc += ssum[v][lane];
    s.sum[tl.c] = acc;
  }
}

// ------------------------------------------------------------------------------------------------- elementwise kernels
enum Pass { FF_FWD = 0, FF_BWD = 1, HI_FWD = 2, HI_BWD = 3 };

template <int PASS>
__global__ __launch_bounds__(TPB) void qat_elem_kernel(Table t, Rng rng) {
  int local;
  const QSeg& s = t.s[t.find(blockIdx.x, local)];
  const unsigned e0 = ((unsigned)local * TPB + threadIdx.x) * VEC;   // < n + ELEMS <= 2^31 + 1024
  if (e0 >= s.n) return;
  const int cnt = s.n - e0 < (unsigned)VEC ? (int)(s.n - e0) : VEC;
  const bool vec = s.vec && cnt == VEC;
  constexpr bool BWD = PASS == FF_BWD || PASS == HI_BWD;
  float w[VEC] = {0.f, 0.f, 0.f, 0.f}, g[VEC] = {0.f, 0.f, 0.f, 0.f}, y[VEC];
  if (vec) {
    const float4 v = *reinterpret_cast<const float4*>(s.w + e0);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    if (BWD) {
      const float4 u = *reinterpret_cast<const float4*>(s.g + e0);
      g[0] = u.x, g[1] = u.y, g[2] = u.z, g[3] = u.w;
    }
  } else {
    for (int i = 0; i < cnt; ++i) {
      w[i] = s.w[e0 + i];
      if (BWD) g[i] = s.g[e0 + i];
    }
  }
  if (PASS == FF_FWD) {
    const float nl = (float)((1 << (s.bits - 1)) - 1);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const float th = tanhf(w[i]);
      y[i] = (nq_qat_ff_floor(th, nl) / nl) * sign_of(th);
    }
  } else if (PASS == FF_BWD) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const float th = tanhf(w[i]);
      y[i] = g[i] * (1.f - th * th);
    }
  } else {
    float m[VEC] = {0.f, 0.f, 0.f, 0.f};
    if (rng.noise) mask4(e0 >> 2, s.index, rng, (unsigned)*rng.step, m);
    const unsigned K = (unsigned)s.K;
    unsigned row = e0 / K, c = e0 - row * K;
    const double two_over_R = 2.0 / (double)((1 << s.bits) - 1);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      if (i < cnt) {
        if (PASS == HI_FWD) {
          const float sc = s.scale[c];
          const float wq = level_of(w[i], sc, s.bits) * sc;
          y[i] = rng.noise ? w[i] * m[i] + wq * (1.f - m[i]) : wq;
        } else {
          float term = 0.f;
          if ((unsigned)s.arg[c] == row) term = (float)((double)sign_of(w[i]) * two_over_R * s.sum[c]);   // its single owner
          y[i] = g[i] * m[i] + term;
        }
        if (++c == K) {
          c = 0;
          ++row;
        }
      }
    }
  }
  if (vec) {
    *reinterpret_cast<float4*>(s.out + e0) = make_float4(y[0], y[1], y[2], y[3]);
  } else {
    for (int i = 0; i < cnt; ++i) s.out[e0 + i] = y[i];
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// everything the entries refuse, before the device is touched
inline bool segs_ok(const nq_qat_seg* segs, int nseg, int mode, bool bwd, int64_t* columns) {
  if (!segs || nseg <= 0 || (mode != NQ_QAT_FFNERV && mode != NQ_QAT_HINERV)) return false;
  int64_t k = 0;
  for (int i = 0; i < nseg; ++i) {
    const nq_qat_seg& h = segs[i];
    if (!h.w || !h.out || (bwd && !h.g) || h.bits < 2 || h.bits > 8 || h.Cout <= 0 || h.K <= 0 || h.index < 0) return false;
    if ((int64_t)h.Cout * h.K > 0x7fffffffLL) return false;
    if ((reinterpret_cast<uintptr_t>(h.w) | reinterpret_cast<uintptr_t>(h.out) | reinterpret_cast<uintptr_t>(h.g)) & 3u) return false;
    k += h.K;
  }
  *columns = k;
  return true;
}

int run(const nq_qat_seg* segs, int nseg, int mode, int noise, uint64_t seed, const int* step, float* ws, bool bwd, hipStream_t st,
        bool columns_only = false) {
  int64_t columns;
  if (!segs_ok(segs, nseg, mode, bwd, &columns)) return NQ_ERR_INVALID;
  const bool hi = mode == NQ_QAT_HINERV;
  noise = hi && noise;
  if (hi && (!ws || !aligned16(ws) || (noise && !step))) return NQ_ERR_INVALID;
  const Rng rng{(unsigned)seed, (unsigned)(seed >> 32), step, noise};
  // per column of segment i, behind the columns of the segments before it: {s_c, a(c), sum [double]} = 4 floats
  auto fill_seg = [&](int i, QSeg& d) {
    int64_t k0 = 0;
    for (int j = 0; j < i; ++j) k0 += segs[j].K;
    const nq_qat_seg& h = segs[i];
    d = QSeg{h.w, bwd ? h.g : nullptr, h.out, nullptr, nullptr, nullptr, (unsigned)((int64_t)h.Cout * h.K), h.Cout, h.K, h.bits,
             (unsigned)h.index, aligned16(h.w) && aligned16(h.out) && (!bwd || aligned16(h.g))};
    if (hi) {
      d.scale = ws + 4 * k0;
      d.arg = reinterpret_cast<int*>(d.scale + h.K);
      d.sum = reinterpret_cast<double*>(d.scale + 2 * (int64_t)h.K);
    }
  };
  if (hi) {   // the column launch of every chunk of 16 segments, then its elementwise launch: one stream, in order
    int rc = Table::launch_all(
        segs, nseg,
        [&](int i, QSeg& d) {
          fill_seg(i, d);
          return (int64_t)((d.K + TILE - 1) / TILE);
        },
        [&](const Table& t, unsigned blocks) {
          if (bwd)
            hipLaunchKernelGGL(qat_colsum_kernel, dim3(blocks), dim3(CTPB), 0, st, t, rng);
          else
            hipLaunchKernelGGL(qat_colmax_kernel, dim3(blocks), dim3(CTPB), 0, st, t);
        });
    if (rc || columns_only) return rc;
  }
  return Table::launch_all(
      segs, nseg,
      [&](int i, QSeg& d) {
        fill_seg(i, d);
        return (int64_t)(((int64_t)d.n + ELEMS - 1) / ELEMS);
      },
      [&](const Table& t, unsigned blocks) {
        const dim3 grid(blocks), block(TPB);
        if (!hi && !bwd) hipLaunchKernelGGL(qat_elem_kernel<FF_FWD>, grid, block, 0, st, t, rng);
        if (!hi && bwd) hipLaunchKernelGGL(qat_elem_kernel<FF_BWD>, grid, block, 0, st, t, rng);
        if (hi && !bwd) hipLaunchKernelGGL(qat_elem_kernel<HI_FWD>, grid, block, 0, st, t, rng);
        if (hi && bwd) hipLaunchKernelGGL(qat_elem_kernel<HI_BWD>, grid, block, 0, st, t, rng);
      });
}

}  // namespace

int nq_qat_column_stats(const nq_qat_seg* segs, int nseg, float* ws, hipStream_t st) {
  return run(segs, nseg, NQ_QAT_HINERV, 0, 0, nullptr, ws, false, st, true);
}

extern "C" {

int64_t nq_qat_ws_floats(const nq_qat_seg* segs, int nseg, int mode) {
  int64_t columns;
  if (!segs_ok(segs, nseg, mode, false, &columns)) return NQ_ERR_INVALID;
  return mode == NQ_QAT_HINERV ? 4 * columns : 0;
}

int nq_qat_forward(const nq_qat_seg* segs, int nseg, int mode, int noise, uint64_t seed, const int* step, float* ws,
                   nq_stream_t stream) {
  return run(segs, nseg, mode, noise, seed, step, ws, false, nq_s(stream));
}

int nq_qat_backward(const nq_qat_seg* segs, int nseg, int mode, int noise, uint64_t seed, const int* step, float* ws,
                    nq_stream_t stream) {
  return run(segs, nseg, mode, noise, seed, step, ws, true, nq_s(stream));
}

}  // extern "C"

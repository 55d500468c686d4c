// K order of the pre-split bf16x3 weight operand, in ONE place: which (channel, tap) a k-value is, how many k-steps a chunk has,
// what the last chunk looks like, how large the operand is.  nq_weight_layout3 (conv3.hip) writes the operand by these
// functions and the kernels read it by them (conv_igemm3_impl.h at compile time, conv_flat3.hip at run time).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

// Kind of the LAST 16-channel chunk by the channels r it really holds (Conv3Args::tail): 1: r <= 4, 2: r <= 8, 3: r <= 12,
// 0: a full chunk.  A short chunk is laid out (and run) with fewer, denser k-steps: no MFMAs on all-zero k-values.
__host__ __device__ constexpr int wl3_tail_kind(int Cin) {
  const int r = Cin - 16 * ((Cin + 15) / 16 - 1);
  return r <= 4 ? 1 : (r <= 8 ? 2 : (r <= 12 ? 3 : 0));
}
// k-steps (32 k-values each) of a chunk of that kind for KK taps: 13 / 4 / 7 / 10 at k = 5 (element order: wl3_elem below)
__host__ __device__ constexpr int wl3_steps(int KK, int kind) {
  const int half = (KK + 1) / 2;   // (4 channels x 2 taps) slots of a half octet
  return kind == 1 ? (half + 3) / 4 : (kind == 2 ? (KK + 3) / 4 : (kind == 3 ? (KK + half + 3) / 4 : (KK + 1) / 2));
}
// k-steps of the whole operand: every chunk in front of the last one is a full chunk
__host__ __device__ constexpr int64_t wl3_total_steps(int Cin, int KK) {
  return (int64_t)((Cin + 15) / 16 - 1) * wl3_steps(KK, 0) + wl3_steps(KK, wl3_tail_kind(Cin));
}
// 16-byte fragment slots of ONE plane (hi or lo), [k-step][co tile][kq][MT], and the bytes of both
__host__ __device__ constexpr int64_t wl3_plane_slots(int Cin, int KK, int co_tiles, int MT) {
  return wl3_total_steps(Cin, KK) * co_tiles * 4 * MT;
}
__host__ __device__ constexpr int64_t wl3_bytes(int Cin, int KK, int co_tiles, int MT) {
  return wl3_plane_slots(Cin, KK, co_tiles, MT) * 2 * 16;
}

// k-value e (0..7) of lane group kq at k-step s of a 16-channel chunk -> (channel within the chunk, tap); tap >= KK: zero weight.
//   kind 0 full chunk : 2 octets x 2 taps per step          ch = (kq&1)*8 + e, tap = 2s + (kq>>1)
//   kind 2 <= 8 ch    : 1 octet x 4 taps per step           ch = e,            tap = 4s + kq
//   kind 1 <= 4 ch    : slot j = 4s + kq = 4 channels x taps (2j, 2j+1)        ch = e & 3, tap = 2j + (e >> 2)
//   kind 3 <= 12 ch   : slots j < KK: octet 0 at tap j; slots KK + h: channels 8..11 x taps (2h, 2h+1)
__host__ __device__ __forceinline__ void wl3_elem(int kind, int KK, int s, int kq, int e, int& ch, int& tap) {
  const int j = 4 * s + kq;
  if (kind == 2) {
    ch = e;
    tap = j;
  } else if (kind == 1) {
    ch = e & 3;
    tap = 2 * j + (e >> 2);
  } else if (kind == 3) {
    if (j < KK) {
      ch = e;
      tap = j;
    } else {
      ch = 8 + (e & 3);
      tap = 2 * (j - KK) + (e >> 2);
    }
  } else {
    ch = (kq & 1) * 8 + e;
    tap = 2 * s + (kq >> 1);
  }
}

// Launch plan of the few-pixel kernel (nq_conv_flat3_plan, conv_flat3.hip): everything its launch derives from the shape.
// route_fwd3 (conv3.hip) asks for it once per call; the queries read that route and nq_conv_flat3 launches from it.
struct NqFlat3Plan {
  int nw, nb, mi;            // template instantiation: waves per workgroup, 16-pixel blocks and 16-channel blocks per workgroup
  int nsplit, per_split;     // workgroup-level split over 16-channel chunks
  int ngroups, cgroups;      // pixel groups (16*nb pixels) and channel groups (16*mi channels) of the grid
  int ppix;                  // 16-byte units per (plane, octet) of a wave's patch
  int lds_bytes;             // dynamic LDS of the launch: wave-private patches, re-used by the cross-wave reduction
};

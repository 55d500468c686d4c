// The element arithmetic of the QAT weight quantisers (include/nq_hip.h above nq_qat_forward) that qat.hip (the trainer's forward
// and backward) and qat_stream.hip (symbols for the bit stream and the player's restore) share, and the one
// launch they share: the column statistics of 'hinerv'.  Both files are compiled with -ffp-contract=off and IEEE division.
#pragma once
#include "nq_common.h"

#include <cmath>

// hinerv: q = clamp(rint(w / s), -2^(b-1), 2^(b-1) - 1), an integer held as a float
__device__ __forceinline__ float nq_qat_level(float w, float s, int bits) {
  const float hi = (float)((1 << (bits - 1)) - 1), lo = -(float)(1 << (bits - 1));
  return fminf(fmaxf(rintf(w / s), lo), hi);
}
__device__ __forceinline__ float nq_qat_sign(float v) { return (float)((v > 0.f) - (v < 0.f)); }
// ffnerv: floor(|t| n) of t = tanh(w), the integer magnitude the forward divides by n
__device__ __forceinline__ float nq_qat_ff_floor(float th, float nl) { return floorf(fabsf(th) * nl); }

// The column launch of the hinerv forward ALONE (qat.hip): s_c and a(c) of every segment into `ws`, laid out as nq_qat_forward
// lays it out; `out` of a segment is checked like the forward's and never written.  Not exported.
int nq_qat_column_stats(const nq_qat_seg* segs, int nseg, float* ws, hipStream_t st);

// "Several tensors in ONE launch": the segment table that travels as a kernel argument (<= MAXSEG segments, ~1.5 KB), the
// scan by which a workgroup finds its segment, and the host loop that fills, chunks and launches it.  The one copy for
// quant.hip, fwht.hip, conv.hip and conv3.hip.
#pragma once
#include "nq_common.h"

template <class Seg, int MAXSEG = 16>
struct NqSegTable {
  Seg s[MAXSEG];
  int blk0[MAXSEG + 1];   // first workgroup of segment k; blk0[nseg] = workgroups of the launch
  int nseg;

  // segment that owns workgroup `blk` (a short scan of the block prefix); local = the workgroup's number inside it
  __device__ __forceinline__ int find(int blk, int& local) const {
    int k = 0;
    while (k + 1 < nseg && blk >= blk0[k + 1]) ++k;
    local = blk - blk0[k];
    return k;
  }

  void clear() {
    nseg = 0;
    blk0[0] = 0;
  }
  __host__ __device__ __forceinline__ int blocks() const { return blk0[nseg]; }

  // Appends the caller's n segments.  fill(i, seg) writes the device form of host segment i and returns its workgroups, 0
  // when the segment needs none in this table (nothing pending, or the fill sent it elsewhere), or a negative NQ_ERR_*
  // code.  full() is called when a segment needs room in a full table and must leave it empty.
  template <class Fill, class Full>
  int fill_all(int n, Fill fill, Full full) {
    for (int i = 0; i < n; ++i) {
      Seg d;
      const int64_t nb = fill(i, d);
      if (nb < 0) return (int)nb;
      if (nb == 0) continue;
      if (nseg == MAXSEG) full();
      if (blk0[nseg] + nb > 0x7fffffffLL) return NQ_ERR_INVALID;   // grid.x
      s[nseg] = d;
      blk0[nseg + 1] = blk0[nseg] + (int)nb;
      ++nseg;
    }
    return NQ_OK;
  }

  // The whole host side of a multi-tensor entry: launch(table, workgroups) once per MAXSEG segments.  `segs` is the caller's
  // array (only checked here; fill indexes it).
  template <class Fill, class Launch>
  static int launch_all(const void* segs, int n, Fill fill, Launch launch) {
    if (!segs || n <= 0) return NQ_ERR_INVALID;
    NqSegTable t;
    t.clear();
    auto flush = [&]() {
      if (t.nseg) launch(t, (unsigned)t.blocks());
      t.clear();
    };
    if (int rc = t.fill_all(n, fill, flush)) return rc;
    flush();
    return nq_launch_status();
  }
};

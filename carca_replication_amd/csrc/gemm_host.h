// Host helpers of the launchers: the timed launch (every kernel that can bind carca_forward's timing events) and the row
// GEMMs' row-block table (gemm.hip, gemm_stream.hip, gemm_split.hip).
#pragma once
#include <hip/hip_ext.h>
#include "carca_common.h"

// The row-block table of a by-value kernel argument (GemmDev, StreamDev, SplitDev: d, rb_start[], nrb) for blocks of `bm`
// rows: rb_start[0 .. nseg] are the prefix sums, a segment's T < 1 becomes 1.  The entries behind nseg stay as they are
// (zeros) unless pad_tail repeats the total there.  Returns the number of row blocks.
template <class Dev>
static inline int carca_fill_row_blocks(Dev& g, int bm, bool pad_tail = false) {
  int rb = 0;
  for (int s = 0; s < g.d.nseg; ++s) {
    if (g.d.seg[s].T < 1) g.d.seg[s].T = 1;
    g.rb_start[s] = rb;
    rb += (g.d.seg[s].rows + bm - 1) / bm;
  }
  for (int s = g.d.nseg; s <= (pad_tail ? CARCA_MAX_SEGS : g.d.nseg); ++s) g.rb_start[s] = rb;
  g.nrb = rb;
  return rb;
}

// One kernel launch.  timed: this thread's armed timing events, if any, are taken and bound to the launch's own dispatch
// packet (carca_arm_launch_events); a launch that must leave them armed for a later one passes false.
template <class Kernel, class... Args>
static inline void carca_launch(Kernel kernel, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, bool timed,
                                const Args&... args) {
  hipEvent_t e0, e1;
  if (timed && carca_take_launch_events(&e0, &e1))
    hipExtLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, e0, e1, 0, args...);
  else
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, args...);
}

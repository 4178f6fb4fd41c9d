// The R_it draw store (include/seir_hip.h, "R_t intervals on the device"): k_rt_trace_keep is k_rt_trace
// (rt_trace_kernels.h) with one thing more -- every live cell's r of every draw is left in
//   keepR [B][D][M][stride]   fp64, the draw index innermost, stride = the store's cap rounded up to RT_KEEP_RUN,
// at position count[b] (at the kernel's entry; it moves in k_rt_finish, a launch of its own) + the draw's index in the
// launch.  While the store is on it is launched IN PLACE of k_rt_trace: R_it is formed once, by the same inline functions
// (rt_row_factor, rt_cell, rt_combine, rt_period, rt_fold, rt_wave_sum, rt_weighted) in the same order, so fold, national
// partials and the stored r are the bits of k_rt_trace.  Both are wrappers over the one rt_trace_body (rt_trace_kernels.h):
// this one is its RT_SINK_KEEP instance, and the code of the write described below is there.
//
// The write.  A lane owns a column j, so successive draws of its cell are 8 B apart while the lanes of a wave are
// stride x 8 B apart: one store per lane per draw would be 64 separate 8-byte writes.  A thread therefore stages
// RT_KEEP_RUN = 4 consecutive draws of its cell in registers and writes them as one 32-byte run aligned to 32 bytes (two
// 16-byte stores; the store's base and stride keep every run aligned).  A run is cut by positions, not by the launch: the
// first run of a launch that starts off a run boundary and the last run of a launch that ends off one are ragged and go
// out as 8-byte stores of exactly the positions the launch owns.  Nothing is read back, nothing beyond the launch's
// positions is written: a launch of n draws writes B x D x M x n x 8 bytes into the store, whatever the cut.
#pragma once

#include "rt_trace_kernels.h"

namespace seir {

// grid (ncb, ceil(D / DT), B), 256 threads, k_rt_trace's dynamic LDS.  keep [B][D][M][stride], stride % RT_KEEP_RUN == 0.
template <int DT>
__global__ __launch_bounds__(256) void k_rt_trace_keep(Dims d, Consts c, RtBufs rb, const double *__restrict__ tr_theta, int B,
                                                       int first, int count, double *__restrict__ keep, long long stride) {
    rt_trace_body<DT, RT_SINK_KEEP>(d, c, rb, tr_theta, B, first, count, keep, stride);
}

}  // namespace seir

// Which updated row a cell of an E->I-type proposal's own-rows enumeration belongs to (own_rows_delta, sampler_kernels.h):
// host + device, plain C++ for tests/test_move_cells.py.
//
// The cells of such a proposal are numbered row by row: cell = i0 * total_w + pos, i0 < n updated rows (n <= MM, the
// instance's bound on the sub-moves), pos < total_w days of the sub-moves' windows.  i0 = cell / total_w is a run-time
// 32-bit division (30 to 40 instructions) on a path a thread walks once, cold, up to three times per step; with
// i0 < n <= MM the quotient is a count of compares -- one compare and one select at MM = 2, three at MM = 4.
#pragma once

#if defined(__HIPCC__)
#define SEIR_MC_HD __host__ __device__ __forceinline__
#else
#define SEIR_MC_HD inline
#endif

namespace seir {

// cell / total_w for 0 <= cell < n * total_w, 1 <= n <= MM, total_w >= 1 (i * total_w <= 4 x 4 x 1024: no overflow)
template <int MM>
SEIR_MC_HD int cell_row(int cell, int total_w, int n) {
    int i0 = 0;
#pragma unroll
    for (int i = 1; i < MM; ++i) i0 += (i < n && cell >= i * total_w) ? 1 : 0;
    return i0;
}

}  // namespace seir

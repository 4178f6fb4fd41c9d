// Setting one forecast draw against the later observation: the one definition of the verification counts (include/seir_hip.h,
// "Scoring the forecast against later data"), host + device (plain C++ for tests/test_verify_host.py, __device__ for
// k_verify_fold of verify_kernels.h).
//
// Per chain, cell (m, s) and target, over the forecast draws x folded since the forecast's reset, with y the truth:
//     lt      = draws with x <  y                     (uint32)
//     eq      = draws with x == y                     (uint32)
//     abs_sum = sum of |x - y|                        (uint64)
// y < 0 is "no truth": the cell keeps its zeros.  The comparison and the difference are made in int64, so a running total
// past 2^31 is compared as what it is.  Integers only: no result depends on the order of the draws.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SEIR_VU_HD __host__ __device__ __forceinline__
#else
#define SEIR_VU_HD inline
#endif

namespace seir {

SEIR_VU_HD void verify_cell_update(uint32_t &lt, uint32_t &eq, uint64_t &abs_sum, int64_t x, int64_t y) {
    if (y < 0) return;
    lt += x < y ? 1u : 0u;
    eq += x == y ? 1u : 0u;
    abs_sum += x < y ? (uint64_t)y - (uint64_t)x : (uint64_t)x - (uint64_t)y;
}

}  // namespace seir

// Setting one simulated count against the observed one: the one definition of the comparison counts of the in-sample
// check (include/seir_hip.h, "In-sample predictive check on the device"), host + device (plain C++ for
// tests/test_check_host.py, __device__ for the compare kernels of check_kernels.h).
//
// Per chain and cell (m, s), over the draws folded since the last reset:
//     obs = the observed count: the recorded I->R count of the first draw folded   (int32)
//     lt  = draws whose simulated count is  < obs                                   (uint32)
//     eq  = draws whose simulated count is == obs                                   (uint32)
// gt = count - lt - eq is never stored.  The observed count is the data and the same in every draw (no MH kernel targets
// the I->R plane); check_cell_update returns true when a later draw's count differs from the stored one, and the caller keeps
// that flag sticky.  The comparison is then made with the stored value.  Totals (a row over the window, a day over the rows,
// the whole window) are compared by check_total_update.  Integers only: no result depends on the order of the draws.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SEIR_CU_HD __host__ __device__ __forceinline__
#else
#define SEIR_CU_HD inline
#endif

namespace seir {

// One draw's cell: `sim` the simulated count, `seen` the draw's recorded count; `first`: the first draw after a reset, whose
// recorded count becomes obs.  Returns "the data moved".
SEIR_CU_HD bool check_cell_update(int32_t &obs, uint32_t &lt, uint32_t &eq, int32_t sim, int32_t seen, bool first) {
    if (first) obs = seen;
    lt += sim < obs ? 1u : 0u;
    eq += sim == obs ? 1u : 0u;
    return seen != obs;
}

// One draw's total against the observed total.
SEIR_CU_HD void check_total_update(uint32_t &lt, uint32_t &eq, int64_t sim, int64_t obs) {
    lt += sim < obs ? 1u : 0u;
    eq += sim == obs ? 1u : 0u;
}

}  // namespace seir

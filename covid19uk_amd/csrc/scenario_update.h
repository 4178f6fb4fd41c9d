// Setting one scenario rollout against the baseline rollout of the same draw: the one definition of the paired differences
// and of the update of a cell's accumulators (include/seir_hip.h, "Scenario forecasts on the device"), host + device
// (plain C++ for tests/test_scenarios_host.py, __device__ for k_scenario_diff of scenario_kernels.h).  NumPy:
// covid19uk_amd/posterior/scenarios.py.
//
// Per chain, cell (m, s) of the H forecast days and draw, with d_x[s] = k_x^k[m][s] - k_x^0[m][s] the scenario's simulated
// count of transition x (se, ei, ir) minus the baseline's, the SCENARIO_Q = 4 differences are
//     0 cases           d_ir[s]
//     1 cum_cases       sum_{s' <= s} d_ir[s']
//     2 prevalence      I at the START of day s, scenario minus baseline: sum_{s' < s} d_ei[s'] - sum_{s' < s} d_ir[s']
//                       (both rollouts start from the same state at day T, so day 0 is always 0)
//     3 cum_infections  sum_{s' <= s} d_se[s']
// Each fits int32 while the states of both rollouts are populations below 2^31 (a difference of two of them).  Over the
// draws folded since the last reset a cell keeps, per difference, summary_update.h's (ref, sum, sumsq) with its overflow
// test, and the comparison counts of check_update.h against zero:
//     lt = draws whose difference is  < 0     (uint32)
//     eq = draws whose difference is == 0     (uint32)
// gt = count - lt - eq is never stored.  Integers only: no result depends on the order of the draws or of the cells.
#pragma once

#include "summary_update.h"

#if defined(__HIPCC__)
#define SEIR_SC_HD __host__ __device__ __forceinline__
#else
#define SEIR_SC_HD inline
#endif

namespace seir {

constexpr int SCENARIO_Q = 4;    // cases, cum_cases, prevalence, cum_infections

// The four differences of a cell from the day's count differences d (se, ei, ir) and their EXCLUSIVE prefixes ex over the
// days before it.
SEIR_SC_HD void scenario_diff_values(const int32_t (&d)[3], const int32_t (&ex)[3], int32_t (&val)[SCENARIO_Q]) {
    val[0] = d[2];
    val[1] = ex[2] + d[2];
    val[2] = ex[1] - ex[2];
    val[3] = ex[0] + d[0];
}

// One draw's four differences into a cell; `first`: the first draw after a reset, whose values become ref.  Returns the
// overflow test of summary_fold (the caller keeps the flag sticky).
SEIR_SC_HD bool scenario_cell_update(int32_t (&ref)[SCENARIO_Q], int64_t (&sum)[SCENARIO_Q], uint64_t (&sumsq)[SCENARIO_Q],
                                     uint32_t (&lt)[SCENARIO_Q], uint32_t (&eq)[SCENARIO_Q], const int32_t (&val)[SCENARIO_Q],
                                     bool first) {
    bool ovf = false;
    for (int q = 0; q < SCENARIO_Q; ++q) {
        ovf |= summary_fold(ref[q], sum[q], sumsq[q], val[q], first);
        lt[q] += val[q] < 0 ? 1u : 0u;
        eq[q] += val[q] == 0 ? 1u : 0u;
    }
    return ovf;
}

}  // namespace seir

// Folding one kept draw into a cell's running moments: the one definition of the shift, the sums and the overflow test,
// host + device (plain C++ for tests/test_summary_host.py, __device__ for k_summarize of summary_kernels.h).
//
// Per chain, cell (m, t) and quantity q -- in this order k_se, k_ei, k_ir, S, E, I, the state being the one at the start
// of day t (covid19uk_amd.model_spec.compute_state from the context's initial state) -- over the draws x_0 .. x_{n-1}
// folded since the last reset:
//     ref   = x_0                          (int32: the value in the first draw folded)
//     sum   = sum_j (x_j - ref)            (int64)
//     sumsq = sum_j (x_j - ref)^2          (uint64)
// The shift keeps sumsq small (S is ~1e6 with a spread of tens) and makes the host's float64 conversion harmless:
//     mean = ref + sum / n,   var = (sumsq - sum^2 / n) / (n - 1).
// Everything is integer arithmetic: no result depends on the order in which draws or cells are visited.
//
// Overflow is detected, not assumed away: summary_fold returns true when sumsq has reached 2^63 (or wrapped past 2^64).
// While it has not, |sum| <= sumsq < 2^63 fits int64, because |x - ref| <= (x - ref)^2 for integers.  The caller keeps
// the flag sticky; the moments of a sampler whose flag is up are refused (seir_sampler_read_summary).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SEIR_SU_HD __host__ __device__ __forceinline__
#else
#define SEIR_SU_HD inline
#endif

namespace seir {

constexpr int SUMMARY_Q = 6;     // k_se, k_ei, k_ir, S, E, I

// Fold x into (ref, sum, sumsq); `first`: x is the first draw after a reset and becomes ref.  Returns the overflow test.
SEIR_SU_HD bool summary_fold(int32_t &ref, int64_t &sum, uint64_t &sumsq, int32_t x, bool first) {
    if (first) ref = x;
    const int64_t dlt = (int64_t)x - (int64_t)ref;                  // |dlt| <= 2^32 - 1
    const uint32_t a = (uint32_t)(dlt < 0 ? -dlt : dlt);
    const uint64_t sq = (uint64_t)a * (uint64_t)a;                  // < 2^64: one 32 x 32 -> 64 multiply
    const uint64_t before = sumsq;
    sum = (int64_t)((uint64_t)sum + (uint64_t)dlt);                 // wraps only once the flag is up
    sumsq = before + sq;
    return sumsq >= (1ull << 63) || sumsq < before;
}

}  // namespace seir

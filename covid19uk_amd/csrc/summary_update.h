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

// Batch sums for the convergence diagnostics (include/seir_hip.h, "Convergence diagnostics"): the draws folded since the
// reset are cut into batches of L, batch k being draws [kL, (k+1)L).  Per chain, cell and quantity, next to the moments:
//     bsum   = sum of (x_j - ref) over the draws of the batch that is open            (int64)
//     bsumsq = sum over the closed batches of B_k^2, B_k that batch's bsum at its end   (uint64)
// The variance of the B_k is what the batch-means estimate of the autocorrelation time is made of
// (covid19uk_amd/posterior/diagnostics.py); like the moments it is exact integer arithmetic.
//
// summary_batch_add takes the draw AFTER summary_fold has seen it (so that ref is the first draw's value for that draw too).
SEIR_SU_HD void summary_batch_add(int64_t &bsum, int32_t ref, int32_t x) {
    bsum = (int64_t)((uint64_t)bsum + (uint64_t)((int64_t)x - (int64_t)ref));    // wraps only once the moments' flag is up
}

// The draw just added was the last of its batch: bsumsq += bsum^2, bsum = 0.  Returns the overflow test: |bsum| >= 2^32
// (its square does not fit 64 bits: bsumsq is then left as it is), or bsumsq has reached 2^63 or wrapped.  The caller raises
// the same sticky flag as for the moments.
SEIR_SU_HD bool summary_batch_close(int64_t &bsum, uint64_t &bsumsq) {
    const uint64_t a = bsum < 0 ? (uint64_t)0 - (uint64_t)bsum : (uint64_t)bsum;
    bsum = 0;
    if (a >> 32) return true;
    const uint64_t before = bsumsq;
    bsumsq = before + a * a;
    return bsumsq >= (1ull << 63) || bsumsq < before;
}

// Is draw j of a launch (0-based) the last of a batch?  `count` is the number of draws folded before the launch.
SEIR_SU_HD bool summary_batch_closes(uint64_t count, uint64_t j, uint64_t L) { return (count + j + 1) % L == 0; }

}  // namespace seir

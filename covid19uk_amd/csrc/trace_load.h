// Taking one stored count into the burst buffer: the one definition of what a cell of a posterior file's samples/seir may
// hold (include/seir_hip.h, "Stored draws into trace slots"), host + device (plain C++ for tests/test_replay_host.py,
// __device__ for k_trace_load of trace_load_kernels.h), and the layout of the status words.
//
// A cell is fp64 in the file and uint16 or int32 in the trace.  load_classify gives the count to store and a code, the
// first of these that applies:
//     LOAD_NOT_INTEGER   NaN, +-inf, a fractional part, or a magnitude at or above 2^53 (where fp64 has no fractions left
//                        to tell an integer by)
//     LOAD_NEGATIVE      below 0
//     LOAD_OVER_WIDTH    above 65535 (width 16) / above 2^31 - 1 (width 32)
//     LOAD_OK            everything else; -0.0 is 0
// A cell that is not LOAD_OK is stored as 0.  Comparisons and the two conversions only: no floating-point arithmetic.
//
// Beyond the cells, a loaded draw can be wrong in two more ways, which have codes of their own in the key of the first bad
// item: LOAD_NEG_STATE, a compartment S, E or I below zero at a day boundary 1 .. T (load_state_below_zero), and
// LOAD_BAD_THETA, a theta entry that is not finite (load_theta_bad, on the bits).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SEIR_TL_HD __host__ __device__ __forceinline__
#else
#define SEIR_TL_HD inline
#endif

namespace seir {

enum : int { LOAD_OK = 0, LOAD_NOT_INTEGER = 1, LOAD_NEGATIVE = 2, LOAD_OVER_WIDTH = 3, LOAD_NEG_STATE = 4, LOAD_BAD_THETA = 5 };

// seir_sampler_load_status: out[code - 1] counts the items of `code`; then the key of the first bad item and its call
enum : int { LOAD_ST_FIRST_KEY = 5, LOAD_ST_CHAIN = 6, LOAD_ST_FIRST = 7, LOAD_ST_WORDS = 8 };

// The key of a bad item: flat_index * 8 + code.  flat_index is the item's position in the call's arrays: events
// [count][M][T][3] for a cell, the same shape read as (draw, location, boundary - 1, compartment) for a state, theta
// [count][P] for a theta entry.
constexpr int LOAD_KEY_BITS = 43;           // a key is below 2^43 (the host checks); the call's tag lies above
SEIR_TL_HD uint64_t load_key(uint64_t flat_index, int code) { return flat_index * 8u + (uint64_t)code; }

struct LoadCell { int64_t value; int code; };

SEIR_TL_HD LoadCell load_classify(double x, int width) {
    // NaN fails both comparisons
    if (!(x > -9007199254740992.0 && x < 9007199254740992.0)) return {0, LOAD_NOT_INTEGER};
    const int64_t k = (int64_t)x;           // |x| < 2^53: the truncation is exact
    if ((double)k != x) return {0, LOAD_NOT_INTEGER};
    if (k < 0) return {0, LOAD_NEGATIVE};
    if (k > (width == 16 ? (int64_t)65535 : (int64_t)2147483647)) return {0, LOAD_OVER_WIDTH};
    return {k, LOAD_OK};
}

// The state at the boundary behind a day from the initial state and the inclusive sums of the three transitions up to that
// day, in int64: S = S0 - se, E = E0 + se - ei, I = I0 + ei - ir.  A file's counts are bounded by the width only, so the
// sums are not bounded by the population: 1024 days of 2^31 - 1 stay below 2^41.  Returns a bit per compartment below zero.
SEIR_TL_HD int load_state_below_zero(const int64_t (&s0)[3], int64_t se, int64_t ei, int64_t ir) {
    return (s0[0] - se < 0 ? 1 : 0) | (s0[1] + se - ei < 0 ? 2 : 0) | (s0[2] + ei - ir < 0 ? 4 : 0);
}

// A theta entry that is not finite, told by its exponent bits.
SEIR_TL_HD bool load_theta_bad(uint64_t bits) { return ((bits >> 52) & 0x7ffu) == 0x7ffu; }

}  // namespace seir

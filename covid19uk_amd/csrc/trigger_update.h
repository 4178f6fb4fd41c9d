// The step of a triggered scenario's rule: what a review does to one (scenario, location, draw) -- the one definition
// (include/seir_hip.h, "Triggered scenarios on the device"), host + device (plain C++ for tests/test_scenario_triggers_host.py,
// __device__ for k_scenario_trigger_day of scenario_trigger_kernels.h).  NumPy: covid19uk_amd/posterior/scenarios.py,
// trigger_states.
//
// At the start of rollout day s, before the day's rates are formed, with c the sum of the I->R counts of the `window` days
// before the day, and review = s >= from_day && (s - from_day) % review_every == 0:
//     on a review:  if not active and c >= on:                        active <- 1, age <- 0
//                   otherwise, if active and age >= min_days and c < off:   active <- 0
// The day is rolled with the on pair iff active; behind the day, trigger_after_day: if active, age <- age + 1.  So age is the
// number of days already rolled under the measure since it last switched on, and a measure that fires on day s can be released
// on day s + min_days at the earliest.  While not active age is not read (firing sets it), and is kept as it is.
// 0 <= off <= on: a review that fires cannot also release, and on = INT32_MAX never fires (c is a sum of counts of one
// location's recoveries, below 2^31 - 1 for populations below 2^31).  Branch-free: the kernel's lanes differ in every input
// but on, off, min_days and review.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SEIR_TR_HD __host__ __device__ __forceinline__
#else
#define SEIR_TR_HD inline
#endif

namespace seir {

constexpr int TRIGGER_MAX_WINDOW = 28;   // SEIR_TRIGGER_MAX_WINDOW

SEIR_TR_HD void trigger_step(int32_t &active, int32_t &age, int32_t c, int32_t on, int32_t off, int32_t min_days, bool review) {
    const bool fire = review && !active && c >= on;
    const bool release = review && active && age >= min_days && c < off;
    age = fire ? 0 : age;
    active = fire ? 1 : (release ? 0 : active);
}

SEIR_TR_HD void trigger_after_day(int32_t active, int32_t &age) { age += active ? 1 : 0; }

SEIR_TR_HD bool trigger_review(int32_t s, int32_t from_day, int32_t review_every) {
    return s >= from_day && (s - from_day) % review_every == 0;
}

}  // namespace seir

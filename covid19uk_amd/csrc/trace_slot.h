// Which trace slot a sweep is recorded in, if any: the one definition of the thinning rule, host + device (plain C++
// for tests/test_trace_slot.py, __device__ for every trace writer of sampler_kernels.h / moves_kernel.h).
//
// After a trace reset the sweeps are numbered i = 0, 1, 2, ...  With thinning interval k >= 1, sweep i is recorded iff
// (i + 1) % k == 0, in slot first_slot + i / k: the last sweep of every group of k, the rule of
// tfp.mcmc.sample_chain(num_steps_between_results = k - 1), and what the reference's configuration describes
// (example_config.yaml:33 "Thin MCMC samples every 'thin' iterations"; inference.py:455 counts
// num_burst_samples * thin iterations per burst).
//
// One word carries the origin (Chains::slot0, a STATE word):
//     slot0 = sweep_at_reset - first_slot * k          (trace_slot0)
//     j     = sweep - slot0 = i + first_slot * k
//     recorded iff (j + 1) % k == 0, in slot j / k
// k = 1 is slot = sweep - slot0, as before thinning existed, for every input.
//
// The arithmetic is unsigned and wraps with the 32-bit sweep counter.  For k = 1 that is exact; for k > 1 the
// remainder of j is that of i only while sweep - slot0 does not wrap, unless k is a power of two (2^32 is a multiple of
// it).  No run comes near 2^32 sweeps (the pair tokens limit a run to 2^25).
#pragma once

#if defined(__HIPCC__)
#define SEIR_TS_HD __host__ __device__ __forceinline__
#else
#define SEIR_TS_HD inline
#endif

namespace seir {

constexpr unsigned TRACE_NOT_RECORDED = 0xffffffffu;

// slot0 for "the sweep numbered `sweep` is sweep 0 of a burst whose first kept draw goes to slot `first`"
SEIR_TS_HD unsigned trace_slot0(unsigned sweep, unsigned first, unsigned k) { return sweep - first * (k < 1u ? 1u : k); }

// The slot sweep number `sweep` is recorded in, or a value >= cap when it is not recorded (a dropped sweep of a group,
// or a kept one beyond the burst buffer): every writer tests `slot < cap` and skips its stores otherwise.
SEIR_TS_HD unsigned trace_slot(unsigned sweep, unsigned slot0, unsigned k, unsigned cap) {
    const unsigned j = sweep - slot0;
    if (k <= 1u) return j;
    const unsigned q = j / k;
    return (j - q * k == k - 1u && q < cap) ? q : TRACE_NOT_RECORDED;
}

}  // namespace seir

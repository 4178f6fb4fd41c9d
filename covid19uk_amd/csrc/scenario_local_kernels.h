// Targeted scenarios: what-if rollouts whose two operands differ by location (include/seir_hip.h, "Targeted scenarios on the
// device").  It extends scenario_kernels.h and changes nothing of it.
//
// THE definition of a targeted scenario.  Scenario k is two tensors over the M locations and the H forecast days:
//     log_shift[k][m][s]   any finite double
//     commute[k][m][s]     finite and >= 0
// and the rollout of a draw in column (k, nd) is k_scenario_day's -- rollout_day_cell (forecast_kernels.h) -- with its two operands:
//     ea   = exp(base_0[s][nd] + log_shift[k][m][s])     one rounded add, then the same exp
//     psiW = psi * Wk[k][m][s],  Wk[k][m][s] = W[s] * commute[k][m][s]     one rounded multiply, formed on the host
// Everything else is the forecast's: the state at day T, eb, psi, gamma0, gamma1, wd, the Philox key and counter (attempt,
// 64 + transition, s M + m, draw id), the draw id (global chain id << 20) + j, the simulator's device functions and the
// k_gemm<64> contraction over K ndp columns -- common random numbers couple a targeted scenario to the baseline variate by
// variate as they do a global one.  Tensors that are constant over m give bit for bit what seir_sampler_scenarios_set gives
// with the [K][H] arrays: the same rounded add (k_scenario_begin forms it into a plane, here it is formed in the day kernel
// from the same two operands) and the same rounded multiply.
//
// A local commute scales the commuting-borne pressure ON location m -- the psi W F term of its hazard.  It does not scale
// what m exports: F = Cstar . X is one contraction for every scenario.  A symmetric travel ban changes Cstar and is not this.
//
// Layout.  The device tensors are [K][H][M], the transpose of the caller's [K][M][H] (the host transposes at the set): the
// day launch of day s reads, per scenario, ONE contiguous run of M doubles of each tensor (3 KB at UK-380), which the
// workgroups of neighbouring rows share by cache line; with [K][M][H] the same launch would touch M lines H doubles apart
// and use 8 bytes of each.
//
// ndp is a multiple of 64, so the 64 columns of a wave lie in one scenario; a wave has one row.  k, m and s are therefore
// wave-uniform: k comes from blockIdx, m is made uniform for the compiler (readfirstlane), and the two operands are two
// scalar loads per wave and day, not 64 identical vector loads.
//
// The local path has no base[K][H][ndp] plane: the add has moved into the day kernel, which reads the forecast's own
// base_0[s][nd].  k_scenario_local_begin is scenario_begin_planes alone, without k_scenario_begin's write of that plane.
#pragma once

#include "scenario_kernels.h"

namespace seir {

// The operands of a local set next to ScenarioBufs (whose log_shift, Wk and base the local kernels do not read).
struct ScenarioLocalBufs {
    const double *log_shift;       // [K][H][M]
    const double *Wk;              // [K][H][M] W[s] * commute[k][m][s]
};

// grid (ceil(Mp ndp / T), K), T threads: element i of block k's planes (row i / ndp, draw i mod ndp).
template <int T>
__global__ __launch_bounds__(T) void k_scenario_local_begin(Dims d, Consts c, ForecastBufs fb, ScenarioBufs sb, int ND, int ndp) {
    debug_skew(d);
    const size_t i = (size_t)blockIdx.x * T + threadIdx.x;
    const int r = (int)(i / ndp), nd = (int)(i - (size_t)r * ndp);
    scenario_begin_planes(d, c, fb, sb, blockIdx.y, r, nd, ND, ndp);
}

// Forecast day s for every (row, scenario, draw): grid (K ndp / 64, ceil(M / R)), 64 R threads; rollout_day_cell on
// k_scenario_day's planes, with the two operands the row's own.
template <int R>
__global__ __launch_bounds__(64 * R) void k_scenario_local_day(Dims d, Consts c, ForecastBufs fb, ScenarioBufs sb,
                                                               ScenarioLocalBufs lb, int B, int chain0, int j0, int ND, int ndp,
                                                               int s) {
    debug_skew(d);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane, m = blockIdx.y * R + wv;
    const int k = (blockIdx.x * 64) / ndp, nd = col - k * ndp;       // ndp is a multiple of 64: the wave's scenario
    if (nd >= ND || m >= d.M) return;
    const size_t ndk = (size_t)sb.K * ndp;
    const int op = __builtin_amdgcn_readfirstlane((k * fb.H + s) * d.M + m);   // k < 4, H <= 128: below 2^31 for every M
    rollout_day_cell(d, c, fb, sb.St, sb.X, sb.F, (size_t)d.Mp * ndk, (size_t)m * ndk + col, (size_t)m * ndp + nd, nd, m, B,
                     chain0, j0, ndp, s, sb.sev, (size_t)k * ND + nd,
                     [&] { return exp(fb.base[(size_t)s * ndp + nd] + lb.log_shift[op]); },
                     [&](double psi) { return psi * lb.Wk[op]; });
}

}  // namespace seir

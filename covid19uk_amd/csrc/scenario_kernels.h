// Scenario forecasts: what-if rollouts set against the forecast draw by draw (include/seir_hip.h, "Scenario forecasts on
// the device").
//
// THE definition of a scenario.  Up to SEIR_SCENARIO_MAX = 4 scenarios ride on a forecast of H days.  Scenario k is two arrays
// over the forecast days s = 0 .. H-1:
//     log_shift[k][s]   any finite double, added to the log baseline: exp of it is the multiplier on transmission
//     commute[k][s]     finite and >= 0: it multiplies the commuting volume
// and, for every draw the forecast rolls forward, the same rollout with two changes:
//     base_k[s] = base_0[s] + log_shift[k][s]   one rounded add on the forecast's baseline (a_last, plus the walk where on)
//     W_k[s]    = W[s] * commute[k][s]          one rounded multiply
// Everything else is the forecast's (forecast_kernels.h): the state at day T, eb, psi, gamma0, gamma1, wd, the Philox key and
// counter (attempt, 64 + transition, s M + m, draw id), the draw id (global chain id << 20) + j, and the simulator's device
// functions.  A scenario that keeps key and counter is coupled to the baseline variate by variate -- common random numbers --
// so the paired difference of a draw is sharp where two independent rollouts bury a 10 % effect in binomial noise: with
// log_shift = 0 and commute = 1 every difference is 0.  In NumPy: SeirModel.simulate(par, a_path + log_shift[k], spatial,
// W * commute[k], wd, st0, seed, first_draw_id) per chain gives scenario k's counts (covid19uk_amd/posterior/scenarios.py).
//
// k_scenario_diff<U> is the fold of the paired differences: it reads the baseline's staging tensor fev and a scenario's sev,
// both [ND][M][H][3] int32 with nd = slot_in_batch * B + chain (k_forecast_day's layout), forms the SCENARIO_Q differences of
// scenario_update.h per cell (b, m, s) and draw, and folds them into the cell's accumulators.  k_forecast_fold's shape:
//   - a wave per (row, chain), a lane per forecast day, SC_ROWS waves on neighbouring rows per workgroup; 64-day chunks, the
//     prefixes over days by a DPP wave scan per transition inside a chunk and a carry per draw from chunk to chunk (3 ints, LDS;
//     only the owning wave touches it): chunk_excl_scan of summary_kernels.h;
//   - the batch's draws are the INNER loop: a cell's accumulators (4 x 28 B) are loaded before it, held in registers across
//     it and stored after it, so they cross memory once per launch; the loads of U draws (a 12-byte access of each tensor per
//     lane, contiguous over the wave) are issued before the first of them is used.
// Integers only: no result depends on the order of the draws, on the geometry, on debug_skew or on how the draws are cut into
// launches.  An ordinary launch: no hand-off, no persistence.
//
// The rollout rides on the forecast's batch (seir_sampler_forecast, behind the batch's fold, while its planes and its staging
// tensor live).  The scenario axis goes into the COLUMN axis: column c = k ndp + nd, so a forecast day costs one contraction
// and one day launch whatever K is -- the forecast is latency-bound at two launches per day.
//   k_scenario_begin<T>   once per batch, a thread per plane element (grid.y = k): the running state St <- St0 of every
//       column block, X = I0 * invN by forecast_prepare_draws' operation, and base_k = base_0 + log_shift[k] (one rounded
//       add).  St0, eb and sc are read from the forecast's planes of the same batch, which it leaves intact: the T-long event
//       sums are not repeated.
//   k_gemm<64>            per day, unchanged, with Tp := K ndp: F[Mp][K ndp] = Cstar . X.
//   k_scenario_day<R>     per day: k_forecast_day's cell (rollout_day_cell, forecast_kernels.h) on K ndp columns with base_k[s]
//       and W_k[s]; the scalars and eb indexed by nd = c mod ndp, the RNG key built from nd alone; the counts into the staging
//       tensor sev[K][ND][M][H][3].
// Fold and finish of scenario k are k_forecast_fold and k_forecast_finish on k's slice of sev and a MomentBufs of its own.
#pragma once

#include "forecast_kernels.h"
#include "scenario_update.h"

namespace seir {

constexpr int SC_MAX_K = 4;        // SEIR_SCENARIO_MAX
constexpr int SC_ROWS = 8;         // waves (rows) per workgroup
constexpr int SC_JMAX = 128;       // draws per chain and launch (12 KiB of carries)
constexpr int SC_U = 4;            // draws whose loads are in flight together
constexpr int SC_BEGIN_THREADS = 256;
static_assert(SC_JMAX == FC_JMAX, "a batch of the forecast is one launch of the difference fold");

// The planes of the K column blocks of a batch, row stride K ndp (column c = k ndp + nd), and the scenarios themselves.
struct ScenarioBufs {
    int K;
    const double *log_shift;       // [K][H]
    const double *Wk;              // [K][H] W[s] * commute[k][s]
    int *St;                       // [3][Mp][K ndp] running state
    double *X, *F;                 // [Mp][K ndp]
    double *base;                  // [K][H][ndp] log baseline of scenario k on forecast day s
    int *sev;                      // [K][ND][M][H][3] the simulated counts
};

// What a begin kernel does whatever the operands are: the element (row r, draw nd) of column block k's planes, St <- St0 and
// X = I0 * invN by forecast_prepare_draws' operation (zero in the padded rows and draws: the contraction reads them).
__device__ __forceinline__ void scenario_begin_planes(Dims d, Consts c, ForecastBufs fb, ScenarioBufs sb, int k, int r, int nd,
                                                      int ND, int ndp) {
    const size_t ndk = (size_t)sb.K * ndp, fplane = (size_t)d.Mp * ndp, splane = (size_t)d.Mp * ndk;
    if (r < d.Mp) {
        const size_t src = (size_t)r * ndp + nd, dst = (size_t)r * ndk + (size_t)k * ndp + nd;
        const int I = fb.St0[2 * fplane + src];
        sb.St[dst] = fb.St0[src];
        sb.St[splane + dst] = fb.St0[fplane + src];
        sb.St[2 * splane + dst] = I;
        sb.X[dst] = (r < d.M && nd < ND) ? (double)I * c.invN[r] : 0.0;
    }
}

// grid (ceil(max(Mp, H) ndp / T), K), T threads: element i of block k's planes (row i / ndp, draw i mod ndp).
template <int T>
__global__ __launch_bounds__(T) void k_scenario_begin(Dims d, Consts c, ForecastBufs fb, ScenarioBufs sb, int ND, int ndp) {
    debug_skew(d);
    const int k = blockIdx.y, H = fb.H;
    const size_t i = (size_t)blockIdx.x * T + threadIdx.x;
    const int r = (int)(i / ndp), nd = (int)(i - (size_t)r * ndp);
    scenario_begin_planes(d, c, fb, sb, k, r, nd, ND, ndp);
    if (r < H) sb.base[((size_t)k * H + r) * ndp + nd] = nd < ND ? fb.base[(size_t)r * ndp + nd] + sb.log_shift[k * H + r] : 0.0;
}

// Forecast day s for every (row, scenario, draw): grid (K ndp / 64, ceil(M / R)), 64 R threads; rollout_day_cell on column
// c = k ndp + nd of the scenarios' planes, with the column block's baseline and commuting volume.
template <int R>
__global__ __launch_bounds__(64 * R) void k_scenario_day(Dims d, Consts c, ForecastBufs fb, ScenarioBufs sb, int B, int chain0,
                                                         int j0, int ND, int ndp, int s) {
    debug_skew(d);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane, m = blockIdx.y * R + wv;
    const int k = col / ndp, nd = col - k * ndp;
    if (nd >= ND || m >= d.M) return;
    const int H = fb.H;
    const size_t ndk = (size_t)sb.K * ndp;
    rollout_day_cell(d, c, fb, sb.St, sb.X, sb.F, (size_t)d.Mp * ndk, (size_t)m * ndk + col, (size_t)m * ndp + nd, nd, m, B,
                     chain0, j0, ndp, s, sb.sev, (size_t)k * ND + nd,
                     [&] { return exp(sb.base[((size_t)k * H + s) * ndp + nd]); },
                     [&](double psi) { return psi * sb.Wk[k * H + s]; });
}

// A scenario's difference accumulators, [B][M][H][SCENARIO_Q] each.
struct ScenarioDiffBufs {
    int32_t *ref;
    int64_t *sum;
    uint64_t *sumsq;
    uint32_t *lt, *eq;
    unsigned *overflow;            // [1] sticky: some sumsq reached 2^63
};

// grid (ceil(M / SC_ROWS), B), 64 SC_ROWS threads.  1 <= count <= SC_JMAX draws per chain; fresh: they are the first since the
// reset (the accumulators are written, not read, and draw 0 gives ref).  M and H are the call's own, not the context's.
template <int U>
__global__ __launch_bounds__(64 * SC_ROWS) void k_scenario_diff(Dims d, ScenarioDiffBufs o, const int *__restrict__ fev,
                                                                const int *__restrict__ sev, int M, int H, int B, int count,
                                                                int fresh) {
    debug_skew(d);
    __shared__ int carry[SC_ROWS][SC_JMAX][3];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y, m = blockIdx.x * SC_ROWS + wv;
    const bool row_ok = m < M;
    const int mr = row_ok ? m : 0;
    for (int i = lane; i < count * 3; i += 64) (&carry[wv][0][0])[i] = 0;
    __syncthreads();

    bool ovf = false;
    for (int h0 = 0; h0 < H; h0 += 64) {
        const int s = h0 + lane;
        const bool live = row_ok && s < H;
        const int sr = s < H ? s : 0;
        const size_t cell = (((size_t)b * M + mr) * H + sr) * SCENARIO_Q;
        int32_t ref[SCENARIO_Q];
        int64_t sm[SCENARIO_Q];
        uint64_t sq[SCENARIO_Q];
        uint32_t lt[SCENARIO_Q], eq[SCENARIO_Q];
#pragma unroll
        for (int q = 0; q < SCENARIO_Q; ++q) { ref[q] = 0; sm[q] = 0; sq[q] = 0; lt[q] = 0; eq[q] = 0; }
        if (live && !fresh) {
#pragma unroll
            for (int q = 0; q < SCENARIO_Q; ++q) {
                ref[q] = o.ref[cell + q]; sm[q] = o.sum[cell + q]; sq[q] = o.sumsq[cell + q];
                lt[q] = o.lt[cell + q]; eq[q] = o.eq[cell + q];
            }
        }
        for (int ju = 0; ju < count; ju += U) {
            int kf[U][3], ks[U][3];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool on = ju + u < count;
                const size_t at = (((size_t)(on ? ju + u : 0) * B + b) * M + mr) * H + sr;
                summary_load<0>(fev, at, live && on, kf[u]);
                summary_load<0>(sev, at, live && on, ks[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (ju + u >= count) break;                        // uniform: the scans see every lane
                const int j = ju + u;
                int32_t dx[3], ex[3];
#pragma unroll
                for (int x = 0; x < 3; ++x) {
                    dx[x] = ks[u][x] - kf[u][x];
                    ex[x] = chunk_excl_scan(dx[x], lane, carry[wv][j][x]);
                }
                if (live) {
                    int32_t val[SCENARIO_Q];
                    scenario_diff_values(dx, ex, val);
                    ovf |= scenario_cell_update(ref, sm, sq, lt, eq, val, fresh && j == 0);
                }
            }
        }
        if (live) {
#pragma unroll
            for (int q = 0; q < SCENARIO_Q; ++q) {
                if (fresh) o.ref[cell + q] = ref[q];
                o.sum[cell + q] = sm[q]; o.sumsq[cell + q] = sq[q];
                o.lt[cell + q] = lt[q]; o.eq[cell + q] = eq[q];
            }
        }
    }
    if (ovf) o.overflow[0] = 1u;
}

}  // namespace seir

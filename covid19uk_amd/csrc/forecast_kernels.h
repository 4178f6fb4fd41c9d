// Posterior predictive of the next H days, formed where the burst buffer lies (include/seir_hip.h, "Forecast on the
// device"): for every kept draw of a burst the chain-binomial model of sim_kernels.h is run H days forward from the state
// the draw's recorded events leave at the end of the series, and the simulated counts are folded into moments and
// per-draw marginals with the definitions of summary_update.h.  No event tensor leaves the device.
//
// The parallel axis is the draws of the call, ND = slots x chains of them, nd = slot_in_batch * B + chain; the days are
// sequential for all of them together.  Every plane has the draw index contiguous (row stride ndp = ceil64(ND)):
//   k_forecast_prepare<EV16>  once per batch.  A wave per (row, draw) sums the draw's recorded events over T (loads as
//       summary_load does) and writes the state at day T (St0 for the fold, St the running copy), X = I / N and
//       eb = exp(beta l_m + sigma s_m) / N_m.  One lane per draw forms a_last = alpha_0 + cumsum(alpha_t)[T-2] by the
//       sequential sum (NumPy's order: the host can restate it to the bit) and the H baselines a_last + c_s.
//   k_gemm<64>                per day: F[Mp][ndp] = Cstar . X on v_mfma_f64_16x16x4_f64 -- logprob_kernels.h's tile
//       code through a Dims / Work that put the draw index in the place of the day index (one "chain", Tp := ndp).  An
//       output element's sum runs over K ascending whatever its column: F does not depend on where a draw sits.
//   k_forecast_day            per day: a lane per (row, draw), the draw contiguous over the wave, so F, St, eb and the
//       draw's scalars are coalesced loads.  Rates through the simulator's functions (sim_eb, sim_p_se, sim_p_ir),
//       three sim_binomial variates, state update, X of the next day, and the day's counts as int32 into the staging
//       tensor fev[ND][M][H][3]: rollout_day_cell, the one statement of a cell's day, which the scenarios' day kernels
//       (scenario_kernels.h, scenario_local_kernels.h) call on their own planes with their own two operands.
//   k_forecast_fold           once per batch: k_summarize<0, 0> over the H forecast days of the staging tensor, with its
//       pieces (summary_kernels.h) and the state scanned from the PER-DRAW initial state St0.
//   k_forecast_keep           once per batch, behind the fold and only while the draw store is on: cases, cumulative cases
//       and prevalence of every (row, day, draw) into keep[B][3][M][H][cap], for the exact quantiles of k_order_stats.
//   k_forecast_finish         k_summary_finish's body with St0: state_by_day from the finished by-day sums; advances count[b].
// The accumulators and marginals are a MomentBufs (ForecastBufs::mom), as the summaries' are.
// Random numbers are k_simulate's protocol: Philox4x32-10, key = forecast seed, counter = (attempt, 64 + transition,
// s M + m, draw id) with draw id = (global chain id << 20) + j, j the number of that chain's draws forecast since the last
// reset: nothing depends on how bursts are cut into calls or batches, on the launch geometry or on the sharding of chains.
// Ordinary launches on the context stream: no hand-off inside a launch, no persistence.
#pragma once

#include "sim_kernels.h"
#include "summary_kernels.h"

namespace seir {

constexpr int FC_MAX_H = 128;      // SEIR_FORECAST_MAX_H
constexpr int FC_JMAX = 128;       // trace slots per batch (the staging tensor and ndp are bounded by it)
constexpr int FC_ROWS = 8;         // waves (rows) per workgroup of prepare and fold
constexpr int FC_JB = 16;          // draws per flush of the fold's by-day tile
constexpr int FC_DAY_ROWS = 4;     // rows per workgroup of k_forecast_day (x 64 draws)
constexpr int FC_ID_SHIFT = 20;    // draw id = (global chain id << 20) + j
constexpr int FC_MAX_CHAIN = 2048; // global chain ids below this keep the draw id in 31 bits

struct ForecastBufs {
    int H;
    uint32_t k0, k1;
    const double *W, *wd;          // [H] calendar of the forecast days
    // planes of a batch, draw index contiguous with row stride ndp
    int *St0;                      // [3][Mp][ndp] state at day T (the fold's initial state)
    int *St;                       // [3][Mp][ndp] running state
    double *X, *F;                 // [Mp][ndp] I / N and Cstar . X
    double *eb;                    // [Mp][ndp]
    double *sc;                    // [3][ndp] psi, gamma0, gamma1
    double *base;                  // [H][ndp] log baseline of forecast day s
    const double *steps;           // [ND][H] random-walk steps of the batch (or null: the baseline is held)
    int *fev;                      // [ND][M][H][3] the simulated counts
    MomentBufs mom;                // accumulators and marginals over [H]: forecast_by_day, _by_location, _state_by_day
};

// What a prepare kernel does whatever the rollout starts from (grid (Mp / FC_ROWS, ndp), 64 FC_ROWS threads): draws
// [ND, ndp) and rows [M, Mp) get zeros (the contraction reads them); a wave per (row, draw) sums the draw's recorded events
// over the days before t_end and writes the state at t_end, X and eb; one thread per draw writes the three scalars and
// calls baselines(theta of the draw, nd), which forms the draw's log baselines.
template <int EV16, typename Baselines>
__device__ __forceinline__ void forecast_prepare_draws(const Dims &d, const Consts &c, const ForecastBufs &fb,
                                                       const double *__restrict__ tr_theta, const void *__restrict__ tr_events,
                                                       int B, int first, int ND, int ndp, int t_end, Baselines baselines) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nd = blockIdx.y, m = blockIdx.x * FC_ROWS + wv;
    const int M = d.M, T = d.T;
    const size_t plane = (size_t)d.Mp * ndp, idx = (size_t)m * ndp + nd;
    if (nd >= ND || m >= M) {
        if (lane == 0) {
#pragma unroll
            for (int x = 0; x < 3; ++x) { fb.St0[x * plane + idx] = 0; fb.St[x * plane + idx] = 0; }
            fb.X[idx] = 0.0;
            fb.eb[idx] = 0.0;
        }
        return;
    }
    const int jj = nd / B, b = nd - jj * B, slot = first + jj;
    const double *th = tr_theta + ((size_t)slot * B + b) * d.P;
    const size_t row = (((size_t)slot * B + b) * M + m) * T;
    int tot[3] = {0, 0, 0};
    for (int t = lane; t < t_end; t += 64) {
        int k[3];
        summary_load<EV16>(tr_events, row + t, true, k);
        tot[0] += k[0]; tot[1] += k[1]; tot[2] += k[2];
    }
#pragma unroll
    for (int x = 0; x < 3; ++x)
        for (int o = 32; o > 0; o >>= 1) tot[x] += __shfl_xor(tot[x], o, 64);
    if (lane == 0) {
        const int S = (int)c.init[(size_t)m * 4 + 0] - tot[0];
        const int E = (int)c.init[(size_t)m * 4 + 1] + tot[0] - tot[1];
        const int I = (int)c.init[(size_t)m * 4 + 2] + tot[1] - tot[2];
        fb.St0[idx] = S; fb.St0[plane + idx] = E; fb.St0[2 * plane + idx] = I;
        fb.St[idx] = S; fb.St[plane + idx] = E; fb.St[2 * plane + idx] = I;
        fb.X[idx] = (double)I * c.invN[m];
        fb.eb[idx] = sim_eb(th[2], c.la[m], th[1], th[6 + T - 1 + m], c.invN[m]);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        fb.sc[nd] = th[0]; fb.sc[ndp + nd] = th[3]; fb.sc[2 * ndp + nd] = th[4];
        baselines(th, nd);
    }
}

// The state at day T; one lane per draw forms the H baselines from a_last (forecast_prepare_draws' geometry).
template <int EV16>
__global__ __launch_bounds__(64 * FC_ROWS) void k_forecast_prepare(Dims d, Consts c, ForecastBufs fb,
                                                                   const double *__restrict__ tr_theta,
                                                                   const void *__restrict__ tr_events, int B, int first,
                                                                   int ND, int ndp) {
    debug_skew(d);
    const int T = d.T;
    forecast_prepare_draws<EV16>(d, c, fb, tr_theta, tr_events, B, first, ND, ndp, T, [&](const double *th, int nd) {
        // alpha_0 + cumsum(alpha_t)[T-2]: the running sum in index order, then added to alpha_0 (np.cumsum's order)
        double a_last = th[5];
        if (T > 1) {
            double cs = th[6];
            for (int i = 1; i < T - 1; ++i) cs += th[6 + i];
            a_last = th[5] + cs;
        }
        double walk = 0.0;
        for (int s = 0; s < fb.H; ++s) {
            double a = a_last;
            if (fb.steps) {
                walk = s == 0 ? fb.steps[(size_t)nd * fb.H] : walk + fb.steps[(size_t)nd * fb.H + s];
                a = a_last + walk;
            }
            fb.base[(size_t)s * ndp + nd] = a;
        }
    });
}

// THE rollout day of one (row m, draw nd) cell, whoever rolls it: the forecast, a scenario (scenario_kernels.h) or a targeted
// scenario (scenario_local_kernels.h).  The running state is St[x plane + idx], x = S, E, I, with X and F at idx; eb is the
// forecast's, at ebi; the draw's scalars, wd and the Philox key (k0, k1, draw id, s M + m) are the forecast's and depend on nd,
// m and s alone -- never on the column block -- which is what couples a scenario to the baseline variate by variate.  The
// callers differ in where the planes lie, in the two operands ea_of() = exp(log baseline) and psiW_of(psi) = psi W, called
// where the rates are formed, and in the draw's position `draw` in the staging tensor ev [..][M][H][3].
// Dims, Consts and ForecastBufs by value, as the kernels take them.  Returns the day's I->R count,
// which a triggered scenario's window takes (scenario_trigger_kernels.h); the other callers drop it.
template <typename Ea, typename PsiW>
__device__ __forceinline__ int rollout_day_cell(Dims d, Consts c, ForecastBufs fb, int *St, double *X, const double *Fp,
                                                 size_t plane, size_t idx, size_t ebi, int nd, int m, int B, int chain0, int j0,
                                                 int ndp, int s, int *ev, size_t draw, Ea ea_of, PsiW psiW_of) {
    const int M = d.M, H = fb.H;
    const int jj = nd / B, b = nd - jj * B;
    int S = St[idx], E = St[plane + idx], I = St[2 * plane + idx];
    const double F = Fp[idx], eb = fb.eb[ebi];
    const double psi = fb.sc[nd], g0 = fb.sc[ndp + nd], g1 = fb.sc[2 * ndp + nd];
    const double ea = ea_of();
    const double psiW = psiW_of(psi);
    const double p_ir = sim_p_ir(g0, g1, fb.wd[s], d.dt);
    const double p_ei = sim_p_ei(d.nu, d.dt);
    const double p_se = sim_p_se(ea, eb, (double)I, psiW, F, d.rate_floor, d.dt);
    RngKey key{fb.k0, fb.k1, ((uint32_t)(chain0 + b) << FC_ID_SHIFT) + (uint32_t)(j0 + jj), (uint32_t)(s * M + m)};
    const int y0 = sim_binomial(S, p_se, key, RS_SIM_BASE + 0);
    const int y1 = sim_binomial(E, p_ei, key, RS_SIM_BASE + 1);
    const int y2 = sim_binomial(I, p_ir, key, RS_SIM_BASE + 2);
    SumEv32 out;
    out.k[0] = y0; out.k[1] = y1; out.k[2] = y2;
    reinterpret_cast<SumEv32 *>(ev)[(draw * M + m) * H + s] = out;
    S -= y0; E += y0 - y1; I += y1 - y2;
    St[idx] = S; St[plane + idx] = E; St[2 * plane + idx] = I;
    X[idx] = (double)I * c.invN[m];
    return y2;
}

// Forecast day s for every (row, draw): grid (ndp / 64, ceil(M / FC_DAY_ROWS)), 64 FC_DAY_ROWS threads.
// j0: the chain's draws forecast before this batch (the draw of slot_in_batch jj has j = j0 + jj).
__global__ __launch_bounds__(64 * FC_DAY_ROWS) void k_forecast_day(Dims d, Consts c, ForecastBufs fb, int B, int chain0,
                                                                   int j0, int ND, int ndp, int s) {
    debug_skew(d);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nd = blockIdx.x * 64 + lane, m = blockIdx.y * FC_DAY_ROWS + wv;
    if (nd >= ND || m >= d.M) return;
    const size_t idx = (size_t)m * ndp + nd;
    rollout_day_cell(d, c, fb, fb.St, fb.X, fb.F, (size_t)d.Mp * ndp, idx, idx, nd, m, B, chain0, j0, ndp, s, fb.fev, (size_t)nd,
                     [&] { return exp(fb.base[(size_t)s * ndp + nd]); }, [&](double psi) { return psi * fb.W[s]; });
}

static_assert(FC_ROWS == SUM_ROWS && FC_JB == SUM_JB && FC_JMAX == SUM_JMAX, "k_forecast_fold uses k_summarize's pieces");

// k_summarize<0, 0> over the H forecast days of the staging tensor, with its pieces (summary_kernels.h), but for: each
// draw's state is scanned from ITS OWN initial state St0; one draw's load is in flight, not SUM_U; the draws are always folded.
// grid (ceil(M / FC_ROWS), B), 64 FC_ROWS threads.  1 <= count <= FC_JMAX slots starting at trace slot `first`.
__global__ __launch_bounds__(64 * FC_ROWS) void k_forecast_fold(Dims d, ForecastBufs fb, int B, int first, int count,
                                                                int ndp) {
    debug_skew(d);
    __shared__ unsigned long long bd[FC_JB][64][3];
    __shared__ int carry[FC_ROWS][FC_JMAX][3];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y, m = blockIdx.x * FC_ROWS + wv;
    const int M = d.M, H = fb.H;
    const MomentBufs &sb = fb.mom;
    const bool row_ok = m < M;
    const bool fresh = sb.count[b] == 0;               // count moves in k_forecast_finish, a launch of its own: no race
    const size_t plane = (size_t)d.Mp * ndp;
    fold_lds_zero(bd, carry[wv], count, lane);
    __syncthreads();

    bool ovf = false;
    for (int h0 = 0; h0 < H; h0 += 64) {
        const int s = h0 + lane;
        const bool live = row_ok && s < H;
        const size_t cell = ((size_t)b * M + (row_ok ? m : 0)) * H + (s < H ? s : 0);
        int32_t ref[SUMMARY_Q];
        int64_t sm[SUMMARY_Q];
        uint64_t sq[SUMMARY_Q];
#pragma unroll
        for (int q = 0; q < SUMMARY_Q; ++q) { ref[q] = 0; sm[q] = 0; sq[q] = 0; }
        if (live && !fresh) fold_load(sb, cell, ref, sm, sq);
        for (int jb = 0; jb < count; jb += FC_JB) {
            const int nj = min(FC_JB, count - jb);
            for (int jj = 0; jj < nj; ++jj) {
                const int j = jb + jj, nd = j * B + b;
                int kk[3];
                summary_load<0>(fb.fev, ((size_t)nd * M + (row_ok ? m : 0)) * H + (s < H ? s : 0), live, kk);
                int s0[3] = {0, 0, 0}, ex[3];
                if (row_ok)
#pragma unroll
                    for (int x = 0; x < 3; ++x) s0[x] = fb.St0[x * plane + (size_t)m * ndp + nd];
#pragma unroll
                for (int x = 0; x < 3; ++x) ex[x] = chunk_excl_scan(kk[x], lane, carry[wv][j][x]);
                if (live) {
#pragma unroll
                    for (int x = 0; x < 3; ++x)
                        if (kk[x] != 0) atomicAdd(&bd[jj][lane][x], (unsigned long long)kk[x]);
                    int val[SUMMARY_Q];
                    fold_values(kk, s0, ex, val);
                    const bool is_first = fresh && j == 0;
#pragma unroll
                    for (int q = 0; q < SUMMARY_Q; ++q) ovf |= summary_fold(ref[q], sm[q], sq[q], val[q], is_first);
                }
            }
            __syncthreads();
            fold_tile_flush(bd, nj, sb.by_day, first + jb, B, b, H, h0);
            __syncthreads();
        }
        if (live) {
#pragma unroll
            for (int q = 0; q < SUMMARY_Q; ++q) {
                if (fresh) sb.ref[cell * SUMMARY_Q + q] = ref[q];
                sb.sum[cell * SUMMARY_Q + q] = sm[q];
                sb.sumsq[cell * SUMMARY_Q + q] = sq[q];
            }
        }
    }
    // the carries after the last chunk are the row totals over the horizon
    if (row_ok)
        for (int i = lane; i < count * 3; i += 64) {
            const int j = i / 3, x = i - j * 3;
            sb.by_loc[(((size_t)(first + j) * B + b) * M + m) * 3 + x] = (int64_t)carry[wv][j][x];
        }
    if (ovf) sb.overflow[0] = 1u;
}

// The draw store of the forecast intervals (include/seir_hip.h, "Forecast intervals on the device"): three int32 per
// (chain, location, day, draw) kept in keep[B][3][M][H][cap], the draw index innermost, so that a cell's draws are one
// contiguous run for k_order_stats (order_stats_kernels.h).  The planes, for day s of the window:
//     0 cases       k_ir[m][s]
//     1 cum_cases   sum_{s' <= s} k_ir[m][s']
//     2 prevalence  I at the START of day s: I0 + exclusive scan of k_ei - exclusive scan of k_ir (quantity 5 of the fold)
// ev is a batch's staging tensor [ND][M][H][3] (nd = slot_in_batch * B + chain) and I0 [Mp][ndp] the I plane of the
// per-draw state at the window's start; the draw of slot_in_batch jj goes to position j0 + jj of its chain's cells (the
// host checks j0 + count <= cap).  Nothing here is the forecast's alone: the in-sample check has the same two tensors.
// A wave per (row, chain), a lane per day, the draws in flushes of KEEP_JB: the three values go through an LDS tile
// [plane][day][draw of the flush] (rows padded by one word: the lanes of a store are a row apart) and leave it with the
// lanes along the DRAW axis -- every cell receives one run of up to KEEP_JB int32, not a 4-byte store at a stride of cap.
// grid (ceil(M / KEEP_ROWS), B), 64 KEEP_ROWS threads.  1 <= count <= FC_JMAX.
constexpr int KEEP_ROWS = 2;       // waves (rows) per workgroup
constexpr int KEEP_JB = 32;        // draws per flush: a cell's run is up to 128 B
constexpr int KEEP_U = 4;          // draws whose loads are in flight together
static_assert(KEEP_JB <= 64 && KEEP_JB % KEEP_U == 0, "a lane per carry; whole groups of loads");

__global__ __launch_bounds__(64 * KEEP_ROWS) void k_forecast_keep(Dims d, const int *__restrict__ ev,
                                                                  const int *__restrict__ I0, int *__restrict__ keep,
                                                                  long long cap, long long j0, int H, int B, int count,
                                                                  int ndp) {
    debug_skew(d);
    __shared__ int tile[KEEP_ROWS][3][64][KEEP_JB + 1];
    __shared__ int carry[KEEP_ROWS][KEEP_JB][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y, m = blockIdx.x * KEEP_ROWS + wv;
    const int M = d.M;
    const bool row_ok = m < M;
    const int mr = row_ok ? m : 0;
    for (int jb = 0; jb < count; jb += KEEP_JB) {
        const int nj = min(KEEP_JB, count - jb);
        if (lane < KEEP_JB) { carry[wv][lane][0] = 0; carry[wv][lane][1] = 0; }
        __syncthreads();
        for (int h0 = 0; h0 < H; h0 += 64) {
            const int s = h0 + lane;
            const bool live = row_ok && s < H;
            for (int ju = 0; ju < nj; ju += KEEP_U) {
                int kk[KEEP_U][3], i0[KEEP_U];
#pragma unroll
                for (int u = 0; u < KEEP_U; ++u) {
                    const bool on = ju + u < nj;
                    const int nd = (jb + (on ? ju + u : 0)) * B + b;
                    summary_load<0>(ev, ((size_t)nd * M + mr) * H + (s < H ? s : 0), live && on, kk[u]);
                    i0[u] = I0[(size_t)mr * ndp + nd];
                }
#pragma unroll
                for (int u = 0; u < KEEP_U; ++u) {
                    const int jj = ju + u;
                    if (jj < nj) {                                     // uniform over the wave: the scans see every lane
                        const int inc_ei = wave_incl_scan(kk[u][1], lane), inc_ir = wave_incl_scan(kk[u][2], lane);
                        const int c_ei = carry[wv][jj][0], c_ir = carry[wv][jj][1];
                        tile[wv][0][lane][jj] = kk[u][2];
                        tile[wv][1][lane][jj] = c_ir + inc_ir;
                        tile[wv][2][lane][jj] = i0[u] + (c_ei + inc_ei - kk[u][1]) - (c_ir + inc_ir - kk[u][2]);
                        if (lane == 63) { carry[wv][jj][0] = c_ei + inc_ei; carry[wv][jj][1] = c_ir + inc_ir; }
                    }
                }
            }
            __syncthreads();
            const int cnt = min(64, H - h0) * nj;
            if (row_ok)
                for (int i = lane; i < cnt; i += 64) {
                    const int tl = i / nj, jj = i - tl * nj;
#pragma unroll
                    for (int x = 0; x < 3; ++x)
                        keep[((((size_t)b * 3 + x) * M + m) * H + (h0 + tl)) * (size_t)cap + (size_t)(j0 + jb + jj)] =
                            tile[wv][x][tl][jj];
                }
            __syncthreads();
        }
    }
}

// k_summary_finish over the H forecast days, with the draw's own initial state St0.  grid (count, B), one wave.
__global__ __launch_bounds__(64) void k_forecast_finish(Dims d, ForecastBufs fb, int B, int first, int count, int ndp) {
    const size_t plane = (size_t)d.Mp * ndp;
    const int nd = blockIdx.x * B + blockIdx.y;
    moment_finish(fb.mom, d.M, fb.H, B, first + blockIdx.x, count, true,
                  [&](int m, int x) { return fb.St0[x * plane + (size_t)m * ndp + nd]; });
}

}  // namespace seir

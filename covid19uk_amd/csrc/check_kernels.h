// In-sample predictive check, formed where the burst buffer lies (include/seir_hip.h, "In-sample predictive check on the
// device"): for every kept draw of a burst the last K observed days are simulated again from the state the draw's recorded
// events leave at day T - K, folded into moments and marginals as the forecast's are, and set against the observed removals,
// which are the I->R plane of the draw itself.
//
// The per-day machinery is the forecast's on a second ForecastBufs with H := K (forecast_kernels.h: k_gemm<64> over the
// draws, k_forecast_day, k_forecast_fold, k_forecast_finish, unchanged).  This file adds
//   k_check_prepare<EV16>  k_forecast_prepare's shape, but the row sums run over the days before T - K and the K log baselines
//       are the draw's own: alpha_0 at day 0, else alpha_0 + cumsum(alpha_t)[t - 1], the running sum sequential in index order
//       and then added to alpha_0 (np.cumsum's order: the host can restate it to the bit).
//   k_check_compare<EV16>  behind the finish: a wave per (row, chain), a lane per check day, the draw loop inside.  lt / eq of
//       the cell stay in registers across the draws (check_update.h), obs is stored from the first draw after a reset and
//       verified by the others, and the row's total over the window is compared (by_location against the wave sum of obs).
//   k_check_totals         behind it: a workgroup per chain sums obs over the rows and compares every draw's check_by_day
//       with it, per day and over the whole window.
// Ordinary launches on the context stream: no hand-off inside a launch, no persistence.  Integers only in the comparison.
#pragma once

#include "check_update.h"
#include "forecast_kernels.h"

namespace seir {

constexpr int CK_MAX_K = 128;                // SEIR_CHECK_MAX_DAYS
constexpr int CK_CH = CK_MAX_K / 64;         // 64-day chunks a lane of k_check_compare holds
constexpr int CK_TOT_THREADS = 512;          // k_check_totals: 128 days x 4 row groups
static_assert(CK_MAX_K <= FC_MAX_H, "the check runs on a ForecastBufs");

// The comparison with the data, one set per chain; the host owns it as one allocation of 32-bit words.
struct CheckCmp {
    int32_t *obs;                  // [B][M][K] observed I->R counts: those of the first draw folded after a reset
    uint32_t *lt, *eq;             // [B][M][K] draws with simulated < / == obs
    uint32_t *loc_lt, *loc_eq;     // [B][M]    the row's total over the window
    uint32_t *day_lt, *day_eq;     // [B][K]    the day's total over the rows
    uint32_t *all_lt, *all_eq;     // [B]       the whole window, all rows
    unsigned *moved;               // [B] sticky: a later draw's I->R counts in the window differ from obs
};

// forecast_prepare_draws up to day T - K (its geometry); one lane per draw forms the K baselines of the draw's own days.
template <int EV16>
__global__ __launch_bounds__(64 * FC_ROWS) void k_check_prepare(Dims d, Consts c, ForecastBufs fb,
                                                                const double *__restrict__ tr_theta,
                                                                const void *__restrict__ tr_events, int B, int first,
                                                                int ND, int ndp) {
    debug_skew(d);
    const int T = d.T, t0 = d.T - fb.H;
    forecast_prepare_draws<EV16>(d, c, fb, tr_theta, tr_events, B, first, ND, ndp, t0, [&](const double *th, int nd) {
        // day t of the window: alpha_0 at t = 0, else alpha_0 + cumsum(alpha_t)[t - 1] -- the running sum in index order,
        // then added to alpha_0 (np.cumsum's order).  t <= T - 1, so the reference's clip at T - 2 never binds in sample.
        if (t0 == 0) fb.base[nd] = th[5];
        double cs = 0.0;
        for (int i = 0; i < T - 1; ++i) {
            cs = i == 0 ? th[6] : cs + th[6 + i];
            const int s = i + 1 - t0;
            if (s >= 0) fb.base[(size_t)s * ndp + nd] = th[5] + cs;
        }
    });
}

// grid (ceil(M / FC_ROWS), B), 64 FC_ROWS threads.  1 <= count <= FC_JMAX slots from trace slot `first`, whose simulated
// counts lie in fb.fev and whose row totals in fb.mom.by_loc.  fresh: the first of them is the first draw since the reset.
template <int EV16>
__global__ __launch_bounds__(64 * FC_ROWS) void k_check_compare(Dims d, ForecastBufs fb, CheckCmp cc,
                                                                const void *__restrict__ tr_events, int B, int first,
                                                                int count, int fresh) {
    debug_skew(d);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y, m = blockIdx.x * FC_ROWS + wv;
    const int M = d.M, T = d.T, K = fb.H, t0 = d.T - fb.H;
    if (m >= M) return;
    const size_t cell0 = ((size_t)b * M + m) * K;
    int32_t obs[CK_CH];
    uint32_t lt[CK_CH], eq[CK_CH];
#pragma unroll
    for (int ch = 0; ch < CK_CH; ++ch) {
        const int s = ch * 64 + lane;
        obs[ch] = 0; lt[ch] = 0u; eq[ch] = 0u;
        if (s < K) { obs[ch] = cc.obs[cell0 + s]; lt[ch] = cc.lt[cell0 + s]; eq[ch] = cc.eq[cell0 + s]; }
    }
    uint32_t rlt = 0u, req = 0u;
    if (lane == 0) { rlt = cc.loc_lt[(size_t)b * M + m]; req = cc.loc_eq[(size_t)b * M + m]; }
    bool moved = false;
    for (int j = 0; j < count; ++j) {
        const int nd = j * B + b, slot = first + j;
        const size_t row = (((size_t)slot * B + b) * M + m) * T + t0;
        const size_t srow = ((size_t)nd * M + m) * K;
        long long osum = 0;
#pragma unroll
        for (int ch = 0; ch < CK_CH; ++ch) {
            const int s = ch * 64 + lane;
            if (s < K) {
                const int sim = fb.fev[(srow + s) * 3 + 2];
                int k[3];
                summary_load<EV16>(tr_events, row + s, true, k);
                moved |= check_cell_update(obs[ch], lt[ch], eq[ch], sim, k[2], fresh != 0 && j == 0);
                osum += (long long)obs[ch];
            }
        }
        for (int o = 32; o > 0; o >>= 1) osum += __shfl_xor(osum, o, 64);
        if (lane == 0)
            check_total_update(rlt, req, fb.mom.by_loc[(((size_t)slot * B + b) * M + m) * 3 + 2], (int64_t)osum);
    }
#pragma unroll
    for (int ch = 0; ch < CK_CH; ++ch) {
        const int s = ch * 64 + lane;
        if (s < K) {
            if (fresh) cc.obs[cell0 + s] = obs[ch];
            cc.lt[cell0 + s] = lt[ch];
            cc.eq[cell0 + s] = eq[ch];
        }
    }
    if (lane == 0) { cc.loc_lt[(size_t)b * M + m] = rlt; cc.loc_eq[(size_t)b * M + m] = req; }
    if (moved) cc.moved[b] = 1u;
}

// grid (B), CK_TOT_THREADS threads.  Behind k_check_compare (obs is stored) and k_forecast_finish (by_day is complete).
__global__ __launch_bounds__(CK_TOT_THREADS) void k_check_totals(Dims d, ForecastBufs fb, CheckCmp cc, int B, int first,
                                                                 int count) {
    debug_skew(d);
    __shared__ unsigned long long od[CK_MAX_K];      // observed total of check day s over the rows
    __shared__ unsigned long long otot;              // ... and over the window
    __shared__ unsigned cnt[2];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int M = d.M, K = fb.H;
    if (tid < CK_MAX_K) od[tid] = 0ull;
    if (tid == 0) { otot = 0ull; cnt[0] = 0u; cnt[1] = 0u; }
    __syncthreads();
    {
        const int s = tid & (CK_MAX_K - 1), g = tid / CK_MAX_K;
        if (s < K) {
            unsigned long long a = 0ull;             // counts are not negative
            for (int m = g; m < M; m += CK_TOT_THREADS / CK_MAX_K) a += (unsigned long long)cc.obs[((size_t)b * M + m) * K + s];
            if (a != 0ull) atomicAdd(&od[s], a);
        }
    }
    __syncthreads();
    if (tid < 64) {
        unsigned long long v = od[tid] + od[tid + 64];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (tid == 0) otot = v;
    }
    __syncthreads();
    if (tid < K) {
        uint32_t dl = cc.day_lt[(size_t)b * K + tid], de = cc.day_eq[(size_t)b * K + tid];
        const int64_t o = (int64_t)od[tid];
        for (int j = 0; j < count; ++j)
            check_total_update(dl, de, fb.mom.by_day[(((size_t)(first + j) * B + b) * K + tid) * 3 + 2], o);
        cc.day_lt[(size_t)b * K + tid] = dl;
        cc.day_eq[(size_t)b * K + tid] = de;
    } else if (tid >= CK_MAX_K) {
        for (int j = tid - CK_MAX_K; j < count; j += CK_TOT_THREADS - CK_MAX_K) {
            const int64_t *bd = fb.mom.by_day + ((size_t)(first + j) * B + b) * K * 3;
            int64_t sim = 0;
            for (int s = 0; s < K; ++s) sim += bd[(size_t)s * 3 + 2];
            uint32_t l = 0u, e = 0u;
            check_total_update(l, e, sim, (int64_t)otot);
            if (l) atomicAdd(&cnt[0], 1u);
            if (e) atomicAdd(&cnt[1], 1u);
        }
    }
    __syncthreads();
    if (tid == 0) { cc.all_lt[b] += cnt[0]; cc.all_eq[b] += cnt[1]; }
}

}  // namespace seir

// Triggered scenarios: measures that switch on and off by the draw's own simulated case counts (include/seir_hip.h,
// "Triggered scenarios on the device").  It extends scenario_local_kernels.h and changes nothing of it.
//
// THE definition of a triggered scenario.  Scenario k is a targeted scenario with TWO operand pairs per (m, s) and a rule
// that picks one of them per draw:
//     off pair   log_shift[k][m][s], commute[k][m][s]          exactly the targeted tensors
//     on pair    log_shift_on[k][m][s], commute_on[k][m][s]    under the same refusals (finite; commute >= 0)
// On the device all four are [K][H][M], with Wk = W[s] * commute and Wk_on = W[s] * commute_on, each one rounded multiply
// formed on the host at every forecast reset.
// Rule parameters.  Per scenario: window w in [1, SEIR_TRIGGER_MAX_WINDOW = 28], from_day in [0, H], min_days >= 0,
// review_every >= 1.  Per location: integer thresholds 0 <= off[k][m] <= on[k][m] <= INT32_MAX; on = INT32_MAX: never.
// State.  Per (scenario k, location m, draw), at the start of rollout day s and before the day's rates are formed:
//     c = the sum of the I->R counts of the w days before absolute day T + s: for a day >= T scenario k's own simulated
//         count of that draw, for a day in [0, T) the draw's recorded I->R count in the trace slot the forecast rolls from,
//         for a day < 0 zero;
//     review = s >= from_day && (s - from_day) % review_every == 0;
//     on a review: if not active and c >= on: active <- 1, age <- 0; otherwise, if active and age >= min_days and c < off:
//         active <- 0                                                                       (trigger_update.h: trigger_step)
//     day s is rolled with the on pair iff active; behind the day, if active, age <- age + 1.  At day 0 active = 0.
// The day itself is rollout_day_cell (forecast_kernels.h) with the two operands selected per draw:
//     ea   = exp(base_0[s][nd] + (active ? log_shift_on : log_shift)[k][m][s])     one rounded add, then the same exp
//     psiW = psi * (active ? Wk_on : Wk)[k][m][s]                                  one rounded multiply
// so a rule that never fires is bit for bit the targeted scenario with the off tensors, and a rule that fires everywhere at
// day 0 and never releases is the targeted scenario with the on tensors.  Key, counter, draw id, the state at day T, eb, the
// scalars and the contraction over K ndp columns are the forecast's: common random numbers couple every scenario to the
// baseline, whatever its rule does.
//
// Planes of a batch, next to ScenarioBufs' (row stride K ndp, column c = k ndp + nd):
//     hist [wmax][Mp][ndp] int32   row i: the draw's recorded I->R count of day T - wmax + i (0 before day 0, 0 in padded rows
//                                  and draws); wmax the largest window of the set; shared by all k (scenario k reads its
//                                  last w_k rows)
//     win  [Mp][K ndp] int32       c, the running window sum
//     age  [Mp][K ndp] int32
//     mask [2][Mp][K ndp] uint64   THE record of the rule: bit s of the 128 is set iff active on day s (H <= 128)
// The launches.  k_trigger_begin<EV16> once per batch, in k_scenario_local_begin's place: scenario_begin_planes, hist, and
// win, age, mask of every column block.  k_scenario_trigger_day<R> per day behind the contraction, k_scenario_local_day's
// geometry.  k_trigger_fold once per batch and scenario behind the day loop: the masks into two integer products,
//     active_count  [K][B][M][H] uint32      draws of chain b in which m is under the measure on day s (an accumulator)
//     active_by_day [K][cap][B][H] int32     locations under the measure, by draw position since the forecast reset
// The fold is sums of bits: no float, no atomics, every output element has one owner (a wave per (row, chain) for the
// counts, a wave per (draw, chain) for the curves, a lane per day), so nothing depends on the geometry, on debug_skew or on
// how the draws are cut into calls, and a burst run again overwrites its own positions.  No per-cell, per-draw store: the
// 16 bytes of mask per (row, column) are all the rule leaves behind.
#pragma once

#include "scenario_local_kernels.h"
#include "trigger_update.h"

namespace seir {

constexpr int TRIG_ROWS = 8;       // waves per workgroup of the fold
constexpr int TRIG_U = 4;          // mask words whose loads are in flight together

// The operands and planes of a triggered set next to ScenarioBufs and ScenarioLocalBufs (the off pair).
struct ScenarioTriggerBufs {
    const double *log_shift_on;    // [K][H][M]
    const double *Wk_on;           // [K][H][M] W[s] * commute_on[k][m][s]
    const int32_t *on, *off;       // [K][M]
    const int32_t *params;         // [K][4] window, from_day, min_days, review_every
    int wmax;                      // the largest window of the set: hist's rows
    int32_t *hist;                 // [wmax][Mp][ndp]
    int32_t *win, *age;            // [Mp][K ndp]
    uint64_t *mask;                // [2][Mp][K ndp]
};

// grid (ceil(Mp ndp / T), K), T threads: element i of block k's planes (row i / ndp, draw i mod ndp).  `first`: the trace slot
// of the batch's first draw (the draw nd = jj B + b rolls from slot first + jj).
template <int EV16>
__global__ __launch_bounds__(SC_BEGIN_THREADS) void k_trigger_begin(Dims d, Consts c, ForecastBufs fb, ScenarioBufs sb,
                                                                    ScenarioTriggerBufs tb, const void *__restrict__ tr_events,
                                                                    int B, int first, int ND, int ndp) {
    debug_skew(d);
    const int k = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * SC_BEGIN_THREADS + threadIdx.x;
    const int r = (int)(i / ndp), nd = (int)(i - (size_t)r * ndp);
    scenario_begin_planes(d, c, fb, sb, k, r, nd, ND, ndp);
    if (r >= d.Mp) return;
    const int T = d.T, wmax = tb.wmax, w = tb.params[k * 4];
    const bool live = r < d.M && nd < ND;
    const int jj = nd / B, b = nd - jj * B;
    const size_t row = live ? (((size_t)(first + jj) * B + b) * d.M + r) * T : 0;
    const size_t hplane = (size_t)d.Mp * ndp, hidx = (size_t)r * ndp + nd;
    int sum = 0;
    for (int h = 0; h < wmax; ++h) {
        const int t = T - wmax + h;
        int ev[3];
        summary_load<EV16>(tr_events, row + (t >= 0 ? t : 0), live && t >= 0, ev);
        if (k == 0) tb.hist[(size_t)h * hplane + hidx] = ev[2];
        sum += h >= wmax - w ? ev[2] : 0;
    }
    const size_t ndk = (size_t)sb.K * ndp, idx = (size_t)r * ndk + (size_t)k * ndp + nd;
    tb.win[idx] = sum;
    tb.age[idx] = 0;
    tb.mask[idx] = 0;
    tb.mask[(size_t)d.Mp * ndk + idx] = 0;
}

// Forecast day s for every (row, scenario, draw): k_scenario_local_day's geometry -- grid (K ndp / 64, ceil(M / R)), 64 R
// threads; a wave has one row and one scenario, a lane is a draw.  k, m and s are wave-uniform, and so are the four operands,
// the two thresholds, the rule's parameters and `review`: scalar loads through indices made uniform for the compiler.  The
// lanes differ in `active` alone, and the pair is picked by a select: a divergent branch would run the exp and the three
// binomials of rollout_day_cell twice.
template <int R>
__global__ __launch_bounds__(64 * R) void k_scenario_trigger_day(Dims d, Consts c, ForecastBufs fb, ScenarioBufs sb,
                                                                 ScenarioLocalBufs lb, ScenarioTriggerBufs tb, int B, int chain0,
                                                                 int j0, int ND, int ndp, int s) {
    debug_skew(d);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane, m = blockIdx.y * R + wv;
    const int k = (blockIdx.x * 64) / ndp, nd = col - k * ndp;       // ndp is a multiple of 64: the wave's scenario
    if (nd >= ND || m >= d.M) return;
    const int H = fb.H;
    const size_t ndk = (size_t)sb.K * ndp, plane = (size_t)d.Mp * ndk, idx = (size_t)m * ndk + col;
    const int op = __builtin_amdgcn_readfirstlane((k * H + s) * d.M + m);   // k < 4, H <= 128: below 2^31 for every M
    const int km = __builtin_amdgcn_readfirstlane(k * d.M + m);
    const int32_t on = tb.on[km], off = tb.off[km];
    const int32_t w = tb.params[k * 4], from_day = tb.params[k * 4 + 1], min_days = tb.params[k * 4 + 2],
                  review_every = tb.params[k * 4 + 3];
    const bool review = trigger_review(s, from_day, review_every);
    // the state: three plane words in
    const int32_t win = tb.win[idx];
    int32_t age = tb.age[idx];
    const size_t word = (size_t)(s >> 6) * plane + idx;
    uint64_t bits = tb.mask[word];
    // active on the day before: bit s - 1 -- of the word before for s = 64 (uniform)
    int32_t active = 0;
    if (s & 63) active = (int32_t)((bits >> ((s & 63) - 1)) & 1u);
    else if (s) active = (int32_t)(tb.mask[idx] >> 63);
    // the count that leaves the window behind the day, of absolute day T + s - w: recorded while s < w, else the lane's own
    // simulated count of rollout day s - w (uniform); loaded here, used behind the day
    const size_t cell = (((size_t)k * ND + nd) * d.M + m) * H;
    const int32_t leaves = s < w ? tb.hist[(size_t)(tb.wmax - w + s) * ((size_t)d.Mp * ndp) + (size_t)m * ndp + nd]
                                 : sb.sev[(cell + (size_t)(s - w)) * 3 + 2];
    trigger_step(active, age, win, on, off, min_days, review);
    const double ls = active ? tb.log_shift_on[op] : lb.log_shift[op];
    const double Wk = active ? tb.Wk_on[op] : lb.Wk[op];
    const int y_ir = rollout_day_cell(d, c, fb, sb.St, sb.X, sb.F, plane, idx, (size_t)m * ndp + nd, nd, m, B, chain0, j0, ndp,
                                      s, sb.sev, (size_t)k * ND + nd,
                                      [&] { return exp(fb.base[(size_t)s * ndp + nd] + ls); },
                                      [&](double psi) { return psi * Wk; });
    trigger_after_day(active, age);
    bits |= (uint64_t)active << (s & 63);
    tb.win[idx] = win + y_ir - leaves;
    tb.age[idx] = age;
    tb.mask[word] = bits;
}

// The fold of the masks of nj draws per chain, nd = jj B + b at mask[x plane + m stride + col0 + nd], x = 0, 1.
// grid (ceil(M / TRIG_ROWS) + ceil(nj / TRIG_ROWS), B), 64 TRIG_ROWS threads; a lane is a day of a 64-day chunk.
//   blocks [0, ceil(M / TRIG_ROWS)): a wave per (row m, chain b) counts the draws whose bit s is set into count[b][m][s]
//       ([B][M][H] uint32): loaded before the loop over draws (fresh: written, not read), held in a register, stored behind it;
//   the blocks behind them: a wave per (draw jj, chain b) counts the rows whose bit s is set into by_day[jj][b][s]
//       ([nj][B][H] int32, the caller's pointer at the batch's first draw position): written, never read.
// A word's address is wave-uniform; U of them are in flight.  M and H are the call's own, not the context's.  (A template, so that it
// is emitted with the other instances where the host code first names it and no kernel in front of it moves.)
template <int U>
__global__ __launch_bounds__(64 * TRIG_ROWS) void k_trigger_fold(Dims d, const uint64_t *__restrict__ mask, size_t plane,
                                                                  size_t stride, size_t col0, uint32_t *__restrict__ count,
                                                                  int32_t *__restrict__ by_day, int M, int H, int B, int nj,
                                                                  int fresh) {
    debug_skew(d);
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y, mblocks = (M + TRIG_ROWS - 1) / TRIG_ROWS;
    const uint64_t *__restrict__ at = mask + col0 + b;
    if ((int)blockIdx.x < mblocks) {
        const int m = blockIdx.x * TRIG_ROWS + wv;
        if (m >= M) return;
        for (int h0 = 0; h0 < H; h0 += 64) {
            const int s = h0 + lane;
            const uint64_t *__restrict__ src = at + (size_t)(h0 >> 6) * plane + (size_t)m * stride;
            const size_t cell = ((size_t)b * M + m) * H + s;
            uint32_t n = (s < H && !fresh) ? count[cell] : 0u;
            for (int ju = 0; ju < nj; ju += U) {
                uint64_t wd[U];
#pragma unroll
                for (int u = 0; u < U; ++u) wd[u] = ju + u < nj ? src[(size_t)(ju + u) * B] : 0ull;
#pragma unroll
                for (int u = 0; u < U; ++u) n += (uint32_t)((wd[u] >> lane) & 1u);
            }
            if (s < H) count[cell] = n;
        }
    } else {
        const int jj = ((int)blockIdx.x - mblocks) * TRIG_ROWS + wv;
        if (jj >= nj) return;
        for (int h0 = 0; h0 < H; h0 += 64) {
            const int s = h0 + lane;
            const uint64_t *__restrict__ src = at + (size_t)(h0 >> 6) * plane + (size_t)jj * B;
            int32_t n = 0;
            for (int mu = 0; mu < M; mu += U) {
                uint64_t wd[U];
#pragma unroll
                for (int u = 0; u < U; ++u) wd[u] = mu + u < M ? src[(size_t)(mu + u) * stride] : 0ull;
#pragma unroll
                for (int u = 0; u < U; ++u) n += (int32_t)((wd[u] >> lane) & 1u);
            }
            if (s < H) by_day[((size_t)jj * B + b) * H + s] = n;
        }
    }
}

}  // namespace seir

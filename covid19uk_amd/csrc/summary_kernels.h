// Summaries of the recorded latent epidemic, formed where the burst buffer lies (include/seir_hip.h, "Summaries of
// samples/seir on the device"): per-cell moments of the event counts and of the state over the kept draws, and per-draw
// marginals (events by day, events by location, state by day).  The definitions are summary_update.h's.
//
// The accumulators are a MomentBufs, the one type the summaries, the diagnostics and the forecast (forecast_kernels.h)
// accumulate into; the forecast's fold and finish are built from the pieces and the finish body below.
//
// k_summarize<EV16> reads trace slots [first, first + count) of all chains once.  The shape of the work:
//   - a WAVE owns a row m of a chain and walks its 64-day chunks, a lane per day; a workgroup is SUM_ROWS such waves on
//     neighbouring rows.  The state is a prefix over days: inside a chunk a DPP wave scan per transition, from chunk to
//     chunk a carry per draw (3 ints, LDS; only the owning wave touches it).  The carry after the last chunk is
//     events_by_location;
//   - the loop over the call's draws is the INNER one: a cell's six (ref, sum, sumsq) triples are loaded before it, held
//     in registers across it and stored after it, so the accumulators (20 B per cell and quantity) cross memory once per
//     launch whatever the number of draws.  The host cuts a call into launches of at most SUM_JMAX draws (the carries'
//     LDS); integer sums do not care;
//   - a lane reads its day's three counts as one 12-byte access (int32: global_load_dwordx3) or a 4-byte and a 2-byte one
//     (uint16, whose rows are only 2-byte aligned), contiguous over the wave: nothing to de-interleave.  The loads of SUM_U
//     draws are issued before the first of them is used;
//   - events_by_day is a sum over rows, i.e. over waves and workgroups: the waves of a workgroup add their counts into an
//     LDS tile [SUM_JB draws][64 days][3] (64-bit integer LDS adds), and after every SUM_JB draws the workgroup issues
//     one global 64-bit atomicAdd per (draw, day, transition) that is not zero, 1536 contiguous bytes per draw, onto
//     arrays the call has zeroed.  At UK-380 x 8 and 100 draws that is 4.2e7 atomics instead of 7e8, and integer adds
//     are exact in any order;
//   - state_by_day needs no pass over the cells at all: sum_m S[m][t] = sum_m S0[m] - sum_{s<t} events_by_day[s][0], and
//     so on -- k_summary_finish scans the finished events_by_day (a wave per draw and chain) and also advances count[b].
// No hand-off inside a launch, no persistence, nothing of the sweep's plan: ordinary launches on the context stream.
//
// k_summarize<EV16, 1> is the instance launched while the convergence diagnostics are on (seir_sampler_diag_reset): next
// to the moments it carries a cell's batch sums (summary_update.h: bsum, bsumsq; 16 B per cell and quantity) the same
// way -- loaded before the draw loop, in registers across it, stored after it.  Which draws close a batch is the same for
// every cell of a chain: the position in the open batch, count[b] % L, is read once at the start of the launch and then
// counted along with the draws (uniform: no 64-bit division per draw).  The DIAG = 0 instances take an empty argument in
// its place and compile to what they were before the parameter existed.
#pragma once

#include "summary_update.h"

namespace seir {

constexpr int SUM_ROWS = 8;        // waves (rows) per workgroup
constexpr int SUM_JB = 16;         // draws per flush of the by-day tile (24 KiB of LDS)
constexpr int SUM_JMAX = 128;      // draws per launch (12 KiB of carries)
constexpr int SUM_U = 4;           // draws whose loads are in flight together

// One set of moment accumulators and per-draw marginals over a day axis of extent E: E = T for the recorded events
// (summaries, diagnostics), E = H for the forecast.  The host's MomentAcc owns ref .. overflow as one allocation.
struct MomentBufs {
    int32_t *ref;                  // [B][M][E][6]
    int64_t *sum;                  // [B][M][E][6]
    uint64_t *sumsq;               // [B][M][E][6]
    uint64_t *count;               // [B] draws folded since the last reset
    unsigned *overflow;            // [1] sticky: some sumsq reached 2^63
    int64_t *by_day;               // [cap][B][E][3] events by day
    int64_t *by_loc;               // [cap][B][M][3] events by location
    int64_t *state_by_day;         // [cap][B][E][3]
};

// the batch accumulators of the diagnostics; the DIAG = 0 instances of k_summarize get the empty one
template <int DIAG> struct SummaryDiag {};
template <> struct SummaryDiag<1> {
    int64_t *bsum;                 // [B][M][T][6] sum of (x - ref) over the open batch
    uint64_t *bsumsq;              // [B][M][T][6] sum of the closed batches' squared sums
    uint64_t *nbatch;              // [B] closed batches (= count / L, kept for the reader)
    uint64_t L;                    // batch length, >= 1
};

struct __attribute__((aligned(4))) SumEv32 { int32_t k[3]; };
struct __attribute__((aligned(2))) SumEv16 { uint16_t k[3]; };

template <int EV16>
__device__ __forceinline__ void summary_load(const void *__restrict__ tr, size_t cell, bool live, int (&k)[3]) {
    k[0] = k[1] = k[2] = 0;
    if (!live) return;
    if (EV16) {
        const SumEv16 v = reinterpret_cast<const SumEv16 *>(tr)[cell];
        k[0] = v.k[0]; k[1] = v.k[1]; k[2] = v.k[2];
    } else {
        const SumEv32 v = reinterpret_cast<const SumEv32 *>(tr)[cell];
        k[0] = v.k[0]; k[1] = v.k[1]; k[2] = v.k[2];
    }
}

// The pieces of the fold that k_summarize and k_forecast_fold (forecast_kernels.h) share.  Pieces, and not one body templated
// on where the draws come from: as ONE inlined function the loop nest takes 81 VGPRs in k_summarize<0,0> and k_forecast_fold
// where it takes 73 and 69 in the kernels, a wave or two of occupancy.  fold_values, fold_tile_flush, fold_lds_zero and
// fold_load leave the machine code of all five kernels what it was with the text written out; so does chunk_excl_scan, but
// for two independent instructions that change places in the two DIAG instances.  The store of the
// accumulators and the row totals stay written out in both kernels, with the loop nest ("One accumulator, three
// users").

// The chunk step of a prefix over days, also k_scenario_diff's (scenario_kernels.h): the lane's exclusive prefix of v over
// the days so far, from the wave scan inside the 64-day chunk and the carry (LDS, the owning wave's alone) from the chunks
// before, which lane 0 then moves on by the chunk's total.  Every lane of the wave calls it.
__device__ __forceinline__ int chunk_excl_scan(int v, int lane, int &carry) {
    const int inc = wave_incl_scan(v, lane);
    const int cr = carry;
    const int ex = cr + inc - v;
    const int tot = cr + __builtin_amdgcn_readlane(inc, 63);
    if (lane == 0) carry = tot;
    return ex;
}

// The six quantities of a cell: the day's counts, and the state before them from the initial state s0 and the prefix.
__device__ __forceinline__ void fold_values(const int (&k)[3], const int (&s0)[3], const int (&ex)[3], int (&val)[SUMMARY_Q]) {
    val[0] = k[0]; val[1] = k[1]; val[2] = k[2];
    val[3] = s0[0] - ex[0]; val[4] = s0[1] + ex[0] - ex[1]; val[5] = s0[2] + ex[1] - ex[2];
}

// The workgroup's by-day tile, into which the lanes have added their counts with 64-bit LDS atomics: its nj draws onto
// by_day [cap][B][E][3] from slot0, days from t0 -- one global atomic per entry that is not zero, which is zero again
// afterwards.  Between two __syncthreads of the caller.
__device__ __forceinline__ void fold_tile_flush(unsigned long long (&bd)[SUM_JB][64][3], int nj, int64_t *by_day, int slot0, int B,
                                                int b, int E, int t0) {
    for (int i = threadIdx.x; i < nj * 64 * 3; i += 64 * SUM_ROWS) {
        const unsigned long long v = (&bd[0][0][0])[i];
        const int jj = i / 192, r = i - jj * 192, tl = r / 3, x = r - tl * 3;
        if (v != 0ull) {
            (&bd[0][0][0])[i] = 0ull;
            atomicAdd(reinterpret_cast<unsigned long long *>(by_day) + (((size_t)(slot0 + jj) * B + b) * E + (t0 + tl)) * 3 + x, v);
        }
    }
}

// Zero the workgroup's by-day tile and the wave's carries of `count` draws.  Before a __syncthreads of the caller.
__device__ __forceinline__ void fold_lds_zero(unsigned long long (&bd)[SUM_JB][64][3], int (&carry)[SUM_JMAX][3], int count, int lane) {
    for (int i = lane; i < count * 3; i += 64) (&carry[0][0])[i] = 0;
    for (int i = threadIdx.x; i < SUM_JB * 64 * 3; i += 64 * SUM_ROWS) (&bd[0][0][0])[i] = 0ull;
}

// A cell's six (ref, sum, sumsq) triples into registers.
__device__ __forceinline__ void fold_load(const MomentBufs &sb, size_t cell, int32_t (&ref)[SUMMARY_Q], int64_t (&sm)[SUMMARY_Q],
                                          uint64_t (&sq)[SUMMARY_Q]) {
#pragma unroll
    for (int q = 0; q < SUMMARY_Q; ++q) {
        ref[q] = sb.ref[cell * SUMMARY_Q + q];
        sm[q] = sb.sum[cell * SUMMARY_Q + q];
        sq[q] = sb.sumsq[cell * SUMMARY_Q + q];
    }
}
// grid (ceil(M / SUM_ROWS), B), 64 SUM_ROWS threads.  1 <= count <= SUM_JMAX, first + count <= cap (the host checks).
template <int EV16, int DIAG = 0>
__global__ __launch_bounds__(64 * SUM_ROWS) void k_summarize(Dims d, Consts c, MomentBufs sb,
                                                             const void *__restrict__ tr_events, int B, int first,
                                                             int count, int accumulate, SummaryDiag<DIAG> dg) {
    debug_skew(d);
    __shared__ unsigned long long bd[SUM_JB][64][3];
    __shared__ int carry[SUM_ROWS][SUM_JMAX][3];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y, m = blockIdx.x * SUM_ROWS + wv;
    const int M = d.M, T = d.T;
    const bool row_ok = m < M;
    const bool fold = accumulate != 0;
    const bool fresh = fold && sb.count[b] == 0;      // count moves in k_summary_finish, a launch of its own: no race
    unsigned long long phase = 0ull, blen = 1ull;     // draws already in the open batch at the start of the launch; L
    if constexpr (DIAG) {
        blen = dg.L;
        phase = fold ? sb.count[b] % blen : 0ull;
    }
    int s0[3] = {0, 0, 0};
    if (row_ok)
#pragma unroll
        for (int x = 0; x < 3; ++x) s0[x] = (int)c.init[(size_t)m * 4 + x];
    fold_lds_zero(bd, carry[wv], count, lane);
    __syncthreads();

    const size_t draw_cells = (size_t)B * M * T;      // cells of one trace slot
    bool ovf = false;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const bool live = row_ok && t < T;
        const size_t cell = ((size_t)b * M + (row_ok ? m : 0)) * T + (t < T ? t : 0);
        int32_t ref[seir::SUMMARY_Q];
        int64_t sm[seir::SUMMARY_Q];
        uint64_t sq[seir::SUMMARY_Q];
#pragma unroll
        for (int q = 0; q < seir::SUMMARY_Q; ++q) { ref[q] = 0; sm[q] = 0; sq[q] = 0; }
        int64_t bs[DIAG ? seir::SUMMARY_Q : 1];
        uint64_t bq[DIAG ? seir::SUMMARY_Q : 1];
        if constexpr (DIAG) {
#pragma unroll
            for (int q = 0; q < seir::SUMMARY_Q; ++q) { bs[q] = 0; bq[q] = 0; }
        }
        if (fold && live && !fresh) {
            fold_load(sb, cell, ref, sm, sq);
            if constexpr (DIAG) {
#pragma unroll
                for (int q = 0; q < seir::SUMMARY_Q; ++q) {
                    bs[q] = dg.bsum[cell * seir::SUMMARY_Q + q];
                    bq[q] = dg.bsumsq[cell * seir::SUMMARY_Q + q];
                }
            }
        }
        unsigned long long pos = phase;                // uniform: the same draws close a batch in every cell
        for (int jb = 0; jb < count; jb += SUM_JB) {
            const int nj = min(SUM_JB, count - jb);
            for (int ju = 0; ju < nj; ju += SUM_U) {
                int kk[SUM_U][3];
#pragma unroll
                for (int u = 0; u < SUM_U; ++u)
                    summary_load<EV16>(tr_events, (size_t)(first + jb + ju + u) * draw_cells + cell,
                                       live && ju + u < nj, kk[u]);
#pragma unroll
                for (int u = 0; u < SUM_U; ++u) {
                    if (ju + u >= nj) break;                       // uniform
                    const int jj = ju + u, j = jb + jj;
                    int ex[3];
#pragma unroll
                    for (int x = 0; x < 3; ++x) ex[x] = chunk_excl_scan(kk[u][x], lane, carry[wv][j][x]);
                    if (live) {
#pragma unroll
                        for (int x = 0; x < 3; ++x)
                            if (kk[u][x] != 0) atomicAdd(&bd[jj][lane][x], (unsigned long long)kk[u][x]);
                        if (fold) {
                            int val[seir::SUMMARY_Q];
                            fold_values(kk[u], s0, ex, val);
                            const bool is_first = fresh && j == 0;
#pragma unroll
                            for (int q = 0; q < seir::SUMMARY_Q; ++q)
                                ovf |= seir::summary_fold(ref[q], sm[q], sq[q], val[q], is_first);
                            if constexpr (DIAG) {
#pragma unroll
                                for (int q = 0; q < seir::SUMMARY_Q; ++q) seir::summary_batch_add(bs[q], ref[q], val[q]);
                                if (pos + 1 == blen) {             // uniform
#pragma unroll
                                    for (int q = 0; q < seir::SUMMARY_Q; ++q) ovf |= seir::summary_batch_close(bs[q], bq[q]);
                                }
                            }
                        }
                    }
                    if constexpr (DIAG) pos = pos + 1 == blen ? 0ull : pos + 1;
                }
            }
            __syncthreads();
            fold_tile_flush(bd, nj, sb.by_day, first + jb, B, b, T, t0);
            __syncthreads();
        }
        if (fold && live) {
#pragma unroll
            for (int q = 0; q < seir::SUMMARY_Q; ++q) {
                if (fresh) sb.ref[cell * seir::SUMMARY_Q + q] = ref[q];
                sb.sum[cell * seir::SUMMARY_Q + q] = sm[q];
                sb.sumsq[cell * seir::SUMMARY_Q + q] = sq[q];
            }
            if constexpr (DIAG) {
#pragma unroll
                for (int q = 0; q < seir::SUMMARY_Q; ++q) {
                    dg.bsum[cell * seir::SUMMARY_Q + q] = bs[q];
                    dg.bsumsq[cell * seir::SUMMARY_Q + q] = bq[q];
                }
            }
        }
    }
    if constexpr (DIAG)
        if (fold && blockIdx.x == 0 && threadIdx.x == 0) dg.nbatch[b] = (sb.count[b] + (unsigned long long)count) / blen;
    // the carries after the last chunk are the row totals
    if (row_ok)
        for (int i = lane; i < count * 3; i += 64) {
            const int j = i / 3, x = i - j * 3;
            sb.by_loc[(((size_t)(first + j) * B + b) * M + m) * 3 + x] = (int64_t)carry[wv][j][x];
        }
    if (ovf) sb.overflow[0] = 1u;
}

// state_by_day from the finished by_day of trace slot `slot` and count[b] += count when the draws were folded: the body of
// k_summary_finish and k_forecast_finish (one wave per draw and chain).  init0(m, x): the draw's initial state in row m.
template <class Init0>
__device__ __forceinline__ void moment_finish(const MomentBufs sb, int M, int T, int B, int slot, int count,
                                              bool accumulate, Init0 init0) {
    const int lane = threadIdx.x, b = blockIdx.y;
    long long tot0[3] = {0, 0, 0};
    for (int m = lane; m < M; m += 64)
#pragma unroll
        for (int x = 0; x < 3; ++x) tot0[x] += (long long)init0(m, x);
#pragma unroll
    for (int x = 0; x < 3; ++x)
        for (int o = 32; o > 0; o >>= 1) tot0[x] += __shfl_xor(tot0[x], o, 64);
    long long cr[3] = {0, 0, 0};
    const size_t base = ((size_t)slot * B + b) * T;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        long long ex[3];
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            const long long v = t < T ? sb.by_day[(base + t) * 3 + x] : 0ll;
            long long inc = v;
            for (int o = 1; o < 64; o <<= 1) {
                const long long up = __shfl_up(inc, o, 64);
                if (lane >= o) inc += up;
            }
            ex[x] = cr[x] + inc - v;
            cr[x] += __shfl(inc, 63, 64);
        }
        if (t < T) {
            sb.state_by_day[(base + t) * 3 + 0] = tot0[0] - ex[0];
            sb.state_by_day[(base + t) * 3 + 1] = tot0[1] + ex[0] - ex[1];
            sb.state_by_day[(base + t) * 3 + 2] = tot0[2] + ex[1] - ex[2];
        }
    }
    if (accumulate && blockIdx.x == 0 && lane == 0) sb.count[b] += (uint64_t)count;
}

// grid (count, B), one wave.
__global__ __launch_bounds__(64) void k_summary_finish(Dims d, Consts c, MomentBufs sb, int B, int first, int count,
                                                       int accumulate) {
    moment_finish(sb, d.M, d.T, B, first + blockIdx.x, count, accumulate != 0,
                  [&](int m, int x) { return c.init[(size_t)m * 4 + x]; });
}

}  // namespace seir

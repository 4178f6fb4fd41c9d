// Reproduction number of the kept draws, formed where the burst buffer lies (include/seir_hip.h, "Reproduction number on
// the device"): for every draw of trace slots [first, first + count), every day t of the window [T - D, T) and every
// location j, R_it[t][j] exactly as k_rt (rt_kernels.h) forms it -- the same expressions (rt_row_factor, rt_cell,
// rt_combine, rt_period below), the same four partial sums over the source rows -- folded into per-chain moments and into the
// national curve R_t of the draw.  Neither the event tensor nor an [n][D][M] tensor leaves the device, and the sampler's
// live workspace (Work::KS, Work::ea) is not touched: everything below is written into buffers of the feature's own.
//
//   k_rt_tables (rt_kernels.h)  exp(a_t) of the batch's draws from the trace's theta, into RtBufs::ea.
//   k_rt_prepare<EV16>          a wave per (row i, draw): sums k_se of the draw's recorded events over [0, T - D) and scans
//       the D window days, S_it = S0 - sum_{u<t} k_se[u] as integers, into the plane S [ND][Mp][D] (loads as summary_load
//       does, for both trace widths).
//   k_rt_trace<DT>              a workgroup owns, for one chain, 64 destination columns (lane = j) x DT window days.  The
//       loop over the batch's draws is INSIDE: a thread's DT / 4 cells keep ref / sum / sumsq / gt1 in registers across it,
//       so the accumulators cross memory once per launch and no [ND][D][M] staging tensor exists.  Per draw the workgroup
//       puts E_it and S_it of its days into LDS (as k_rt does), wave p sums the rows i = p mod 4 ascending, the partials
//       meet in LDS and are combined as (p0 + p1) + (p2 + p3).  The fold is sequential in draw order with separately
//       rounded operations (no FMA): a NumPy loop restates every bit, and nothing depends on how a burst is cut.
//       R_t: the 64 columns' r * weight[j] are summed over the wave by a butterfly (a fixed order) into
//       part [ND][D][column blocks] -- no floating-point atomics.
//   k_rt_finish                 R_t[slot][b][t] = the column blocks' partials in ascending order; advances count[b].
// The day tile is 4 whatever the size: at D = 14, UK-380 and 8 chains that is 192 workgroups of 32 KiB of LDS, five to a
// CU; 136 KiB at Mp = 2048.  The host bounds the S plane (RT_STAGING_BYTES) by cutting a call into batches of slots.
// Ordinary launches on the context stream: no hand-off inside a launch, no persistence.
#pragma once

#include "rt_kernels.h"
#include "summary_kernels.h"

namespace seir {

constexpr int RT_DT = 4;                         // window days per workgroup of k_rt_trace
constexpr int RT_PREP_ROWS = 8;                  // waves (rows) per workgroup of k_rt_prepare
constexpr size_t RT_STAGING_BYTES = 64u << 20;   // bound on the S plane of a batch (at least one slot is always taken)

struct RtBufs {
    int D;                         // window days
    int t0;                        // first day of the window, T - D
    int ncb;                       // column blocks, ceil(M / 64)
    const double *weight;          // [ncb * 64] national weights, zero beyond M
    double *ea;                    // [ND][Tp] exp(a_t) of the batch's draws
    int *S;                        // [ND][Mp][D] S_it of the batch's draws over the window
    double *part;                  // [ND][D][ncb] partial national sums of the batch
    double *Rt;                    // [cap][B][D] national curve per kept draw, indexed by trace slot
    double *ref, *sum, *sumsq;     // [B][D][M]
    uint32_t *gt1;                 // [B][D][M] draws with r > 1
    uint64_t *count;               // [B] draws folded since the last reset
};

// grid (ceil(M / RT_PREP_ROWS), ND), 64 RT_PREP_ROWS threads; nd = slot_in_batch * B + chain
template <int EV16>
__global__ __launch_bounds__(64 * RT_PREP_ROWS) void k_rt_prepare(Dims d, Consts c, RtBufs rb,
                                                                  const void *__restrict__ tr_events, int B, int first) {
    debug_skew(d);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nd = blockIdx.y, i = blockIdx.x * RT_PREP_ROWS + wv;
    const int M = d.M, T = d.T, D = rb.D;
    if (i >= M) return;
    const int jj = nd / B, b = nd - jj * B, slot = first + jj;
    const size_t row = (((size_t)slot * B + b) * M + i) * T;
    int pre = 0;
    for (int t = lane; t < rb.t0; t += 64) {
        int k[3];
        summary_load<EV16>(tr_events, row + t, true, k);
        pre += k[0];
    }
    for (int o = 32; o > 0; o >>= 1) pre += __shfl_xor(pre, o, 64);
    int run = (int)c.init[(size_t)i * 4] - pre;      // S at the start of day T - D
    int *out = rb.S + ((size_t)nd * d.Mp + i) * D;
    for (int w0 = 0; w0 < D; w0 += 64) {
        const int tw = w0 + lane;
        const bool live = tw < D;
        int k[3];
        summary_load<EV16>(tr_events, row + rb.t0 + (live ? tw : 0), live, k);
        const int inc = wave_incl_scan(k[0], lane);
        if (live) out[tw] = run - (inc - k[0]);
        run -= __builtin_amdgcn_readlane(inc, 63);
    }
}

// The cell arithmetic of R_it, with k_rt's expressions repeated operation for operation (rt_kernels.h; k_rt itself calling
// these functions moves one instruction of its machine code, so its text stays as it is and tests/test_rt_device_gpu.py
// holds the two to the same bits):
//   rt_row_factor  E_it = exp(a_t) exp(beta l_i) / N_i
//   rt_cell        one source row's term added to a partial sum: acc + S_it (1 - exp(-x)),
//                  x = E_it f_j (delta_ij + psi W_t Cstar_ij / N_j)
//   rt_combine     the four partials (i = p mod 4, ascending) as (p0 + p1) + (p2 + p3), times the infectious period
//   rt_period      1 / (1 - exp(-exp(gamma0))), model_spec.py:361-363
__device__ __forceinline__ double rt_row_factor(double ea, double beta, double la, double invN) { return ea * exp(beta * la) * invN; }
__device__ __forceinline__ double rt_cell(double acc, double E, double S, double fj, double dlt, double pw, double cij) {
    const double x = E * fj * (dlt + pw * cij);
    acc += S * prob_of_rate(x);
    return acc;
}
__device__ __forceinline__ double rt_combine(double p0, double p1, double p2, double p3, double period) {
    const double v = (p0 + p1) + (p2 + p3);
    return v * period;
}
__device__ __forceinline__ double rt_period(double g0) { return 1.0 / (1.0 - exp(-exp(g0))); }

// One draw's r into a cell's accumulators: separately rounded operations, no FMA, so that the host restates them bit for bit.
__device__ __forceinline__ void rt_fold(double r, double ref, double &sm, double &sq) {
#pragma clang fp contract(off)
    const double dv = r - ref;
    const double d2 = dv * dv;
    sm = sm + dv;
    sq = sq + d2;
}
// sum over the wave of v, by a butterfly: every lane ends with the same value, formed in one fixed order
__device__ __forceinline__ double rt_wave_sum(double v) {
#pragma clang fp contract(off)
    for (int o = 32; o > 0; o >>= 1) {
        const double u = __shfl_xor(v, o, 64);
        v = v + u;
    }
    return v;
}
__device__ __forceinline__ double rt_weighted(double r, double w) {
#pragma clang fp contract(off)
    const double v = r * w;
    return v;
}

template <int DT>
constexpr size_t k_rt_trace_lds_bytes(int Mp) { return sizeof(double) * ((size_t)2 * DT * Mp + 4 * DT * WAVE); }
// k_rt_trace has no static LDS: the dynamic part is all of it
static_assert(k_rt_trace_lds_bytes<RT_DT>(2048) <= 160 * 1024, "k_rt_trace's day tile must fit a workgroup's LDS at Mp = 2048");

// Where a live cell's r goes besides the fold and the national partials (rt_trace_body's SINK):
//   RT_SINK_NONE    nowhere (k_rt_trace);
//   RT_SINK_KEEP    the draw store out [B][D][M][ld], the draw index innermost, at position count[b] (at the kernel's entry)
//                   + the draw's index in the launch (k_rt_trace_keep, rt_keep_kernels.h, which describes the write);
//   RT_SINK_CELLS   the plane out [count * B][D][ld], ld >= M (k_rt_trace_cells, group_curve_kernels.h).
constexpr int RT_SINK_NONE = 0, RT_SINK_KEEP = 1, RT_SINK_CELLS = 2;
constexpr int RT_KEEP_RUN = 4;                   // draws staged per cell of the draw store: a 32-byte run along the draw axis

// The one statement of the R_it contraction of a batch: the loop over the draws, the fold, the national partials and the
// sink.  Its three kernels are __global__ wrappers with nothing else in them, so fold, partials and the r a sink receives
// are the same bits whichever runs.  Dims, Consts and RtBufs come BY VALUE, as a kernel's own parameters: taken by
// reference the keep instance spills scalar registers.
template <int DT, int SINK>
__device__ __forceinline__ void rt_trace_body(Dims d, Consts c, RtBufs rb, const double *__restrict__ tr_theta, int B, int first,
                                              int count, double *__restrict__ out, long long ld) {
    static_assert(DT % 4 == 0 && (DT & (DT - 1)) == 0, "a wave owns the days tt = wave mod 4 of the tile");
    static_assert(RT_KEEP_RUN == 4, "a run is two double2 stores");
    debug_skew(d);
    extern __shared__ double lds[];                      // E [DT][Mp] | S [DT][Mp] | red [4][DT][64]
    constexpr int NC = DT / 4;                           // cells per thread: days tt = cc * 4 + wave, column j
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.z, j = blockIdx.x * WAVE + lane, w0 = blockIdx.y * DT;
    const int M = d.M, D = rb.D;
    double *E = lds, *S = lds + DT * d.Mp, *red = S + DT * d.Mp;
    const bool jin = j < M;
    const double inj = jin ? c.invN[j] : 0.0;
    const double wj = rb.weight[j];
    const unsigned long long pos0 = rb.count[b];         // count moves in k_rt_finish, a launch of its own: no race
    const bool fresh = pos0 == 0;
    double ref[NC], sm[NC], sq[NC], st[NC][RT_KEEP_RUN];
    uint32_t g1[NC];
    bool live[NC];
    size_t cell[NC];
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) {
        const int tw = w0 + cc * 4 + wave;
        live[cc] = jin && tw < D;
        cell[cc] = ((size_t)b * D + (tw < D ? tw : 0)) * M + (jin ? j : 0);
        ref[cc] = sm[cc] = sq[cc] = 0.0;
        g1[cc] = 0u;
        if constexpr (SINK == RT_SINK_KEEP) {
#pragma unroll
            for (int k = 0; k < RT_KEEP_RUN; ++k) st[cc][k] = 0.0;
        }
        if (live[cc] && !fresh) {
            ref[cc] = rb.ref[cell[cc]]; sm[cc] = rb.sum[cell[cc]]; sq[cc] = rb.sumsq[cell[cc]]; g1[cc] = rb.gt1[cell[cc]];
        }
    }
    int lo = (int)(pos0 & (RT_KEEP_RUN - 1));            // KEEP: first position of the current run that this launch owns
    for (int jd = 0; jd < count; ++jd) {
        const int nd = jd * B + b;
        const double *th = tr_theta + ((size_t)(first + jd) * B + b) * d.P;
        const double psi = th[0], sig = th[1], beta = th[2], g0 = th[3];
        for (int idx = threadIdx.x; idx < DT * d.Mp; idx += 256) {
            const int i = idx / DT, tt = idx - i * DT, tw = w0 + tt;
            double e = 0.0, sv = 0.0;
            if (i < M && tw < D) {
                e = rt_row_factor(rb.ea[(size_t)nd * d.Tp + rb.t0 + tw], beta, c.la[i], c.invN[i]);
                sv = (double)rb.S[((size_t)nd * d.Mp + i) * D + tw];         // S at the start of day t
            }
            E[tt * d.Mp + i] = e;
            S[tt * d.Mp + i] = sv;
        }
        __syncthreads();
        double pw[DT], acc[DT];
#pragma unroll
        for (int tt = 0; tt < DT; ++tt) { pw[tt] = (w0 + tt < D) ? psi * c.W[rb.t0 + w0 + tt] : 0.0; acc[tt] = 0.0; }
        const double fj = jin ? exp(sig * th[6 + d.T - 1 + j]) : 0.0;
        for (int i = wave; i < M; i += 4) {
            const double cij = jin ? c.Cstar[(size_t)i * d.Kp0 + j] * inj : 0.0;
            const double dlt = (i == j) ? 1.0 : 0.0;
#pragma unroll
            for (int tt = 0; tt < DT; ++tt) acc[tt] = rt_cell(acc[tt], E[tt * d.Mp + i], S[tt * d.Mp + i], fj, dlt, pw[tt], cij);
        }
#pragma unroll
        for (int tt = 0; tt < DT; ++tt) red[(wave * DT + tt) * WAVE + lane] = acc[tt];
        __syncthreads();
        const double period = rt_period(g0);
        const bool is_first = fresh && jd == 0;
        // KEEP: this draw's place in the store: position pos, slot `at` of the run that starts at pos - at (uniform in the grid)
        const unsigned long long pos = pos0 + (unsigned long long)jd;
        const int at = (int)(pos & (RT_KEEP_RUN - 1));
        const bool flush = at == RT_KEEP_RUN - 1 || jd == count - 1;
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) {
            const int tt = cc * 4 + wave, tw = w0 + tt;
            const double r = rt_combine(red[(0 * DT + tt) * WAVE + lane], red[(1 * DT + tt) * WAVE + lane],
                                        red[(2 * DT + tt) * WAVE + lane], red[(3 * DT + tt) * WAVE + lane], period);
            if (live[cc]) {
                if (is_first) ref[cc] = r;
                rt_fold(r, ref[cc], sm[cc], sq[cc]);
                g1[cc] += r > 1.0 ? 1u : 0u;
                if constexpr (SINK == RT_SINK_CELLS)
                    out[((size_t)nd * D + tw) * (size_t)ld + j] = r;         // the wave's 64 columns: 512 contiguous bytes
            }
            const double nat = rt_wave_sum(live[cc] ? rt_weighted(r, wj) : 0.0);
            if (lane == 0 && tw < D) rb.part[((size_t)nd * D + tw) * rb.ncb + blockIdx.x] = nat;
            if constexpr (SINK == RT_SINK_KEEP) {
#pragma unroll
                for (int k = 0; k < RT_KEEP_RUN; ++k) st[cc][k] = (k == at) ? r : st[cc][k];
                if (flush && live[cc] && pos < (unsigned long long)ld) {     // the host has refused a call past the cap
                    double *run = out + cell[cc] * (size_t)ld + (size_t)(pos - (unsigned long long)at);
                    if (lo == 0 && at == RT_KEEP_RUN - 1) {
                        // a whole run: 32 bytes, aligned to 32
                        reinterpret_cast<double2 *>(run)[0] = make_double2(st[cc][0], st[cc][1]);
                        reinterpret_cast<double2 *>(run)[1] = make_double2(st[cc][2], st[cc][3]);
                    } else {
                        // ragged: the positions [lo, at] of the run are this launch's, the others are not touched
#pragma unroll
                        for (int k = 0; k < RT_KEEP_RUN; ++k)
                            if (k >= lo && k <= at) run[k] = st[cc][k];
                    }
                }
            }
        }
        if constexpr (SINK == RT_SINK_KEEP)
            if (flush) lo = 0;
        // the next draw's E and S are written behind the barrier above, its partials behind the one that follows them:
        // red is read here before this wave reaches that barrier
    }
#pragma unroll
    for (int cc = 0; cc < NC; ++cc)
        if (live[cc]) {
            if (fresh) rb.ref[cell[cc]] = ref[cc];
            rb.sum[cell[cc]] = sm[cc]; rb.sumsq[cell[cc]] = sq[cc]; rb.gt1[cell[cc]] = g1[cc];
        }
}

// grid (ncb, ceil(D / DT), B), 256 threads.  Slots [first, first + count) of the trace; nd0 = 0 .. of the batch's planes.
template <int DT>
__global__ __launch_bounds__(256) void k_rt_trace(Dims d, Consts c, RtBufs rb, const double *__restrict__ tr_theta, int B,
                                                  int first, int count) {
    rt_trace_body<DT, RT_SINK_NONE>(d, c, rb, tr_theta, B, first, count, nullptr, 0);
}

// grid (ceil(count * B * D / 256)), 256 threads: the national curve of the batch's draws from their column-block partials,
// summed in ascending block order; count[b] += count.
__global__ __launch_bounds__(256) void k_rt_finish(RtBufs rb, int B, int first, int count) {
    const int D = rb.D;
    const size_t n = (size_t)count * B * D, idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < n) {
        const double *p = rb.part + idx * rb.ncb;        // idx = (nd * D + tw), nd = jd * B + b: the slot-major order of Rt
        double v = p[0];
        for (int cb = 1; cb < rb.ncb; ++cb) v += p[cb];
        rb.Rt[(size_t)first * B * D + idx] = v;
    }
    if (blockIdx.x == 0)
        for (int b = threadIdx.x; b < B; b += 256) rb.count[b] += (uint64_t)count;
}

}  // namespace seir

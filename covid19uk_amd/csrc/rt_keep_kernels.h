// The R_it draw store (include/seir_hip.h, "R_t intervals on the device"): k_rt_trace_keep is k_rt_trace
// (rt_trace_kernels.h) with one thing more -- every live cell's r of every draw is left in
//   keepR [B][D][M][stride]   fp64, the draw index innermost, stride = the store's cap rounded up to RT_KEEP_RUN,
// at position count[b] (at the kernel's entry; it moves in k_rt_finish, a launch of its own) + the draw's index in the
// launch.  While the store is on it is launched IN PLACE of k_rt_trace: R_it is formed once, by the same inline functions
// (rt_row_factor, rt_cell, rt_combine, rt_period, rt_fold, rt_wave_sum, rt_weighted) in the same order, so fold, national
// partials and the stored r are the bits of k_rt_trace.  k_rt_trace's text is restated, not shared: it stays the parent's
// machine code.
//
// The write.  A lane owns a column j, so successive draws of its cell are 8 B apart while the lanes of a wave are
// stride x 8 B apart: one store per lane per draw would be 64 separate 8-byte writes.  A thread therefore stages
// RT_KEEP_RUN = 4 consecutive draws of its cell in registers and writes them as one 32-byte run aligned to 32 bytes (two
// 16-byte stores; the store's base and stride keep every run aligned).  A run is cut by positions, not by the launch: the
// first run of a launch that starts off a run boundary and the last run of a launch that ends off one are ragged and go
// out as 8-byte stores of exactly the positions the launch owns.  Nothing is read back, nothing beyond the launch's
// positions is written: a launch of n draws writes B x D x M x n x 8 bytes into the store, whatever the cut.
#pragma once

#include "rt_trace_kernels.h"

namespace seir {

constexpr int RT_KEEP_RUN = 4;                   // draws staged per cell: a 32-byte run along the draw axis

// grid (ncb, ceil(D / DT), B), 256 threads, k_rt_trace's dynamic LDS.  keep [B][D][M][stride], stride % RT_KEEP_RUN == 0.
template <int DT>
__global__ __launch_bounds__(256) void k_rt_trace_keep(Dims d, Consts c, RtBufs rb, const double *__restrict__ tr_theta, int B,
                                                       int first, int count, double *__restrict__ keep, long long stride) {
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
#pragma unroll
        for (int k = 0; k < RT_KEEP_RUN; ++k) st[cc][k] = 0.0;
        if (live[cc] && !fresh) {
            ref[cc] = rb.ref[cell[cc]]; sm[cc] = rb.sum[cell[cc]]; sq[cc] = rb.sumsq[cell[cc]]; g1[cc] = rb.gt1[cell[cc]];
        }
    }
    int lo = (int)(pos0 & (RT_KEEP_RUN - 1));            // first position of the current run that this launch owns
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
        // this draw's place in the store: position pos, slot `at` of the run that starts at pos - at (uniform in the grid)
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
            }
            const double nat = rt_wave_sum(live[cc] ? rt_weighted(r, wj) : 0.0);
            if (lane == 0 && tw < D) rb.part[((size_t)nd * D + tw) * rb.ncb + blockIdx.x] = nat;
#pragma unroll
            for (int k = 0; k < RT_KEEP_RUN; ++k) st[cc][k] = (k == at) ? r : st[cc][k];
            if (flush && live[cc] && pos < (unsigned long long)stride) {      // the host has refused a call past the cap
                double *run = keep + cell[cc] * (size_t)stride + (size_t)(pos - (unsigned long long)at);
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

}  // namespace seir

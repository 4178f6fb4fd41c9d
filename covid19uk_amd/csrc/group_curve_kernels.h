// Group curves: R_t and the within / between pressures of every kept draw per group of locations (include/seir_hip.h,
// "Group curves on the device").  THE definition of a group sum of fp64 values:
//
//   For one draw, one day and one group g of the table (a CSR pair, group_kernels.h) let the members be m_0 < ... < m_{n-1}
//   in CSR order, w_k the optional weights aligned with `members`, and v the day's vector over the locations.
//     - lane l in [0, 64) starts from a_l = +0.0;
//     - for k = l, l + 64, l + 128, ... < n, ascending:  p = w_k * v[m_k] (one rounding; unweighted: p = v[m_k]), then
//       a_l = a_l + p (one rounding);
//     - then for o = 32, 16, 8, 4, 2, 1, all lanes at once:  a_l = a_l + a_{l xor o};
//     - the result is a_0.
//   No FMA anywhere (#pragma clang fp contract(off), as rt_fold and rt_wave_sum), no floating-point atomics.  The order
//   depends on the table alone: not on the launch geometry, on debug_skew, or on how a burst is cut into calls, buffer
//   halves or batches.  covid19uk_amd/posterior/groups.py (weighted_sum_rows) restates it in NumPy.
//
//   k_group_wsums<WEIGHTED>   a WAVE owns one (draw, group, day), a lane a member position modulo 64; the input is a cell plane
//       v [nd][L][ld] (fp64, day-major, the members along the contiguous axis, ld >= M the row length), the output
//       out [.][G][L].  A workgroup is GC_WAVES = 4 waves: four consecutive days of one (draw, group), so the member indices
//       and weights a wave loads are the same addresses in its three neighbours (L1 hits) and the four results are 32
//       contiguous bytes.  Nothing is shared between the waves: no LDS, no barrier, so the day tile cannot enter the bits.
//       A lane's loads of GC_U positions are issued before the first add; the adds stay in ascending order.
//   k_rt_trace_cells<DT>      k_rt_trace (rt_trace_kernels.h) with one thing more: every live cell's r, the bits it folds, is
//       stored into the plane Rc [nd][D][ld].  Launched in place of k_rt_trace while group R_t is on and the draw store is
//       off; through the same inline functions in the same order, so fold and national partials are k_rt_trace's bits.
//       k_rt_trace's text is restated, not shared: it stays the parent's machine code.
//   k_rt_cells_from_keep      while the draw store is on k_rt_trace_keep has left every draw's r in keepR [B][D][M][stride]:
//       a gather of the batch's positions into the same plane Rc.  A thread owns a cell and walks the batch's draws: its
//       reads are consecutive 8-byte words of one run of the store, its writes are contiguous over the wave.
//   k_wb_trace_cells<DT>      k_wb_trace (wb_kernels.h) likewise: wi and be of every live cell into two planes [nd][D][ld],
//       whether the draw is defined or not, as the national sums take them.
// All are ordinary launches on the context stream: no hand-off inside a launch, no persistence.
#pragma once

#include "group_kernels.h"
#include "rt_keep_kernels.h"
#include "wb_kernels.h"

namespace seir {

constexpr int GC_WAVES = 4;        // waves per workgroup of k_group_wsums: consecutive days of one (draw, group)
constexpr int GC_U = 4;            // member positions of a lane whose loads are in flight together

// One term into a lane's sum, and the butterfly over the wave: separately rounded operations.
__device__ __forceinline__ double gc_add(double a, double p) {
#pragma clang fp contract(off)
    const double s = a + p;
    return s;
}
__device__ __forceinline__ double gc_term(double w, double v) {
#pragma clang fp contract(off)
    const double p = w * v;
    return p;
}
__device__ __forceinline__ double gc_wave_sum(double v) {
#pragma clang fp contract(off)
    for (int o = 32; o > 0; o >>= 1) {
        const double u = __shfl_xor(v, o, 64);
        v = v + u;
    }
    return v;
}

// grid (G * ceil(L / GC_WAVES), nd <= GRP_NDMAX), 64 GC_WAVES threads.  Draw blockIdx.y of the launch is draw v_d0 + blockIdx.y
// of v [.][L][ld] and draw out_d0 + blockIdx.y of out [.][G][L].  offsets [G + 1], members / weights [nnz]; every member is in
// [0, M) with M <= ld (the host checks).  weights is not read when WEIGHTED == 0.
template <int WEIGHTED>
__global__ __launch_bounds__(64 * GC_WAVES) void k_group_wsums(Dims d, const int *__restrict__ offsets,
                                                               const int *__restrict__ members,
                                                               const double *__restrict__ weights,
                                                               const double *__restrict__ v, int G, int L, long long ld,
                                                               int nchunk, long long v_d0, long long out_d0,
                                                               double *__restrict__ out) {
    debug_skew(d);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int g = blockIdx.x / nchunk, t = (blockIdx.x - g * nchunk) * GC_WAVES + wv;
    if (t >= L) return;                                  // the whole wave: nothing is shared with the others
    const int beg = offsets[g], end = offsets[g + 1];
    const double *row = v + ((size_t)(v_d0 + blockIdx.y) * L + t) * (size_t)ld;
    double a = 0.0;
    for (int k0 = beg + lane; k0 < end; k0 += 64 * GC_U) {
        double p[GC_U];
#pragma unroll
        for (int u = 0; u < GC_U; ++u) {
            const int k = k0 + u * 64;
            const bool on = k < end;
            const int kk = on ? k : beg;
            const double x = row[members[kk]];
            p[u] = WEIGHTED ? gc_term(weights[kk], x) : x;
            if (!on) p[u] = 0.0;
        }
#pragma unroll
        for (int u = 0; u < GC_U; ++u)
            if (k0 + u * 64 < end) a = gc_add(a, p[u]);
    }
    a = gc_wave_sum(a);
    if (lane == 0) out[((size_t)(out_d0 + blockIdx.y) * G + g) * L + t] = a;
}

// grid (ncb, ceil(D / DT), B), 256 threads, k_rt_trace's dynamic LDS.  Rc [count * B][D][ld], ld >= M.
template <int DT>
__global__ __launch_bounds__(256) void k_rt_trace_cells(Dims d, Consts c, RtBufs rb, const double *__restrict__ tr_theta, int B,
                                                        int first, int count, double *__restrict__ Rc, long long ld) {
    static_assert(DT % 4 == 0 && (DT & (DT - 1)) == 0, "a wave owns the days tt = wave mod 4 of the tile");
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
    const bool fresh = rb.count[b] == 0;                 // count moves in k_rt_finish, a launch of its own: no race
    double ref[NC], sm[NC], sq[NC];
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
        if (live[cc] && !fresh) {
            ref[cc] = rb.ref[cell[cc]]; sm[cc] = rb.sum[cell[cc]]; sq[cc] = rb.sumsq[cell[cc]]; g1[cc] = rb.gt1[cell[cc]];
        }
    }
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
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) {
            const int tt = cc * 4 + wave, tw = w0 + tt;
            const double r = rt_combine(red[(0 * DT + tt) * WAVE + lane], red[(1 * DT + tt) * WAVE + lane],
                                        red[(2 * DT + tt) * WAVE + lane], red[(3 * DT + tt) * WAVE + lane], period);
            if (live[cc]) {
                if (is_first) ref[cc] = r;
                rt_fold(r, ref[cc], sm[cc], sq[cc]);
                g1[cc] += r > 1.0 ? 1u : 0u;
                Rc[((size_t)nd * D + tw) * (size_t)ld + j] = r;              // the wave's 64 columns: 512 contiguous bytes
            }
            const double nat = rt_wave_sum(live[cc] ? rt_weighted(r, wj) : 0.0);
            if (lane == 0 && tw < D) rb.part[((size_t)nd * D + tw) * rb.ncb + blockIdx.x] = nat;
        }
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

// grid (ceil(M / 256), D, B), 256 threads.  keep [B][D][M][stride]; the draw jd of the batch is position pos0 + jd of every
// cell (pos0 + count <= stride: the host has refused a call past the cap).  Rc [count * B][D][ld].
__global__ __launch_bounds__(256) void k_rt_cells_from_keep(Dims d, const double *__restrict__ keep, long long stride,
                                                            long long pos0, int B, int D, int count, double *__restrict__ Rc,
                                                            long long ld) {
    debug_skew(d);
    const int m = blockIdx.x * 256 + threadIdx.x, tw = blockIdx.y, b = blockIdx.z;
    if (m >= d.M) return;
    const double *src = keep + (((size_t)b * D + tw) * d.M + m) * (size_t)stride + (size_t)pos0;
    for (int jd = 0; jd < count; ++jd)
        Rc[(((size_t)jd * B + b) * D + tw) * (size_t)ld + m] = src[jd];
}

// grid (ncb, ceil(D / DT), B), 256 threads, k_wb_trace's dynamic LDS.  Wc, Bc [count * B][D][ld], ld >= M.
template <int DT>
__global__ __launch_bounds__(256) void k_wb_trace_cells(Dims d, Consts c, WbBufs wb, const double *__restrict__ tr_theta, int B,
                                                        int first, int count, double *__restrict__ Wc, double *__restrict__ Bc,
                                                        long long ld) {
    static_assert(DT % 4 == 0 && (DT & (DT - 1)) == 0, "a wave owns the days tt = wave mod 4 of the tile");
    debug_skew(d);
    extern __shared__ double lds[];                      // x [DT][Mp] | red [4][DT][64]
    constexpr int NC = DT / 4;                           // cells per thread: days tt = cc * 4 + wave, column m
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.z, m = blockIdx.x * WAVE + lane, w0 = blockIdx.y * DT;
    const int M = d.M, D = wb.D, Mp = d.Mp;
    double *X = lds, *red = lds + (size_t)DT * Mp;
    const bool min_ = m < M;
    const int mm = min_ ? m : 0;
    const double cmm = min_ ? c.Cstar[(size_t)m * d.Kp0 + m] : 0.0;
    uint32_t n[NC], gt[NC];
    double ref_w[NC], sum_w[NC], sumsq_w[NC], ref_b[NC], sum_b[NC];
    bool live[NC];
    size_t cell[NC];
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) {
        const int tw = w0 + cc * 4 + wave;
        live[cc] = min_ && tw < D;
        cell[cc] = ((size_t)b * D + (tw < D ? tw : 0)) * M + mm;
        n[cc] = gt[cc] = 0u;
        ref_w[cc] = sum_w[cc] = sumsq_w[cc] = ref_b[cc] = sum_b[cc] = 0.0;
        if (live[cc]) {
            n[cc] = wb.n[cell[cc]]; gt[cc] = wb.gt[cell[cc]];
            ref_w[cc] = wb.ref_w[cell[cc]]; sum_w[cc] = wb.sum_w[cell[cc]]; sumsq_w[cc] = wb.sumsq_w[cell[cc]];
            ref_b[cc] = wb.ref_b[cell[cc]]; sum_b[cc] = wb.sum_b[cell[cc]];
        }
    }
    for (int jd = 0; jd < count; ++jd) {
        const int nd = jd * B + b;
        const double psi = tr_theta[((size_t)(first + jd) * B + b) * d.P];
        const int *Ip = wb.I + (size_t)nd * D * Mp;
        for (int idx = threadIdx.x; idx < DT * Mp; idx += 256) {
            const int tt = idx / Mp, i = idx - tt * Mp, tw = w0 + tt;
            double x = 0.0;
            if (i < M && tw < D) x = wb_x((double)Ip[(size_t)tw * Mp + i], c.invN[i]);
            X[idx] = x;
        }
        __syncthreads();
        double F[DT];
#pragma unroll
        for (int tt = 0; tt < DT; ++tt) F[tt] = 0.0;
        for (int j = wave; j < M; j += 4) {
            const double cjm = min_ ? c.Cstar[(size_t)j * d.Kp0 + m] : 0.0;
            const bool diag = j == m;
#pragma unroll
            for (int tt = 0; tt < DT; ++tt) F[tt] = wb_row(F[tt], cjm, diag, X[tt * Mp + j]);
        }
#pragma unroll
        for (int tt = 0; tt < DT; ++tt) red[(wave * DT + tt) * WAVE + lane] = F[tt];
        // x of the cell's own row is read here, in front of the barrier: behind it another wave may already write the next draw's
        double xm[NC], Iv[NC], pw[NC];
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) {
            const int tt = cc * 4 + wave, tw = w0 + tt;
            xm[cc] = X[tt * Mp + mm];
            Iv[cc] = live[cc] ? (double)Ip[(size_t)tw * Mp + m] : 0.0;
            pw[cc] = tw < D ? psi * c.W[wb.t0 + tw] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) {
            const int tt = cc * 4 + wave, tw = w0 + tt;
            double wi, be, fw, fb;
            wb_cell(Iv[cc], pw[cc], cmm, xm[cc], red[(0 * DT + tt) * WAVE + lane], red[(1 * DT + tt) * WAVE + lane],
                    red[(2 * DT + tt) * WAVE + lane], red[(3 * DT + tt) * WAVE + lane], wi, be, fw, fb);
            if (live[cc] && wb_finite(fw) && wb_finite(fb))
                wb_fold(fw, fb, n[cc], ref_w[cc], sum_w[cc], sumsq_w[cc], ref_b[cc], sum_b[cc], gt[cc]);
            if (live[cc]) {                                                  // defined or not, as the national sums
                const size_t at = ((size_t)nd * D + tw) * (size_t)ld + m;
                Wc[at] = wi; Bc[at] = be;
            }
            const double nw = wb_wave_sum(live[cc] ? wi : 0.0), nb = wb_wave_sum(live[cc] ? be : 0.0);
            if (lane == 0 && tw < D) {
                double *p = wb.part + (((size_t)nd * D + tw) * wb.ncb + blockIdx.x) * 2;
                p[0] = nw; p[1] = nb;
            }
        }
        // the next draw's x is written behind the barrier above, its partials behind the one that follows them: red is read
        // here before this wave reaches that barrier
    }
#pragma unroll
    for (int cc = 0; cc < NC; ++cc)
        if (live[cc]) {
            wb.n[cell[cc]] = n[cc]; wb.gt[cell[cc]] = gt[cc];
            wb.ref_w[cell[cc]] = ref_w[cc]; wb.sum_w[cell[cc]] = sum_w[cc]; wb.sumsq_w[cell[cc]] = sumsq_w[cc];
            wb.ref_b[cell[cc]] = ref_b[cc]; wb.sum_b[cell[cc]] = sum_b[cc];
        }
}

}  // namespace seir

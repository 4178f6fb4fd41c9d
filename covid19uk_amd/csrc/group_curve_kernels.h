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
//       off; both are wrappers over the one rt_trace_body (this one its RT_SINK_CELLS instance), so fold and national
//       partials are k_rt_trace's bits.
//   k_rt_cells_from_keep      while the draw store is on k_rt_trace_keep has left every draw's r in keepR [B][D][M][stride]:
//       a gather of the batch's positions into the same plane Rc.  A thread owns a cell and walks the batch's draws: its
//       reads are consecutive 8-byte words of one run of the store, its writes are contiguous over the wave.
//   k_wb_trace_cells<DT>      k_wb_trace (wb_kernels.h) likewise, over wb_trace_body: wi and be of every live cell into two
//       planes [nd][D][ld], whether the draw is defined or not, as the national sums take them.
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
    rt_trace_body<DT, RT_SINK_CELLS>(d, c, rb, tr_theta, B, first, count, Rc, ld);
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
    wb_trace_body<DT, true>(d, c, wb, tr_theta, B, first, count, Wc, Bc, ld);
}

}  // namespace seir

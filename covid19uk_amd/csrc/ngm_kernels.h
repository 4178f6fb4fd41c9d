// Group next-generation matrix of the kept draws (include/seir_hip.h, "Group next-generation matrix on the device"):
// K[g][h][t], the expected infections in group g caused by one typical infective of group h on day t -- who infects whom
// by region.  R_t_by_group[h] is its sum over every destination; the split by destination group is what this file keeps.
// THE definition (covid19uk_amd/posterior/groups.py restates it in NumPy: ngm_rows, group_ngm):
//
//   For one draw, one window day t in [T - D, T) and the table of groups (a CSR pair offsets / members, members ascending
//   within a group, group_kernels.h); weights [nnz] aligned with members.
//
//   Rows plane.  For a destination group g with members m_0 < ... < m_{n-1} and every source column j:
//     - partial sum p in {0, 1, 2, 3} starts from +0.0 and adds the member POSITIONS k = p, p + 4, ... ascending:
//         acc = rt_cell(acc, E[m_k][t], S[m_k][t], f_j, delta(m_k, j), psi W_t, Cstar[m_k][j] / N_j)
//       with the inline functions of rt_trace_kernels.h as they stand (rt_row_factor, rt_cell, rt_combine, rt_period);
//     - P[g][t][j] = rt_combine(p0, p1, p2, p3, period).
//   A group with fewer than four members leaves some partials at +0.0.  For the group of all locations in index order the
//   positions are the indices, and P is R_it bit for bit (k_rt, k_rt_trace).
//
//   Matrix.  K[g][h][t] is the group sum of P[g][t][.] over the members of h with `weights`, by the one definition of a
//   group sum of fp64 values (group_curve_kernels.h's header; kernel k_group_wsums<1>, reused unchanged with (draw, g) as
//   its "draw" axis).
//
//   No FMA beyond what rt_cell already has, no floating-point atomics.  The bits depend on the table and the draw alone:
//   not on the launch geometry, on debug_skew, or on the cut into calls, batches, buffer halves or shards.
//
//   k_ngm_rows<DT>   a workgroup owns, for one draw of the batch (nd = slot_in_batch * B + chain), 64 source columns
//       (lane = j) x DT window days.  It fills E and S of its days into LDS from RtBufs::ea / RtBufs::S exactly as
//       rt_trace_body does, then loops over the groups: wave p walks the positions p, p + 4, ... of the group (members[k] is
//       wave-uniform), the four partials meet in `red`, and the wave that owns day tt = cc * 4 + wave stores
//       P[((nd G + g) D + tw) ld + j], 64 contiguous columns per store.  No draw loop and no accumulators: nothing is folded
//       per cell.  Work per draw: nnz M D cell evaluations (a partition: k_rt_trace's own count).
// An ordinary launch on the context stream: no hand-off inside a launch, no persistence.
#pragma once

#include "group_curve_kernels.h"

namespace seir {

constexpr int NGM_NDMAX = 65535;   // grid.z of k_ngm_rows: (slot, chain) pairs per launch

// grid (ncb, ceil(D / DT), nd <= NGM_NDMAX), 256 threads, k_rt_trace's dynamic LDS (E | S | red).  Draw nd0 + blockIdx.z of
// the batch's planes rb.ea / rb.S; its theta is that of trace slot first + nd / B, chain nd % B.  offsets [G + 1],
// members [nnz], every member in [0, M) (the host checks).  P [batch nd][G][D][ld], ld >= M.
template <int DT>
__global__ __launch_bounds__(256) void k_ngm_rows(Dims d, Consts c, RtBufs rb, const double *__restrict__ tr_theta, int B,
                                                  int first, int nd0, const int *__restrict__ offsets,
                                                  const int *__restrict__ members, int G, double *__restrict__ P, long long ld) {
    static_assert(DT % 4 == 0 && (DT & (DT - 1)) == 0, "a wave owns the days tt = wave mod 4 of the tile");
    debug_skew(d);
    extern __shared__ double lds[];                      // E [DT][Mp] | S [DT][Mp] | red [4][DT][64]
    constexpr int NC = DT / 4;                           // cells per thread and group: days tt = cc * 4 + wave, column j
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nd = nd0 + blockIdx.z, j = blockIdx.x * WAVE + lane, w0 = blockIdx.y * DT;
    const int M = d.M, D = rb.D;
    double *E = lds, *S = lds + DT * d.Mp, *red = S + DT * d.Mp;
    const bool jin = j < M;
    const double inj = jin ? c.invN[j] : 0.0;
    const int jj = nd / B, b = nd - jj * B;
    const double *th = tr_theta + ((size_t)(first + jj) * B + b) * d.P;
    const double psi = th[0], sig = th[1], beta = th[2], g0 = th[3];
    for (int idx = threadIdx.x; idx < DT * d.Mp; idx += 256) {
        const int i = idx / DT, tt = idx - i * DT, tw = w0 + tt;
        double e = 0.0, sv = 0.0;
        if (i < M && tw < D) {
            e = rt_row_factor(rb.ea[(size_t)nd * d.Tp + rb.t0 + tw], beta, c.la[i], c.invN[i]);
            sv = (double)rb.S[((size_t)nd * d.Mp + i) * D + tw];             // S at the start of day t
        }
        E[tt * d.Mp + i] = e;
        S[tt * d.Mp + i] = sv;
    }
    __syncthreads();
    double pw[DT];
#pragma unroll
    for (int tt = 0; tt < DT; ++tt) pw[tt] = (w0 + tt < D) ? psi * c.W[rb.t0 + w0 + tt] : 0.0;
    const double fj = jin ? exp(sig * th[6 + d.T - 1 + j]) : 0.0;
    const double period = rt_period(g0);
    for (int g = 0; g < G; ++g) {
        const int beg = offsets[g], end = offsets[g + 1];
        double acc[DT];
#pragma unroll
        for (int tt = 0; tt < DT; ++tt) acc[tt] = 0.0;
        for (int k = beg + wave; k < end; k += 4) {
            const int i = members[k];                    // the same for the whole wave
            const double cij = jin ? c.Cstar[(size_t)i * d.Kp0 + j] * inj : 0.0;
            const double dlt = (i == j) ? 1.0 : 0.0;
#pragma unroll
            for (int tt = 0; tt < DT; ++tt) acc[tt] = rt_cell(acc[tt], E[tt * d.Mp + i], S[tt * d.Mp + i], fj, dlt, pw[tt], cij);
        }
#pragma unroll
        for (int tt = 0; tt < DT; ++tt) red[(wave * DT + tt) * WAVE + lane] = acc[tt];
        __syncthreads();
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) {
            const int tt = cc * 4 + wave, tw = w0 + tt;
            const double r = rt_combine(red[(0 * DT + tt) * WAVE + lane], red[(1 * DT + tt) * WAVE + lane],
                                        red[(2 * DT + tt) * WAVE + lane], red[(3 * DT + tt) * WAVE + lane], period);
            if (jin && tw < D)
                P[(((size_t)nd * G + g) * D + tw) * (size_t)ld + j] = r;     // the wave's 64 columns: 512 contiguous bytes
        }
        __syncthreads();                                 // red is read: the next group's partials may be written
    }
}

}  // namespace seir

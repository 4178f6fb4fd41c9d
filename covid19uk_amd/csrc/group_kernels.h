// Region totals, formed where the burst buffer lies (include/seir_hip.h, "Region totals on the device"): for every draw of
// a batch, every group g of locations and every day t of an L-day tensor ev[ND][M][L][3],
//     out[nd][g][t][x] = sum over m in members(g) of ev[nd][m][t][x]          (int64)
// The recorded events (either trace width, through summary_load) and the int32 staging tensors of the forecast and the
// in-sample check have that one layout, ((slot * B + b) * M + m) * L + day with nd = slot * B + b, so one kernel serves all
// three.  Where the caller has a per-draw initial state St0 [3][Mp][ndp] (forecast_kernels.h) the same launch also forms
// state0[nd][g][x], the members' sum of S, E, I at the window's start.
//
// Groups are a CSR pair (offsets [G + 1], members [nnz], ascending and unique within a group); they may overlap and need not
// cover every location.  The shape of the work:
//   - the host cuts every group into SEGMENTS of at most GRP_SEG consecutive members (GroupTable::seg); a workgroup owns a
//     (segment, 64-day chunk, draw).  England's 315 members are five workgroups per chunk and draw, Northern Ireland's 11
//     are one, and no wave ever walks more than GRP_SEG / GRP_WAVES = 8 rows: the largest group does not serialise a
//     launch, and the grid is (segments x chunks, draws) whatever the sizes;
//   - a lane per day, as in k_summarize / k_forecast_keep: a lane reads its day's three counts as one access, contiguous
//     over the wave.  The members of a segment are spread over the GRP_WAVES waves of the workgroup (member i of the
//     segment to wave i % GRP_WAVES), whose loads of GRP_U rows are issued before the first is used; a lane keeps three
//     64-bit sums in registers;
//   - the waves meet in an LDS tile [64 days][3] (64-bit integer LDS adds), and the workgroup then issues one global
//     64-bit atomicAdd per (day, transition) that is not zero, 1536 contiguous bytes, onto arrays the call has zeroed.
// Integers only: the result is exact and cannot depend on the order of the adds, on the geometry, on debug_skew or on how a
// burst is cut into calls.  Ordinary launches on the context stream, behind the work that fills the tensor: no hand-off
// inside a launch, no persistence.
#pragma once

#include "summary_kernels.h"

namespace seir {

constexpr int GRP_MAX_G = 256;     // SEIR_GROUPS_MAX
constexpr int GRP_WAVES = 8;       // waves per workgroup
constexpr int GRP_SEG = 64;        // members of a group per workgroup
constexpr int GRP_U = 4;           // rows whose loads are in flight together
constexpr int GRP_NDMAX = 1024;    // draws per launch (grid.y)
static_assert(GRP_SEG % (GRP_WAVES * GRP_U) == 0, "whole groups of loads per wave");

struct GroupTable {
    const int *seg;                // [nseg][3] group, first and one-past-last position in members
    const int *members;            // [nnz] rows, every one in [0, M) (the host checks)
    int nseg, G;
};

// grid (nseg * nchunk, nd <= GRP_NDMAX), 64 GRP_WAVES threads; nchunk = ceil(L / 64).  Draw blockIdx.y of the launch is draw
// ev_d0 + blockIdx.y of ev (and column ev_d0 + blockIdx.y of St0's planes, row stride ndp, plane stride `plane`) and draw
// out_d0 + blockIdx.y of out [.][G][L][3] and state0 [.][G][3].  St0 may be null: no state0 then.
template <int EV16>
__global__ __launch_bounds__(64 * GRP_WAVES) void k_group_sums(Dims d, GroupTable gt, const void *__restrict__ ev, int M, int L,
                                                               int nchunk, long long ev_d0, long long out_d0,
                                                               unsigned long long *__restrict__ out,
                                                               const int *__restrict__ St0, long long plane, int ndp,
                                                               unsigned long long *__restrict__ state0) {
    debug_skew(d);
    __shared__ unsigned long long tile[64][3];
    __shared__ unsigned long long st[3];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int sg = blockIdx.x / nchunk, ch = blockIdx.x - sg * nchunk;
    const int g = gt.seg[sg * 3], beg = gt.seg[sg * 3 + 1], end = gt.seg[sg * 3 + 2];
    const size_t nd_in = (size_t)ev_d0 + blockIdx.y, nd_out = (size_t)out_d0 + blockIdx.y;
    if (threadIdx.x < 192) (&tile[0][0])[threadIdx.x] = 0ull;
    if (threadIdx.x < 3) st[threadIdx.x] = 0ull;
    __syncthreads();

    const int t = ch * 64 + lane;
    const bool live = t < L;
    long long acc[3] = {0, 0, 0};
    for (int i0 = beg + wv; i0 < end; i0 += GRP_WAVES * GRP_U) {          // uniform over the wave
        int kk[GRP_U][3];
#pragma unroll
        for (int u = 0; u < GRP_U; ++u) {
            const int i = i0 + u * GRP_WAVES;
            const bool on = i < end;
            const int m = gt.members[on ? i : beg];
            summary_load<EV16>(ev, (nd_in * M + m) * L + (live ? t : 0), live && on, kk[u]);
        }
#pragma unroll
        for (int u = 0; u < GRP_U; ++u)
#pragma unroll
            for (int x = 0; x < 3; ++x) acc[x] += (long long)kk[u][x];
    }
    if (live)
#pragma unroll
        for (int x = 0; x < 3; ++x)
            if (acc[x] != 0) atomicAdd(&tile[lane][x], (unsigned long long)acc[x]);
    // the members' initial state: the first chunk's workgroup of the segment, a lane per compartment
    const bool with_state = St0 != nullptr && ch == 0;
    if (with_state && lane < 3) {
        long long s0 = 0;
        for (int i = beg + wv; i < end; i += GRP_WAVES)
            s0 += (long long)St0[(size_t)lane * plane + (size_t)gt.members[i] * ndp + nd_in];
        if (s0 != 0) atomicAdd(&st[lane], (unsigned long long)s0);
    }
    __syncthreads();
    if (threadIdx.x < 192) {
        const unsigned long long v = (&tile[0][0])[threadIdx.x];
        const int tl = threadIdx.x / 3, x = threadIdx.x - tl * 3;
        if (v != 0ull && ch * 64 + tl < L)
            atomicAdd(out + ((nd_out * gt.G + g) * L + (ch * 64 + tl)) * 3 + x, v);
    }
    if (with_state && threadIdx.x < 3 && st[threadIdx.x] != 0ull)
        atomicAdd(state0 + (nd_out * gt.G + g) * 3 + threadIdx.x, st[threadIdx.x]);
}

}  // namespace seir

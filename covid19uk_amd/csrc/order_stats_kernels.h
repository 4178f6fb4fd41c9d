// Exact order statistics of many small cells of int32 or fp64 values (include/seir_hip.h, "Forecast intervals on the
// device" and "R_t intervals on the device"): for every cell and each of R <= 16 sorted ranks r the r-th value in the order
// of order_select.h -- np.sort(values)[r] for int32; for fp64 the total order on the bit patterns, np.sort's on arrays
// without NaN bit for bit -- by an MSB-first radix select whose one narrowing step is order_select.h's.  The doubles are only
// ever looked at as bit patterns: no floating point, no sort, nothing approximate.
//
// A cell is n = segs x seg_len values: `segs` runs of seg_len contiguous values, seg_stride apart; the cells are
// cell_stride apart.  One chain's cell of a draw store (the forecast's, the R_it store) is one run (segs = 1); the cell
// pooled over the process's chains is B runs a chain's plane apart.
//
// order_stats_cell<V, WAVES> is the one body; k_order_stats<WAVES> (int32) and k_order_stats_f64<WAVES> (fp64 bit patterns)
// are its wrappers: a workgroup of WAVES waves per cell (the host takes one wave while n <= ORDER_WAVE_N, four above).
// One pass over the cell's values per 8-bit digit of the key, four or eight.  Ranks are sorted, so their order statistics
// and with them their prefixes are non-decreasing: ranks with the same prefix are neighbours and share ONE histogram -- in
// the first pass all of them, and for the zero-heavy counts this is made for usually until the last.  Per pass: thread 0
// lists the distinct prefixes, the threads count the digit of every value under the one prefix it matches (LDS integer
// adds, the only atomics), and a thread per rank narrows its (prefix, rank).  The first pass reads the cell from memory, the
// others from cache: a 5000-draw cell is 20 KB of int32, 40 KB of fp64.  After the last pass the prefix is the key of the
// answer.
// Ordinary launches on the context stream: no hand-off inside a launch, no persistence.
#pragma once

#include <hip/hip_runtime.h>

#include "order_select.h"

namespace seir {

constexpr int ORDER_WAVE_N = 256;    // cells up to this many values get one wave, larger ones four

template <typename V>
struct OrderStatsArgs {
    const V *values;
    long long cells;
    int segs;
    long long seg_len, seg_stride, cell_stride;
    int R;
    uint32_t ranks[ORDER_MAX_RANKS];   // strictly increasing, each below segs x seg_len (the host checks)
    V *out;                            // [R][cells]
};
using OrderArgs = OrderStatsArgs<int32_t>;
using Order64Args = OrderStatsArgs<uint64_t>;          // the doubles' bit patterns

// The arguments BY VALUE, as rt_trace_body takes its structs: by reference the kernels are two instructions shorter and
// 1.5 % slower.
template <typename V, int WAVES>
__device__ __forceinline__ void order_stats_cell(OrderStatsArgs<V> a) {
    using K = decltype(order_key(V()));
    __shared__ uint32_t hist[ORDER_MAX_RANKS][ORDER_BINS];
    __shared__ K prefix[ORDER_MAX_RANKS], upref[ORDER_MAX_RANKS];
    __shared__ uint32_t rem[ORDER_MAX_RANKS];
    __shared__ int grp[ORDER_MAX_RANKS];
    __shared__ int ngroups;
    const int tid = threadIdx.x, R = a.R;
    const size_t cell = blockIdx.x;
    const V *__restrict__ base = a.values + cell * (size_t)a.cell_stride;
    if (tid < R) { prefix[tid] = (K)0; rem[tid] = a.ranks[tid]; }
    for (int pass = 0; pass < order_passes<K>(); ++pass) {
        __syncthreads();
        if (tid == 0) {
            int g = 0;
            for (int r = 0; r < R; ++r) {
                if (r == 0 || prefix[r] != prefix[r - 1]) upref[g++] = prefix[r];
                grp[r] = g - 1;
            }
            ngroups = g;
        }
        for (int i = tid; i < R * ORDER_BINS; i += 64 * WAVES) (&hist[0][0])[i] = 0u;
        __syncthreads();
        const int G = ngroups;
        for (int sg = 0; sg < a.segs; ++sg) {
            const V *__restrict__ run = base + (size_t)sg * (size_t)a.seg_stride;
            for (long long i = tid; i < a.seg_len; i += 64 * WAVES) {
                const K key = order_key(run[i]);
                const uint32_t dg = order_digit(key, pass);
                for (int g = 0; g < G; ++g)
                    if (order_matches(key, upref[g], pass)) { atomicAdd(&hist[g][dg], 1u); break; }
            }
        }
        __syncthreads();
        if (tid < R) {
            K p = prefix[tid];
            uint32_t r = rem[tid];
            (void)order_select_narrow(hist[grp[tid]], pass, p, r);
            prefix[tid] = p; rem[tid] = r;
        }
    }
    if (tid < R) a.out[(size_t)tid * (size_t)a.cells + cell] = order_value(prefix[tid]);
}

// grid (cells), 64 WAVES threads.
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_order_stats(OrderArgs a) { order_stats_cell<int32_t, WAVES>(a); }
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_order_stats_f64(Order64Args a) { order_stats_cell<uint64_t, WAVES>(a); }

}  // namespace seir

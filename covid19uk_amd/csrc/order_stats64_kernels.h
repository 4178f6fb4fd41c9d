// Exact order statistics of many small cells of fp64 values (include/seir_hip.h, "R_t intervals on the device"): the twin of
// order_stats_kernels.h for doubles.  For every cell and each of R <= 16 sorted ranks r the r-th value in the total order of
// order_select64.h (np.sort's on arrays without NaN, bit for bit), by an MSB-first radix select whose one narrowing step is
// order_select64.h's.  The values are only ever looked at as bit patterns: no floating-point operation, no sort, nothing
// approximate.
//
// The cell geometry is k_order_stats's: n = segs x seg_len values, `segs` runs of seg_len contiguous values, seg_stride
// apart; the cells are cell_stride apart.  One chain's cell of the R_it draw store is one run (segs = 1); the cell pooled over
// the process's chains is B runs a chain's plane apart.
//
// k_order_stats_f64<WAVES>: a workgroup of WAVES waves per cell (one wave while n <= ORDER_WAVE_N, four above).  Eight
// passes over the cell's values, one per 8-bit digit of the key.  Ranks are sorted, so their prefixes are non-decreasing:
// ranks with the same prefix are neighbours and share ONE histogram.  Per pass: thread 0 lists the distinct prefixes, the
// threads count the digit of every value under the one prefix it matches (LDS integer adds, the only atomics), and a thread
// per rank narrows its (prefix, rank).  The first pass reads the cell from memory, the other seven from cache: a 5000-draw
// cell is 40 KB.  After the last pass the prefix is the key of the answer.
// Ordinary launches on the context stream: no hand-off inside a launch, no persistence.
#pragma once

#include <hip/hip_runtime.h>

#include "order_select64.h"
#include "order_stats_kernels.h"

namespace seir {

struct Order64Args {
    const unsigned long long *values;  // the doubles' bit patterns
    long long cells;
    int segs;
    long long seg_len, seg_stride, cell_stride;
    int R;
    uint32_t ranks[ORDER_MAX_RANKS];   // strictly increasing, each below segs x seg_len (the host checks)
    unsigned long long *out;           // [R][cells]
};

// grid (cells), 64 WAVES threads.
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_order_stats_f64(Order64Args a) {
    __shared__ uint32_t hist[ORDER_MAX_RANKS][ORDER_BINS];
    __shared__ uint64_t prefix[ORDER_MAX_RANKS], upref[ORDER_MAX_RANKS];
    __shared__ uint32_t rem[ORDER_MAX_RANKS];
    __shared__ int grp[ORDER_MAX_RANKS];
    __shared__ int ngroups;
    const int tid = threadIdx.x, R = a.R;
    const size_t cell = blockIdx.x;
    const unsigned long long *__restrict__ base = a.values + cell * (size_t)a.cell_stride;
    if (tid < R) { prefix[tid] = 0ull; rem[tid] = a.ranks[tid]; }
    for (int pass = 0; pass < ORDER64_PASSES; ++pass) {
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
            const unsigned long long *__restrict__ run = base + (size_t)sg * (size_t)a.seg_stride;
            for (long long i = tid; i < a.seg_len; i += 64 * WAVES) {
                const uint64_t key = order64_key((uint64_t)run[i]);
                const uint32_t dg = order64_digit(key, pass);
                for (int g = 0; g < G; ++g)
                    if (order64_matches(key, upref[g], pass)) { atomicAdd(&hist[g][dg], 1u); break; }
            }
        }
        __syncthreads();
        if (tid < R) {
            uint64_t p = prefix[tid];
            uint32_t r = rem[tid];
            (void)order64_select_narrow(hist[grp[tid]], pass, p, r);
            prefix[tid] = p; rem[tid] = r;
        }
    }
    if (tid < R) a.out[(size_t)tid * (size_t)a.cells + cell] = (unsigned long long)order64_value(prefix[tid]);
}

}  // namespace seir

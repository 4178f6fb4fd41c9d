// Scoring the forecast against later data (include/seir_hip.h, "Scoring the forecast against later data"): the fold of a
// forecast batch against the truth, and the one term of the sample CRPS that cannot be streamed.
//
// k_verify_fold    a batch's staging tensor ev [ND][M][H][3] (nd = slot_in_batch * B + chain) against truth [M][H] and its
//                  host-formed running total cum [M][H] (int64; both < 0: no truth), into lt | eq (uint32) and abs_sum
//                  (uint64) per [B][M][H][2]: target 0 the I->R count of the day, target 1 its running total over the
//                  horizon -- planes 0 and 1 of the draw store (forecast_kernels.h, above k_forecast_keep).  A wave per
//                  (row, chain), a lane per day; the running total by wave_incl_scan in int64 with a carry per draw across
//                  the 64-day chunks; the per-cell update is verify_update.h's.  The accumulators of a (chain, row, day) are
//                  read and written by one lane of one launch: no atomics, nothing depends on the geometry.
//                  The carries carry[wv][jj] are written by lane 63 of wave wv and read, a chunk later, by the lanes of the SAME
//                  wave: row wv of `carry` belongs to wave wv alone whatever ROWS is, and no barrier stands between the store
//                  and the load.  What orders them is program order within a wave: a wave's LDS operations complete in
//                  order and the compiler keeps a store in front of a load that may alias it.  A carry read by ANOTHER wave
//                  (rows shared between waves, a carry across workgroups) would need a barrier that this kernel does not have.
//
// k_pair_abs       D = sum_{i<j} |x_i - x_j| of every cell of int32 values, the cells addressed as OrderStatsArgs addresses
//                  them (order_stats_kernels.h: `segs` runs of seg_len values seg_stride apart, cells cell_stride apart), into
//                  out [cells] int64.  One workgroup of 256 threads per cell.  The cell is taken in chunks of PAIR_CHUNK
//                  values: a chunk is sorted in LDS (bitonic network over the next power of two, the padding INT32_MAX behind
//                  the c values that count), its inclusive prefix sums P are formed in int64, and
//                      within the chunk     sum_k (2k - c + 1) xs[k]
//                      against the later    for every value b behind the chunk, r = #{xs <= b} by binary search in LDS:
//                                           b (2r - c) + P[c-1] - 2 P[r-1]
//                  are added up per thread and reduced over the block.  A pair inside a chunk is counted by the first term,
//                  a pair across chunks once, by the earlier chunk.  Sorting costs c log^2 c compare-exchanges per chunk and
//                  the cross phase n^2 / (2 PAIR_CHUNK) searches of log2 PAIR_CHUNK steps: a 5000-draw cell is two chunks, the
//                  cell pooled over 8 chains ten.  All sums are 64-bit integers modulo 2^64, so the result is exact while
//                  D < 2^63, whatever the thread order: D <= floor(n^2 / 4) (2^32 - 1), which stays below 2^63 up to
//                  n = PAIR_ABS_MAX_N = 92 681 (92 682^2 / 4 = 2 147 488 281 > 2^31).  The host refuses a larger n; a launch
//                  that gets one all the same writes nothing and raises *overflow.
//                  LDS: keys 16 KB + prefix sums 32 KB: three workgroups per CU.  The sort's compare-exchange partners are
//                  a power of two apart: lanes l and l + 2^k of a 32-lane group hit different banks while 2^k < 32 and the
//                  same lane's pair otherwise -- at most 2-way, which costs a ds_write_b32 nothing.
// Ordinary launches on the context stream: no hand-off inside a launch, no persistence.
#pragma once

#include <hip/hip_runtime.h>

#include "device_math.h"
#include "verify_update.h"

namespace seir {

constexpr int VF_ROWS = 2;                     // waves (rows) per workgroup of k_verify_fold
constexpr int VF_U = 4;                        // draws whose loads are in flight together
constexpr int VF_JMAX = 128;                   // draws per chain of a launch (FC_JMAX: a batch of the forecast)
constexpr int PAIR_CHUNK = 4096;               // SEIR_PAIR_ABS_CHUNK
constexpr int PAIR_THREADS = 256;
constexpr long long PAIR_ABS_MAX_N = 92681;    // SEIR_PAIR_ABS_MAX_N
static_assert((PAIR_CHUNK & (PAIR_CHUNK - 1)) == 0 && PAIR_CHUNK % PAIR_THREADS == 0, "a power of two, whole rounds of the block");
static_assert((PAIR_ABS_MAX_N * PAIR_ABS_MAX_N / 4) <= (1ll << 31) && ((PAIR_ABS_MAX_N + 1) * (PAIR_ABS_MAX_N + 1) / 4) > (1ll << 31),
              "floor(n^2 / 4) (2^32 - 1) < 2^63 exactly while floor(n^2 / 4) <= 2^31");

struct VerifyBufs {
    const int32_t *truth;      // [M][H], < 0: missing
    const int64_t *cum;        // [M][H] running total of truth over the days, < 0: a day up to here is missing
    uint32_t *lt, *eq;         // [B][M][H][2]
    uint64_t *abs_sum;         // [B][M][H][2]
};

// grid (ceil(M / ROWS), B), 64 ROWS threads.  1 <= count <= VF_JMAX draws per chain.  (Templates, both kernels: a template is
// emitted where the host code first names it, behind every kernel the library had -- those keep their places in the code
// object)
template <int ROWS>
__global__ __launch_bounds__(64 * ROWS) void k_verify_fold(Dims d, VerifyBufs v, const int *__restrict__ ev, int H, int B,
                                                              int count) {
    debug_skew(d);
    __shared__ long long carry[ROWS][VF_JMAX];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y, m = blockIdx.x * ROWS + wv;
    const int M = d.M;
    const bool row_ok = m < M;
    const int mr = row_ok ? m : 0;
    for (int h0 = 0; h0 < H; h0 += 64) {
        const int s = h0 + lane;
        const bool live = row_ok && s < H;
        const int sr = s < H ? s : 0;
        const long long y0 = live ? (long long)v.truth[(size_t)mr * H + sr] : -1ll;
        const long long y1 = live ? (long long)v.cum[(size_t)mr * H + sr] : -1ll;
        const size_t cell = (((size_t)b * M + mr) * H + sr) * 2;
        uint32_t lt[2] = {0u, 0u}, eq[2] = {0u, 0u};
        uint64_t ab[2] = {0ull, 0ull};
        if (live) {
            lt[0] = v.lt[cell]; lt[1] = v.lt[cell + 1];
            eq[0] = v.eq[cell]; eq[1] = v.eq[cell + 1];
            ab[0] = v.abs_sum[cell]; ab[1] = v.abs_sum[cell + 1];
        }
        for (int ju = 0; ju < count; ju += VF_U) {
            int k[VF_U];
#pragma unroll
            for (int u = 0; u < VF_U; ++u) {
                const int nd = (ju + u < count ? ju + u : 0) * B + b;
                k[u] = live && ju + u < count ? ev[(((size_t)nd * M + mr) * H + sr) * 3 + 2] : 0;
            }
#pragma unroll
            for (int u = 0; u < VF_U; ++u) {
                const int jj = ju + u;
                if (jj < count) {                                  // uniform over the wave: the scan sees every lane
                    const long long run = (h0 ? carry[wv][jj] : 0ll) + wave_incl_scan((long long)k[u], lane);
                    verify_cell_update(lt[0], eq[0], ab[0], (int64_t)k[u], (int64_t)y0);
                    verify_cell_update(lt[1], eq[1], ab[1], (int64_t)run, (int64_t)y1);
                    if (lane == 63) carry[wv][jj] = run;           // read again by this wave alone, a chunk later
                }
            }
        }
        if (live) {
            v.lt[cell] = lt[0]; v.lt[cell + 1] = lt[1];
            v.eq[cell] = eq[0]; v.eq[cell + 1] = eq[1];
            v.abs_sum[cell] = ab[0]; v.abs_sum[cell + 1] = ab[1];
        }
    }
}

struct PairAbsArgs {
    const int32_t *values;
    long long cells;
    int segs;
    long long seg_len, seg_stride, cell_stride;
    int64_t *out;              // [cells]
    unsigned *overflow;        // raised for n above PAIR_ABS_MAX_N (the host refuses those)
};

// Value i of a cell in the order of its runs; n <= PAIR_ABS_MAX_N, so 32-bit arithmetic finds the run.
__device__ __forceinline__ int32_t pair_abs_value(const int32_t *__restrict__ base, unsigned i, unsigned seg_len, long long seg_stride) {
    const unsigned sg = i / seg_len;
    return base[(size_t)sg * (size_t)seg_stride + (i - sg * seg_len)];
}

// grid (cells), THREADS threads.  The arguments by value, as order_stats_cell takes them.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_pair_abs(Dims d, PairAbsArgs a) {
    debug_skew(d);
    __shared__ int32_t xs[PAIR_CHUNK];
    __shared__ long long P[PAIR_CHUNK];
    __shared__ unsigned long long red[THREADS / 64];
    __shared__ long long wtot[THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t cell = blockIdx.x;
    const long long nn = (long long)a.segs * a.seg_len;
    if (nn > PAIR_ABS_MAX_N) {
        if (tid == 0) a.overflow[0] = 1u;
        return;
    }
    const unsigned n = (unsigned)nn, seg_len = (unsigned)a.seg_len;
    const int32_t *__restrict__ base = a.values + cell * (size_t)a.cell_stride;
    unsigned long long acc = 0ull;
    for (unsigned c0 = 0; c0 < n; c0 += PAIR_CHUNK) {
        const int c = (int)min((unsigned)PAIR_CHUNK, n - c0);
        int N2 = 1;
        while (N2 < c) N2 <<= 1;
        for (int k = tid; k < N2; k += THREADS)
            xs[k] = k < c ? pair_abs_value(base, c0 + (unsigned)k, seg_len, a.seg_stride) : 0x7fffffff;
        __syncthreads();
        // bitonic sort of xs[0, N2), ascending
        for (int size = 2; size <= N2; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < (N2 >> 1); t += THREADS) {
                    const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), hi = lo + stride;
                    const bool up = (lo & size) == 0;
                    const int32_t x = xs[lo], y = xs[hi];
                    if ((x > y) == up) { xs[lo] = y; xs[hi] = x; }
                }
                __syncthreads();
            }
        // inclusive prefix sums in rounds of the block, and the term within the chunk
        long long before = 0;
        for (int k0 = 0; k0 < c; k0 += THREADS) {
            const int k = k0 + tid;
            const long long x = k < c ? (long long)xs[k] : 0ll;
            const long long inc = wave_incl_scan(x, lane);
            if (lane == 63) wtot[wave] = inc;
            __syncthreads();
            long long pre = before;
#pragma unroll
            for (int w = 0; w < THREADS / 64; ++w)
                if (w < wave) pre += wtot[w];
            if (k < c) {
                P[k] = pre + inc;
                acc += (unsigned long long)((long long)(2 * k - c + 1) * x);
            }
#pragma unroll
            for (int w = 0; w < THREADS / 64; ++w) before += wtot[w];
            __syncthreads();
        }
        // every value behind the chunk against the chunk
        const long long ptot = P[c - 1];
        for (unsigned i = c0 + (unsigned)c + (unsigned)tid; i < n; i += THREADS) {
            const int32_t bv = pair_abs_value(base, i, seg_len, a.seg_stride);
            int lo = 0, hi = c;                                // r = #{xs <= bv}: the first index with xs > bv
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (xs[mid] <= bv) lo = mid + 1;
                else hi = mid;
            }
            const long long below = lo ? P[lo - 1] : 0ll;
            acc += (unsigned long long)((long long)bv * (long long)(2 * lo - c) + ptot - 2 * below);
        }
        __syncthreads();                                       // the next chunk overwrites xs and P
    }
    // the block's sum, modulo 2^64
    for (int off = 32; off > 0; off >>= 1) acc += (unsigned long long)__shfl_down((long long)acc, off, 64);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0ull;
        for (int w = 0; w < THREADS / 64; ++w) t += red[w];
        a.out[cell] = (int64_t)t;
    }
}

}  // namespace seir

// Stored draws into trace slots (include/seir_hip.h, "Stored draws into trace slots"): the rows of a posterior file, staged
// on the device as the file has them (fp64), go into the burst buffer in the sampler's width, and are checked on the way.
// The definitions are trace_load.h's.
//
// k_trace_load<EV16> takes the nj staged draws of a chunk into trace slots [first, first + nj) of one chain.  The shape of
// the work is k_summarize's (summary_kernels.h):
//   - a WAVE owns a row m of a draw and walks its 64-day chunks; a workgroup is LOAD_ROWS such waves on neighbouring rows,
//     the grid runs over (row block, draw of the chunk).  One wave per (row, draw): the carry from chunk to chunk stays in
//     its registers, there is no LDS and no barrier;
//   - a 64-day chunk of a row is 192 contiguous doubles in the file and 192 contiguous counts in the trace.  The wave reads
//     them FLAT, three loads of 64 consecutive doubles (512 contiguous bytes each), classifies and converts element by
//     element, and stores them flat again: 64 consecutive counts per store.  Nothing is strided on either side;
//   - the state needs the three counts of a DAY in one lane: element 3 l + x of the chunk lies in load (3 l + x) / 64, lane
//     (3 l + x) mod 64 -- nine 32-bit lane reads (a count that is not LOAD_OK travels as the 0 it was stored as).  Then a
//     DPP wave scan per transition in int64 and the carry: S, E, I at every boundary 1 .. T, tested for a sign;
//   - what is counted is counted per wave in uniform registers (ballot, popcount) and leaves the wave as at most one integer
//     atomic add per category, and one integer atomic min for the key of the first bad item, when the row is done.
// No floating-point arithmetic beyond the conversion, no floating-point atomics.
//
// k_trace_load_theta copies the chunk's theta rows bit for bit (as 64-bit words), counts the entries that are not finite by
// their exponent bits, and writes zeros to the hmc and moves entries of the slots.
#pragma once

#include "sampler_kernels.h"
#include "trace_load.h"

namespace seir {

constexpr int LOAD_ROWS = 8;                        // waves (rows) per workgroup
constexpr int LOAD_JMAX = 64;                       // draws per chunk of a call
constexpr int LOAD_THETA_THREADS = 256;             // threads of k_trace_load_theta
constexpr size_t LOAD_STAGING_BYTES = 256u << 20;   // bound on the staging buffer (at least one draw is always taken)

struct LoadArgs {
    const double *ev;                // staged events [nj][M][T][3]
    const double *theta;             // staged theta [nj][P]
    unsigned long long *status;      // [LOAD_ST_FIRST_KEY + 1]: the counts by code - 1, then the smallest tagged key
    unsigned long long tag;          // the call's number since the last clear << LOAD_KEY_BITS
    int chain, first;                // staged draw 0 goes to trace slot `first` of chain `chain`
    int j0;                          // ... and is draw j0 of the call: flat indices are the call's
};

// One atomic add per category that is not zero and one atomic min, by lane 0.
__device__ __forceinline__ void load_report(const LoadArgs &a, const unsigned (&n)[LOAD_BAD_THETA], unsigned long long kmin, int lane) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(kmin, o, 64);
        kmin = other < kmin ? other : kmin;
    }
    if (lane != 0) return;
#pragma unroll
    for (int q = 0; q < LOAD_BAD_THETA; ++q)
        if (n[q] != 0u) atomicAdd(a.status + q, (unsigned long long)n[q]);
    if (kmin != ~0ull) atomicMin(a.status + LOAD_ST_FIRST_KEY, a.tag | kmin);
}

// grid (ceil(M / LOAD_ROWS), nj), 64 LOAD_ROWS threads.  first + nj <= cap, chain < B (the host checks).
template <int EV16>
__global__ __launch_bounds__(64 * LOAD_ROWS) void k_trace_load(Dims d, Consts c, LoadArgs a, void *__restrict__ tr_events, int B) {
    debug_skew(d);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int m = blockIdx.x * LOAD_ROWS + wv, j = blockIdx.y;
    const int M = d.M, T = d.T;
    if (m >= M) return;                                // a whole wave: nothing below waits for it
    int64_t s0[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) s0[x] = (int64_t)c.init[(size_t)m * 4 + x];
    const size_t row_len = (size_t)T * 3;
    const double *src = a.ev + ((size_t)j * M + m) * row_len;
    const size_t flat0 = ((size_t)(a.j0 + j) * M + m) * row_len;
    const size_t out0 = (((size_t)(a.first + j) * B + a.chain) * M + m) * row_len;
    long long cr[3] = {0, 0, 0};
    unsigned n[LOAD_BAD_THETA] = {0u, 0u, 0u, 0u, 0u};
    unsigned long long kmin = ~0ull;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int nel = min(64, T - t0) * 3;
        int v[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int e = i * 64 + lane;
            const bool live = e < nel;
            const double x = live ? src[(size_t)t0 * 3 + e] : 0.0;
            const LoadCell r = load_classify(x, EV16 ? 16 : 32);
            v[i] = (int)r.value;
            if (live) {
                if (EV16) reinterpret_cast<uint16_t *>(tr_events)[out0 + (size_t)t0 * 3 + e] = (uint16_t)r.value;
                else reinterpret_cast<int32_t *>(tr_events)[out0 + (size_t)t0 * 3 + e] = (int32_t)r.value;
            }
#pragma unroll
            for (int code = LOAD_NOT_INTEGER; code <= LOAD_OVER_WIDTH; ++code)
                n[code - 1] += (unsigned)__popcll(__ballot(r.code == code));
            if (r.code != LOAD_OK) {
                const unsigned long long key = load_key(flat0 + (size_t)t0 * 3 + e, r.code);
                kmin = key < kmin ? key : kmin;
            }
        }
        // the day's three counts into the day's lane
        long long k[3];
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            const int e = 3 * lane + x, sl = e & 63, sr = e >> 6;
            const int g0 = __shfl(v[0], sl, 64), g1 = __shfl(v[1], sl, 64), g2 = __shfl(v[2], sl, 64);
            k[x] = (long long)(sr == 0 ? g0 : sr == 1 ? g1 : g2);
        }
        long long inc[3];
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            inc[x] = cr[x] + wave_incl_scan(k[x], lane);
            cr[x] = lane_value(inc[x], 63);
        }
        const bool day = t0 + lane < T;
        const int neg = day ? load_state_below_zero(s0, inc[0], inc[1], inc[2]) : 0;
#pragma unroll
        for (int x = 0; x < 3; ++x) n[LOAD_NEG_STATE - 1] += (unsigned)__popcll(__ballot((neg >> x) & 1));
        if (neg) {
            const int x = (neg & 1) ? 0 : (neg & 2) ? 1 : 2;           // the first compartment below zero
            const unsigned long long key = load_key(flat0 + (size_t)(t0 + lane) * 3 + x, LOAD_NEG_STATE);
            kmin = key < kmin ? key : kmin;
        }
    }
    load_report(a, n, kmin, lane);
}

// grid (nj), NT threads.  tr_theta [cap][B][P], tr_hmc [cap][B][3], tr_mv [cap][B][4 NMVTR].  A template, like every kernel
// added since the code's address was pinned: the instances of templates are emitted behind the plain kernels, so a new one
// moves no kernel of the sweep (a plain kernel here moved them all by 0x500 bytes, measured).
template <int NT>
__global__ __launch_bounds__(NT) void k_trace_load_theta(Dims d, LoadArgs a, double *__restrict__ tr_theta, double *__restrict__ tr_hmc,
                                                          double *__restrict__ tr_mv, int B) {
    debug_skew(d);
    const int lane = threadIdx.x & 63, j = blockIdx.x, P = d.P;
    const unsigned long long *src = reinterpret_cast<const unsigned long long *>(a.theta) + (size_t)j * P;
    const size_t slot = (size_t)(a.first + j) * B + a.chain;
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(tr_theta) + slot * P;
    unsigned n[LOAD_BAD_THETA] = {0u, 0u, 0u, 0u, 0u};
    unsigned long long kmin = ~0ull;
    for (int p0 = 0; p0 < P; p0 += NT) {              // uniform trip count: every lane reaches the ballot
        const int p = p0 + threadIdx.x;
        const unsigned long long bits = p < P ? src[p] : 0ull;
        if (p < P) dst[p] = bits;
        const bool bad = load_theta_bad(bits);
        n[LOAD_BAD_THETA - 1] += (unsigned)__popcll(__ballot(bad));
        if (bad) {
            const unsigned long long key = load_key((size_t)(a.j0 + j) * P + p, LOAD_BAD_THETA);
            kmin = key < kmin ? key : kmin;
        }
    }
    for (int i = threadIdx.x; i < 3; i += NT) tr_hmc[slot * 3 + i] = 0.0;
    for (int i = threadIdx.x; i < 4 * NMVTR; i += NT) tr_mv[slot * 4 * NMVTR + i] = 0.0;
    load_report(a, n, kmin, lane);
}

}  // namespace seir

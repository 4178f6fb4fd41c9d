// Hand-offs between the workgroups of ONE launch -- the persistent launches k_leap, k_move_pairs / k_move_pair, k_se_chunk
// and k_eval_all: the only place that polls or publishes.
//
// The rules, for every hand-off of the library:
//   * All of a chain's workgroups share one L2 (every hand-off runs only where the XCC_ID probe at creation shows a
//     chain's workgroups on one XCD), so what a producer hands over is read past the L1 (relaxed, agent scope) and no
//     release / acquire is needed beyond what a call site states itself.
//   * Every wait is bounded (hs_wait).  A wait that gives up counts itself -- in the chain's fatal counter
//     (Chains::late + late_fatal), in a counter of its own, or not at all -- and goes on with whatever it has; once the
//     fatal counter is non-zero every later wait of the chain gives up at its next look at it, so that a launch that
//     cannot complete drains in about a second instead of a second per wait.  The host finds the counter at the next read
//     of the trace (check_handoffs) or at the next synchronisation (check_eval_handoffs), fails with SEIR_ERR_HANDOFF and
//     can restore the last snapshot (seir_sampler_restore).
//   * A value that travels on its own carries its own flag (the hand-off words below); everything else is published
//     after the producer's stores are acknowledged (s_waitcnt vmcnt(0)) with a counter, flag or token the consumer polls.
//     Words may also vouch for plain stores, on the same terms: k_move_pairs' band workgroups write their rows of F, wait
//     for the acknowledgement, and only then issue the words of their partial sums -- a role that has seen the words
//     may load F.
//   * Plain loads and the L1.  A consumer may read with plain loads what another workgroup wrote only if its CU's L1 cannot
//     hold an older copy: the workgroup has the CU to itself (k_move_pairs' LDS request), one of its waves has emptied the
//     L1 (agent-scope acquire fence: buffer_inv sc1 -- sc0 does not empty it on this part) after the workgroup's last load
//     of the step before, and it loads nothing of that data again before the wait that declares it final.  Anything read
//     earlier than that wait is read past the L1 (ld_l2, the word loads).  Each workgroup drops its own L1, once per step,
//     by one wave: the roles where they meet (pair_chain_barrier), a band workgroup on its own (pair_band_next_step).
#pragma once
#include <hip/hip_runtime.h>

// ---- relaxed agent-scope access: at the XCD's L2, past the L1
template <typename T> __device__ __forceinline__ T ld_l2(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T, typename V> __device__ __forceinline__ void st_l2(T *p, V v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T, typename V> __device__ __forceinline__ T add_l2(T *p, V v) { return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T, typename V> __device__ __forceinline__ T min_l2(T *p, V v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T, typename V> __device__ __forceinline__ T max_l2(T *p, V v) { return __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// true in every lane once `ok` holds in every active lane of the wave
__device__ __forceinline__ bool hs_all(bool ok) { return __builtin_amdgcn_ballot_w64(!ok) == 0ull; }

// ---- the bounded wait
// Limits, in polls.  A time-out has never been seen outside the test hooks and a GPU shared with another persistent launch.
constexpr int HS_LIMIT = 1 << 22;        // k_move_pair(s), k_se_chunk, k_eval_all: ~0.1 .. 1 s, counted, no hang
constexpr int HS_LIMIT_LEAP = 1 << 21;   // k_leap's flags (leap_wait, the roles' wait for the tiles): ~1 s
constexpr int HS_LIMIT_LL = 1 << 19;     // k_leap's hand-off words (ll_poll): each poll is up to six 16-byte loads
constexpr int HS_LIMIT_ROLES = 4000;     // k_move_pair's role 0 waiting for a speculative role: not fatal, role 0 then
                                         // draws the proposal itself (Chains::late[b], seir_sampler_pair_timeouts)
// How often a wait looks at the fatal counter, in polls (a power of two; 0: never)
constexpr int HS_CHECK = 256;
constexpr int HS_CHECK_LL = 64;
// Who counts a time-out: every thread that runs the wait (the call site runs it on one), thread 0 of the workgroup,
// lane 0 of each wave, or nobody (the call site counts from the return value)
enum HsCount { HS_CALLER, HS_THREAD0, HS_LANE0, HS_NONE };

// Polls ready() until it holds: s_sleep SLEEP between polls (FIRST after the first one when `backoff`), a look at the
// fatal counter *cnt every CHECK polls, at most LIMIT polls + 1, a time-out counted in *cnt by WHO.  PRIO >= 0: the wave's
// priority is dropped to 0 while it sleeps and put back to PRIO when the wait ends.  A back-off before the FIRST poll
// is the call site's own.  Returns whether the wait gave up (time-out, or the fatal counter seen non-zero).
template <int SLEEP, int CHECK, int LIMIT, int WHO, int FIRST = SLEEP, int PRIO = -1, typename Ready, typename C = unsigned>
__device__ __forceinline__ bool hs_wait(Ready ready, C *cnt = nullptr, bool backoff = false) {
    static_assert((CHECK & (CHECK - 1)) == 0, "CHECK: a power of two, or 0");
    int spins = 0;
    bool gave_up = false;
    while (!ready()) {
        if (PRIO >= 0 && spins == 0) __builtin_amdgcn_s_setprio(0);
        if (FIRST != SLEEP && spins == 0 && backoff) __builtin_amdgcn_s_sleep(FIRST); else __builtin_amdgcn_s_sleep(SLEEP);
        ++spins;
        if (CHECK > 0 && (spins & (CHECK - 1)) == 0 && ld_l2(cnt) != 0) { gave_up = true; break; }
        if (spins > LIMIT) {
            if (WHO == HS_CALLER || (WHO == HS_THREAD0 && threadIdx.x == 0) || (WHO == HS_LANE0 && (threadIdx.x & 63) == 0))
                add_l2(cnt, 1);
            gave_up = true;
            break;
        }
    }
    if (PRIO >= 0 && spins > 0) __builtin_amdgcn_s_setprio(PRIO);
    return gave_up;
}

// ---- hand-off words
// A value handed from one workgroup of a launch to another through the XCD's L2 used to cost the producer its stores, the
// wait for their acknowledgement (s_waitcnt vmcnt(0), ~0.3 us), a returning atomic on the chain's counter (~0.4 us) and --
// for the last one in -- a flag store; the consumer a poll of the flag (a round trip, ~0.5 us) and only then the loads of the
// values (another).  Here every value carries its own flag: two dwords travel as 16 bytes {a, seq, b, seq} -- two aligned
// 8-byte halves, each written whole by the memory system, each with the sequence number -- so the producer only issues its
// stores and the consumer's first look at the DATA is also its wait: it loads past the L1 and looks again until both halves
// of everything it asked for show the number.  k_leap's seq = the step's number over all launches of the sampler with the
// top bit set (ll_seq); k_move_pair's = the launch's token (pair_token): never the zero of a reset buffer, never the number
// before.  Both sides are written as inline asm, so that each word is ONE 16-byte access whatever the compiler would make of
// it (tests/test_handoff_codegen.py holds the kernels to that).
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ unsigned ll_seq(unsigned long long step) { return (unsigned)step | 0x80000000u; }
// (s_nop 1: gfx950 needs two wait states between a 16-byte VMEM store and a VALU write of its data registers, and the
// compiler's hazard recognizer does not look inside inline asm)
__device__ __forceinline__ void ll_store_word(uint4 *p, unsigned a, unsigned b, unsigned seq) {
    const u32x4 x = {a, seq, b, seq};
    asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" : : "v"(p), "v"(x) : "memory");
}
__device__ __forceinline__ void ll_store(uint4 *p, double v, unsigned seq) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    ll_store_word(p, (unsigned)u, (unsigned)(u >> 32), seq);
}
__device__ __forceinline__ bool ll_ok(const u32x4 &x, unsigned seq) { return x.y == seq && x.w == seq; }
__device__ __forceinline__ double ll_value(const u32x4 &x) {
    return __longlong_as_double((long long)(((unsigned long long)x.z << 32) | (unsigned long long)x.x));
}
// N 16-byte loads past the L1 and the wait for them, as ONE asm block: the compiler does not count these loads, so nothing
// may touch the destination registers between the issue and the wait
template <int N> __device__ __forceinline__ void ll_load(const uint4 *const (&p)[N], u32x4 (&x)[N]) {
    static_assert(N >= 1 && N <= 6, "groups of up to six");
    if constexpr (N == 1)
        asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(x[0]) : "v"(p[0]) : "memory");
    else if constexpr (N == 2)
        asm volatile("global_load_dwordx4 %0, %2, off sc1\n\tglobal_load_dwordx4 %1, %3, off sc1\n\ts_waitcnt vmcnt(0)"
                     : "=&v"(x[0]), "=&v"(x[1]) : "v"(p[0]), "v"(p[1]) : "memory");
    else if constexpr (N == 3)
        asm volatile("global_load_dwordx4 %0, %3, off sc1\n\tglobal_load_dwordx4 %1, %4, off sc1\n\tglobal_load_dwordx4 %2, %5, off sc1\n\t"
                     "s_waitcnt vmcnt(0)" : "=&v"(x[0]), "=&v"(x[1]), "=&v"(x[2]) : "v"(p[0]), "v"(p[1]), "v"(p[2]) : "memory");
    else if constexpr (N == 4)
        asm volatile("global_load_dwordx4 %0, %4, off sc1\n\tglobal_load_dwordx4 %1, %5, off sc1\n\tglobal_load_dwordx4 %2, %6, off sc1\n\t"
                     "global_load_dwordx4 %3, %7, off sc1\n\ts_waitcnt vmcnt(0)"
                     : "=&v"(x[0]), "=&v"(x[1]), "=&v"(x[2]), "=&v"(x[3]) : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]) : "memory");
    else if constexpr (N == 5)
        asm volatile("global_load_dwordx4 %0, %5, off sc1\n\tglobal_load_dwordx4 %1, %6, off sc1\n\tglobal_load_dwordx4 %2, %7, off sc1\n\t"
                     "global_load_dwordx4 %3, %8, off sc1\n\tglobal_load_dwordx4 %4, %9, off sc1\n\ts_waitcnt vmcnt(0)"
                     : "=&v"(x[0]), "=&v"(x[1]), "=&v"(x[2]), "=&v"(x[3]), "=&v"(x[4])
                     : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4]) : "memory");
    else
        asm volatile("global_load_dwordx4 %0, %6, off sc1\n\tglobal_load_dwordx4 %1, %7, off sc1\n\tglobal_load_dwordx4 %2, %8, off sc1\n\t"
                     "global_load_dwordx4 %3, %9, off sc1\n\tglobal_load_dwordx4 %4, %10, off sc1\n\tglobal_load_dwordx4 %5, %11, off sc1\n\t"
                     "s_waitcnt vmcnt(0)"
                     : "=&v"(x[0]), "=&v"(x[1]), "=&v"(x[2]), "=&v"(x[3]), "=&v"(x[4]), "=&v"(x[5])
                     : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4]), "v"(p[5]) : "memory");
}
// The consumer's wait: load, look, again -- until every lane of the wave has words showing seq in all N places; a time-out
// is counted in the fatal counter `late` by lane 0 of each wave, and the words are then whatever was there.  (Looking again
// at only the places that were late, one load at a time, was slower -- 140.7 us per k_leap launch against 134.7: with several
// tiles late, each place's round trip came behind the last one's.)
template <int N, int SLEEP, int CHECK, int LIMIT, int PRIO = -1>
__device__ __forceinline__ void ll_wait(const uint4 *const (&p)[N], unsigned seq, unsigned *late, u32x4 (&x)[N]) {
    hs_wait<SLEEP, CHECK, LIMIT, HS_LANE0, SLEEP, PRIO>([&] {
        ll_load<N>(p, x);
        bool ok = true;
#pragma unroll
        for (int j = 0; j < N; ++j) ok = ok && ll_ok(x[j], seq);
        return hs_all(ok);
    }, late);
}
// k_leap's form, for doubles.  RPRIO >= 0 (a role's waves): the wave's priority is dropped while it looks again and again,
// and put back to RPRIO when the words are there
#ifndef LL_POLL_SLEEP
#define LL_POLL_SLEEP 2
#endif
#ifndef LEAP_ROLE_PRIO
#define LEAP_ROLE_PRIO 3            // k_leap's role waves (see there)
#endif
#define LL_RPRIO -1                 // the roles' polls keep their priority
template <int N, int RPRIO = -1> __device__ __forceinline__ void ll_poll(const uint4 *const (&p)[N], unsigned seq, unsigned *late, double (&v)[N]) {
    u32x4 x[N];
    ll_wait<N, LL_POLL_SLEEP, HS_CHECK_LL, HS_LIMIT_LL, RPRIO>(p, seq, late, x);
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = ll_value(x[j]);
}
// k_move_pair's form: a run of NDW dwords (a proposal descriptor) in (NDW + 1) / 2 words {dword, seq, dword, seq}, lane i of
// one wave at word i.  The band workgroups used to wait for role 1's token (after its stores were acknowledged) and then
// copy the descriptor -- two round trips behind each other; now each lane of one wave looks at its word until it shows the
// launch's token (the lanes beyond the descriptor at its last one).
template <int NDW> __device__ __forceinline__ void move_store_ll(uint4 *dst, const int *src, int lane, unsigned seq) {
    if (lane < (NDW + 1) / 2) ll_store_word(dst + lane, (unsigned)src[2 * lane], 2 * lane + 1 < NDW ? (unsigned)src[2 * lane + 1] : 0u, seq);
}
template <int NDW> __device__ __forceinline__ void move_wait_ll(int *dst, const uint4 *src, int lane, unsigned seq, unsigned *late) {
    constexpr int NW = (NDW + 1) / 2;
    const uint4 *pp[1] = {src + min(lane, NW - 1)};
    u32x4 x[1];
    ll_wait<1, 1, HS_CHECK, HS_LIMIT>(pp, seq, late, x);
    if (lane < NW) {
        dst[2 * lane] = (int)x[0].x;
        if (2 * lane + 1 < NDW) dst[2 * lane + 1] = (int)x[0].z;
    }
}

// k_move_pairs' form: what a band workgroup leaves for the roles of the next step -- its two partial sums {theta part,
// constant part} -- as two words numbered by the token of the step that wrote them, one lane per band workgroup at the
// reading end (the lanes beyond the last workgroup look at the last one's)
__device__ __forceinline__ void pair_sums_store(uint4 *dst, double th, double cn, unsigned seq) {
    ll_store(dst, th, seq);
    ll_store(dst + 1, cn, seq);
}
__device__ __forceinline__ void pair_sums_wait(const uint4 *src, unsigned seq, unsigned *late, double &th, double &cn) {
    const uint4 *pp[2] = {src, src + 1};
    u32x4 x[2];
    ll_wait<2, 1, HS_CHECK, HS_LIMIT>(pp, seq, late, x);
    th = ll_value(x[0]);
    cn = ll_value(x[1]);
}

// ---- k_move_pair's tokens: unique per (sweep, launch of the sweep) since lidx < 63, never 0.  31 bits: the top bit of the
// authoritative role's last token carries which descriptor stands (Chains::mvsel); the token wraps after 2^25 sweeps.
__device__ __forceinline__ unsigned pair_token(unsigned sweep, int lidx) { return (sweep * 64u + (unsigned)lidx + 1u) & 0x7fffffffu; }

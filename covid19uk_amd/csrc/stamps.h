// Developer timelines of the kernels: time stamps taken inside a launch, stated once.
//
// A stamp is a store (plain, min or max) of the 100 MHz clock (s_memrealtime) by one thread of a chosen workgroup to a
// word of a stamp region, compiled in by ONE family flag and read back by a tools/dev or tools/probes script through
// tools/dev/stamps.py.  In the default build every macro of this header expands to `do {} while (0)` (or an empty
// context) and evaluates none of its arguments: the library's machine code does not know the facility exists.
//
// The families -- one per build, each region starts at word 0 of its storage (tools/dev/build_variant.sh <tag> builds
// them; the tags and flag lines are VARIANTS below, tests/test_stamps_table.py holds the script to this table):
//
//   SEIR  -DSEIR_STAMPS   storage Chains::stamps, 16 plain words (reset 0), chain 0 only.  One launch is stamped at a time;
//         the sub-switches pick it: SEIR_STAMP_STAGE (k_hmc_step's STAGE, default 2), SEIR_STAMP_SLOT (the event update's
//         slot, default 1; the pair kernels take SLOT & 2 as their S->E slot), SEIR_STAMP_ROLE (the speculative role, default
//         1), SEIR_STAMP_BLOCK (k_move_delta's block, default 0), SEIR_STAMP_PROPOSE (the phases INSIDE the speculative
//         role's mv_propose; role 0's and k_move_delta's stamps are then off).  Read by tools/probes/stamp_probe.py
//         (tag seirst) and tools/probes/propose_probe.py (tag propst).  Words:
//           k_hmc_step<STAGE>:  0 entry | 10 scalars + L/P parts loaded (drained) | 11 K parts + T vectors (drained) |
//                               12 R parts + M vectors (drained) | 1 past the first barrier | 2..9 the phases in order
//           k_move_pa2 block 0: 0 entry | 1 pending decided | 2 finalized | 3 tables in LDS | 4..9 inside mv_propose (4 entry,
//                               5 rows selected, 6 rows staged, 7 days selected, 8 bounds, 9 lanes finished) | 10 proposed |
//                               11 descriptor stored
//           k_move_pair(s) role 0: 0 entry | 1 finalized | 2 S->E tables | 3 S->E proposed | 4 S->E delta | 5 accepted, applied,
//                               traced | 6 next tables | 7 next proposed and stored
//             speculative role: SW_ROLE + 0 entry | + 1 pending known | + 2 tables + proposal | + 3 stored + own rows
//                               (SW_ROLE = 8; 12 under SEIR_STAMP_PROPOSE, where 4..9 are its mv_propose's)
//           k_move_delta block: SW_DELTA + 0 entry | + 1 descriptor and log table | + 2 band | + 3 own rows   (SW_DELTA = 12)
//   PAIR  -DPAIR_STAMPS   Chains::stamps, [PAIR_SLOTS 27][PAIR_STEPS 12][16] plain words (reset 0): thread 0 of the workgroup
//         in `slot` of the launch's first chain, per step of the event-update launch.  tools/dev/pair_timeline.py (pairst).
//           0 entry | roles: 6 entry loads issued, 12 back, 13 past the barrier, 14 uniforms drawn, 15 pending descriptors
//           in LDS | 7 the band's words of the step before seen | 1..5 inside the step | 8 step done | roles: 10 drained,
//           11 the roles' barrier released, 9 L1 dropped | band: 10 partial sums published, 9 own L1 dropped
//   LEAP  -DLEAP_STAMPS=1|2 [-DLEAP_CPROBE]   Chains::stamps, (B + 6) * 128 + 4096 words.  tools/dev/leap_timeline.py
//         (leapst: level 1; leapst2: level 2 with the stamps inside the roles).  Step = it & 15.
//           chains [B][16 steps][8]      level 2 only; min-words (even, reset ~0) / max-words (odd, reset 0) over the chain's
//                                        workgroups: 0, 1 tiles past the wait for the tables | 2, 3 tiles counted in |
//                                        4, 5 roles past the wait for the tiles | 6, 7 roles done
//           tiles  [2][16 steps][8]      plain: chain 0's tile 0 and tile nwg / 2 + 5: 0 past the wait | 1 tables in LDS |
//                                        2 cells done | 3 past the middle barrier | 4 reductions issued | 5 stores
//                                        acknowledged | 6 counted in
//           roles  [2][16 steps][16]     plain: chain 0's T-chunk 0 and M-chunk 0: 0 previous roles done | 1 at the wait for
//                                        the tiles | 2 stores issued | 3 acknowledged | 4 counted in | LEAP_CPROBE: 5..12
//                                        inside hmc_chunk_role (the comments at its CPROBE sites)
//           all    [LEAP_ALL_TILES 1024][4]  plain: every tile workgroup of chain 0 in step 7: 0 past the wait | 1 cells done
//                                        | 2 counted in | 3 XCC_ID << 32 | HW_ID
//   TAIL  -DTAIL_STAMPS   Chains::stamps, [B][8]: k_se_chunk's launches with par = 1 since the last reset (the probe runs
//         trajectories of three leapfrog steps: exactly one such launch).  tools/dev/tail_timeline.py (tailst).
//           0 first tile start (min) | 1 last tile arrival (max) | 2 first role past its wait (min) | 3 last role past
//           its wait (max) | 4 last role done (max) | 5 first role start (min) | 6, 7 unused
//   SE    -DSE_STAMPS     no Chains in k_se: words 2 and 3 of every tile's four tile scalars (Work::TS, [tiles][4]; free in
//         the TSM = 1 instance): 2 the tile workgroup's start | 3 its end (low 48 bits) with XCC_ID (60..63) and HW_ID bits
//         8..19 (48..59).  Plain, rewritten by every launch.  tools/dev/se_timeline.py (sest).
//   EVAL  -DEVAL_STAMPS   no Chains in k_eval_all: 7 plain words (reset 0) behind the counters of the launch's chains,
//         cnt[aff_nb * EVC_STRIDE + i], by tile 0 and the finish block of chain 0: 0 tile enters | 1 its share of the state
//         scan done | 2 the chain's state complete | 3 tile done | 4 finish block enters | 5 all counted in | 6 finish
//         done.  tools/dev/eval_timeline.py (evst).
#pragma once
#include <stddef.h>

#if (defined(SEIR_STAMPS) + defined(PAIR_STAMPS) + defined(LEAP_STAMPS) + defined(TAIL_STAMPS) + defined(SE_STAMPS) + \
     defined(EVAL_STAMPS)) > 1
#error "one stamp family per build: every family's region starts at word 0"
#endif
#define STAMPS_SEIR 0
#define STAMPS_PAIR 0
#define STAMPS_LEAP 0
#define STAMPS_TAIL 0
#define STAMPS_SE 0
#define STAMPS_EVAL 0
#if defined(SEIR_STAMPS)
#undef STAMPS_SEIR
#define STAMPS_SEIR 1
#elif defined(PAIR_STAMPS)
#undef STAMPS_PAIR
#define STAMPS_PAIR 1
#elif defined(LEAP_STAMPS)
#undef STAMPS_LEAP
#define STAMPS_LEAP 1
#elif defined(TAIL_STAMPS)
#undef STAMPS_TAIL
#define STAMPS_TAIL 1
#elif defined(SE_STAMPS)
#undef STAMPS_SE
#define STAMPS_SE 1
#elif defined(EVAL_STAMPS)
#undef STAMPS_EVAL
#define STAMPS_EVAL 1
#endif
#define STAMPS_ON (STAMPS_SEIR || STAMPS_PAIR || STAMPS_LEAP || STAMPS_TAIL || STAMPS_SE || STAMPS_EVAL)
// the sub-switches, defaulted here and nowhere else
#ifndef SEIR_STAMP_SLOT
#define SEIR_STAMP_SLOT 1
#endif
#ifndef SEIR_STAMP_ROLE
#define SEIR_STAMP_ROLE 1
#endif
#ifndef SEIR_STAMP_BLOCK
#define SEIR_STAMP_BLOCK 0
#endif
#ifndef SEIR_STAMP_STAGE
#define SEIR_STAMP_STAGE 2
#endif
#ifdef SEIR_STAMP_PROPOSE
#define STAMPS_SEIR_PROPOSE 1
#else
#define STAMPS_SEIR_PROPOSE 0
#endif
#if STAMPS_LEAP
#define STAMPS_LEAP_LEVEL (LEAP_STAMPS + 0)
#else
#define STAMPS_LEAP_LEVEL 0
#endif
#if STAMPS_LEAP && defined(LEAP_CPROBE)
#define STAMPS_LEAP_INSIDE 1
#else
#define STAMPS_LEAP_INSIDE 0
#endif

namespace seir {
namespace stamps {

// ---------------------------------------------------------------------------------------------
// The table: plain C++, shared by the kernels' macros below, the host's reader and tests/test_stamps_table.py
// ---------------------------------------------------------------------------------------------
enum Family : int { F_NONE = 0, F_SEIR, F_PAIR, F_LEAP, F_TAIL, F_SE, F_EVAL };
constexpr Family FAMILY = STAMPS_SEIR ? F_SEIR : STAMPS_PAIR ? F_PAIR : STAMPS_LEAP ? F_LEAP : STAMPS_TAIL ? F_TAIL
                        : STAMPS_SE ? F_SE : STAMPS_EVAL ? F_EVAL : F_NONE;

// the stamped builds: tag (tools/dev/variants/libseirhip_<tag>.so), family, compiler flags, the tool that reads it
struct Variant { const char *tag; Family family; const char *flags; const char *tool; };
constexpr Variant VARIANTS[] = {
    {"seirst", F_SEIR, "-DSEIR_STAMPS -DSEIR_STAMP_SLOT=1", "tools/probes/stamp_probe.py"},
    {"propst", F_SEIR, "-DSEIR_STAMPS -DSEIR_STAMP_PROPOSE -DSEIR_STAMP_SLOT=1 -DSEIR_STAMP_ROLE=1", "tools/probes/propose_probe.py"},
    {"pairst", F_PAIR, "-DPAIR_STAMPS=1 -mllvm -disable-machine-licm", "tools/dev/pair_timeline.py"},
    {"leapst", F_LEAP, "-DLEAP_STAMPS=1 -mllvm -disable-machine-licm", "tools/dev/leap_timeline.py"},
    {"leapst2", F_LEAP, "-DLEAP_STAMPS=2 -DLEAP_CPROBE -mllvm -disable-machine-licm", "tools/dev/leap_timeline.py"},
    {"tailst", F_TAIL, "-DTAIL_STAMPS -mllvm -disable-machine-licm", "tools/dev/tail_timeline.py"},
    {"sest", F_SE, "-DSE_STAMPS", "tools/dev/se_timeline.py"},
    {"evst", F_EVAL, "-DEVAL_STAMPS=1 -mllvm -disable-machine-licm", "tools/dev/eval_timeline.py"},
};
constexpr int NVARIANTS = (int)(sizeof(VARIANTS) / sizeof(VARIANTS[0]));

// SEIR: named words
constexpr int SEIR_WORDS = 16;
constexpr int SW_ROLE = STAMPS_SEIR_PROPOSE ? 12 : 8;      // the speculative role's four phases
constexpr int SW_DELTA = 12;                               // k_move_delta's four phases
// PAIR: who may stamp (the guards of QSTAMP)
constexpr int PAIR_SLOTS = 27, PAIR_STEPS = 12, PAIR_NW = 16;
// LEAP: steps per block, the all-tiles block
constexpr int LEAP_STEPS = 16, LEAP_ALL_TILES = 1024;
constexpr int TAIL_NW = 8, EVAL_WORDS = 7, SE_NW = 4;

constexpr size_t pair_word(int slot, int step, int i) { return ((size_t)slot * PAIR_STEPS + step) * PAIR_NW + i; }
constexpr size_t leap_chain_word(int b, int it, int k) { return ((size_t)b * LEAP_STEPS + (it & 15)) * 8 + k; }
constexpr size_t leap_tiles_base(int B) { return (size_t)B * LEAP_STEPS * 8; }
constexpr size_t leap_tile_word(int B, int which, int it, int k) {      // which: 0 tile 0, 1 the middle tile
    return leap_tiles_base(B) + ((size_t)which * LEAP_STEPS + (it & 15)) * 8 + k;
}
constexpr size_t leap_roles_base(int B) { return leap_tiles_base(B) + 2 * LEAP_STEPS * 8; }
constexpr size_t leap_role_word(int B, int which, int it, int k) {      // which: 0 T-chunk 0, 1 M-chunk 0
    return leap_roles_base(B) + ((size_t)which * LEAP_STEPS + (it & 15)) * 16 + k;
}
constexpr size_t leap_all_base(int B) { return leap_roles_base(B) + 2 * LEAP_STEPS * 16; }
constexpr size_t leap_all_word(int B, int tix, int k) { return leap_all_base(B) + (size_t)tix * 4 + k; }
constexpr size_t tail_word(int b, int k) { return (size_t)b * TAIL_NW + k; }

// words of the family's region at a sampler of B chains (SE: per tile of the context; EVAL: whatever B)
constexpr size_t extent(Family f, int B) {
    return f == F_SEIR ? (size_t)SEIR_WORDS
         : f == F_PAIR ? (size_t)PAIR_SLOTS * PAIR_STEPS * PAIR_NW
         : f == F_LEAP ? leap_all_base(B) + (size_t)LEAP_ALL_TILES * 4
         : f == F_TAIL ? (size_t)B * TAIL_NW
         : f == F_SE ? (size_t)SE_NW
         : f == F_EVAL ? (size_t)EVAL_WORDS : 0;
}
// a min-word is reset to ~0, every other word (max, plain) to 0
constexpr bool min_word(Family f, int B, size_t w) {
    return f == F_LEAP ? (w < leap_tiles_base(B) && (w & 1) == 0)
         : f == F_TAIL ? (w % TAIL_NW == 0 || w % TAIL_NW == 2 || w % TAIL_NW == 5) : false;
}
// what the host allocates for Chains::stamps: the largest region of the sampler's families
constexpr size_t larger(size_t a, size_t b) { return a > b ? a : b; }
constexpr size_t buffer_words(int B) {
    return larger(larger(extent(F_SEIR, B), extent(F_PAIR, B)), larger(extent(F_LEAP, B), extent(F_TAIL, B)));
}
// every family's highest word lies inside its extent, whatever B (B = 1: the smallest sampler)
static_assert(pair_word(PAIR_SLOTS - 1, PAIR_STEPS - 1, PAIR_NW - 1) < extent(F_PAIR, 1) && extent(F_PAIR, 1) <= buffer_words(1), "PAIR");
static_assert(leap_chain_word(0, 15, 7) < leap_tiles_base(1) && leap_tile_word(1, 1, 15, 7) < leap_roles_base(1) &&
              leap_role_word(1, 1, 15, 15) < leap_all_base(1) && leap_all_word(1, LEAP_ALL_TILES - 1, 3) < extent(F_LEAP, 1), "LEAP");
static_assert(tail_word(0, TAIL_NW - 1) < extent(F_TAIL, 1) && SW_DELTA + 3 < SEIR_WORDS && SW_ROLE + 3 < SEIR_WORDS, "TAIL, SEIR");

}  // namespace stamps
}  // namespace seir

// ---------------------------------------------------------------------------------------------
// The kernels' side
// ---------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include "handoff.h"

namespace seir {

// THE primitive: after `drain` (nothing, or an instruction that holds the wave until what went before has come back), the
// thread(s) for which `who` holds do `op` (stamp_set, min_l2 or max_l2) of `val` on `word`
#define STAMP_WRITE_(drain, op, who, word, val) do { drain; if (who) op((word), (val)); } while (0)
#define STAMP_NONE_ do {} while (0)
#define STAMP_CLOCK_ __builtin_amdgcn_s_memrealtime()
#define STAMP_DRAIN_ALL_ asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory")
#define STAMP_DRAIN_VM_ asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define STAMP_DRAIN_NOP_ asm volatile("s_nop 0" ::: "memory")
__device__ __forceinline__ void stamp_set(unsigned long long *p, unsigned long long v) { *p = v; }
// XCC_ID << 32 | HW_ID of the wave (HW_ID: wave 0-3, simd 4-5, cu 8-11, sh 12, se 13-15)
__device__ __forceinline__ unsigned long long stamp_hw_id() {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    return ((unsigned long long)xcc << 32) | hw;
}

// ---- SEIR.  STAMP / STAMP_DRAIN: k_hmc_step (in scope: ch, b, STAGE).  MSTAMP(st, i): the event-update kernels, `st` a
// MoveStamp -- who stamps is decided once per launch (MOVE_STAMP_CTX), narrowed (MOVE_STAMP_AND) and handed to mv_propose
// inside MvLds, which derives from it (MOVE_STAMP_PASS; MOVE_STAMP_PASS_INSIDE: only under SEIR_STAMP_PROPOSE)
#if STAMPS_SEIR
struct MoveStamp { bool on; };
#define STAMP(i) STAMP_WRITE_(, stamp_set, threadIdx.x == 0 && b == 0 && STAGE == SEIR_STAMP_STAGE, ch.stamps + (i), STAMP_CLOCK_)
#define STAMP_DRAIN(i) STAMP_WRITE_(STAMP_DRAIN_ALL_, stamp_set, threadIdx.x == 0 && b == 0 && STAGE == SEIR_STAMP_STAGE, ch.stamps + (i), STAMP_CLOCK_)
#define MOVE_STAMP_CTX(cond) MoveStamp{(cond)}
#define MOVE_STAMP_AND(st, cond) ((st).on = (st).on && (cond))
#define MOVE_STAMP_PASS(L, st) (static_cast<MoveStamp &>(L) = (st))
#define MSTAMP(st, i) STAMP_WRITE_(, stamp_set, threadIdx.x == 0 && (st).on, ch.stamps + (i), STAMP_CLOCK_)
// chain 0's role 0 in the pair launch whose S->E slot matches | its speculative role | k_move_delta's block
#define PAIR_ROLE0_STAMPS(do_se, b, se) MOVE_STAMP_CTX(!STAMPS_SEIR_PROPOSE && (do_se) && (b) == 0 && (se).slot == (SEIR_STAMP_SLOT & 2) && (se).scan == 0)
#define PAIR_SPEC_STAMPS(role, b, se) MOVE_STAMP_CTX((role) == SEIR_STAMP_ROLE && (b) == 0 && (se).slot == (SEIR_STAMP_SLOT & 2) && (se).scan == 0)
#define DELTA_STAMPS(b, bx) MOVE_STAMP_CTX(!STAMPS_SEIR_PROPOSE && (b) == 0 && (bx) == SEIR_STAMP_BLOCK)
#if STAMPS_SEIR_PROPOSE
#define MOVE_STAMP_PASS_INSIDE(L, st) MOVE_STAMP_PASS(L, st)
#else
#define MOVE_STAMP_PASS_INSIDE(L, st) STAMP_NONE_
#endif
#else
struct MoveStamp {};
#define STAMP(i) STAMP_NONE_
#define STAMP_DRAIN(i) STAMP_NONE_
#define MOVE_STAMP_CTX(cond) MoveStamp{}
#define MOVE_STAMP_AND(st, cond) STAMP_NONE_
#define MOVE_STAMP_PASS(L, st) STAMP_NONE_
#define MOVE_STAMP_PASS_INSIDE(L, st) STAMP_NONE_
#define MSTAMP(st, i) STAMP_NONE_
#define PAIR_ROLE0_STAMPS(do_se, b, se) MoveStamp{}
#define PAIR_SPEC_STAMPS(role, b, se) MoveStamp{}
#define DELTA_STAMPS(b, bx) MoveStamp{}
#endif

// ---- PAIR.  QSTAMP(st, i): thread 0 of the workgroup `st` (a PairStamp: chain within the launch, slot, step) describes;
// QSTAMP_T: by another thread.  In scope: ch
#if STAMPS_PAIR
struct PairStamp { int chain, slot, step; };
#define PAIR_STAMP_CTX(chain, slot, step) (PairStamp{(chain), (slot), (step)})
#define QSTAMP_T(st, thread, i) STAMP_WRITE_(, stamp_set, (thread) && (st).chain == 0 && (st).step < stamps::PAIR_STEPS && (st).slot < stamps::PAIR_SLOTS, \
                                             ch.stamps + stamps::pair_word((st).slot, (st).step, (i)), STAMP_CLOCK_)
#else
struct PairStamp {};
#define PAIR_STAMP_CTX(chain, slot, step) PairStamp{}
#define QSTAMP_T(st, thread, i) STAMP_NONE_
#endif
#define QSTAMP(st, i) QSTAMP_T(st, threadIdx.x == 0, i)

// ---- LEAP (k_leap; in scope: ch, s, b, it, and tix, nwg in the tiles, role, d in the roles).  LSTAMP_*: inside thread 0's
// own blocks.  CPROBE(st, k): inside hmc_chunk_role, `st` a RoleStamp (ROLE_STAMP_CTX: the role's words, or none).
// THE ONE SITE LEFT IN ITS EARLIER FORM: RoleStamp carries its pointer in every build and CPROBE_HOLD -- the values a stamped
// role must have back by its next CPROBE, "used" by an empty asm -- stays an `if` on it.  In the default build the pointer
// is null and the branch is dead, but it is dead only once hmc_chunk_role has been inlined: without those eleven dead
// branches the compiler allocates two instances of k_se_chunk (<1, 1> and <2, 1>) differently, 8 bytes more each
// ("Developer timelines").
struct RoleStamp { unsigned long long *p; };
#define CPROBE_HOLD(st, ...) do { if ((st).p) { asm volatile("" :: __VA_ARGS__); } } while (0)
#if STAMPS_LEAP
#if STAMPS_LEAP_LEVEL >= 2      // (atomics on one line per chain: they stretch what they time)
#define LSTAMP_MIN(k) STAMP_WRITE_(, min_l2, true, ch.stamps + stamps::leap_chain_word(b, it, (k)), STAMP_CLOCK_)
#define LSTAMP_MAX(k) STAMP_WRITE_(, max_l2, true, ch.stamps + stamps::leap_chain_word(b, it, (k)), STAMP_CLOCK_)
#else
#define LSTAMP_MIN(k) STAMP_NONE_
#define LSTAMP_MAX(k) STAMP_NONE_
#endif
#define LPROBE(k) STAMP_WRITE_(, stamp_set, b == 0 && threadIdx.x == 0 && (tix == 0 || tix == nwg / 2 + 5), \
                               ch.stamps + stamps::leap_tile_word(s.B, tix == 0 ? 0 : 1, it, (k)), STAMP_CLOCK_)
#define LALL_IS_ (b == 0 && threadIdx.x == 0 && it == 7 && tix < stamps::LEAP_ALL_TILES)
#define LALL(k) STAMP_WRITE_(, stamp_set, LALL_IS_, ch.stamps + stamps::leap_all_word(s.B, tix, (k)), STAMP_CLOCK_)
#define LALL_HW_ID() STAMP_WRITE_(, stamp_set, LALL_IS_, ch.stamps + stamps::leap_all_word(s.B, tix, 3), stamp_hw_id())
#define RPROBE(k) STAMP_WRITE_(, stamp_set, b == 0 && threadIdx.x == 0 && (role == 0 || role == d.ntc), \
                               ch.stamps + stamps::leap_role_word(s.B, role == 0 ? 0 : 1, it, (k)), STAMP_CLOCK_)
#if STAMPS_LEAP_INSIDE          // (the stamps INSIDE a role force its loads back early: they show the order of things, not the role's duration)
#define ROLE_STAMP_CTX() RoleStamp{(b == 0 && (role == 0 || role == d.ntc)) ? ch.stamps + stamps::leap_role_word(s.B, role == 0 ? 0 : 1, it, 0) : nullptr}
#else
#define ROLE_STAMP_CTX() RoleStamp{nullptr}
#endif
#define CPROBE(st, k) STAMP_WRITE_(STAMP_DRAIN_NOP_, stamp_set, (st).p && threadIdx.x == 0, (st).p + (k), STAMP_CLOCK_)
#else
#define LSTAMP_MIN(k) STAMP_NONE_
#define LSTAMP_MAX(k) STAMP_NONE_
#define LPROBE(k) STAMP_NONE_
#define LALL(k) STAMP_NONE_
#define LALL_HW_ID() STAMP_NONE_
#define RPROBE(k) STAMP_NONE_
#define ROLE_STAMP_CTX() RoleStamp{nullptr}
#define CPROBE(st, k) STAMP_NONE_
#endif

// ---- TAIL (k_se_chunk; in scope: ch, par): thread 0 of every workgroup of chain b_, min / max over them
#if STAMPS_TAIL
#define TSTAMP_IS_ (threadIdx.x == 0 && par == 1)
#define TSTAMP_MIN(b_, k) STAMP_WRITE_(, min_l2, TSTAMP_IS_, ch.stamps + stamps::tail_word((b_), (k)), STAMP_CLOCK_)
#define TSTAMP_MAX(b_, k) STAMP_WRITE_(, max_l2, TSTAMP_IS_, ch.stamps + stamps::tail_word((b_), (k)), STAMP_CLOCK_)
#define TSTAMP_MAX_DRAINED(b_, k) STAMP_WRITE_(STAMP_DRAIN_VM_, max_l2, TSTAMP_IS_, ch.stamps + stamps::tail_word((b_), (k)), STAMP_CLOCK_)
// one reading of the clock into a min-word and a max-word
#define TSTAMP_MINMAX(b_, kmin, kmax) do { if (TSTAMP_IS_) { const unsigned long long now_ = STAMP_CLOCK_; \
    STAMP_WRITE_(, min_l2, true, ch.stamps + stamps::tail_word((b_), (kmin)), now_); \
    STAMP_WRITE_(, max_l2, true, ch.stamps + stamps::tail_word((b_), (kmax)), now_); } } while (0)
#else
#define TSTAMP_MIN(b_, k) STAMP_NONE_
#define TSTAMP_MAX(b_, k) STAMP_NONE_
#define TSTAMP_MAX_DRAINED(b_, k) STAMP_NONE_
#define TSTAMP_MINMAX(b_, kmin, kmax) STAMP_NONE_
#endif

// ---- SE (se_tile): SE_STAMP_BEGIN(on) is the tile's start, kept in a SeStamp; SE_STAMP_END(st, on, ts, tile) stores it and the end
#if STAMPS_SE
struct SeStamp { unsigned long long t0; };
#define SE_STAMP_BEGIN(on) SeStamp{(on) ? STAMP_CLOCK_ : 0ull}
__device__ __forceinline__ unsigned long long se_stamp_end() {
    const unsigned long long id = stamp_hw_id();
    return (STAMP_CLOCK_ & 0xffffffffffffull) | ((id >> 32 & 0xf) << 60) | ((id >> 8 & 0xfff) << 48);
}
#define SE_STAMP_END(st, on, ts, tile) do { if (on) { \
    __syncthreads();                                  /* every wave's stores issued and acknowledged */ \
    STAMP_WRITE_(, stamp_set, threadIdx.x == 0, reinterpret_cast<unsigned long long *>(ts) + (tile) * stamps::SE_NW + 2, (st).t0); \
    STAMP_WRITE_(, stamp_set, threadIdx.x == 0, reinterpret_cast<unsigned long long *>(ts) + (tile) * stamps::SE_NW + 3, se_stamp_end()); } } while (0)
#else
struct SeStamp {};
#define SE_STAMP_BEGIN(on) SeStamp{}
#define SE_STAMP_END(st, on, ts, tile) STAMP_NONE_
#endif

// ---- EVAL (k_eval_all; in scope: cnt, NB, chain): thread 0 of chain 0's workgroup of tile 0 (the finish block passes 0)
#if STAMPS_EVAL
#define ESTAMP(tile, i) STAMP_WRITE_(, stamp_set, threadIdx.x == 0 && chain == 0 && (tile) == 0, cnt + (size_t)NB * EVC_STRIDE + (i), STAMP_CLOCK_)
#else
#define ESTAMP(tile, i) STAMP_NONE_
#endif

}  // namespace seir
#endif  // __HIPCC__

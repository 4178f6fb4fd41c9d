// Which kernels one sampler sweep launches, as data.  plan_sweep() reads the shape, the form the caller asked for
// (seir_sampler_desc::hmc_mode / moves_mode / leap_rows), where the chains run and what the chip holds, and returns every
// decision; enqueue_sweep (seir_hip.hip) launches what the plan says and decides nothing.  Host-only C++17 without HIP, so
// that tests/test_sweep_plan.py compiles it on its own.
#pragma once

namespace seir {

// the kernel constants the planner reads (seir_hip.hip holds them to the kernel headers)
namespace plan {
constexpr int WAVE = 64;         // device_math.h
constexpr int CT_MAXC = 16;      // logprob_kernels.h: day chunks the chunked leapfrog handles
constexpr int ROLE_SLOTS = 64;   // sampler_kernels.h: chunk roles per chain that leave parts of the trajectory's ends
constexpr int MMAX = 4;          // sampler_kernels.h: sub-moves of an event update (config["m"]) the library serves
constexpr int MM_SMALL = 2;      // sampler_kernels.h: ... and those the event-update kernels have instances of their own for
}  // namespace plan

// Can a 1-D grid of per * nb blocks keep every chain whole on one XCD (xcd_affine, logprob_kernels.h)?
inline bool xcd_affinity_applies(int per, int nb) {
    return (nb == 1 || nb == 2 || nb == 4 || (nb > 0 && nb % 8 == 0)) && ((long long)per * nb) % 8 == 0;
}

// the moves_mode in force: k_move_pair's launch tokens cover 62 launches per sweep, so more than 30 scans take the split form
inline int moves_form(int moves_mode, int n_scans) { return n_scans > 30 ? 1 : moves_mode; }
// the bound on the sub-moves the event-update instances of a sweep are compiled for (every kernel of the plan's `moves`,
// `fpend` and `record`, and k_move_delta): MM_SMALL -- the kernels' plain names -- where m allows it and the caller has not
// asked for the generic ones (SEIR_OPT_GENERIC_MOVES), else MMAX -- the `_m4` kernels.  Not part of SweepPlan: which
// launches a sweep makes does not depend on it
inline int move_mm(int m, bool generic) { return (m <= plan::MM_SMALL && !generic) ? plan::MM_SMALL : plan::MMAX; }
// tile scalars of the chunked leapfrog: 1 = column scalars only (the M-chunks sum the row partials themselves), 2 = all four
inline int chunk_ts_mode(int Mp) { return Mp <= 512 ? 1 : 2; }
// rows per band workgroup of the pair launches (pair_band_block, moves_kernel.h): ceil(M / nband), a constant of the launch
// that the kernels take as an argument (0: no band workgroups)
inline int band_rows(int M, int nband) { return nband > 0 ? (M + nband - 1) / nband : 0; }
// 64-day chunks a row of the series is held in by the proposing wave (moves_kernel.h; sampler_create caps T at 1024)
inline int move_nch(int Tp) { return Tp <= 6 * plan::WAVE ? 6 : Tp <= 12 * plan::WAVE ? 12 : 16; }

// hmc_mode -> the forms it allows; plan_sweep takes the first one that the shape and the placement permit.
//   chunked:  inner steps by 64-lane chunks (else every step by k_hmc_step<1>)
//   roles:    chunk roles inside the gradient launch (k_se_chunk, k_leap)
//   leap:     the inner steps in one persistent launch (k_leap)
//   fold:     ... with the trajectory's first step and both end-point gradients
//   end:      ... and its last half kick, accept test, adaptation and trace (else k_hmc_step<2>)
//   tailfold: the trajectory's first and last step by the chunk roles of L + 1 k_se_chunk launches, then k_hmc_final
struct HmcForm { bool chunked, roles, leap, fold, end, tailfold; };
constexpr HmcForm HMC_FORMS[7] = {
    //  chunked roles  leap   fold   end    tailfold
    {true,  true,  true,  true,  true,  true},    // 0 chunk
    {false, false, false, false, false, false},   // 1 single
    {true,  false, false, false, false, false},   // 2 chunk-split
    {true,  true,  false, false, false, false},   // 3 chunk-launch
    {true,  true,  true,  false, false, false},   // 4 chunk-leap
    {true,  true,  true,  true,  false, false},   // 5 chunk-stage
    {true,  true,  false, false, false, true},    // 6 chunk-launch-fold
};

struct SweepInputs {
    int M, Mp, Tp, ntc, nmt, nrb_d;       // shape (Dims, SamplerCfg)
    int nb, L, n_scans, record_events;    // the group's chains, leapfrog steps, scans, seir_sampler_desc::record_events
    int hmc_mode, moves_mode, leap_rows;  // the form asked for
    bool xcd_local;                       // blocks with the same id mod 8 share an XCD (probed at creation)
    bool one_group, use_graph;            // one chain group; replay of the captured graph
    int affinity;                         // SEIR_OPT_XCD_AFFINITY
    int cus;                              // compute units
    int leap_occ24, leap_occ32;           // workgroups per CU of k_leap<1,6,1,6> and of this shape's k_leap<TSM,NTC,2,4>
    bool pairs_lds;                       // k_move_pairs was granted its dynamic LDS (one workgroup per CU)
};

// hmc: the HMC path; inner: how STAGE runs the inner steps; ts_mode: 0 unchunked, else chunk_ts_mode.
// end_in_leap: FOLD closes the trajectory by k_leap's roles (hmc_mode 0), else by k_hmc_step<2> (5).  chunk_aff / final_aff:
// k_hmc_chunk (SPLIT) / k_hmc_final (TAILFOLD) on the 1-D XCD-affine grid.  per: chunk roles per chain (T- + M-chunks).
// nbv / nlive: chains of the 8-chain layout of the role launches, and those that exist when fewer (else 0).
// k_leap: 16-row tiles per workgroup (nst 1: one 24-row tile), row tiles, tile workgroups, chains per launch, those of them
// that exist, launches one after the other.  section_*: what seir_sampler_time_leapfrog reports (0: no section).
// moves: the event-update form; pre: a third role of k_move_pair pre-draws the next pair's S->E-type proposal; nband: band
// workgroups per chain in the pair launch (0: k_move_delta launches); nbk / pair_nlive: chains of the pair launch's layout
// and those that exist; nch: move_nch; move_aff: the event-update grid is the 1-D XCD-affine one; fpend: who applies the
// last accepted E->I update's F band; record / advance: k_record (events to the trace) / k_advance (the sweep counter, where
// no update launch advanced it) are launched.
struct SweepPlan {
    enum { FOLD, TAILFOLD, STAGE };                  // hmc
    enum { SINGLE, LEAP, SE_CHUNK, SPLIT };          // inner
    enum { PAIRS, PAIR, SPLIT_MOVES };               // moves: k_move_pairs / k_move_pair per pair / k_move_pa2 per update
    enum { F_NONE, F_PAIRS, F_RECORD, F_APPLY };     // fpend: none / k_move_pairs / k_record / k_apply_fpend
    int hmc, inner, ts_mode, per, nbv, nlive;
    bool end_in_leap, chunk_aff, final_aff;
    int leap_nst, leap_nmt, leap_wgs, leap_nbv, leap_nlive, leap_launches;
    int section_launches, section_evals;
    int moves, nband, nbk, pair_nlive, nch, fpend;
    bool pre, move_aff, record, advance;
};

inline SweepPlan plan_sweep(const SweepInputs &in) {
    SweepPlan p{};
    const HmcForm f = HMC_FORMS[in.hmc_mode];
    // [HMC] L + 1 gradient evaluations
    const bool chunked = f.chunked && in.L >= 3 && in.ntc <= plan::CT_MAXC;
    p.ts_mode = chunked ? chunk_ts_mode(in.Mp) : 0;
    p.per = in.ntc + in.Mp / plan::WAVE;
    const int ntile = in.ntc * in.nmt;
    // not a multiple of 8 chains: the layout of the next multiple with the missing chains' blocks retiring at once, so that
    // every chain is still whole on one XCD
    p.nbv = (in.nb + 7) / 8 * 8;
    p.nlive = p.nbv != in.nb ? in.nb : 0;
    // chunk roles inside a gradient launch: every chain on one XCD (probed at creation), one stream, the XCD-affine grid, no
    // graph capture (the tile counter does not care, but keep the two apart), an instance for the day chunks.  per <=
    // ROLE_SLOTS always holds under the sampler's caps, so hmc_mode 0 never reaches STAGE with SE_CHUNK
    const bool roles = chunked && f.roles && in.xcd_local && in.one_group && (in.affinity & 1) && !in.use_graph &&
                       (in.ntc == 1 || in.ntc == 6 || in.ntc == 12) && xcd_affinity_applies(ntile, p.nbv) &&
                       p.per <= plan::ROLE_SLOTS;
    // k_leap: every workgroup of the launch resident at once (its tiles wait for the roles).  Tile shape: 24-row workgroups
    // (k_leap<1,6,1,6>, one tile each) where they exist for the size and the launch fits, else 32 rows (two 16-row tiles)
    p.leap_nst = 2; p.leap_nmt = in.nmt; p.leap_wgs = ntile / 2; p.leap_nbv = p.nbv;
    bool leap = false;
    if (roles && f.leap && in.nmt <= plan::WAVE && in.nmt % 2 == 0) {
        const int nmt24 = in.Mp / 24, wgs24 = in.ntc * nmt24;
        auto fit = [&](int nbv) {
            if (in.leap_rows != 32 && p.ts_mode == 1 && in.ntc == 6 && in.Mp % 24 == 0 && xcd_affinity_applies(wgs24, nbv) &&
                (long long)(wgs24 + p.per) * nbv <= (long long)in.leap_occ24 * in.cus) {
                p.leap_nst = 1; p.leap_nmt = nmt24; p.leap_wgs = wgs24;
                return true;
            }
            return in.leap_rows != 24 && (long long)(ntile / 2 + p.per) * nbv <= (long long)in.leap_occ32 * in.cus;
        };
        // chains per launch: all of them -- or, for 16 chains, which do not fit the chip at once, two launches of 8 one
        // after the other (2 x 134 us at UK-380 against 335 us for the 18 launches of the per-step form; from 24 chains on
        // the per-step form is the faster one)
        leap = fit(p.nbv);
        if (!leap && in.nb == 16 && fit(8)) { leap = true; p.leap_nbv = 8; }
    }
    p.leap_nlive = p.leap_nbv == p.nbv ? p.nlive : 0;
    p.leap_launches = p.nbv / p.leap_nbv;
    p.hmc = leap && f.fold ? SweepPlan::FOLD : roles && f.tailfold ? SweepPlan::TAILFOLD : SweepPlan::STAGE;
    p.end_in_leap = p.hmc == SweepPlan::FOLD && f.end;
    p.inner = !chunked ? SweepPlan::SINGLE : leap ? SweepPlan::LEAP : roles ? SweepPlan::SE_CHUNK : SweepPlan::SPLIT;
    p.chunk_aff = (in.affinity & 1) && xcd_affinity_applies(p.per, in.nb);
    p.final_aff = xcd_affinity_applies(p.per, in.nb);          // (affinity bit 0 is not read for k_hmc_final)
    // the section time_leapfrog times: the trajectory (FOLD, TAILFOLD) or the inner steps (STAGE; LEAP counts one launch
    // even where it makes two of 8 chains)
    p.section_evals = p.hmc != SweepPlan::STAGE ? in.L + 1 : chunked ? in.L - 1 : 0;
    p.section_launches = p.hmc == SweepPlan::FOLD ? p.leap_launches : p.hmc == SweepPlan::TAILFOLD ? in.L + 2
                       : !chunked ? 0 : leap ? 1 : roles ? in.L - 1 : 2 * (in.L - 1);
    // [event updates] MultiScan(n_scans, Gibbs[move S->E, move E->I, occult S->E, occult E->I])
    const int moves = moves_form(in.moves_mode, in.n_scans);
    p.move_aff = (in.affinity & 2) && xcd_affinity_applies(in.nrb_d, in.nb);
    p.nch = move_nch(in.Tp);
    p.nbk = in.nb;
    if (moves == 1) {
        p.moves = SweepPlan::SPLIT_MOVES;
    } else {
        // band workgroups of 16 rows, two per wave; 32 (four per wave) where that is what lets every workgroup of the launch
        // hold a CU: sixteen chains at UK-380 are (3 + 12) x 16 = 240 workgroups
        int nband = (in.M + 15) / 16;
        if ((3 + nband) * p.nbv > in.cus && (3 + (in.M + 31) / 32) * p.nbv <= in.cus) nband = (in.M + 31) / 32;
        // the band inside the pair launch: every chain on one XCD, one stream, every workgroup resident at once (affinity
        // bit 1 is not read here)
        if (moves != 3 && in.xcd_local && in.one_group && !in.use_graph && (3 + nband) * p.nbv <= in.cus) {
            p.nband = nband;
            p.nbk = p.nbv;
            p.pair_nlive = p.nlive;
        }
        p.pre = moves == 0 || moves == 3 || moves == 4;
        // every pair of the sweep and the closing step in ONE launch: the grid of a pair launch with band workgroups
        const bool pairs = p.nband > 0 && moves == 0 && in.n_scans > 0 && in.pairs_lds;
        p.moves = pairs ? SweepPlan::PAIRS : SweepPlan::PAIR;
        p.fpend = pairs ? SweepPlan::F_PAIRS : in.n_scans == 0 ? SweepPlan::F_NONE
                : in.record_events ? SweepPlan::F_RECORD : SweepPlan::F_APPLY;
    }
    p.record = in.record_events && p.moves != SweepPlan::PAIRS;
    p.advance = in.n_scans == 0;
    return p;
}

}  // namespace seir

/* seir_hip.h -- C-ABI of libseirhip.so, the MI355X (gfx950) implementation of the
 * covid19uk spatial SEIR posterior hot path.
 *
 * The reference has no FFI for this path: the seam is the Python callable
 *     joint_log_prob(unconstrained_params[P], events[M,T,3]) -> scalar
 * (covid19uk/inference/inference.py:537-557) handed to the Gibbs/HMC/MH kernels
 * (inference.py:97-101, mcmc_kernel_factory.py:14-168), and below it
 *     DiscreteTimeStateTransitionModel(...).log_prob(events)
 * (covid19uk/model_spec.py:278-285).  Each entry point below names the
 * reference interface it stands in for.  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success and a negative seir_status on
 *     failure; seir_last_error() then returns a thread-local message;
 *   - the caller owns every host buffer, nothing is retained past the call;
 *   - a context owns its device buffers and one HIP stream, is bound to one
 *     device and is not thread-safe;
 *   - no exceptions, no global mutable state, no torch types;
 *   - layouts are the reference's: events[B][M][T][3] (M-major, fp64 counts),
 *     u[B][P] with P = 6 + (T-1) + M ordered psi, sigma_space, beta_area,
 *     gamma0, gamma1, alpha_0, alpha_t[T-1], spatial_effect[M]
 *     (inference.py:541-552); psi and sigma_space are unconstrained by
 *     softplus + eps (inference.py:525-535).
 *   - there is NO CPU fallback: without a HIP device seir_create fails.
 */
#ifndef SEIR_HIP_H
#define SEIR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEIR_ABI_VERSION 4

typedef enum {
    SEIR_OK = 0,
    SEIR_ERR_INVALID = -1,   /* bad argument / shape */
    SEIR_ERR_DEVICE = -2,    /* HIP runtime failure (no device, OOM, launch error) */
    SEIR_ERR_STATE = -3,     /* call made in the wrong state */
    SEIR_ERR_HANDOFF = -4    /* a wait inside a persistent launch timed out (see seir_sampler_pair_timeouts) */
} seir_status;

typedef struct seir_ctx seir_ctx;
typedef struct seir_sampler seir_sampler;

/* Everything `seir()`'s closure holds that does not depend on parameters
 * (model_spec.py:216-230), the CAR precision of spatial_effect() (:171-175),
 * the initial state handed to CovidUK (:139) and the constants of :22-26.
 * All pointers are host pointers, copied during seir_create. */
typedef struct {
    int32_t M;                 /* metapopulations (LADs) */
    int32_t T;                 /* time steps (days) */
    int32_t max_chains;        /* largest batch B any later call will use */
    int32_t device;            /* HIP device ordinal */
    const double *Cstar;       /* [M*M] row-major: C+C^T, diag = -colsum(C)  (:216-219) */
    const double *N;           /* [M] population */
    const double *W;           /* [T] commute volume (:221) */
    const double *weekday_c;   /* [T] centred weekday (:224-225) */
    const double *log_area_c;  /* [M] centred log(area/1e8) (:228-230) */
    const double *car_Q;       /* [M*M] D_w - 0.25 W_adj (:172-175) */
    double car_half_logdet;    /* 0.5*logdet(car_Q) */
    const double *init_state;  /* [M*4] S,E,I,R at step 0 (inference.py:511) */
    double nu;                 /* E->I rate, 0.28 (:26) */
    double time_delta;         /* 1.0 (:25) */
    double rate_floor;         /* 1e-9 (:264-266) */
} seir_desc;

int seir_abi_version(void);
const char *seir_last_error(void);

/* Shape limits.  seir_create accepts 1 <= M <= SEIR_MAX_M and 1 <= T <= SEIR_MAX_T and refuses anything else with
 * SEIR_ERR_INVALID before it allocates.  SEIR_MAX_T = 1088 = 17 x 64 is the longest series at which every launch a
 * context can make keeps its LDS within the 160 KiB of a gfx950 workgroup: the state scans of the four-launch and
 * prepared forms and of R_it hold [8 rows][ceil64(T)][2] fp64 next to a 2048-entry log-factorial table and 4.5 KiB of
 * static LDS (at T = 1152 that is 164.5 KiB).  The other entry points add limits of their own:
 *   seir_sampler_create       ceil64(T) <= 1024 and M <= 2048
 *   seir_reproduction_number  the context's limits (day tile of 16 up to ceil64(M) = 512, of 4 beyond)
 *   seir_within_between       the context's limits
 *   seir_simulate             M <= 1280 (124 ceil64(M) bytes of LDS per workgroup), any num_steps with num_steps x M < 2^31 */
#define SEIR_MAX_M 2048
#define SEIR_MAX_T 1088

/* CovidUK(covariates, initial_state, initial_step=0, num_steps=T)  (model_spec.py:139) */
int seir_create(const seir_desc *desc, seir_ctx **out);
void seir_destroy(seir_ctx *ctx);
int seir_num_params(const seir_ctx *ctx);          /* P */

/* Replace the initial state S,E,I,R [M*4] of the context (CovidUK's `initial_state`, model_spec.py:139;
 * inference.py:511).  Host pointer; ordered on the context stream.  Used by the T-sharded evaluation
 * (SURVEY.md 8e): a shard's state at its first day follows from the events of the shards before it.
 * With a sampler attached, call seir_sampler_set_state / _refresh afterwards. */
int seir_set_initial_state(seir_ctx *ctx, const double *init_state);

/* joint_log_prob(unconstrained_params, events) for a batch of B chains
 * (inference.py:537-557).  Host pointers; blocking. */
int seir_log_prob(seir_ctx *ctx, int32_t B, const double *u, const double *events,
                  double *logp /* [B] */);

/* The same value plus d/du, which the reference obtains by TF autodiff inside
 * PreconditionedHamiltonianMonteCarlo (mcmc_kernel_factory.py:21-27). */
int seir_log_prob_grad(seir_ctx *ctx, int32_t B, const double *u, const double *events,
                       double *logp /* [B] */, double *grad /* [B*P] */);

/* Device-pointer form of the two calls above: asynchronous on the context's
 * stream, no host copies.  grad_dev may be NULL (value only). */
int seir_log_prob_dev(seir_ctx *ctx, int32_t B, const double *u_dev, const double *events_dev,
                      double *logp_dev, double *grad_dev);

/* Stage split used when many parameter vectors are evaluated against the same
 * events (the 16 leapfrogs of one HMC step): `prepare` runs the parameter-free
 * part (state scan, binomial coefficients, mobility contraction F = Cstar.I/N),
 * `eval_prepared` only the parameter-dependent part. */
int seir_prepare_events_dev(seir_ctx *ctx, int32_t B, const double *events_dev);
int seir_eval_prepared_dev(seir_ctx *ctx, int32_t B, const double *u_dev,
                           double *logp_dev, double *grad_dev);

int seir_sync(seir_ctx *ctx);
void *seir_stream(seir_ctx *ctx);                  /* hipStream_t of the context */

/* Launch options of a context (no reference counterpart; the first two do not change a result):
 *   SEIR_OPT_DEBUG_SKEW      0 off; 1..3: test hook, a pseudo-random third of the workgroups of every
 *                            launch starts ~30 us late (results must not depend on workgroup timing)
 *   SEIR_OPT_XCD_AFFINITY    bit 0 gradient kernel, bit 1 event-update kernels: chain <-> XCD affine block
 *                            mapping (default 3); speed only
 *   SEIR_OPT_GEMM_F32        1: the mobility contraction F = Cstar . I/N (model_spec.py:262 for all days) with fp32
 *                            operands on v_mfma_f32_32x32x2_f32 instead of the fp64 matrix instruction (BASELINE
 *                            config 5).  THIS ONE CHANGES RESULTS: F carries ~1e-7 relative error, the log-prob
 *                            ~1e-8 -- outside the 1e-9 the fp64 path is held to; off by default.  Needs
 *                            ceil64(M) and ceil64(T) to be multiples of 128.
 *   SEIR_OPT_EVAL_FORM       launch form of seir_log_prob_dev (speed only): 0 (default) = the S->E term evaluated on the
 *                            contraction's accumulators and the row constants beside the matrix-core tiles, as ONE
 *                            launch for a batch of 8 or 16 chains (a multiple of 8 whose tile workgroups all fit the chip) on a
 *                            GPU that places block ids congruent mod 8 on one XCD each (state, tiles and reduction hand
 *                            over through that XCD's L2), as three launches otherwise; 1 = the four-launch form (scan, contraction, S->E tiles, reduction); 2 = always
 *                            three launches.  0 and 2 give the same bits
 *   SEIR_OPT_RT_STAGING_KIB  test hook: bound in KiB on the staging plane of a seir_sampler_rt batch (0, the default:
 *                            64 MiB), read by seir_sampler_rt_reset.  A smaller bound cuts a call into more batches of
 *                            trace slots; no result depends on it
 *   SEIR_OPT_GENERIC_MOVES   1: a sampler's event updates run the instances that serve every m <= SEIR_MMAX (the
 *                            `_m4` kernels) also where m <= 2 has instances of its own (the kernels' plain names, the
 *                            default); no result depends on it (speed only: the m <= 2 instances carry no code for
 *                            sub-moves that cannot exist).  seir_sampler_move_instance tells which ones a sweep launches
 * Options are read when a launch is enqueued (for a sampler using graph replay: at capture). */
enum { SEIR_OPT_DEBUG_SKEW = 0, SEIR_OPT_XCD_AFFINITY = 1, SEIR_OPT_GEMM_F32 = 2, SEIR_OPT_EVAL_FORM = 3,
       SEIR_OPT_RT_STAGING_KIB = 4, SEIR_OPT_GENERIC_MOVES = 5 };
int seir_set_option(seir_ctx *ctx, int32_t option, int32_t value);

/* Device memory helpers so that a ctypes host can keep inputs resident
 * without torch (torch tensors' data_ptr() work just as well). */
int seir_malloc(void **dev_ptr, uint64_t bytes);
int seir_free(void *dev_ptr);
int seir_memcpy_h2d(void *dst_dev, const void *src_host, uint64_t bytes);
int seir_memcpy_d2h(void *dst_host, const void *src_dev, uint64_t bytes);

/* HIP-event timing on the context's stream (torch.cuda.Event only sees
 * torch's own streams).  start/stop bracket whatever was enqueued between
 * them; stop blocks and returns milliseconds. */
int seir_timer_start(seir_ctx *ctx);
int seir_timer_stop(seir_ctx *ctx, float *ms);

/* Per-kernel timing: launches kernel `which` `iters` times back to back on the
 * context stream with the arguments of the last evaluation and returns the
 * mean launch duration in milliseconds (HIP events). */
enum { SEIR_K_SCAN = 0, SEIR_K_GEMM = 1, SEIR_K_SE_VALUE = 2, SEIR_K_SE_GRAD = 3,
       SEIR_K_FINISH = 4,
       /* the launches of the fused form (SEIR_OPT_EVAL_FORM 0) */
       SEIR_K_STATE = 5, SEIR_K_TILES_VALUE = 6, SEIR_K_TILES_GRAD = 7, SEIR_K_FINISH_FUSED = 8 };
int seir_time_kernel(seir_ctx *ctx, int32_t which, int32_t B, int32_t iters, float *mean_ms);

/* Self-test hook for the device math the kernels share (csrc/device_math.h):
 * for each x[i] > 0 returns L[i] = log(1-exp(-x)), inv[i] = 1/expm1(x) and
 * lfact[i] = log Gamma(floor(x)+1) as the kernels evaluate them.  Host pointers. */
int seir_selftest_math(seir_ctx *ctx, int32_t n, const double *x, double *L, double *inv, double *lfact);
/* the 8-term variant used where rates are not small (the I->R terms of the HMC kernels): L, inv as above */
int seir_selftest_math_wide(seir_ctx *ctx, int32_t n, const double *x, double *L, double *inv);

/* Every scalar function of csrc/device_math.h by itself (csrc/selftest_kernels.h): out0[i] = fn(x[i] [, y[i]]) as the
 * kernels evaluate it, one element per thread of 256-thread blocks, so the lanes of a wave take different branches.
 * Host pointers; y and out1 may be null for an op that has no second argument / second result.
 *   FAST_LOG, FAST_LOG_K, MV_LOG, FAST_RCP     x positive, normal and finite
 *   SOFTPLUS_TAB, SOFTPLUS                     x finite
 *   SOFTPLUS_SIGMOID_TAB                       x finite; out1 = sigmoid(x)
 *   LFACT_BF                                   x = n, an integer 0 .. 2^31 - 1
 *   LBINOM_TAB / _CONST / _BF                  x = n as above, y = k, any integer of |k| <= 2^31 (k < 0, k > n: -inf);
 *                                              _CONST is the form with the table in constant memory
 *   LOG1MEXP_TAB, LOG1MEXP                     x = r finite (r < 0: NaN)
 *   LOG1MEXP_SERIES                            x = r finite; out1 = 1 where `odd` was raised, else 0
 *   L1ME_INV_SERIES, L1ME_INV_K, L1ME_INV_SERIES_K   x = r finite; out0 = L, out1 = inv (the _K forms with SeK::load())
 *   LOG1MEXP_DIFF_SLOW                         x = r1, y = r0 finite: L(r1) - L(r0)
 * Arguments outside these domains, n < 1 and an unknown op are refused with SEIR_ERR_INVALID before any launch. */
enum { SEIR_FN_FAST_LOG = 0, SEIR_FN_FAST_RCP = 1, SEIR_FN_MV_LOG = 2, SEIR_FN_SOFTPLUS_TAB = 3,
       SEIR_FN_SOFTPLUS_SIGMOID_TAB = 4, SEIR_FN_SOFTPLUS = 5, SEIR_FN_LFACT_BF = 6, SEIR_FN_LBINOM_TAB = 7,
       SEIR_FN_LBINOM_CONST = 8, SEIR_FN_LBINOM_BF = 9, SEIR_FN_LOG1MEXP_TAB = 10, SEIR_FN_LOG1MEXP = 11,
       SEIR_FN_LOG1MEXP_SERIES = 12, SEIR_FN_L1ME_INV_SERIES = 13, SEIR_FN_L1ME_INV_K = 14,
       SEIR_FN_L1ME_INV_SERIES_K = 15, SEIR_FN_LOG1MEXP_DIFF_SLOW = 16, SEIR_FN_FAST_LOG_K = 17, SEIR_FN_COUNT = 18 };
int seir_selftest_fn(seir_ctx *ctx, int32_t op, int32_t n, const double *x, const double *y, double *out0, double *out1);

/* The delta log-ratios of the event updates, per element (arrays of n, host pointers; all values finite):
 *   SEIR_DELTA_BAND    band_delta(S, I, K0, F, dF, ee, psiW, rate_floor * dt, dt): a cell whose F moves by dF
 *   SEIR_DELTA_OWN_EI  the S->E piece of own_rows_delta for an E->I-type update, K0 (L(rr1) - L(rr0)) - (S - K0)(rr1 - rr0)
 *                      with rr0 = (ee (I + psiW F) + rate_floor) dt and rr1 the same with F + dF
 *   SEIR_DELTA_OWN_SE  the same piece for an S->E-type update: k_se goes from K0 to K0 + dk0 and S by dS at the rate rr0;
 *                      `dF` holds dk0 and `S` holds dS */
enum { SEIR_DELTA_BAND = 0, SEIR_DELTA_OWN_EI = 1, SEIR_DELTA_OWN_SE = 2 };
int seir_selftest_band_delta(seir_ctx *ctx, int32_t op, int32_t n, const double *S, const double *I, const double *K0,
                             const double *F, const double *dF, const double *ee, const double *psiW, double rate_floor,
                             double dt, double *out);

/* The wave and block primitives of csrc/device_math.h: thread tid of each of `nblocks` (1 .. 1024) 256-thread blocks
 * feeds in[block * 256 + tid] and stores what the primitive hands back in out[...]; `total` (block forms; may be null)
 * receives the block total every thread was handed.  is_int != 0: int32 arrays (SUM, INCL_SCAN, BLOCK_EXCL_SCAN only),
 * else double.  Host pointers. */
enum { SEIR_WAVE_SUM = 0, SEIR_WAVE_MIN = 1, SEIR_WAVE_INCL_SCAN = 2, SEIR_WAVE_INCL_SUFFIX_SCAN = 3,
       SEIR_BLOCK_EXCL_SCAN = 4, SEIR_BLOCK_INCL_SUFFIX_SCAN = 5, SEIR_BLOCK_SUM = 6 };
int seir_selftest_wave(seir_ctx *ctx, int32_t op, int32_t is_int, int32_t nblocks, const void *in, void *out, void *total);


/* ------------------------------------------------------------------------
 * Device-resident Metropolis-within-Gibbs sampler.
 *
 * Stands in for the kernel stack the reference assembles per window in
 * inference.py:86-101 / :151-167 / :219-228 and mcmc_kernel_factory.py:14-168:
 *   GibbsKernel[ (0, HMC [+DualAveraging [+DiagonalMassMatrixAdaptation]]),
 *                (1, MultiScanKernel(num_event_time_updates,
 *                      GibbsKernel[ MH(EventTimesUpdate S->E), MH(EventTimesUpdate E->I),
 *                                   MH(OccultUpdate S->E),     MH(OccultUpdate E->I) ])) ]
 * and for tfp.mcmc.sample_chain(num_results, ..., trace_fn=trace_results_fn)
 * (inference.py:107-115,232-240,245-282).  One "sweep" = one posterior draw of
 * every chain.  All state stays in HBM between calls; draws and traces are
 * written to a device-side burst buffer and read back with
 * seir_sampler_read_trace (the reference's per-burst posterior.write_samples,
 * inference.py:453-468).
 * ------------------------------------------------------------------------ */
#define SEIR_MMAX 4           /* upper bound on config["m"] */
#define SEIR_MOVE_TRACE (2 + 4 * SEIR_MMAX)   /* is_accepted, target_log_prob, m[], t[], delta_t[], x_star[] */

typedef struct {
    int32_t num_chains;             /* B <= ctx max_chains */
    int32_t dmax, nmax, m;          /* config["dmax"], ["nmax"], ["m"]   (mcmc_kernel_factory.py:79-81) */
    int32_t occult_nmax;            /* config["occult_nmax"]             (:106) */
    int32_t num_event_time_updates; /* config["num_event_time_updates"]  (:123) */
    int32_t t_range_lo, t_range_hi; /* occult window [lo, hi)            (inference.py:336-339) */
    int32_t num_leapfrog_steps;     /* 16                                (inference.py:326) */
    int32_t trace_capacity;         /* slots of the burst buffer: the kept draws it holds (= sweeps / thin) */
    int32_t first_chain_id;         /* global id of chain 0: selects the RNG stream (multi-GPU sharding) */
    int32_t record_events;          /* 0: no samples/seir; 1: int32 counts for every kept draw; 2: uint16 counts (half the
                                       burst buffer and half the bytes over PCIe; a count > 65535 in a kept draw makes
                                       the read fail -- sweeps dropped by `thin` are not looked at) */
    uint64_t seed;
    /* ---- ABI v2: launch form and test hooks; all-zero = the defaults ---------------------------- */
    int32_t moves_mode;             /* 0: paired event updates (k_move_pair's steps) with the S->E-type proposal
                                       pre-drawn one pair ahead -- every pair of a sweep and the closing step in ONE
                                       launch (k_move_pairs: the pair launch's grid with band workgroups, resident for
                                       the sweep; between two steps a chain's workgroups meet at a counter and drop
                                       their L1) where all of a chain's workgroups share an XCD
                                       (seir_sampler_xcd_local; any number of chains in the layout of the next multiple
                                       of 8, while every workgroup of the launch fits the chip), else one launch per
                                       pair; 4: always one launch per pair (k_move_pair, band workgroups in the launch
                                       under the same condition); 1: one proposal kernel per update (k_move_pa2) --
                                       kept as a cross-check; 2: as 4 without the pre-draw; 3: as 4 with the band part
                                       of the E->I-type log-ratio always as its own launch (k_move_delta).
                                       Same draws in all five.  The persistent forms (this one and hmc_mode 0) need
                                       every workgroup of their launch resident at once: one sampler at a time per GPU
                                       -- two such launches from different streams or processes can each hold part of
                                       the chip and wait for the rest; their waits are bounded, the sampler then fails
                                       loudly at the next read of the trace (seir_sampler_pair_timeouts), and modes 4 /
                                       hmc_mode 3 are the forms for a shared GPU */
    int32_t hmc_mode;               /* 0: the leapfrog steps by 64-lane chunk roles and the WHOLE trajectory in ONE
                                       persistent launch (k_leap: the gradient tiles keep their cells in registers over the
                                       L+1 gradient evaluations, tiles and chunk roles hand each other the partial sums / the
                                       next tables through the XCD's L2; the roles also draw the momentum, and at the end
                                       make the accept test -- each from the roles' parts, all alike -- restore the start
                                       point on rejection, and do the adaptation and the trace) when all of a chain's
                                       workgroups share an XCD (chain b's block ids are congruent to b mod 8; checked
                                       through XCC_ID at creation) and every workgroup of that launch fits the chip at
                                       once; else one launch per step with the chunk roles inside the gradient launch
                                       (k_se_chunk; needs the XCD placement only) between the stage kernels
                                       (k_hmc_step<0>, <2>); else the chunks as their own launch (k_hmc_chunk).
                                       Sixteen chains run it as two launches of eight, one after the other.
                                       Where the persistent launch does not fit (24+ chains at UK-380, SYN-2048) mode 0 runs
                                       as 6: the whole trajectory as L + 1 per-step launches (k_se_chunk) whose chunk roles also
                                       do the trajectory's first step and last half kick, and k_hmc_final (the accept test,
                                       adaptation and trace by the roles) -- no single-workgroup stage kernel.
                                       5: as 0 with the last half kick, accept test, adaptation and trace by
                                       k_hmc_step<2> as a launch of its own; 4: the persistent launch for the inner steps
                                       only; 3: one launch per step (k_se_chunk), never the persistent one; 2: chunks always
                                       as their own launch (2 and 3: same bits; 0, 4, 5 against them: same draws up to
                                       summation order); 1: every step by the single-workgroup kernel */
    int32_t use_graph;              /* 1: replay the sweep as a captured hipGraph (default: stream launches) */
    int32_t chain_groups;           /* chains split over this many streams (0 or 1: one stream) */
    int32_t disable_mask;           /* bit 0: HMC update, bits 1..4: S->E move, E->I move, S->E occult, E->I
                                       occult.  A disabled sub-kernel still draws its proposal (the random
                                       streams do not shift) but is always rejected -- used by the
                                       invariant-distribution tests to run each MH kernel alone */
    int32_t debug_pair;             /* test hooks of k_move_pair's handshake: 1 late, 2 absent speculative role (4, 8: the
                                       pre-drawing one); of k_move_pairs' steps, delays only: 16 band workgroups, 32 role 0,
                                       64 roles 1 and 2, 128 a third of all workgroups drawn again per step */
    int32_t leap_rows;              /* tile shape of the persistent leapfrog launch (hmc_mode 0, 4, 5; speed only, same draws up
                                       to the order of summation): 0 = auto -- workgroups of 24 rows x 64 days (six rows per
                                       wave) where ceil64(M) is a multiple of 24 with M <= 512 and T in six 64-day chunks
                                       (UK-380: 96 tile workgroups per chain, three on every CU of the chain's XCD) and the
                                       launch is resident, else 32 rows (two 16-row tiles per workgroup); 24 / 32: that shape
                                       only (the per-step form where it cannot be used) */
    int32_t thin;                   /* thinning interval k (0 or 1: every sweep is recorded; negative: SEIR_ERR_INVALID).
                                       The reference's Mcmc.thin, "Thin MCMC samples every 'thin' iterations"
                                       (example_config.yaml:33; inference.py:455 counts num_burst_samples * thin
                                       iterations per burst, the thinning itself it never built).  After a trace reset
                                       sweep i = 0, 1, ... is recorded iff (i + 1) % k == 0, in slot first_slot + i / k:
                                       tfp.mcmc.sample_chain(num_steps_between_results = k - 1).  The chain, its random
                                       streams and its adaptation see every sweep; only the trace writes of the others
                                       are skipped.  Exact across the 2^32 wrap of the sweep counter for k a power of two */
} seir_sampler_desc;

int seir_sampler_create(seir_ctx *ctx, const seir_sampler_desc *desc, seir_sampler **out);
void seir_sampler_destroy(seir_sampler *s);

/* current_state = [unconstrained params u[B][P], events[B][M][T][3]] (inference.py:563-576); host pointers */
int seir_sampler_set_state(seir_sampler *s, const double *u, const double *events);
int seir_sampler_get_state(seir_sampler *s, double *u, double *events, double *logp /* [B] running target_log_prob */);

/* HMC step size per chain and diagonal of the momentum precision ("variance",
 * i.e. M = diag(1/variance); NULL = identity = momentum_distribution None)
 * (hmc_kernel_kwargs, inference.py:324-329,384,405-406) */
int seir_sampler_set_kernel(seir_sampler *s, const double *step_size /* [B] */, const double *variance /* [B][P] */);
int seir_sampler_get_kernel(seir_sampler *s, double *step_size, double *variance);

/* Window mode (inference.py:60-121 fast, :125-196 slow, :199-242 fixed):
 * adapt_step_size -> DualAveragingStepSizeAdaptation(target_accept_prob,
 * num_adaptation_steps) restarted at the current step size;
 * adapt_mass -> DiagonalMassMatrixAdaptation seeded with the running
 * variance (count[B], mean[B][P], variance[B][P]) of get_weighted_running_variance
 * (inference.py:36-47).  Pointers may be NULL when adapt_mass == 0. */
int seir_sampler_set_adaptation(seir_sampler *s, int32_t adapt_step_size, int32_t adapt_mass,
                                int32_t num_adaptation_steps, double target_accept_prob,
                                const double *rv_count, const double *rv_mean, const double *rv_variance);

/* Recompute every cache (state planes, F, tables, running log-prob) from the
 * event planes and u; called implicitly by set_state. */
int seir_sampler_refresh(seir_sampler *s);

/* Start a new burst: the next sweep opens a group of `thin` sweeps whose last one is recorded in trace slot 0
 * (thin 1: trace slot 0 = the next sweep). */
int seir_sampler_reset_trace(seir_sampler *s);
/* The same with the first kept draw in slot `first_slot` (a slot, not a sweep): a burst buffer of 2 n slots used as two
 * halves lets burst k+1 run while burst k leaves the device (seir_sampler_read_trace_async). */
int seir_sampler_reset_trace_at(seir_sampler *s, int32_t first_slot);
/* Thinning interval of a live sampler (seir_sampler_desc::thin; 0 or 1: every sweep, negative: SEIR_ERR_INVALID), e.g.
 * 1 for the warm-up windows, whose running variance is formed from every draw (inference.py:36-47), then Mcmc.thin
 * (example_config.yaml:33) for the sampling bursts (inference.py:453-468).  It takes effect at the next
 * seir_sampler_reset_trace[_at]: sweeps enqueued before that reset are recorded by the old rule.  A captured graph is
 * dropped (the interval is a kernel argument).  A snapshot does not hold the interval: after seir_sampler_restore of a
 * snapshot taken under another interval, reset the trace before running.  seir_sampler_thin reads the value set last. */
int seir_sampler_set_thin(seir_sampler *s, int32_t thin);
int seir_sampler_thin(seir_sampler *s, int32_t *thin);
/* Enqueue num_sweeps sweeps on the context stream (asynchronous).  Sweeps, not kept draws: num_sweeps = n * thin fills
 * n trace slots, and the last kept draw is the chain's current state. */
int seir_sampler_run(seir_sampler *s, int32_t num_sweeps);
/* Blocking read of trace slots [first, first+count) -- slots are kept draws: with thinning interval k, slot j of a burst
 * holds sweep (j + 1) k - 1 of it, exactly what an unthinned run records for that sweep:
 *   theta  [count][B][P]           constrained draws (param_bijector.inverse, inference.py:375)
 *   events [count][B][M][T][3]     int32 counts -- uint16 if record_events == 2 -- (NULL to skip)
 *   hmc    [count][B][3]           is_accepted, target_log_prob, step_size (inference.py:255-261)
 *   moves  [count][B][4][SEIR_MOVE_TRACE]  per sub-kernel S->E move, E->I move, S->E occult,
 *          E->I occult of the LAST inner scan (MultiScanKernel returns the last results,
 *          inference.py:262-280) */
int seir_sampler_read_trace(seir_sampler *s, int32_t first, int32_t count, double *theta, void *events,
                            double *hmc, double *moves);

/* Overlapped egress of a burst (the reference's per-burst posterior.write_samples, inference.py:453-468,
 * without stalling the sampler): the copies are enqueued on a dedicated copy stream behind everything
 * already queued on the context stream and the call returns at once; sweeps enqueued afterwards run
 * concurrently with the transfer.  Arguments as seir_sampler_read_trace; the host buffers should be
 * page-locked (seir_host_alloc) -- pageable memory works but serialises.  seir_sampler_trace_wait
 * blocks until the last async read has landed; call it before touching the host buffers and before
 * re-using the trace slots being read. */
int seir_sampler_read_trace_async(seir_sampler *s, int32_t first, int32_t count, double *theta, void *events,
                                  double *hmc, double *moves);
int seir_sampler_trace_wait(seir_sampler *s);
/* Page-locked host memory for the calls above. */
int seir_host_alloc(void **host_ptr, uint64_t bytes);
int seir_host_free(void *host_ptr);

/* Mean launch duration (ms, HIP events on the context stream) of the sweep's
 * gradient kernel -- the S->E term + d/d eta sums over all B chains that runs
 * num_leapfrog_steps+1 times per sweep -- replayed `iters` times on the current
 * chain state (it only writes its partial-sum buffers). */
int seir_sampler_time_grad_kernel(seir_sampler *s, int32_t iters, float *mean_ms);

/* 1 if the context's GPU places workgroups whose ids are congruent mod 8 on one XCD each (XCC_ID of a probe grid at
 * creation): the condition under which hmc_mode 0 runs the chunk roles inside the gradient launch. */
int seir_sampler_xcd_local(seir_sampler *s);

/* Time-outs of waits inside a launch, per chain: out [B] = (a) k_move_pair launches in which the
 * authoritative workgroup gave up waiting for a speculative one (it then draws the proposal itself:
 * results are unaffected, throughput is not) + (b) waits that cannot be recovered from (band tokens,
 * k_se_chunk's tile flag, k_leap's flags, k_move_pairs' step barrier).  (a) is benign and only counted
 * here.  (b) makes the next seir_sampler_read_trace / seir_sampler_trace_wait fail with SEIR_ERR_HANDOFF
 * and the error is STICKY: a workgroup that gave up went on with stale data (the incrementally updated
 * F = Cstar . I/N can be out of step with the event planes afterwards), so seir_sampler_run and every read
 * of the trace keep failing until seir_sampler_restore, seir_sampler_set_state or seir_sampler_refresh has
 * rebuilt the state.  Both counts stay 0 outside the debug_pair test hooks and a GPU shared with
 * another persistent launch. */
int seir_sampler_pair_timeouts(seir_sampler *s, uint32_t *out);

/* Measurement hook (no reference counterpart): runs `sweeps` ordinary sweeps with a pair of HIP events around the
 * leapfrog section of each, on the stream the kernels are launched on.  What the section is depends on the launch form
 * in force:
 *   hmc_mode 0 (default, where it fits)  ONE launch, the persistent k_leap: the whole trajectory -- all L+1 gradient
 *                                        evaluations, the L leapfrog steps, accept test, adaptation and trace:
 *                                        launches = 1, evals = L+1;
 *   hmc_mode 5                           the same launch without the trajectory's end: launches = 1, evals = L+1;
 *   hmc_mode 4                           k_leap for the inner steps 1..L-1 only: launches = 1, evals = L-1;
 *   hmc_mode 6 (and 0 where k_leap       the whole trajectory as L+1 k_se_chunk launches and k_hmc_final:
 *     does not fit)                      launches = L+2, evals = L+1;
 *   hmc_mode 3 / 2                       the inner steps 1..L-1 as one k_se_chunk launch each (launches = L-1) or as
 *                                        k_se + k_hmc_chunk (launches = 2(L-1)): evals = L-1.
 * mean_ms = mean duration of that section.  The chains advance as in seir_sampler_run. */
int seir_sampler_time_leapfrog(seir_sampler *s, int32_t sweeps, float *mean_ms, int32_t *launches, int32_t *evals);

/* ------------------------------------------------------------------------
 * Surviving a placement failure of the persistent launches (no reference counterpart: the reference carries
 * `current_state` and the kernel results in host memory from burst to burst, inference.py:457-458, and cannot lose
 * a run to what else is on the GPU).
 *
 * hmc_mode 0 and moves_mode 0 need every workgroup of their launch resident at once; a second sampler, another
 * process or a profiler's replay pass can leave part of a grid unplaced, the bounded waits then time out and the
 * sampler reports SEIR_ERR_HANDOFF (see seir_sampler_pair_timeouts).  The burst loop of inference.py:453-468 is kept
 * alive like this:
 *     seir_sampler_snapshot(s, k & 1)            at the start of burst k (in stream order, a few device copies)
 *     seir_sampler_run(s, n); read the trace
 *     on SEIR_ERR_HANDOFF:  seir_sampler_restore(s, k & 1);  seir_sampler_set_launch_form(s, 3, 4);  run burst k again
 * A snapshot holds everything the next sweep's draws are a function of (event planes, state planes, F, the
 * tables, position, step size, adaptation state, sweep counter) -- not the trace.  After a restore the same
 * launch form reproduces the burst bit for bit, the per-step forms (hmc_mode 3, moves_mode 4) draw for draw with
 * continuous quantities equal up to the order of summation.  Two slots, so that a burst that is still being
 * copied out can be re-run as well.
 * ------------------------------------------------------------------------ */
int seir_sampler_snapshot(seir_sampler *s, int32_t slot /* 0 or 1 */);
int seir_sampler_restore(seir_sampler *s, int32_t slot);
/* Change the launch form (seir_sampler_desc::hmc_mode / moves_mode) of an existing sampler; what is sampled does not
 * change.  seir_sampler_launch_form reads the form in force. */
int seir_sampler_set_launch_form(seir_sampler *s, int32_t hmc_mode, int32_t moves_mode);
int seir_sampler_launch_form(seir_sampler *s, int32_t *hmc_mode, int32_t *moves_mode);
/* The launch plan in force: which kernels the next sweep of the first chain group launches.  seir_sampler_launch_form
 * reads the form that was ASKED for; a form that does not fit the shape, the number of chains or the chip is replaced
 * silently by the next one that does (csrc/sweep_plan.h: plan_sweep), and this is what it was replaced by.  Host fields
 * only: no device call, no stream synchronisation.  SEIR_ERR_INVALID for a NULL sampler or a NULL out. */
typedef struct seir_sweep_plan {
    int32_t hmc;            /* 0 FOLD: the trajectory in the persistent k_leap; 1 TAILFOLD: L + 1 k_se_chunk launches and
                             * k_hmc_final; 2 STAGE: k_hmc_step<0>, the inner steps as `inner` says, k_hmc_step<2> */
    int32_t inner;          /* inner steps: 0 k_hmc_step<1>; 1 k_leap; 2 k_se_chunk; 3 k_se + k_hmc_chunk */
    int32_t ts_mode;        /* tile scalars of the chunked leapfrog: 0 not chunked; 1 column scalars (Mp <= 512); 2 all four */
    int32_t per;            /* chunk roles per chain: day chunks + 64-row chunks */
    int32_t nbv, nlive;     /* chains of the layout of the role launches (a multiple of 8); those that exist when fewer, else 0 */
    int32_t end_in_leap, chunk_aff, final_aff;
    int32_t leap_nst;       /* k_leap: 2: 32-row workgroups of two 16-row tiles (k_leap<ts_mode,ntc,2,4>); 1: k_leap<1,6,1,6> */
    int32_t leap_nmt;       /* k_leap: row tiles of that shape */
    int32_t leap_wgs, leap_nbv, leap_nlive;
    int32_t leap_launches;  /* k_leap launches of leap_nbv chains, one after the other */
    int32_t section_launches, section_evals;   /* what seir_sampler_time_leapfrog reports */
    int32_t moves;          /* event updates: 0 k_move_pairs (one launch per sweep); 1 k_move_pair per pair; 2 k_move_pa2 per update */
    int32_t nband;          /* band workgroups per chain inside the pair launch; 0: k_move_delta launches */
    int32_t nbk, pair_nlive;
    int32_t nch;            /* 64-day chunks of the proposal kernels' instance: 6, 12 or 16 */
    int32_t fpend;          /* 0 none; 1 k_move_pairs; 2 k_record; 3 k_apply_fpend */
    int32_t pre, move_aff, record, advance;
    int32_t reserved[5];    /* zero */
} seir_sweep_plan;          /* 32 int32: 128 bytes */
int seir_sampler_sweep_plan(seir_sampler *s, seir_sweep_plan *out);
/* Which instances of the event-update kernels (the kernels of `moves`, `fpend` and `record` above, and k_move_delta) serve
 * updates of m sub-moves: the bound on the sub-moves their code is compiled for -- 2: the kernels under their plain names
 * (k_move_pairs<nch>, k_move_pair<nch>, k_move_pa2<nch>, k_move_delta<..>, k_record, k_apply_fpend), which serve m <= 2;
 * SEIR_MMAX: the `_m4` kernels (k_move_pairs_m4<nch>, ...), which serve every m.  Both give the same draws bit for bit
 * where both apply.  seir_move_instance: the rule itself -- host arithmetic, no device (generic_moves: the value of
 * SEIR_OPT_GENERIC_MOVES); SEIR_ERR_INVALID for m outside [1, SEIR_MMAX].  seir_sampler_move_instance: what the next
 * sweep of this sampler launches, from its m and its context's option as they are now. */
int seir_move_instance(int32_t m, int32_t generic_moves);
int seir_sampler_move_instance(seir_sampler *s, int32_t *mm);
/* Test hook: raises chain `chain`'s fatal time-out counter in stream order, i.e. leaves what a timed-out wait leaves.
 * The sweeps queued behind it run with every long wait of that chain cut short and the next read of the trace fails. */
int seir_sampler_debug_fail_handoff(seir_sampler *s, int32_t chain);

/* ------------------------------------------------------------------------
 * Summaries of samples/seir on the device: moments and marginals.
 *
 * Stand in for the reductions a consumer of the event tensor samples/seir [n][M][T][3] (written per burst by
 * inference.py:285-300 / :453-468) computes after reading it back: posterior mean and spread of incidence and of the
 * state per location and day, national curves per draw, cumulative incidence per location per draw.  They are formed
 * from the burst buffer where it lies, so that kilobytes per draw leave the device instead of megabytes.
 *
 * Definitions (csrc/summary_update.h).  Six integer quantities per cell (m, t), in this order: the event counts
 * k_se, k_ei, k_ir of the draw and the state S, E, I at the start of day t, scanned from the draw's recorded events
 * and the context's initial state (S[t] = S0 - sum_{s<t} k_se[s], ...: model_spec.compute_state; R follows from N).
 *   Moments, per chain b over the draws j = 0 .. n-1 folded since the last reset, exact integers:
 *     ref[b][m][t][q]   (int32)   the value in the first draw folded after the reset
 *     sum               (int64)   sum_j (x_j - ref)
 *     sumsq             (uint64)  sum_j (x_j - ref)^2
 *     count[b]          (uint64)  n
 *   mean = ref + sum / n and the unbiased variance (sumsq - sum^2 / n) / (n - 1) are formed by the host.  A sticky
 *   flag is raised when any sumsq reaches 2^63 (until then |sum| <= sumsq fits int64); seir_sampler_read_summary then
 *   fails with SEIR_ERR_STATE until the next reset.
 *   Marginals per kept draw, int64, indexed by trace slot like the trace itself ([count][B] leading):
 *     events_by_day      [count][B][T][3]  sum_m k
 *     events_by_location [count][B][M][3]  sum_t k
 *     state_by_day       [count][B][T][3]  sum_m (S, E, I)
 * All of it is integer arithmetic: no result depends on the order of additions, on the launch geometry or on how a
 * burst is cut into calls.  Sweeps dropped by thinning are not in the trace and not in the summaries.
 *
 * The feature is switched on by the first seir_sampler_summary_reset; a sampler that never calls it allocates and
 * does nothing more than before.  While it is on, seir_sampler_snapshot / _restore also save and restore the
 * accumulators, count and the flag (device copies in stream order): a burst can be folded as soon as it is enqueued,
 * and a burst that is run again after a hand-off time-out is not counted twice.  A snapshot taken before the first
 * reset holds no accumulators; restoring it leaves them as they are.
 * ------------------------------------------------------------------------ */
/* First call allocates; every call zeroes count, the accumulators and the overflow flag, in stream order: the next
 * draw folded becomes ref.  SEIR_ERR_STATE if the sampler was created with record_events == 0. */
int seir_sampler_summary_reset(seir_sampler *s);
/* Summarise trace slots [first_slot, first_slot + count) of every chain: asynchronous on the context stream, behind the
 * sweeps that fill those slots.  Writes the three marginals of those slots and, if accumulate != 0, folds the draws
 * into the moments in slot order (accumulate == 0: marginals only; accumulators and count untouched).
 * SEIR_ERR_INVALID for slots outside the burst buffer, SEIR_ERR_STATE before a reset or with record_events == 0. */
int seir_sampler_summarize(seir_sampler *s, int32_t first_slot, int32_t count, int32_t accumulate);
/* Blocking read of the marginals of slots [first, first + count) (written by the last seir_sampler_summarize that
 * covered them); any pointer may be NULL to skip that array.  Host pointers. */
int seir_sampler_read_marginals(seir_sampler *s, int32_t first, int32_t count,
                                int64_t *events_by_day, int64_t *events_by_location, int64_t *state_by_day);
/* The same on the copy stream of seir_sampler_read_trace_async, behind everything queued on the context stream so far;
 * completed by seir_sampler_trace_wait.  The host buffers should be page-locked (seir_host_alloc). */
int seir_sampler_read_marginals_async(seir_sampler *s, int32_t first, int32_t count,
                                      int64_t *events_by_day, int64_t *events_by_location, int64_t *state_by_day);
/* Blocking read of the moments: count [B]; ref, sum, sumsq each [B][M][T][6].  Any pointer may be NULL.
 * SEIR_ERR_STATE (and a message) if the overflow flag is up, or before a reset. */
int seir_sampler_read_summary(seir_sampler *s, uint64_t *count, int32_t *ref, int64_t *sum, uint64_t *sumsq);

/* ------------------------------------------------------------------------
 * Convergence diagnostics of the latent epidemic: batch sums and marks.
 *
 * Answer, without the event tensors leaving the device, the two questions a run of several chains is asked first: do
 * the chains agree (split R-hat), and how many independent draws is a chain worth (effective sample size).  Both follow
 * from integer accumulators kept next to the moments above; the formulas are the host's
 * (covid19uk_amd/posterior/diagnostics.py).
 *
 * Definitions (csrc/summary_update.h), per chain, cell (m, t) and quantity q as above.  The draws x_0 .. x_{n-1} folded
 * since the reset are cut into batches of L = batch_len draws, batch k being draws [kL, (k+1)L):
 *     bsum[b][m][t][q]    (int64)   sum of (x_j - ref) over the draws of the batch that is open
 *     bsumsq              (uint64)  sum over the closed batches of B_k^2, B_k being that batch's bsum when it closed
 *     nbatch[b]           (uint64)  closed batches, count[b] / L
 *   The sticky overflow flag of the moments is also raised when a batch closes with |bsum| >= 2^32 or bsumsq reaches
 *   2^63.  Whether a draw closes a batch depends on its number since the reset alone, (j + 1) % L == 0: as for the
 *   moments, no result depends on how a burst is cut into calls, launches or buffer halves.
 *   Marks: two device-side copies, numbered 0 and 1, of (count, sum, sumsq) as they stand when the mark is reached in
 *   stream order.  A mark carries the accumulators' ref, so the moments of the draws between two marks, or between a mark
 *   and the end, are exact integer differences -- the halves of split R-hat without a second set of accumulators.
 *
 * The feature is switched on by the first seir_sampler_diag_reset; a sampler that never calls it allocates, launches and
 * copies nothing more than before.  While it is on, seir_sampler_summarize(..., accumulate != 0) launches the instance
 * of k_summarize that carries the batch sums (16 B more per cell and quantity, read and written once per launch),
 * seir_sampler_summary_reset zeroes batch sums and marks as well (the batch length stays), and seir_sampler_snapshot /
 * _restore carry them: a burst that is run again after a hand-off time-out is counted once, and a mark taken in a burst
 * that is thrown away does not survive it.
 * ------------------------------------------------------------------------ */
/* First call allocates; every call sets the batch length and does what seir_sampler_summary_reset does (enabling the
 * summaries if need be), zeroing batch sums and marks with the moments.  A snapshot does not hold the batch length, so
 * what the snapshots taken before this call hold of moments, batch sums and marks is dropped: restoring one of them
 * afterwards restores the chain and leaves the accumulators as they are.  SEIR_ERR_INVALID for batch_len < 1,
 * SEIR_ERR_STATE if the sampler was created with record_events == 0. */
int seir_sampler_diag_reset(seir_sampler *s, int32_t batch_len);
/* Copy (count, sum, sumsq) into mark `which` (0 or 1), device to device, asynchronous on the context stream behind
 * everything queued so far.  SEIR_ERR_INVALID for another `which`, SEIR_ERR_STATE before a seir_sampler_diag_reset. */
int seir_sampler_diag_mark(seir_sampler *s, int32_t which);
/* Blocking read of the batch accumulators: nbatch [B]; bsum, bsumsq each [B][M][T][6].  Any pointer may be NULL.
 * SEIR_ERR_STATE (and a message) if the overflow flag is up, or before a seir_sampler_diag_reset. */
int seir_sampler_read_diag(seir_sampler *s, uint64_t *nbatch, int64_t *bsum, uint64_t *bsumsq);
/* Blocking read of mark `which`: count [B]; sum, sumsq each [B][M][T][6] (all zero for a mark not taken since the
 * reset).  Any pointer may be NULL.  Refused as seir_sampler_read_diag is. */
int seir_sampler_read_diag_mark(seir_sampler *s, int32_t which, uint64_t *count, int64_t *sum, uint64_t *sumsq);

/* ------------------------------------------------------------------------
 * Forecast on the device: posterior predictive of the next H days.
 *
 * Stands in for covid19uk/posterior/predict.py run on every kept draw: for each draw of trace slots
 * [first_slot, first_slot + count) the chain-binomial model of seir_simulate (below) is simulated `horizon` days forward
 * and the simulated counts are folded into moments and per-draw marginals, the way the summaries above fold the
 * recorded ones.  Neither the recorded nor the simulated event tensor crosses PCIe.
 *
 * Semantics (the one definition; kernels: csrc/forecast_kernels.h).
 *   Start.  Forecast day s = 0 is absolute day T, the day after the last recorded day.  The initial state of a draw is
 *     S0 + stoichiometry . sum_t events of that draw, integers formed on the device from the trace slot.  (The host path
 *     `posterior.predict` cannot start there: compute_state ends at the START of day T - 1.)
 *   Time indexing for t >= T is the reference's clip (model_spec.py:234-256).  The log baseline of every forecast day is
 *     a_last = alpha_0 + cumsum(alpha_t)[T-2] (alpha_0 when T = 1), the cumulative sum taken sequentially in index order in
 *     fp64 and then added to alpha_0, which is what np.cumsum does.  W[s] and the centred weekday weekday_c[s] of the H
 *     days are host arrays handed over at the reset (covid19uk_amd.posterior.predict.forecast_calendar).
 *   Optional random walk.  With log_baseline_steps [count][B][H] the baseline of forecast day s is a_last + c_s, c the
 *     sequential running sum of that draw's steps from zero (c_0 = step_0).  NULL holds the baseline.
 *   Random stream: seir_simulate's protocol unchanged -- Philox4x32-10, key = the forecast seed, counter = (attempt,
 *     64 + transition, s M + m, draw id) -- with draw id = (global chain id << 20) + j, j being the number of that chain's
 *     draws forecast since the last reset.  A forecast therefore does not depend on how bursts are cut into calls, on the
 *     launch geometry or on how chains are sharded over samplers, and one seir_simulate call per chain reproduces it
 *     (first_draw_id = chain << 20, num_draws = n).
 *   Rates, binomial sampler, rate floor, nu, dt: seir_simulate's, through the same device functions.
 *   Quantities and accumulators: those of the summaries (csrc/summary_update.h) with forecast day s in the place of t and
 *     the draw's own initial state in the place of the context's: k_se, k_ei, k_ir and S, E, I at the start of forecast
 *     day s; ref / sum / sumsq [B][M][H][6], count [B], and the sticky overflow flag.
 *   Marginals per kept draw, int64, indexed by trace slot:
 *     forecast_by_day       [count][B][H][3]  sum_m k
 *     forecast_by_location  [count][B][M][3]  sum_s k over the horizon
 *     forecast_state_by_day [count][B][H][3]  sum_m (S, E, I)
 * Limits: 1 <= horizon <= SEIR_FORECAST_MAX_H; M <= 1280 (the simulator's); global chain ids below 2048; fewer than 2^20
 * draws per chain between two resets; record_events != 0.
 *
 * Switched on by the first seir_sampler_forecast_reset; a sampler that never calls it allocates and launches nothing
 * more than before.  While it is on, seir_sampler_snapshot / _restore carry the forecast accumulators, count, flag and
 * the draw counter j, so that a burst run again after a hand-off time-out is forecast and counted once.  A snapshot taken
 * before the last reset holds none of it; restoring it leaves them as they are.
 * ------------------------------------------------------------------------ */
#define SEIR_FORECAST_MAX_H 128
/* First call (and a call with another horizon) allocates; every call zeroes count, moments and flag in stream order,
 * sets horizon, calendar (W, weekday_c: [horizon], copied) and seed and starts j at 0 again.  SEIR_ERR_INVALID for a
 * horizon outside [1, SEIR_FORECAST_MAX_H], M > 1280 or a global chain id >= 2048; SEIR_ERR_STATE with
 * record_events == 0. */
int seir_sampler_forecast_reset(seir_sampler *s, int32_t horizon, const double *W, const double *weekday_c, uint64_t seed);
/* Forecast the draws of trace slots [first_slot, first_slot + count) of every chain and fold them: asynchronous on the
 * context stream, behind the sweeps that fill those slots.  log_baseline_steps: host [count][B][H] or NULL (copied
 * before the call returns).  SEIR_ERR_INVALID for slots outside the burst buffer or when j would reach 2^20,
 * SEIR_ERR_STATE before a reset. */
int seir_sampler_forecast(seir_sampler *s, int32_t first_slot, int32_t count, const double *log_baseline_steps);
/* Blocking read of the forecast marginals of slots [first, first + count); any pointer may be NULL.  Host pointers. */
int seir_sampler_read_forecast_marginals(seir_sampler *s, int32_t first, int32_t count, int64_t *forecast_by_day,
                                         int64_t *forecast_by_location, int64_t *forecast_state_by_day);
/* The same on the copy stream, with the stream and the wait of seir_sampler_read_marginals_async
 * (seir_sampler_trace_wait completes it). */
int seir_sampler_read_forecast_marginals_async(seir_sampler *s, int32_t first, int32_t count, int64_t *forecast_by_day,
                                               int64_t *forecast_by_location, int64_t *forecast_state_by_day);
/* Blocking read of the forecast moments: count [B]; ref, sum, sumsq each [B][M][H][6].  Any pointer may be NULL.
 * SEIR_ERR_STATE (and a message) if the overflow flag is up, or before a reset. */
int seir_sampler_read_forecast(seir_sampler *s, uint64_t *count, int32_t *ref, int64_t *sum, uint64_t *sumsq);

/* ------------------------------------------------------------------------
 * Forecast intervals on the device: exact per-cell order statistics of the forecast draws.
 *
 * The moments above cannot give the interval of a small, zero-heavy, skewed count.  While the draw store is on, every
 * forecast draw leaves three int32 per (chain, location, forecast day) on the device, and at the end of the run exact
 * order statistics are selected from them there; only the selected values cross PCIe.
 *
 * Semantics (the one definition; kernels: k_forecast_keep of csrc/forecast_kernels.h, csrc/order_stats_kernels.h, the
 * narrowing step csrc/order_select.h).
 *   Store.  keep[B][3][M][H][cap] int32, the draw index innermost.  Draw j of chain b -- the j of the forecast's draw id --
 *     fills position j of every cell of that chain: nothing depends on how bursts are cut into calls, host batches or
 *     buffer halves, or on how chains are sharded over samplers; a burst run again after a hand-off time-out overwrites its
 *     own positions (seir_sampler_restore brings j back), so the store has no shadow copy.
 *   Planes, with the definitions of the forecast's quantities, for forecast day s:
 *     0 cases       the day's simulated I->R count k_ir[m][s]
 *     1 cum_cases   sum_{s' <= s} k_ir[m][s']  (day 6: the cases of the next 7 days)
 *     2 prevalence  I at the START of forecast day s (quantity 5 of the moments)
 *     All are non-negative and bounded by the location's population.
 *   Order statistic r of a cell of n values: np.sort(values)[r], exactly, in the order of signed int32.
 *   Size: B x 3 x M x H x cap x 4 bytes (UK-380 x 8 chains, H = 56, 5000 draws: 10.2 GB).
 * A sampler that never calls seir_sampler_forecast_keep allocates and launches nothing more than before.
 * ------------------------------------------------------------------------ */
#define SEIR_ORDER_STATS_MAX_RANKS 16
/* Size the draw store for `cap` draws per chain: after seir_sampler_forecast_reset and before the first
 * seir_sampler_forecast (SEIR_ERR_STATE otherwise).  Allocates on first use (and when cap changes); cap = 0 frees the
 * store, at any time.  A later seir_sampler_forecast_reset with the same horizon empties the store, one with another
 * horizon frees it.  While the store is on, seir_sampler_forecast refuses (SEIR_ERR_INVALID, naming both numbers) a call
 * that would take a chain past cap.  SEIR_ERR_INVALID, before anything is allocated, for cap outside [0, 2^20] and for a
 * store larger than half of what hipMemGetInfo reports free (the message carries both figures): the policy of a device
 * that is shared, not a measurement. */
int seir_sampler_forecast_keep(seir_sampler *s, int64_t cap);
/* Blocking.  Order statistics `ranks` [R] (strictly increasing, 1 <= R <= SEIR_ORDER_STATS_MAX_RANKS) of every cell over
 * the `count` draws per chain kept since the reset.  out is a host pointer: [R][B][3][M][H] with ranks in [0, count), or,
 * pooled != 0, [R][3][M][H] over the B x count values of the process's chains with ranks in [0, B x count).
 * SEIR_ERR_STATE before a reset, without a store, when no draw is kept yet or when the chains' counts differ;
 * SEIR_ERR_INVALID for R outside its range and for ranks out of range, unsorted or repeated. */
int seir_sampler_forecast_order_stats(seir_sampler *s, const int64_t *ranks, int32_t R, int32_t pooled, int32_t *out);
/* The selection alone, stateless, host pointers, blocking.  `cells` cells, cell c starting at values[c x cell_stride]; a
 * cell is n = segs x seg_len values in `segs` runs of seg_len contiguous values, seg_stride apart (values therefore spans
 * (cells - 1) cell_stride + (segs - 1) seg_stride + seg_len elements).  out [R][cells]: np.sort(cell)[ranks[r]].
 * SEIR_ERR_INVALID for counts below 1, n or cells of 2^31 or more, a negative stride, seg_stride < seg_len with segs > 1, and
 * for R and ranks as above. */
int seir_order_stats(seir_ctx *ctx, const int32_t *values, int64_t cells, int32_t segs, int64_t seg_len, int64_t seg_stride,
                     int64_t cell_stride, const int64_t *ranks, int32_t R, int32_t *out);

/* ------------------------------------------------------------------------
 * Reproduction number on the device: R_it moments and R_t per draw.
 *
 * Stands in for covid19uk/posterior/reproduction_number.py run on every kept draw, without samples/seir: for each draw
 * of trace slots [first_slot, first_slot + count), each day t of the window [T - days, T) and each location j the device
 * forms R_it[t][j] and folds it; neither the event tensor nor an [n][days][M] tensor crosses PCIe.
 *
 * Semantics (the one definition; kernels: csrc/rt_trace_kernels.h).
 *   Per-cell value.  R_it of a draw is bit-identical to what seir_reproduction_number (below) returns for that draw's
 *     theta and events: the same expressions, the sum over the source rows i as four partial sums (partial p takes
 *     i = p mod 4, ascending) combined as (p0 + p1) + (p2 + p3) and multiplied by the infectious period.  The reference's
 *     indexing is kept: a_t indexed with t, alpha_0 at t = 0, the clip at T - 1.  theta comes from the trace slot; S_it is
 *     formed as integers, S0 - sum_{u<t} k_se[u], from the recorded events of that slot.  The sampler's live workspace is
 *     not touched.
 *   Accumulators per chain, [B][days][M] (day-major, location-minor, as the reference's R_it [iteration, time, location]):
 *     ref   (double)    R_it of the chain's first draw folded since the reset
 *     sum   (double)    sum of (r - ref)
 *     sumsq (double)    sum of (r - ref)^2
 *     gt1   (uint32)    draws with r > 1.0
 *     count [B] (uint64)
 *     The fold is sequential in draw order per chain and cell, every operation rounded on its own (no FMA):
 *     d = r - ref; sum = sum + d; sumsq = sumsq + d * d.  A loop on the host restates every bit, and nothing depends on
 *     how a burst is cut into calls, buffer halves or batches.  mean = ref + sum / n, the unbiased variance
 *     (sumsq - sum^2 / n) / (n - 1) and P(R > 1) = gt1 / n are formed by the host.
 *   National curve per kept draw, indexed by trace slot: R_t [count][B][days] = sum_j R_it[t][j] weight[j], weight [M]
 *     handed over at the reset (N / sum N, reproduction_number.py:82-83).  No floating-point atomics: blocks of 64
 *     columns are summed in a fixed order each and then in ascending block order, so the value is the same bits in every
 *     run, for every cut and launch geometry.
 * Switched on by the first seir_sampler_rt_reset; a sampler that never calls it allocates and launches nothing more than
 * before.  While it is on, seir_sampler_snapshot / _restore carry the accumulators and count, so that a burst run again
 * after a hand-off time-out is folded once.  A snapshot taken before the last reset holds none of it; restoring it leaves
 * them as they are.
 * ------------------------------------------------------------------------ */
/* First call (and a call with another `days`) allocates; every call zeroes the accumulators and count in stream order and
 * takes weight [M] (copied).  SEIR_ERR_INVALID for days outside [1, T], a null weight pointer, or a sampler created with
 * record_events == 0. */
int seir_sampler_rt_reset(seir_sampler *s, int32_t days, const double *weight);
/* Form and fold R_it of trace slots [first_slot, first_slot + count) of every chain and write their R_t: asynchronous on
 * the context stream, behind the sweeps that fill those slots.  SEIR_ERR_INVALID for slots outside the burst buffer or
 * with record_events == 0, SEIR_ERR_STATE before a reset. */
int seir_sampler_rt(seir_sampler *s, int32_t first_slot, int32_t count);
/* Blocking read of R_t [count][B][days] of slots [first, first + count) (written by the last seir_sampler_rt that covered
 * them).  Host pointer. */
int seir_sampler_read_rt_draws(seir_sampler *s, int32_t first, int32_t count, double *R_t);
/* The same on the copy stream of seir_sampler_read_trace_async, behind everything queued on the context stream so far;
 * completed by seir_sampler_trace_wait.  The host buffer should be page-locked (seir_host_alloc). */
int seir_sampler_read_rt_draws_async(seir_sampler *s, int32_t first, int32_t count, double *R_t);
/* Blocking read of the accumulators: count [B]; ref, sum, sumsq, gt1 each [B][days][M].  Any pointer may be NULL.
 * SEIR_ERR_STATE before a reset. */
int seir_sampler_read_rt(seir_sampler *s, uint64_t *count, double *ref, double *sum, double *sumsq, uint32_t *gt1);

/* ------------------------------------------------------------------------
 * R_t intervals on the device: exact per-cell order statistics of the R_it draws.
 *
 * R_it is a sum of S (1 - exp(-x)) terms times a period that depends on the draw: its posterior per cell is skewed, and a
 * normal band from the moments above is wrong near 1.  While the draw store is on, every draw folded by seir_sampler_rt
 * leaves its R_it, one fp64 per (chain, window day, location), on the device, and at the end of the run exact order
 * statistics are selected from them there; only the selected values cross PCIe.
 *
 * Semantics (the one definition; kernels: k_rt_trace_keep of csrc/rt_keep_kernels.h, csrc/order_stats_kernels.h, the
 * narrowing step csrc/order_select.h).
 *   Store.  keepR[B][D][M][cap] fp64, the draw index innermost (the rows are padded to a multiple of 4 draws).  Draw j of
 *     chain b -- count[b] of seir_sampler_read_rt at the kernel's entry plus the draw's index in the call -- fills position j
 *     of every cell of that chain, with the bits of the R_it that is folded: k_rt_trace_keep runs in place of k_rt_trace
 *     and forms R_it once.  Nothing depends on how bursts are cut into calls, host batches or buffer halves, or on how
 *     chains are sharded over samplers; a burst run again after a hand-off time-out overwrites its own positions
 *     (seir_sampler_restore brings count back), so the store has no shadow copy.
 *   Order.  That of IEEE-754 totalOrder on the bit pattern: key = bits ^ (bits >> 63 ? ~0 : 1 << 63), compared as unsigned
 *     64-bit.  On values without NaN order statistic r is np.sort(values)[r], bit for bit, except that -0.0 sorts before
 *     +0.0; NaNs sort by sign and payload, negative ones first and positive ones last.
 *   Size: B x D x M x cap x 8 bytes (UK-380 x 8 chains, D = 14, 5000 draws: 1.70 GB; D = 365: 44 GB).
 * A sampler that never calls seir_sampler_rt_keep allocates and launches exactly what it did before.
 * ------------------------------------------------------------------------ */
/* Size the draw store for `cap` draws per chain: after seir_sampler_rt_reset and before the first seir_sampler_rt
 * (SEIR_ERR_STATE otherwise).  Allocates on first use (and when cap changes); cap = 0 frees the store, at any time.  A
 * later seir_sampler_rt_reset with the same days empties the store, one with another window frees it.  While the store is
 * on, seir_sampler_rt refuses (SEIR_ERR_INVALID, naming both numbers) a call that would take a chain past cap.
 * SEIR_ERR_INVALID, before anything is allocated, for cap outside [0, 2^20] and for a store larger than half of what
 * hipMemGetInfo reports free (the message carries both figures): the policy of a device that is shared, not a
 * measurement. */
int seir_sampler_rt_keep(seir_sampler *s, int64_t cap);
/* Blocking.  Order statistics `ranks` [R] (strictly increasing, 1 <= R <= SEIR_ORDER_STATS_MAX_RANKS) of every cell over
 * the `count` draws per chain kept since the reset.  out is a host pointer: [R][B][D][M] with ranks in [0, count), or,
 * pooled != 0, [R][D][M] over the B x count values of the process's chains with ranks in [0, B x count).
 * SEIR_ERR_STATE before a reset, without a store, when no draw is kept yet or when the chains' counts differ;
 * SEIR_ERR_INVALID for R outside its range and for ranks out of range, unsorted or repeated. */
int seir_sampler_rt_order_stats(seir_sampler *s, const int64_t *ranks, int32_t R, int32_t pooled, double *out);
/* The fp64 selection alone, stateless, host pointers, blocking: seir_order_stats for doubles in the order above, with the
 * same cell geometry and the same refusals.  out [R][cells]. */
int seir_order_stats_f64(seir_ctx *ctx, const double *values, int64_t cells, int32_t segs, int64_t seg_len, int64_t seg_stride,
                         int64_t cell_stride, const int64_t *ranks, int32_t R, double *out);

/* ------------------------------------------------------------------------
 * Within/between pressure shares on the device: moments per cell and the national pressures per draw.
 *
 * Stands in for covid19uk/posterior/within_between.py run on every kept draw, without samples/seir: for each draw of
 * trace slots [first_slot, first_slot + count), each day t of the window [T - days, T) and each location m the device
 * forms the within- and between-location infection pressure and folds their shares; neither the event tensor nor an
 * [n][days][M] tensor crosses PCIe.
 *
 * Semantics: the header comment of csrc/wb_kernels.h is the one definition.  In short: I_t is scanned as integers from the
 * slot's recorded events, psi is the slot's theta[0], W_t the context's W[t]; within = wi / tot and
 * between = be / tot are bit-identical to what seir_within_between returns for (psi, I_t, W_t), day T - 1 being the
 * reference's product.  A draw is defined for a cell iff both shares are finite; an undefined draw is counted in count[b]
 * and folded into nothing.
 *   Accumulators per chain, [B][days][M]:
 *     n       (uint32)  defined draws of the cell
 *     ref_w, ref_b (double)  the shares of the cell's first defined draw since the reset
 *     sum_w   (double)  sum of (within - ref_w);  sumsq_w  sum of (within - ref_w)^2;  sum_b  sum of (between - ref_b)
 *     gt      (uint32)  draws with within > between
 *     count [B] (uint64) draws folded, defined or not
 *     The fold is sequential in draw order per chain and cell, every operation rounded on its own (no FMA): a loop on the
 *     host restates every bit, and nothing depends on how a burst is cut into calls, buffer halves or batches.
 *   National pressures per kept draw, indexed by trace slot: within_pressure, between_pressure [count][B][days] =
 *     sum_m wi, sum_m be over all locations, defined or not.  No floating-point atomics: blocks of 64 columns are summed in
 *     a fixed order each and then in ascending block order.
 * Switched on by the first seir_sampler_wb_reset; a sampler that never calls it allocates and launches nothing more than
 * before.  While it is on, seir_sampler_snapshot / _restore carry the accumulators and count, so that a burst run again
 * after a hand-off time-out is folded once.  A snapshot taken before the last reset holds none of it; restoring it leaves
 * them as they are.  The staging plane of a call is bounded as seir_sampler_rt's (SEIR_OPT_RT_STAGING_KIB).
 * ------------------------------------------------------------------------ */
/* First call (and a call with another `days`) allocates; every call zeroes the accumulators and count in stream order.
 * SEIR_ERR_INVALID for days outside [1, T] or a sampler created with record_events == 0. */
int seir_sampler_wb_reset(seir_sampler *s, int32_t days);
/* Form and fold the shares of trace slots [first_slot, first_slot + count) of every chain and write their national
 * pressures: asynchronous on the context stream, behind the sweeps that fill those slots.  SEIR_ERR_INVALID for slots
 * outside the burst buffer or with record_events == 0, SEIR_ERR_STATE before a reset. */
int seir_sampler_wb(seir_sampler *s, int32_t first_slot, int32_t count);
/* Blocking read of the accumulators: count [B]; n, ref_w, sum_w, sumsq_w, ref_b, sum_b, gt each [B][days][M].  Any pointer
 * may be NULL.  SEIR_ERR_STATE before a reset. */
int seir_sampler_read_wb(seir_sampler *s, uint64_t *count, uint32_t *n, double *ref_w, double *sum_w, double *sumsq_w,
                         double *ref_b, double *sum_b, uint32_t *gt);
/* Blocking read of the national pressures [count][B][days] of slots [first, first + count) (written by the last
 * seir_sampler_wb that covered them).  Host pointers; either may be NULL. */
int seir_sampler_read_wb_draws(seir_sampler *s, int32_t first, int32_t count, double *within_pressure, double *between_pressure);
/* The same on the copy stream of seir_sampler_read_trace_async, behind everything queued on the context stream so far;
 * completed by seir_sampler_trace_wait.  The host buffers should be page-locked (seir_host_alloc). */
int seir_sampler_read_wb_draws_async(seir_sampler *s, int32_t first, int32_t count, double *within_pressure,
                                     double *between_pressure);

/* ------------------------------------------------------------------------
 * In-sample predictive check on the device: the last K days against the data.
 *
 * Stands in for covid19uk/posterior/predict.py run in sample on every kept draw (`predict -i -K -n K`, predict.py:96-120)
 * and for the comparison of its output with the observed removals: for each draw of trace slots
 * [first_slot, first_slot + count) the last `days` observed days are simulated again from the draw's state at day T - days,
 * folded into moments and per-draw marginals as the forecast's are, and counted against the data.  Neither the recorded
 * nor the simulated event tensor crosses PCIe.
 *
 * Semantics (the one definition; kernels: csrc/check_kernels.h, the per-day machinery is the forecast's).
 *   Window.  Check day s = 0 .. K - 1 is absolute day t = T - K + s.  The initial state of a draw is
 *     S0 + stoichiometry . sum_{t' < T - K} events of that draw, integers formed on the device from the trace slot; K = T
 *     starts from the context's initial state.
 *   Log baseline of day t, the reference's indexing (model_spec.py:242-256; covid19uk_amd.posterior.predict
 *     .log_baseline_path): alpha_0 if t = 0, otherwise alpha_0 + cumsum(alpha_t)[min(t - 1, T - 2)], the cumulative sum
 *     taken sequentially in index order in fp64 and then added to alpha_0, which is what np.cumsum does.  No random walk:
 *     the draw's own alpha_t.
 *   Calendar.  W[t] and the centred weekday of the window, centred over the T observed days: host arrays handed over at the
 *     reset (covid19uk_amd.posterior.predict.check_calendar, what `predict` builds for initial_step = T - K, num_steps = K).
 *   Rates, binomial sampler, rate floor, nu, dt: seir_simulate's, through the same device functions as the forecast.
 *   Random stream: seir_simulate's protocol -- Philox4x32-10, key = the seed given at the reset, counter = (attempt,
 *     64 + transition, s M + m, draw id) -- with draw id = (global chain id << 20) + j, j being the number of that chain's
 *     draws checked since the last check reset: a counter of its own, not the forecast's.  One seir_simulate call per chain
 *     reproduces a check (first_draw_id = chain << 20, num_draws = n); nothing depends on how bursts are cut into calls or
 *     batches, on the launch geometry or on how chains are sharded over samplers.
 *   Moments and marginals: exactly the forecast's with K in the place of H: ref / sum / sumsq [B][M][K][6], count [B], the
 *     sticky overflow flag, and per kept draw, int64, indexed by trace slot
 *       check_by_day       [count][B][K][3]  sum_m k
 *       check_by_location  [count][B][M][3]  sum_s k over the window
 *       check_state_by_day [count][B][K][3]  sum_m (S, E, I)
 *   Comparison with the data (csrc/check_update.h).  The I->R plane of every recorded draw is the data: no MH kernel
 *     targets it (mcmc_kernel_factory.py:127-162 move S->E and E->I only).  Integers, one set per chain, uint32 (a chain
 *     has fewer than 2^20 draws between two resets):
 *       obs [B][M][K]  (int32)  the recorded I->R count at day T - K + s of the first draw folded after a reset
 *       obs_moved [B]           sticky: a later draw's I->R counts in the window differ from obs (cannot happen with this
 *                               sampler; it guards the assumption).  While it is up the reads below fail with SEIR_ERR_STATE
 *       lt, eq [B][M][K]        draws whose simulated I->R count is < / == obs[m][s]
 *       loc_lt, loc_eq [B][M]   the same for sum_s simulated against sum_s obs
 *       day_lt, day_eq [B][K]   for sum_m simulated against sum_m obs
 *       all_lt, all_eq [B]      for the whole window over all locations
 *     gt is count - lt - eq and is not stored.  No floating-point value is accumulated anywhere in the comparison.
 * Limits: 1 <= days <= min(T, SEIR_CHECK_MAX_DAYS); M <= 1280 (the simulator's); global chain ids below 2048; fewer than
 * 2^20 draws per chain between two resets; record_events != 0.
 *
 * Switched on by the first seir_sampler_check_reset; a sampler that never calls it allocates and launches nothing more
 * than before.  While it is on, seir_sampler_snapshot / _restore carry the accumulators, the comparison counts, obs, the
 * flags and j, so that a burst run again after a hand-off time-out is checked and counted once.  A snapshot taken before
 * the last reset holds none of it; restoring it leaves them as they are.
 * ------------------------------------------------------------------------ */
#define SEIR_CHECK_MAX_DAYS 128
/* First call (and a call with another `days`) allocates; every call zeroes count, moments, comparison counts, obs and the
 * flags in stream order, sets the window, calendar (W, weekday_c: [days], copied) and seed and starts j at 0 again.
 * SEIR_ERR_INVALID for days outside [1, min(T, SEIR_CHECK_MAX_DAYS)], M > 1280 or a global chain id >= 2048;
 * SEIR_ERR_STATE with record_events == 0. */
int seir_sampler_check_reset(seir_sampler *s, int32_t days, const double *W, const double *weekday_c, uint64_t seed);
/* Check the draws of trace slots [first_slot, first_slot + count) of every chain: asynchronous on the context stream,
 * behind the sweeps that fill those slots.  SEIR_ERR_INVALID for slots outside the burst buffer or when j would reach
 * 2^20, SEIR_ERR_STATE before a reset. */
int seir_sampler_check(seir_sampler *s, int32_t first_slot, int32_t count);
/* Blocking read of the check's moments: count [B]; ref, sum, sumsq each [B][M][days][6].  Any pointer may be NULL.
 * SEIR_ERR_STATE (and a message) if the overflow flag is up, or before a reset. */
int seir_sampler_read_check(seir_sampler *s, uint64_t *count, int32_t *ref, int64_t *sum, uint64_t *sumsq);
/* Blocking read of the check's marginals of slots [first, first + count); any pointer may be NULL.  Host pointers. */
int seir_sampler_read_check_marginals(seir_sampler *s, int32_t first, int32_t count, int64_t *check_by_day,
                                      int64_t *check_by_location, int64_t *check_state_by_day);
/* The same on the copy stream, with the stream and the wait of seir_sampler_read_marginals_async
 * (seir_sampler_trace_wait completes it). */
int seir_sampler_read_check_marginals_async(seir_sampler *s, int32_t first, int32_t count, int64_t *check_by_day,
                                            int64_t *check_by_location, int64_t *check_state_by_day);
/* Blocking read of the comparison with the data: obs, lt, eq [B][M][days]; loc_lt, loc_eq [B][M]; day_lt, day_eq [B][days];
 * all_lt, all_eq [B].  Any pointer may be NULL.  SEIR_ERR_STATE (and a message) if a chain's obs_moved flag is up, or
 * before a reset. */
int seir_sampler_read_check_counts(seir_sampler *s, int32_t *obs, uint32_t *lt, uint32_t *eq, uint32_t *loc_lt,
                                   uint32_t *loc_eq, uint32_t *day_lt, uint32_t *day_eq, uint32_t *all_lt, uint32_t *all_eq);

/* ------------------------------------------------------------------------
 * Region totals on the device: per-draw sums over groups of locations.
 *
 * What leaves the device per kept draw is per location or national; the locations of a draw are correlated, so a region's
 * curve with its band cannot be rebuilt from either.  While a table of groups is set, every kept draw also leaves exact
 * integer sums of its event counts over each group's members -- for the recorded epidemic, the forecast and the in-sample
 * check -- and the host does the statistics (covid19uk_amd/posterior/groups.py).
 *
 * Semantics (the one definition; kernel: csrc/group_kernels.h).
 *   Table.  G groups as a CSR pair: offsets [G + 1] (offsets[0] = 0, strictly increasing: no empty group) and
 *     members [offsets[G]], rows in [0, M), ascending and unique within a group.  Groups may overlap and need not cover
 *     every location.  1 <= G <= SEIR_GROUPS_MAX.
 *   Sums, int64, indexed by trace slot, rewritten when a slot is summarised / forecast / checked again (no accumulators:
 *     snapshot and restore carry nothing of them):
 *       events_by_group [count][B][G][L][3]   sum over m in members(g) of k[m][t][x]; L = T (which = 0, the recorded events
 *                                             of the slot), H (1, the forecast's simulated counts), K (2, the check's)
 *       state0_by_group [count][B][G][3]      which = 1, 2: the members' sum of the draw's S, E, I at the window's start
 *                                             (day T, day T - K).  Not produced for which = 0: it is the context's initial
 *                                             state summed over the members, the same for every draw.
 *   No floating-point value is formed: the sums do not depend on the order of the adds, on the launch geometry or on how a
 *   burst is cut into calls.
 * A sampler that never sets a table allocates and launches nothing more than before.
 * ------------------------------------------------------------------------ */
#define SEIR_GROUPS_MAX 256
/* Copies the table and sizes the outputs of every source that is on (summaries, forecast, check); a later
 * seir_sampler_summary_reset / _forecast_reset / _check_reset sizes its source's again.  G = 0 frees everything (offsets and
 * members are not read).  SEIR_ERR_INVALID for G outside [0, SEIR_GROUPS_MAX], an empty group, non-monotone offsets, a
 * member outside [0, M), a non-ascending or repeated member, or outputs above half of the device's free memory;
 * SEIR_ERR_STATE with record_events == 0.  A refused table leaves the one in force alone.  When a source's reset cannot
 * size its outputs (the same refusal, returned by that reset) the source is on without group outputs: nothing is launched
 * for them and seir_sampler_read_group_marginals of it fails with SEIR_ERR_STATE until a later reset or groups_set fits. */
int seir_sampler_groups_set(seir_sampler *s, int32_t G, const int32_t *offsets, const int32_t *members);
/* Blocking read of the group sums of slots [first, first + count) of source `which` (0 trace, 1 forecast, 2 check).
 * Either pointer may be NULL; state0_by_group must be NULL for which = 0.  Host pointers.  SEIR_ERR_STATE before a table is
 * set or when the source is off. */
int seir_sampler_read_group_marginals(seir_sampler *s, int32_t which, int32_t first, int32_t count, int64_t *events_by_group,
                                      int64_t *state0_by_group);
/* The same on the copy stream, with the stream and the wait of seir_sampler_read_marginals_async
 * (seir_sampler_trace_wait completes it). */
int seir_sampler_read_group_marginals_async(seir_sampler *s, int32_t which, int32_t first, int32_t count,
                                            int64_t *events_by_group, int64_t *state0_by_group);
/* The kernel alone, on host arrays: events [n][M][L][3] (int32), the table as above; out [n][G][L][3] (int64).
 * M and L are the call's own, not the context's. */
int seir_group_sums(seir_ctx *ctx, const int32_t *events, int64_t n, int32_t M, int32_t L, int32_t G, const int32_t *offsets,
                    const int32_t *members, int64_t *out);

/* ------------------------------------------------------------------------
 * Group curves on the device: R_t and the within / between pressures of every kept draw per group of locations.
 *
 * seir_sampler_rt leaves the national curve R_t of every draw and seir_sampler_wb the national pressures; R_it, wi and be
 * of a draw exist only inside their kernels.  The locations of a draw are correlated through the commuting matrix, so the
 * per-location moments and quantiles do not combine into a region's band.  While a table of groups is set
 * (seir_sampler_groups_set) and a switch below is on, every draw that seir_sampler_rt / seir_sampler_wb folds also leaves
 *     Rg [slot][B][G][D]   sum over the members of weights[k] * R_it[t][m_k]      (seir_sampler_group_rt)
 *     Wg, Bg [slot][B][G][D]   sum over the members of wi[t][m], be[t][m]         (seir_sampler_group_wb)
 * wi and be are the cell values whose national sums are within_pressure and between_pressure: "between" is the pressure
 * from outside each member LOCATION, as in the national figure, not from outside the group.  Defined or not, a draw's cells
 * enter Wg and Bg as they enter the national sums; the host forms the share Wg / (Wg + Bg) and leaves out Wg + Bg == 0.
 *
 * THE definition of a group sum (kernel and its header comment: csrc/group_curve_kernels.h; NumPy:
 * covid19uk_amd/posterior/groups.py, weighted_sum_rows).  Members m_0 < ... < m_{n-1} in CSR order, weights w_k aligned with
 * `members`; lane l in [0, 64) starts from +0.0 and adds p = w_k * v[m_k] (one rounding; unweighted p = v[m_k]) for
 * k = l, l + 64, ... < n ascending, each add one rounding; then for o = 32, 16, 8, 4, 2, 1 all lanes at once
 * a_l = a_l + a_{l xor o}; the result is a_0.  No FMA, no floating-point atomics: the bits depend on the table alone, not on
 * the launch geometry, the debug skew or how a burst is cut into calls, buffer halves or batches.
 *
 * The outputs are indexed by trace slot and rewritten when a slot is folded again: snapshot and restore carry nothing of
 * them.  They are sized at whichever of table, switch and window reset comes last, and refused (SEIR_ERR_INVALID) above half
 * of the device's free memory.  A refusal at a reset leaves rt / within-between on without group outputs: nothing is launched
 * for them and the reads fail with SEIR_ERR_STATE.  While a switch is on the batches of seir_sampler_rt / _wb may shrink so
 * that the integer plane and the cell plane(s) stay within the staging bound (SEIR_OPT_RT_STAGING_KIB); no result depends on
 * the cut.  A sampler that never calls these entry points allocates and launches exactly what it did before.
 * ------------------------------------------------------------------------ */
/* weights [offsets[G]] aligned with the members of the table in force, finite (for a population-weighted curve
 * N[m_k] / the group's population).  NULL switches group R_t off and frees its buffers.  SEIR_ERR_STATE without a table or
 * with record_events == 0.  A later seir_sampler_groups_set switches it off: the weights belonged to the old table. */
int seir_sampler_group_rt(seir_sampler *s, const double *weights);
/* on != 0: group within / between on (SEIR_ERR_STATE without a table); 0: off, its buffers freed.  It stays on across a new
 * table (sized again for it) and goes off with seir_sampler_groups_set(G = 0). */
int seir_sampler_group_wb(seir_sampler *s, int32_t on);
/* Blocking reads of slots [first, first + count): Rg, Wg, Bg [count][B][G][D], host pointers; Wg or Bg may be NULL.
 * SEIR_ERR_STATE while the product or its switch is off or there are no group outputs. */
int seir_sampler_read_group_rt(seir_sampler *s, int32_t first, int32_t count, double *Rg);
int seir_sampler_read_group_wb(seir_sampler *s, int32_t first, int32_t count, double *Wg, double *Bg);
/* The same on the copy stream, with the stream and the wait of seir_sampler_read_marginals_async. */
int seir_sampler_read_group_rt_async(seir_sampler *s, int32_t first, int32_t count, double *Rg);
int seir_sampler_read_group_wb_async(seir_sampler *s, int32_t first, int32_t count, double *Wg, double *Bg);
/* The kernel alone, on host arrays: v [nd][L][M] (fp64), the table as for seir_group_sums, weights [offsets[G]] or NULL;
 * out [nd][G][L].  M and L are the call's own, not the context's. */
int seir_group_wsums(seir_ctx *ctx, const double *v, int64_t nd, int32_t L, int32_t M, int32_t G, const int32_t *offsets,
                     const int32_t *members, const double *weights, double *out);

/* ------------------------------------------------------------------------
 * Group next-generation matrix on the device: who infects whom by region.
 *
 * Rg[h] of seir_sampler_group_rt is the column sum of the next-generation matrix (covid19uk/model_spec.py:302-368) over ALL
 * destinations.  Its split by destination group cannot be rebuilt from anything else the device emits.  While the switch
 * below is on, every draw that seir_sampler_rt folds also leaves
 *     K [draw][B][G][G][D]   K[g][h][t]: the expected infections in group g caused by one typical infective of group h on
 *                            window day t (destination, source, day),
 * indexed by the draw's position since the rt reset.  THE definition (kernel and its header comment: csrc/ngm_kernels.h;
 * NumPy: covid19uk_amd/posterior/groups.py, ngm_rows and group_ngm):
 *   rows plane   P[g][t][j] = rt_combine(p0, p1, p2, p3, period), partial p adding the member POSITIONS k = p, p + 4, ... of
 *                g ascending by rt_cell (the cell arithmetic of R_it, model_spec.py:302-368, as csrc/rt_trace_kernels.h has
 *                it); for the group of all locations P is R_it bit for bit;
 *   matrix       K[g][h][t] = the group sum of P[g][t][.] over the members of h with `weights`, by the one definition of a
 *                group sum above.
 * No FMA beyond rt_cell's, no floating-point atomics: the bits depend on the table and the draw alone, not on the launch
 * geometry, the debug skew or the cut into calls, batches, buffer halves or shards.  A burst folded again after an rt reset
 * overwrites its own positions; snapshot and restore carry nothing of the store.  A sampler that never calls these entry
 * points allocates and launches exactly what it did before.
 * ------------------------------------------------------------------------ */
/* weights [offsets[G]] aligned with the members of the table in force, finite (N[m_k] / the group's population: the array
 * group R_t uses), cap >= 1 draws per chain: on, the store ngm [cap][B][G][G][D] and a batch's rows plane allocated.  NULL or
 * cap == 0: off, both freed.  Sized between seir_sampler_rt_reset and the first seir_sampler_rt, as seir_sampler_rt_keep is:
 * SEIR_ERR_STATE without a table, before an rt reset or once draws have been folded.  Refused (SEIR_ERR_INVALID) above half
 * of the device's free memory: the product is then off, seir_sampler_rt runs as before and the read fails with
 * SEIR_ERR_STATE.  While it is on, the batches of seir_sampler_rt may shrink so that the S plane, the cell plane and the rows
 * plane stay within the staging bound together (SEIR_OPT_RT_STAGING_KIB), and seir_sampler_rt refuses a call past cap
 * before any launch.  An rt reset with the same window empties the store; another window frees it (off), and so does
 * seir_sampler_groups_set: the weights belonged to the old table. */
int seir_sampler_group_ngm(seir_sampler *s, const double *weights, int64_t cap);
/* Blocking read of draws [first_draw, first_draw + count) since the rt reset: out [count][B][G][G][D] (destination, source,
 * day), a host pointer.  SEIR_ERR_STATE while rt or the switch is off; SEIR_ERR_INVALID past the draws folded. */
int seir_sampler_read_group_ngm(seir_sampler *s, int64_t first_draw, int64_t count, double *out);
/* The rows plane alone, on host arrays: theta [n][P] constrained draws, events [n][M][T][3] (int32: the trace layout with
 * one chain), days in [1, T] the window, the table as for seir_group_sums; out [n][G][days][M].  Runs in batches within the
 * staging bound. */
int seir_group_ngm_rows(seir_ctx *ctx, int32_t n, const double *theta, const int32_t *events, int32_t days, int32_t G,
                        const int32_t *offsets, const int32_t *members, double *out);

/* ------------------------------------------------------------------------
 * Stored draws into trace slots: every product from a posterior file.
 *
 * The reference samples once and derives its products afterwards from the stored draws (covid19uk/posterior/thin.py, then
 * predict.py, reproduction_number.py, within_between.py).  Every product above reads tr_theta and tr_events of trace slots
 * [first, first + count) and nothing else, and only range-checks the slots: nothing records which of them sweeps have filled.
 * seir_sampler_load_trace puts the rows of a posterior file (samples/<parameter>, samples/seir) into trace slots, so that
 * seir_sampler_summarize / _forecast / _rt / _check / _wb run on them as they run behind a sweep.
 *
 * THE definition of what a stored cell may hold, of the codes and of the key: csrc/trace_load.h (kernels and their header
 * comment: csrc/trace_load_kernels.h; NumPy: covid19uk_amd/posterior/replay.py, check_draws).  Events are stored in the
 * sampler's width (uint16 for record_events == 2, int32 for 1); a cell that is not an integer in [0, width's maximum] is
 * stored as 0 and counted.  The state S, E, I behind every day (boundaries 1 .. T; boundary T is where the forecast starts)
 * is formed from the context's initial state in int64 -- a file's counts are bounded by the width alone, unlike the
 * sampler's own -- and every compartment below zero is counted.  theta is copied bit for bit and its entries that are not
 * finite are counted; the hmc and moves entries of the slots become zeros.  Integers only: no floating-point arithmetic beyond
 * the conversion, no floating-point atomics; nothing depends on the launch geometry, the debug skew or the cut into chunks.
 * A sampler that never calls these entry points allocates and launches exactly what it did before.
 * ------------------------------------------------------------------------ */
/* Fills trace slots [first, first + count) of chain `chain`: theta [count][P] constrained draws in the order of
 * inference.py:541-552 (the file's values), events [count][M][T][3] fp64 counts in the layout of samples/seir.  Host
 * pointers.  Chain state, the sweep counter, the slot the next sweep records to, the thinning, the other chains' slots and
 * every product's accumulators stay as they are; a later seir_sampler_reset_trace + _run overwrites the slots as always.
 * The rows are staged in a device buffer of at most 64 draws and 256 MiB, allocated at the first load, and cross in chunks
 * (copy, kernels, next chunk) on the context stream.  Returns when the host buffers may be reused: it waits for its copies,
 * not for its kernels.  count == 0 does nothing.  SEIR_ERR_STATE with record_events == 0; SEIR_ERR_INVALID for a chain outside
 * [0, B), a range outside the capacity or a NULL pointer with count > 0 -- all before any launch. */
int seir_sampler_load_trace(seir_sampler *s, int32_t chain, int32_t first, int32_t count, const double *theta,
                            const double *events);
/* Blocking.  The counters since creation or since the last call with clear != 0:
 *   out[0..2]  cells that are not an integer / negative / over the width (LOAD_NOT_INTEGER, _NEGATIVE, _OVER_WIDTH)
 *   out[3]     (draw, location, boundary, compartment) states below zero
 *   out[4]     theta entries that are not finite
 *   out[5]     the smallest key flat_index * 8 + code of a bad item of the first call that had one (flat_index: the item's
 *              position in that call's events, read as (draw, location, boundary - 1, compartment) for a state, or theta)
 *   out[6..7]  that call's chain and first
 * All zeros: every slot loaded is a draw the product kernels may be run on. */
int seir_sampler_load_status(seir_sampler *s, uint64_t out[8], int32_t clear);

/* ------------------------------------------------------------------------
 * The state of the products: what is on, how it is sized and how far it has counted.
 *
 * The sampler is the one owner of this state; a binding asks for it and keeps no copy ("Who owns the product
 * state").  Every member is the value the entry points above act on at the moment of the call -- also after a call that
 * returned an error: a reset that was done before its group outputs were refused shows the new extent and no group outputs.
 * ------------------------------------------------------------------------ */
typedef struct seir_product_state {
    int32_t summary_on;      /* 1: seir_sampler_summary_reset (or _diag_reset) was called, the summaries are enabled */
    int32_t diag_batch_len;  /* batch length of the diagnostics in force; 0: seir_sampler_diag_reset was never called */
    int32_t forecast_H;      /* horizon of the forecast in force; 0: never reset */
    int32_t check_K;         /* window of the in-sample check in force; 0: never reset */
    int32_t rt_D;            /* window of the reproduction number in force; 0: never reset */
    int32_t wb_D;            /* window of the within/between shares in force; 0: never reset */
    int32_t groups_G;        /* groups of the table in force; 0: no table */
    int32_t groups_nnz;      /* its members (offsets[G]) */
    int32_t group_L[3];      /* day extent the group sums of the trace, the forecast and the check are sized for (T, H, K);
                              * 0: none -- no table, the source is off, or its outputs were refused */
    int32_t group_rt_on;     /* the switch of seir_sampler_group_rt */
    int32_t group_wb_on;     /* the switch of seir_sampler_group_wb */
    int32_t group_rt_D;      /* window the outputs of group R_t are sized for; 0: none (switch off, no table, seir_sampler_rt
                              * never reset, or refused) -- seir_sampler_rt forms the curves exactly when this is not 0 */
    int32_t group_wb_D;      /* likewise for group within / between and seir_sampler_wb */
    int32_t ngm_D;           /* window the store of the group next-generation matrix is sized for; 0: off */
    int64_t fc_j;            /* draws per chain forecast since the last seir_sampler_forecast_reset (the j of the draw id) */
    int64_t ck_j;            /* draws per chain checked since the last seir_sampler_check_reset */
    int64_t rt_j;            /* draws per chain folded by seir_sampler_rt since the last seir_sampler_rt_reset */
    int64_t ngm_cap;         /* draws per chain the store of the group next-generation matrix holds; 0: off */
    int64_t fc_keep_cap;     /* draws per chain the forecast's draw store holds (seir_sampler_forecast_keep); 0: none */
    int64_t rt_keep_cap;     /* draws per chain the R_it draw store holds (seir_sampler_rt_keep); 0: none */
    uint64_t reserved[2];    /* zero */
} seir_product_state;        /* 16 int32, 6 int64, 2 reserved words: 128 bytes, no implicit padding */

/* Fills *out from the sampler's host fields alone: no device call, no stream synchronisation, no allocation -- it may be
 * called at any time, between the enqueue of a burst and its wait as well, and it answers for a sampler that reported
 * SEIR_ERR_HANDOFF too, before the seir_sampler_restore that clears it.  SEIR_ERR_INVALID for a NULL sampler or a NULL out, and for nothing else. */
int seir_sampler_product_state(seir_sampler *s, seir_product_state *out);

/* ------------------------------------------------------------------------
 * Scenario forecasts on the device: what-if rollouts, paired differences.
 *
 * A scenario is the forecast's rollout of a draw with two changes, per forecast day s: the log baseline gets
 * log_shift[s] added (exp of it multiplies transmission) and the commuting volume is multiplied by commute[s] >= 0.  State,
 * parameters, Philox key and counter stay the forecast's, so scenario and baseline are coupled variate by variate and the
 * number a scenario is run for -- its difference to the baseline, per location and day, with its uncertainty -- is sharp.
 * THE definition of a scenario and of the fold: csrc/scenario_kernels.h; of the differences and a cell's update:
 * csrc/scenario_update.h; in NumPy: covid19uk_amd/posterior/scenarios.py.
 *
 * Per chain b, cell (m, s) and draw, with d_x[s] = k_x^k[m][s] - k_x^0[m][s] (scenario minus baseline, x = se, ei, ir):
 *     0 cases           d_ir[s]
 *     1 cum_cases       the inclusive scan of d_ir over the days
 *     2 prevalence      I at the start of day s, scenario minus baseline: exclusive scan of d_ei minus that of d_ir (day 0: 0)
 *     3 cum_infections  the inclusive scan of d_se
 * Over the draws folded a cell keeps, per difference, ref (int32, the first draw's value), sum (int64) and sumsq (uint64) of
 * the value minus ref, as the summaries do, and lt / eq (uint32), the draws whose difference is < 0 / == 0 (gt is never
 * stored).  mean = ref + sum / n, var = (sumsq - sum^2 / n) / (n - 1), P(below) = lt / n.  Integers only: no result depends on
 * the order of the draws, on the launch geometry or on how the draws are cut into calls.
 * ------------------------------------------------------------------------ */
#define SEIR_SCENARIO_MAX 4
#define SEIR_SCENARIO_Q 4
/* K scenarios ride on the sampler's forecast: log_shift and commute [K][H], H the horizon of the last
 * seir_sampler_forecast_reset; cap: the draws per chain the per-draw stores hold.  Accepted between a forecast reset and the
 * first seir_sampler_forecast, as seir_sampler_forecast_keep is (SEIR_ERR_STATE otherwise, and before any forecast reset).
 * From then on every draw that seir_sampler_forecast rolls forward is also rolled forward under each scenario, in the same
 * call: per scenario the forecast's moments [B][M][H][6] and per-draw marginals, the difference accumulators above, and the
 * by_day and state_by_day curves of every draw in stores indexed by the draw's position since the forecast reset.  The
 * forecast itself keeps its bits.  K = 0 or cap = 0 frees everything.  A forecast reset empties stores and accumulators and
 * keeps the scenarios (W_k = W[s] * commute[k][s] is formed again from its calendar); a reset to another horizon frees them.
 * A seir_sampler_forecast that would pass cap is refused before any launch.  SEIR_ERR_INVALID for K outside
 * [0, SEIR_SCENARIO_MAX], cap outside [0, 2^20], a non-finite value, a negative commute, or buffers above half of the device's
 * free memory.  The two kinds of refusal differ in what they leave: arguments refused for their values (K, cap, a
 * non-finite value, a negative commute) and a set refused for its place (SEIR_ERR_STATE) leave the scenarios in force alone,
 * as a refused table leaves the table in force; a set refused for memory has already dropped them (its buffers are sized
 * with the old ones gone) -- the forecast then runs on without scenarios.  Snapshot and restore carry the accumulators with the forecast's,
 * so a burst run again after a hand-off time-out is counted once; the stores are overwritten. */
int seir_sampler_scenarios_set(seir_sampler *s, int32_t K, const double *log_shift, const double *commute, int64_t cap);
/* out = K, H, cap, j (the draws per chain rolled forward since the forecast reset); zeros while no scenarios are set.  Host
 * fields only: no device call. */
int seir_sampler_scenario_state(seir_sampler *s, int64_t out[4]);
/* Blocking reads; any pointer may be NULL.  The scenarios' moments: count [K][B], ref, sum, sumsq [K][B][M][H][6] as
 * seir_sampler_read_forecast's; the difference accumulators: ref, sum, sumsq, lt, eq [K][B][M][H][4].  SEIR_ERR_STATE while no
 * scenarios are set, or when an accumulator of what is read has overflowed. */
int seir_sampler_read_scenarios(seir_sampler *s, uint64_t *count, int32_t *ref, int64_t *sum, uint64_t *sumsq);
int seir_sampler_read_scenario_diffs(seir_sampler *s, int32_t *ref, int64_t *sum, uint64_t *sumsq, uint32_t *lt, uint32_t *eq);
/* The curves of draw positions [first, first + count) since the forecast reset: by_day and state_by_day
 * [K][count][B][H][3] (int64), as forecast_by_day and forecast_state_by_day of the forecast's marginals. */
int seir_sampler_read_scenario_draws(seir_sampler *s, int64_t first, int64_t count, int64_t *by_day, int64_t *state_by_day);
/* The difference fold alone, on host arrays, blocking.  base_events and scenario_events are the simulated counts of n draws
 * per chain of the baseline and of one scenario, [n][B][M][H][3] (int32, >= 0; every row's total over the days below 2^31 and
 * the four differences within int32, as they are for populations below 2^31).  B, M and H are the call's own, not the
 * context's.  folded: the draws per chain that earlier calls have folded into the accumulators ref, sum, sumsq, lt, eq
 * [B][M][H][4] and *overflow; with folded == 0 they are outputs only and the call's first draw gives ref.  *overflow is 1
 * once some sumsq has reached 2^63 (the moments are then void), else 0.  SEIR_ERR_INVALID for a null pointer, n, B, M < 1,
 * H outside [1, SEIR_FORECAST_MAX_H], B above 65535, folded + n above 2^32 - 1 (lt and eq are uint32), or tensors above half
 * of the device's free memory. */
int seir_scenario_diffs(seir_ctx *ctx, const int32_t *base_events, const int32_t *scenario_events, int64_t n, int32_t B,
                        int32_t M, int32_t H, uint64_t folded, int32_t *ref, int64_t *sum, uint64_t *sumsq, uint32_t *lt,
                        uint32_t *eq, uint32_t *overflow);

/* ------------------------------------------------------------------------
 * Targeted scenarios on the device: per-location interventions and region totals.  It extends "Scenario forecasts on the
 * device" above and "Region totals on the device"; with neither entry point called every call and every bit is as before.
 *
 * A targeted scenario is a scenario whose two operands differ by location: log_shift[k][m][s] (any finite double) and
 * commute[k][m][s] (finite and >= 0) over the M locations and the H forecast days.  The rollout of a draw is
 * seir_sampler_scenarios_set's with two operands replaced (THE definition: csrc/scenario_local_kernels.h; in NumPy:
 * covid19uk_amd/posterior/scenarios.py, local_inputs):
 *     ea   = exp(base_0[s][nd] + log_shift[k][m][s])                          one rounded add, then the same exp
 *     psiW = psi * Wk[k][m][s],  Wk[k][m][s] = W[s] * commute[k][m][s]        one rounded multiply, formed on the host
 * State, parameters, Philox key and counter, draw id, the simulator's functions and the contraction stay the forecast's, so
 * common random numbers couple a targeted scenario to the baseline variate by variate.  Tensors that are constant over m
 * give bit for bit what seir_sampler_scenarios_set gives with the [K][H] arrays.
 * A local commute scales the commuting-borne pressure ON location m (the psi W F term of its hazard); it does not scale
 * what m exports.  A symmetric travel ban changes Cstar and is out of scope.
 * Launches: per batch one begin launch and, per day, the contraction and one day launch over K ndp columns, as for a
 * global set; a wave reads its two operands by scalar loads.  Device bytes: 2 x K x M x H x 8 in the place of the global
 * set's 2 x K x H x 8 and its base plane K x H x ndmax x 8.
 * ------------------------------------------------------------------------ */
/* seir_sampler_scenarios_set with log_shift and commute [K][M][H] (M the context's): the same place (between a forecast
 * reset and the first seir_sampler_forecast), the same refusals and what they leave (a refused value is named by its
 * [k][m][s]), the same stores, accumulators, K == 0 || cap == 0, memory policy and snapshot / restore.  It replaces what
 * either entry point set before; the global entry point replaces a local set.  A forecast reset to the same horizon keeps a
 * local set (Wk is formed again from the new calendar and the kept commute); a reset to another horizon frees it.
 * seir_sampler_scenario_state and the three reads above work unchanged on a local set. */
int seir_sampler_scenarios_set_local(seir_sampler *s, int32_t K, const double *log_shift, const double *commute, int64_t cap);
/* The per-draw region totals of the scenarios (extends seir_sampler_groups_set to the scenarios' rollouts), opt-in.  With the
 * switch on, a group table in force and scenarios set (either entry point), every batch of seir_sampler_forecast also sums
 * each scenario's simulated counts over the table's groups (k_group_sums on the scenario's slice of the staging tensor) into
 * a store by draw position since the forecast reset, [K][cap][B][G][H][3] int64, cap the scenarios'.  The call's positions
 * are zeroed in stream order before the launch, so a burst run again after a hand-off time-out overwrites them.  The store is
 * sized where the forecast's group outputs are (forecast reset, seir_sampler_groups_set) and at seir_sampler_scenarios_set*;
 * its K x cap x B x G x H x 24 bytes are part of what those calls hold against half of the device's free memory: refused at
 * seir_sampler_groups_set the table in force stays, refused at seir_sampler_scenarios_set* the forecast runs on without
 * scenarios.  A new table or G = 0 behind the first forecast turns the store off until the next forecast reset.
 * SEIR_ERR_STATE for on != 0 without a group table.  on == 0 frees the store. */
int seir_sampler_scenario_groups_set(seir_sampler *s, int32_t on);
/* Blocking read of draw positions [first, first + count) since the forecast reset: by_group [K][count][B][G][H][3], the
 * layout of seir_sampler_read_group_marginals' events_by_group per scenario.  SEIR_ERR_STATE while no scenarios are set or
 * the store is off; SEIR_ERR_INVALID for positions outside the draws forecast since the reset. */
int seir_sampler_read_scenario_group_draws(seir_sampler *s, int64_t first, int64_t count, int64_t *by_group);

/* ------------------------------------------------------------------------
 * Triggered scenarios on the device: measures that switch on and off by the draw's own simulated case counts.  It extends
 * "Targeted scenarios on the device" above; with none of its entry points called every call and every bit is as before.
 *
 * A triggered scenario k is a targeted scenario with two operand pairs per (m, s) -- the off pair log_shift, commute and the
 * on pair log_shift_on, commute_on, each under the targeted tensors' refusals -- and a rule that picks one of them per draw
 * and day (THE definition: csrc/scenario_trigger_kernels.h and csrc/trigger_update.h; in NumPy:
 * covid19uk_amd/posterior/scenarios.py, trigger_states and triggered_inputs).  Per scenario the rule has window w in
 * [1, SEIR_TRIGGER_MAX_WINDOW], from_day in [0, H], min_days >= 0 and review_every >= 1, per location the integer thresholds
 * 0 <= off[k][m] <= on[k][m] <= INT32_MAX (on = INT32_MAX: the location never triggers).  At the start of rollout day s, per
 * (k, m, draw): c = the sum of the I->R counts of the w days before absolute day T + s (scenario k's own simulated counts
 * for days >= T, the draw's recorded counts for days in [0, T), 0 before day 0); on a review day (s >= from_day and
 * (s - from_day) % review_every == 0): not active and c >= on: active <- 1, age <- 0; otherwise active and age >= min_days and
 * c < off: active <- 0.  Day s is rolled with the on pair iff active; behind it, if active, age <- age + 1.  At day 0
 * active = 0.  The day is the targeted scenario's with the selected operands: one rounded add, one rounded multiply either
 * way, so a rule that never fires is bit for bit the targeted scenario with the off tensors and a rule that fires everywhere
 * at day 0 and never releases the targeted scenario with the on tensors.  Common random numbers couple it to the baseline.
 * Products, integers only: active_count [K][B][M][H] (uint32), the draws of chain b in which m is under the measure on day s,
 * and active_by_day [K][cap][B][H] (int32), the locations under the measure by draw position since the forecast reset.
 * Launches: per batch one begin launch, per day the contraction and one day launch (as for a targeted set), and per batch
 * and scenario one fold of the rule's record (two 64-bit words per row and column).  Out of scope: rules on anything but
 * the location's own I->R counts, pooling over ranks.
 * ------------------------------------------------------------------------ */
#define SEIR_TRIGGER_MAX_WINDOW 28
/* seir_sampler_scenarios_set_local with a rule: log_shift, commute (the off pair) and log_shift_on, commute_on (the on pair)
 * [K][M][H]; on, off [K][M]; params [K][4] = window, from_day, min_days, review_every.  The same place, K == 0 || cap == 0,
 * stores, memory policy (the new tensors, planes and outputs are part of the sum held against half of the free memory),
 * snapshot / restore (active_count travels with the scenarios' accumulators) and what a refusal leaves as the other two
 * entry points; a refused value is named by its indices.  It replaces what any entry point set before, and they replace it.
 * The three reads of a scenario set and the scenarios' region totals work unchanged on a triggered set. */
int seir_sampler_scenarios_set_triggered(seir_sampler *s, int32_t K, const double *log_shift, const double *commute,
                                         const double *log_shift_on, const double *commute_on, const int32_t *on,
                                         const int32_t *off, const int32_t *params, int64_t cap);
/* Blocking reads: active_count [K][B][M][H]; active_by_day [K][count][B][H] of draw positions [first, first + count).
 * SEIR_ERR_STATE while no scenarios are set or the set in force is not a triggered one. */
int seir_sampler_read_scenario_triggers(seir_sampler *s, uint32_t *active_count);
int seir_sampler_read_scenario_trigger_draws(seir_sampler *s, int64_t first, int64_t count, int32_t *active_by_day);
/* The fold of the rule's record alone, on host arrays, blocking.  masks [n][B][M][2] (uint64): bit s of the 128 is set iff
 * the location is under the measure on day s in that draw; bits at days >= H are ignored.  B, M and H are the call's own.
 * folded: the draws per chain that earlier calls have folded into active_count [B][M][H]; with folded == 0 it is an output
 * only.  active_by_day [n][B][H] is an output.  SEIR_ERR_INVALID for a null pointer, n, B, M < 1, H outside
 * [1, SEIR_FORECAST_MAX_H], B above 65535, folded + n above 2^32 - 1, or buffers above half of the device's free memory. */
int seir_trigger_counts(seir_ctx *ctx, const uint64_t *masks, int64_t n, int32_t B, int32_t M, int32_t H, uint64_t folded,
                        uint32_t *active_count, int32_t *active_by_day);

/* ------------------------------------------------------------------------
 * Scoring the forecast against later data.
 *
 * Once the days a forecast predicted have been observed, the forecast is scored against them: out of sample, the
 * complement of the in-sample check.  The targets, per location m and forecast day s, are planes 0 and 1 of the draw store:
 *     0 cases       the I->R count of the day
 *     1 cum_cases   its running total over the horizon
 * truth [M][H] is int32 with -1 (any negative value) for "not observed"; cum_cases of (m, s) has a truth only while every
 * day <= s of location m has one.  Per chain, cell and target, over the forecast draws x_1..x_n since the forecast's reset:
 *     lt = #{x_i < y}      eq = #{x_i == y}      abs_sum = sum |x_i - y|      (uint32, uint32, uint64; csrc/verify_update.h)
 *     pair_sum D = sum_{i<j} |x_i - x_j|                                       (int64; k_pair_abs of csrc/verify_kernels.h)
 * from which the host forms the mid-p PIT (lt + eq/2)/n, MAE abs_sum/n and the sample CRPS abs_sum/n - D/n^2
 * (covid19uk_amd/posterior/verify.py is THE definition in NumPy).  lt, eq and abs_sum of several chains or runs pool by a
 * sum; D does not: the pooled D is the same quantity over the union of the draws, computed with segs = B.  A cell without
 * truth keeps zeros.  Everything is integer: no result depends on the launch geometry, the debug skew or how a burst is cut
 * into calls, buffer halves or batches.
 * ------------------------------------------------------------------------ */
#define SEIR_PAIR_ABS_CHUNK 4096      /* values of a cell sorted in LDS at a time */
/* D <= floor(n^2 / 4) (2^32 - 1): below 2^63 exactly while floor(n^2 / 4) <= 2^31, that is n <= 92 681 */
#define SEIR_PAIR_ABS_MAX_N 92681
/* truth [M][H] (H the horizon of the last seir_sampler_forecast_reset) rides on the sampler's forecast: set between that
 * reset and the first seir_sampler_forecast.  From then on every batch that seir_sampler_forecast rolls forward is folded
 * against it in the same call (k_verify_fold, an ordinary launch on the context stream).  A forecast reset to the same
 * horizon empties the accumulators and keeps the truth; a reset to another horizon frees it; truth == NULL turns it off (with or without a forecast: never refused for its place).
 * SEIR_ERR_STATE without a forecast or behind the first forecast call (what is in force stays); SEIR_ERR_INVALID above half
 * of the device's free memory (what was in force is gone: the forecast runs on unscored).  Snapshot and restore carry the
 * accumulators with the forecast's, so a burst run again after a hand-off time-out is counted once. */
int seir_sampler_verify_set(seir_sampler *s, const int32_t *truth);
/* out = on, H, j (the draws per chain folded since the forecast reset), the draw store is on; zeros while no truth is set.
 * Host fields only. */
int seir_sampler_verify_state(seir_sampler *s, int64_t out[4]);
/* Blocking read; any pointer may be NULL.  count [B] (the forecast's), lt, eq, abs_sum [B][M][H][2]. */
int seir_sampler_read_verify(seir_sampler *s, uint64_t *count, uint32_t *lt, uint32_t *eq, uint64_t *abs_sum);
/* D of planes 0 and 1 of the forecast's draw store over the filled positions, per chain (out [B][2][M][H]) or pooled over
 * the process's chains (out [1][2][M][H]), as seir_sampler_forecast_order_stats runs over them.  Blocking.  Needs the draw
 * store (seir_sampler_forecast_keep), not a truth.  SEIR_ERR_INVALID for more than SEIR_PAIR_ABS_MAX_N values per cell. */
int seir_sampler_forecast_pair_sums(seir_sampler *s, int32_t pooled, int64_t *out);
/* k_pair_abs alone, on host arrays, blocking: cells addressed as seir_order_stats addresses them (`segs` runs of seg_len
 * int32 values seg_stride apart, the cells cell_stride apart); out [cells].  Exact for every int32 input.  SEIR_ERR_INVALID
 * for a null pointer, cells, segs or seg_len below 1, a negative stride, overlapping segments, or n = segs x seg_len above
 * SEIR_PAIR_ABS_MAX_N.  *overflow is 1 if a launch met a cell above that all the same (nothing is written then), else 0. */
int seir_pair_abs_sums(seir_ctx *ctx, const int32_t *values, int64_t cells, int32_t segs, int64_t seg_len, int64_t seg_stride,
                       int64_t cell_stride, int64_t *out, uint32_t *overflow);

/* ------------------------------------------------------------------------
 * Reproduction number R_it.
 *
 * calc_posterior_rit (covid19uk/posterior/reproduction_number.py:13-44): for each
 * posterior draw and day, the column sums of next_generation_matrix_fn
 * (covid19uk/model_spec.py:302-368).  theta: n constrained draws [n][P] in the order of
 * inference.py:541-552; events: [n][M][T][3] fp64 counts (samples/seir); R_it: [n][T][M].
 * Host pointers, blocking; n is processed in batches of the context's max_chains.
 * ------------------------------------------------------------------------ */
int seir_reproduction_number(seir_ctx *ctx, int32_t n, const double *theta, const double *events, double *R_it);

/* Within- / between-location infection pressure (second half):
 * calc_pressure_components (covid19uk/posterior/within_between.py:13-57).  For each draw,
 * with I the infectives of the last state and x = I/N:
 *   within  = I - psi x W colsum(C),  between = psi W (C + C^T) x,
 * returned as fractions within/(within+between), between/(within+between), each [n][M].
 * psi [n]; I_last [n][M]; W: the commute volume the reference gathers (W[T-1]). Host pointers. */
int seir_within_between(seir_ctx *ctx, int32_t n, const double *psi, const double *I_last, double W,
                        double *within, double *between);

/* ------------------------------------------------------------------------
 * Chain-binomial forward simulation.
 *
 * Replaces `CovidUK(covar_data, initial_state=init_, initial_step, num_steps).sample(**par)["seir"]`
 * mapped over posterior draws in covid19uk/posterior/predict.py:50-70, i.e. gemlib's
 * DiscreteTimeStateTransitionModel.sample with the rates of covid19uk/model_spec.py:232-276:
 * day by day, y_x[m] ~ Binomial(source_x[m], 1 - exp(-rate_x[m] time_delta)).
 *
 * The caller resolves the model's time indexing on the host (model_spec.py:234-256: W, weekday
 * and b_t are gathered at clipped absolute day t = initial_step + s) and passes per-day arrays:
 *   par          [n][5]     psi, sigma_space, beta_area, gamma0, gamma1 (constrained)
 *   log_baseline [n][S]     a_t of every simulated day
 *   spatial      [n][M]     spatial_effect
 *   W, weekday_c [S]        commute volume and centred weekday of every simulated day
 *   init_state   [n][M][4]  S,E,I,R at the first simulated day (integer-valued)
 *   events       [n][M][S][3] out, fp64 counts in the reference's layout
 * Cstar, N, log-area, nu, time_delta and the rate floor come from the context; the context's T
 * does not limit S.  Random stream: Philox4x32-10 keyed by (seed; attempt, 64 + transition,
 * s*M + m, first_draw_id + draw) -- independent of batching and of the number of GPUs.
 * Host pointers, blocking.
 * ------------------------------------------------------------------------ */
typedef struct seir_sim_desc {
    int32_t num_draws;
    int32_t num_steps;
    int32_t first_draw_id;
    int32_t reserved;
    uint64_t seed;
    const double *par;
    const double *log_baseline;
    const double *spatial;
    const double *W;
    const double *weekday_c;
    const double *init_state;
    double *events;
} seir_sim_desc;

int seir_simulate(seir_ctx *ctx, const seir_sim_desc *sim);

/* One Binomial(n, p) variate per element with the simulator's sampler and stream
 * (cell = element index, transition 0, draw id 0): self-test hook for the distribution tests. */
int seir_selftest_binomial(seir_ctx *ctx, int32_t count, const int32_t *n, const double *p, uint64_t seed,
                           int32_t *out);

#ifdef __cplusplus
}
#endif
#endif /* SEIR_HIP_H */

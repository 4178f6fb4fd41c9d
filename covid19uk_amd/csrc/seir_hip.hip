// libseirhip.so -- C-ABI (include/seir_hip.h) over the gfx950 kernels.
// Host side of the drop-in boundary for joint_log_prob
// (covid19uk/inference/inference.py:537-557).  No CPU fallback anywhere in
// this file: every entry point needs a HIP device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/seir_hip.h"
#include "sampler_kernels.h"
#include "sim_kernels.h"
#include "moves_kernel.h"
#include "selftest_kernels.h"
#include "rt_kernels.h"
#include "sweep_plan.h"
#include "summary_kernels.h"
#include "forecast_kernels.h"
#include "check_kernels.h"
#include "rt_trace_kernels.h"
#include "wb_kernels.h"
#include "order_stats_kernels.h"
#include "rt_keep_kernels.h"
#include "group_kernels.h"

using namespace seir;

static_assert(plan::WAVE == WAVE && plan::CT_MAXC == CT_MAXC && plan::ROLE_SLOTS == ROLE_SLOTS && plan::MMAX == MMAX &&
              plan::MM_SMALL == MM_SMALL && MMAX == SEIR_MMAX,
              "sweep_plan.h reads the kernels' constants");

static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(SEIR_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                              \
    } while (0)

#include "dev_mem.h"

struct seir_ctx {
    Dims d{};
    Consts c{};
    Work w{};
    int Bmax = 0, device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<DevBuf> allocs;
    // staging for the host-pointer entry points
    double *u_stage = nullptr, *ev_stage = nullptr, *logp_stage = nullptr, *grad_stage = nullptr;
    // arguments of the last evaluation (seir_time_kernel replays them)
    const double *last_u = nullptr, *last_events = nullptr;
    double *last_logp = nullptr, *last_grad = nullptr;
    bool prepared = false;
    int opt_skew = 0, opt_affinity = 3;     // seir_set_option
    int opt_gemm_f32 = 0;
    int opt_rt_staging_kib = 0;       // bound on the S plane of a seir_sampler_rt batch in KiB (0: RT_STAGING_BYTES)
    int opt_generic_moves = 0;        // 1: the `_m4` event-update instances also where m <= MM_SMALL (move_mm)
    int opt_eval_form = 0;            // 0 auto (one launch where a chain's blocks share an XCD, else three), 1 four launches, 2 three
    int xcd_local = -1;               // -1 not probed yet; 1: blocks with the same id mod 8 share an XCD, eight different ones
    unsigned long long *eval_cnt = nullptr;   // [8][EVC_STRIDE] k_eval_all's counters
    int *eval_err = nullptr;          // k_eval_all: waits that timed out
    unsigned long long eval_a = 0, eval_b = 0;   // what a chain's counters A and B show after the launches so far
    int eval_nb = -1;                            // batch size of those launches (another size: counters and targets start over)
    int eval_slots[2][2] = {{-1, -1}, {-1, -1}};  // workgroups of k_eval_all<GRAD, TN> the chip holds at once (occupancy API; [TN == 96][GRAD])
    std::vector<float> cstar32_host;        // fp32 copy of the padded Cstar, uploaded when the option is first set
};

static inline int ceil_to(int x, int q) { return (x + q - 1) / q * q; }

// Trace slots per batch of a product: `base` of them, fewer where `per_slot` bytes of staging planes each would pass the staging
// bound (SEIR_OPT_RT_STAGING_KIB, else RT_STAGING_BYTES); at least one slot is always taken.
static int staging_slots(const seir_ctx *ctx, size_t base, size_t per_slot) {
    const size_t bound = ctx->opt_rt_staging_kib ? (size_t)ctx->opt_rt_staging_kib << 10 : RT_STAGING_BYTES;
    return (int)std::max<size_t>(1, std::min<size_t>(base, bound / per_slot));
}

// hipFuncSetAttribute applies to the current device's copy of a kernel: "done once" is kept per device (a bit per
// ordinal), not per process
static bool first_on_device(std::atomic<unsigned long long> &mask, int device) {
    const unsigned long long bit = 1ull << (device & 63);
    return (mask.fetch_or(bit) & bit) == 0ull;
}

template <typename T>
static int dev_alloc(seir_ctx *ctx, T **p, size_t count, bool zero = true) {
    DevBuf b;
    const size_t bytes = count * sizeof(T);
    if (int rc = zero ? b.zeroed(bytes ? bytes : sizeof(T)) : b.alloc(bytes ? bytes : sizeof(T))) return rc;
    *p = b.as<T>();
    ctx->allocs.push_back(std::move(b));
    return 0;
}

template <typename T>
static int dev_upload(seir_ctx *ctx, const T **p, const std::vector<T> &h) {
    T *q = nullptr;
    int rc = dev_alloc(ctx, &q, h.size(), false);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(q, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    *p = q;
    return 0;
}

extern "C" int seir_abi_version(void) { return SEIR_ABI_VERSION; }
extern "C" const char *seir_last_error(void) { return g_err; }

static void release_eval_all(seir_ctx *ctx);
extern "C" void seir_destroy(seir_ctx *ctx) {
    if (!ctx) return;
    release_eval_all(ctx);
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

static int create_impl(const seir_desc *ds, seir_ctx *ctx) {
    const int M = ds->M, T = ds->T, B = ds->max_chains;
    Dims &d = ctx->d;
    d.M = M; d.T = T;
    d.Mp = ceil_to(M, 64);
    d.Tp = ceil_to(T, 64);
    d.Kp = ceil_to(M, 4);
    d.Kp0 = d.Mp;
    d.P = 6 + (T - 1) + M;
    d.Pp = d.P;
    d.b0 = 0;
    d.nrb_scan = (M + SCAN_ROWS - 1) / SCAN_ROWS;
    d.nmt = d.Mp / SE_TM;
    d.ntc = d.Tp / 64;
    d.nu = ds->nu; d.dt = ds->time_delta; d.rate_floor = ds->rate_floor;
    d.car_half_logdet = ds->car_half_logdet;
    {   // constants of the prior log-densities, model_spec.py:140-198 (TFP formulas)
        const double L2PI = 1.8378770664093453;
        d.prior_const = (-std::log(10.0) - 0.5 * L2PI)                       // alpha_0
                        + (-0.5 * L2PI)                                        // beta_area
                        + (3.0 * std::log(10.0) - std::lgamma(3.0))            // psi
                        - (T - 1) * (std::log(0.005) + 0.5 * L2PI)             // alpha_t
                        + (0.5 * std::log(2.0 / M_PI) - std::log(0.1))         // sigma_space
                        + (ds->car_half_logdet - 0.5 * M * L2PI)               // spatial_effect
                        + 2.0 * (-std::log(100.0) - 0.5 * L2PI);               // gamma0, gamma1
    }
    d.L_ei = std::log(-std::expm1(-ds->nu * ds->time_delta));
    ctx->Bmax = B;
    ctx->device = ds->device;

    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ds->device < 0 || ds->device >= ndev)
        return fail(SEIR_ERR_DEVICE, "device %d not present (%d HIP devices visible)", ds->device, ndev);
    HIP_TRY(hipSetDevice(ds->device));
    HIP_TRY(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&ctx->ev0));
    HIP_TRY(hipEventCreate(&ctx->ev1));

    // log-factorial table
    double lf[LFACT_TABLE];
    for (int i = 0; i < LFACT_TABLE; ++i) lf[i] = std::lgamma((double)i + 1.0);
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_lfact), lf, sizeof(lf)));

    // padded constants
    std::vector<double> Cs((size_t)d.Mp * d.Kp0, 0.0), N(d.Mp, 1.0), invN(d.Mp, 0.0), la(d.Mp, 0.0),
        W(d.Tp, 0.0), wd(d.Tp, 0.0), init((size_t)d.Mp * 4, 0.0);
    for (int m = 0; m < M; ++m) {
        for (int j = 0; j < M; ++j) Cs[(size_t)m * d.Kp0 + j] = ds->Cstar[(size_t)m * M + j];
        if (!(ds->N[m] > 0.0)) return fail(SEIR_ERR_INVALID, "N[%d] must be positive", m);
        N[m] = ds->N[m];
        invN[m] = 1.0 / ds->N[m];
        la[m] = ds->log_area_c[m];
        for (int s = 0; s < 4; ++s) init[(size_t)m * 4 + s] = ds->init_state[(size_t)m * 4 + s];
    }
    for (int m = 0; m < M; ++m)          // C + C^T with a diagonal is symmetric (model_spec.py:216-219); k_gemm relies on it
        for (int j = 0; j < m; ++j)
            if (ds->Cstar[(size_t)m * M + j] != ds->Cstar[(size_t)j * M + m])
                return fail(SEIR_ERR_INVALID, "Cstar must be symmetric (entry %d,%d)", m, j);
    for (int t = 0; t < T; ++t) { W[t] = ds->W[t]; wd[t] = ds->weekday_c[t]; }
    std::vector<int> qrow(M + 1, 0), qcol;
    std::vector<double> qval;
    for (int m = 0; m < M; ++m) {
        for (int j = 0; j < M; ++j) {
            const double v = ds->car_Q[(size_t)m * M + j];
            if (v != 0.0) { qcol.push_back(j); qval.push_back(v); }
        }
        qrow[m + 1] = (int)qcol.size();
    }
    if (qcol.empty()) { qcol.push_back(0); qval.push_back(0.0); }
    // table of device_math.h fast_log: c_i = 1 + (i + 1/2)/128, (fl(1/c_i), -log(fl(1/c_i)))
    std::vector<double2> ltab(LDSTAB_N);
    for (int i = 0; i < LFACT_TABLE / 2; ++i) {
        ltab[LOGTAB_N + i].x = lf[2 * i];
        ltab[LOGTAB_N + i].y = lf[2 * i + 1];
    }
    for (int i = 0; i < LOGTAB_N; ++i) {
        const long double cc = 1.0L + ((long double)i + 0.5L) / (long double)LOGTAB_N;
        const double invc = (double)(1.0L / cc);
        ltab[i].x = invc;
        ltab[i].y = (double)(-logl((long double)invc));
    }
    int rc;
    if ((rc = dev_upload(ctx, &ctx->c.logtab, ltab))) return rc;
    {
        std::vector<double> lfb(SCAN_LFT);
        for (int i = 0; i < SCAN_LFT; ++i) lfb[i] = std::lgamma((double)i + 1.0);
        if ((rc = dev_upload(ctx, &ctx->c.lfact_big, lfb))) return rc;
    }
    {   // ELL copy of car_Q (adjacency rows are short): [k][m] so that a wave reads coalesced
        int qw = 0;
        for (int m = 0; m < M; ++m) qw = std::max(qw, qrow[m + 1] - qrow[m]);
        if (qw <= 32) {
            std::vector<int> ec((size_t)std::max(qw, 1) * d.Mp, 0);
            std::vector<double> ev((size_t)std::max(qw, 1) * d.Mp, 0.0);
            for (int m = 0; m < M; ++m)
                for (int e = qrow[m], k = 0; e < qrow[m + 1]; ++e, ++k) {
                    ec[(size_t)k * d.Mp + m] = qcol[e];
                    ev[(size_t)k * d.Mp + m] = qval[e];
                }
            ctx->c.qw = qw;
            if ((rc = dev_upload(ctx, &ctx->c.Qell_col, ec))) return rc;
            if ((rc = dev_upload(ctx, &ctx->c.Qell_val, ev))) return rc;
        } else {
            ctx->c.qw = 0;
        }
    }
    if ((rc = dev_upload(ctx, &ctx->c.Cstar, Cs))) return rc;
    ctx->cstar32_host.assign(Cs.begin(), Cs.end());             // rounded to fp32; goes to the device only if asked for
    if ((rc = dev_upload(ctx, &ctx->c.N, N))) return rc;
    if ((rc = dev_upload(ctx, &ctx->c.invN, invN))) return rc;
    if ((rc = dev_upload(ctx, &ctx->c.la, la))) return rc;
    if ((rc = dev_upload(ctx, &ctx->c.W, W))) return rc;
    if ((rc = dev_upload(ctx, &ctx->c.wd, wd))) return rc;
    if ((rc = dev_upload(ctx, &ctx->c.init, init))) return rc;
    if ((rc = dev_upload(ctx, &ctx->c.Qrow, qrow))) return rc;
    if ((rc = dev_upload(ctx, &ctx->c.Qcol, qcol))) return rc;
    if ((rc = dev_upload(ctx, &ctx->c.Qval, qval))) return rc;

    Work &w = ctx->w;
    const size_t cells = (size_t)B * d.Mp * d.Tp;
    if ((rc = dev_alloc(ctx, &w.Xn, cells))) return rc;
    if ((rc = dev_alloc(ctx, &w.F, cells))) return rc;
    if ((rc = dev_alloc(ctx, &w.KS, cells))) return rc;
    if ((rc = dev_alloc(ctx, &w.rowconst, (size_t)B * d.Mp))) return rc;
    if ((rc = dev_alloc(ctx, &w.colIR, (size_t)B * d.nrb_scan * d.Tp * 2))) return rc;
    if ((rc = dev_alloc(ctx, &w.ea, (size_t)B * d.Tp))) return rc;
    if ((rc = dev_alloc(ctx, &w.eb, (size_t)B * d.Mp))) return rc;
    if ((rc = dev_alloc(ctx, &w.rir, (size_t)B * d.Tp))) return rc;
    if ((rc = dev_alloc(ctx, &w.scal, (size_t)B * NSCAL))) return rc;
    if ((rc = dev_alloc(ctx, &w.Qs, (size_t)B * d.Mp))) return rc;
    if ((rc = dev_alloc(ctx, &w.Kir, (size_t)B * d.Tp))) return rc;
    if ((rc = dev_alloc(ctx, &w.Dir, (size_t)B * d.Tp))) return rc;
    if ((rc = dev_alloc(ctx, &w.constsum, (size_t)B))) return rc;
    if ((rc = dev_alloc(ctx, &w.Lpart, (size_t)B * d.nmt * d.ntc))) return rc;
    if ((rc = dev_alloc(ctx, &w.Ppart, (size_t)B * d.nmt * d.ntc))) return rc;
    if ((rc = dev_alloc(ctx, &w.Kpart, (size_t)B * d.nmt * d.Tp))) return rc;
    if ((rc = dev_alloc(ctx, &w.Rpart, (size_t)B * d.ntc * d.Mp))) return rc;

    if ((rc = dev_alloc(ctx, &ctx->u_stage, (size_t)B * d.P))) return rc;
    if ((rc = dev_alloc(ctx, &ctx->ev_stage, (size_t)B * M * T * 3))) return rc;
    if ((rc = dev_alloc(ctx, &ctx->logp_stage, (size_t)B))) return rc;
    if ((rc = dev_alloc(ctx, &ctx->grad_stage, (size_t)B * d.P))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}

// SEIR_MAX_T is the largest T whose state scan (k_scan, k_scan_params: the tightest launch of a context) fits the 160 KiB
// of a workgroup; k_state_params and k_eval_all hold the same columns without the log-factorial table
static_assert(SEIR_MAX_T % 64 == 0 && scan_lds_bytes(SEIR_MAX_T) + SCAN_STATIC_LDS <= 160 * 1024 &&
              scan_lds_bytes(SEIR_MAX_T + 64) + SCAN_STATIC_LDS > 160 * 1024,
              "SEIR_MAX_T must be the longest series whose state scan fits the LDS of a workgroup");

extern "C" int seir_create(const seir_desc *ds, seir_ctx **out) {
    if (!ds || !out) return fail(SEIR_ERR_INVALID, "null argument");
    *out = nullptr;
    if (ds->M < 1 || ds->T < 1 || ds->max_chains < 1)
        return fail(SEIR_ERR_INVALID, "M, T and max_chains must be >= 1 (got %d, %d, %d)", ds->M, ds->T,
                    ds->max_chains);
    if (ds->M > SEIR_MAX_M || ds->T > SEIR_MAX_T)
        return fail(SEIR_ERR_INVALID, "M=%d, T=%d exceed the supported M <= %d, T <= %d (the state scan's LDS)", ds->M, ds->T,
                    SEIR_MAX_M, SEIR_MAX_T);
    if (!ds->Cstar || !ds->N || !ds->W || !ds->weekday_c || !ds->log_area_c || !ds->car_Q || !ds->init_state)
        return fail(SEIR_ERR_INVALID, "null covariate pointer");
    if (!(ds->time_delta > 0.0) || !(ds->nu > 0.0))
        return fail(SEIR_ERR_INVALID, "nu and time_delta must be positive");
    seir_ctx *ctx = new (std::nothrow) seir_ctx();
    if (!ctx) return fail(SEIR_ERR_DEVICE, "out of host memory");
    int rc = create_impl(ds, ctx);
    if (rc) { seir_destroy(ctx); return rc; }
    *out = ctx;
    return 0;
}

extern "C" int seir_num_params(const seir_ctx *ctx) { return ctx ? ctx->d.P : SEIR_ERR_INVALID; }

extern "C" int seir_set_initial_state(seir_ctx *ctx, const double *init_state) {
    if (!ctx || !init_state) return fail(SEIR_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    const int M = ctx->d.M;
    for (int i = 0; i < 4 * M; ++i)
        if (!(init_state[i] >= 0.0) || init_state[i] != std::floor(init_state[i]))
            return fail(SEIR_ERR_INVALID, "init_state[%d]=%g is not a non-negative integer count", i, init_state[i]);
    // the padded rows [M, Mp) stay zero; blocking copy: the caller's buffer is not retained
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(const_cast<double *>(ctx->c.init), init_state, sizeof(double) * 4 * M, hipMemcpyHostToDevice));
    ctx->prepared = false;
    return 0;
}

static int check_batch(seir_ctx *ctx, int B) {
    if (!ctx) return fail(SEIR_ERR_INVALID, "null context");
    if (B < 1 || B > ctx->Bmax) return fail(SEIR_ERR_INVALID, "B=%d outside [1, max_chains=%d]", B, ctx->Bmax);
    HIP_TRY(hipSetDevice(ctx->device));
    return 0;
}

// --- individual launches ---------------------------------------------------
// `d.b0` selects the first chain, `nb` the number of chains, `st` the stream.
// `affinity`: give every block of a chain the same (block id % 8), see xcd_affine()
struct LaunchCfg { Dims d; hipStream_t st; int nb; int affinity; };
// affinity: bit 0 = gradient kernel, bit 1 = event-move kernels (seir_set_option, default 3)
static LaunchCfg whole(seir_ctx *ctx, int B) {
    LaunchCfg l{ctx->d, ctx->stream, B, ctx->opt_affinity};
    l.d.skew = ctx->opt_skew;                           // test hook, see debug_skew()
    return l;
}

extern "C" int seir_set_option(seir_ctx *ctx, int32_t option, int32_t value) {
    if (!ctx) return fail(SEIR_ERR_INVALID, "null context");
    switch (option) {
        case SEIR_OPT_DEBUG_SKEW:
            if (value < 0 || value > 3) return fail(SEIR_ERR_INVALID, "debug skew must be 0..3");
            ctx->opt_skew = value;
            return 0;
        case SEIR_OPT_XCD_AFFINITY:
            if (value < 0 || value > 3) return fail(SEIR_ERR_INVALID, "xcd affinity is a 2-bit mask");
            ctx->opt_affinity = value;
            return 0;
        case SEIR_OPT_EVAL_FORM:
            if (value < 0 || value > 2) return fail(SEIR_ERR_INVALID, "eval form is 0 (auto), 1 (four launches) or 2 (three launches)");
            ctx->opt_eval_form = value;
            return 0;
        case SEIR_OPT_GENERIC_MOVES:
            if (value < 0 || value > 1) return fail(SEIR_ERR_INVALID, "generic_moves is 0 or 1");
            ctx->opt_generic_moves = value;
            return 0;
        case SEIR_OPT_RT_STAGING_KIB:
            if (value < 0) return fail(SEIR_ERR_INVALID, "the staging bound is a number of KiB (0: the default)");
            ctx->opt_rt_staging_kib = value;
            return 0;
        case SEIR_OPT_GEMM_F32: {
            if (value < 0 || value > 1) return fail(SEIR_ERR_INVALID, "gemm_f32 is 0 or 1");
            if (value && !ctx->c.Cstar32) {
                HIP_TRY(hipSetDevice(ctx->device));
                int rc = dev_upload(ctx, &ctx->c.Cstar32, ctx->cstar32_host);
                if (rc) return rc;
                if ((rc = dev_alloc(ctx, &ctx->w.Xn32, (size_t)ctx->Bmax * ctx->d.Mp * ctx->d.Tp))) return rc;
            }
            if (value && (ctx->d.Mp % GF_T != 0 || ctx->d.Tp % GF_T != 0))
                return fail(SEIR_ERR_INVALID, "the fp32 contraction needs ceil64(M) and ceil64(T) to be multiples of %d (M=%d, T=%d)",
                            GF_T, ctx->d.M, ctx->d.T);
            ctx->opt_gemm_f32 = value;
            ctx->prepared = false;
            return 0;
        }
        default:
            return fail(SEIR_ERR_INVALID, "unknown option %d", option);
    }
}

template <int SRC>
static void launch_scan(seir_ctx *ctx, const LaunchCfg &l, const double *events) {
    const Dims &d = l.d;
    const size_t lds = scan_lds_bytes(d.Tp);
    (void)lds_attribute((const void *)k_scan<SRC>, lds);
    hipLaunchKernelGGL(k_scan<SRC>, dim3(d.nrb_scan, l.nb), dim3(SCAN_WAVES * WAVE), lds,
                       l.st, d, ctx->c, ctx->w, events);
}
static void launch_colreduce(seir_ctx *ctx, const LaunchCfg &l) {
    hipLaunchKernelGGL(k_colreduce, dim3(l.d.Tp / WAVE, l.nb), dim3(256), 0, l.st, l.d, ctx->w);
}
template <int TN>
static void launch_gemm_t(seir_ctx *ctx, const LaunchCfg &l) {
    const Dims &d = l.d;
    const size_t lds = gemm_lds_bytes<TN>();
    static std::atomic<unsigned long long> attr_set{0ull};
    if (lds > 64 * 1024 && first_on_device(attr_set, ctx->device))
        (void)lds_attribute((const void *)k_gemm<TN>, lds);
    hipLaunchKernelGGL((k_gemm<TN>), dim3(d.Tp / TN, d.Mp / GEMM_TM, l.nb), dim3(gemm_threads<TN>()), lds, l.st, d, ctx->c,
                       ctx->w);
}
#ifndef GEMM_NCG
#define GEMM_NCG 3
#endif
static void launch_gemm(seir_ctx *ctx, const LaunchCfg &l) {
    if (ctx->opt_gemm_f32 && ctx->c.Cstar32 && ctx->w.Xn32 && l.d.Mp % GF_T == 0 && l.d.Tp % GF_T == 0) {
        hipLaunchKernelGGL(k_gemm_f32, dim3(l.d.Tp / GF_T, l.d.Mp / GF_T, l.nb), dim3(256), 0, l.st, l.d, ctx->c, ctx->w);
        return;
    }
    // 64 x 96 tiles only where they turn two rounds of workgroups into one (UK-380, 8 chains: 288 -> 192 on
    // 256 CUs, 34.6 -> 32.9 us); on large grids the 6-wave tile loses to the 4-wave one (SYN-2048: 38.6 vs 51.7 TF)
    const Dims &d = l.d;
    const long t64 = (long)(d.Tp / 64) * (d.Mp / GEMM_TM) * l.nb, t96 = (long)(d.Tp / 96) * (d.Mp / GEMM_TM) * l.nb;
    if (d.Tp % 96 == 0 && t64 > 256 && t96 <= 256) {
        // the eight-wave form of the 64 x 96 tile: every SIMD of a CU carries two waves (k_gemm<96>'s six waves: 2,2,1,1)
        const size_t lds = gemm_lds_bytes<96>();
        static std::atomic<unsigned long long> attr_set{0ull};
        if (lds > 64 * 1024 && first_on_device(attr_set, ctx->device))
            (void)lds_attribute((const void *)k_gemm_w8<GEMM_NCG>, lds);
        hipLaunchKernelGGL(k_gemm_w8<GEMM_NCG>, dim3(d.Tp / 96, d.Mp / GEMM_TM, l.nb), dim3(256 * GEMM_NCG), lds, l.st, d, ctx->c, ctx->w);
    } else {
        launch_gemm_t<64>(ctx, l);
    }
}
static void launch_params(seir_ctx *ctx, const LaunchCfg &l, const double *u) {
    hipLaunchKernelGGL(k_params, dim3(l.nb), dim3(256), 0, l.st, l.d, ctx->c, ctx->w, u);
}
template <int SRC>
static void launch_se(seir_ctx *ctx, const LaunchCfg &l, bool grad) {
    Dims d = l.d;
    const bool affinity = (l.affinity & 1) && xcd_affinity_applies(d.ntc * d.nmt, l.nb);
    d.aff_nb = affinity ? l.nb : 0;
    const dim3 grid = affinity ? dim3(d.ntc * d.nmt * l.nb) : dim3(d.ntc, d.nmt, l.nb);
    if (grad && SRC == 1 && d.chunked == 1)
        hipLaunchKernelGGL((k_se<true, SRC, 1>), grid, dim3(256), 0, l.st, d, ctx->c, ctx->w);
    else if (grad && SRC == 1 && d.chunked == 2)
        hipLaunchKernelGGL((k_se<true, SRC, 2>), grid, dim3(256), 0, l.st, d, ctx->c, ctx->w);
    else if (grad)
        hipLaunchKernelGGL((k_se<true, SRC>), grid, dim3(256), 0, l.st, d, ctx->c, ctx->w);
    else
        hipLaunchKernelGGL((k_se<false, SRC>), grid, dim3(256), 0, l.st, d, ctx->c, ctx->w);
}
static void launch_finish(seir_ctx *ctx, const LaunchCfg &l, const double *u, double *logp, double *grad) {
    const size_t lds = (size_t)l.d.Tp * sizeof(double);
    if (grad)
        hipLaunchKernelGGL(k_finish<true>, dim3(l.nb), dim3(256), lds, l.st, l.d, ctx->c, ctx->w, u, logp, grad, 0);
    else
        hipLaunchKernelGGL(k_finish<false>, dim3(l.nb), dim3(256), lds, l.st, l.d, ctx->c, ctx->w, u, logp, grad, 0);
}

extern "C" int seir_prepare_events_dev(seir_ctx *ctx, int32_t B, const double *events_dev) {
    int rc = check_batch(ctx, B);
    if (rc) return rc;
    if (!events_dev) return fail(SEIR_ERR_INVALID, "null events pointer");
    launch_scan<0>(ctx, whole(ctx, B), events_dev);
    launch_colreduce(ctx, whole(ctx, B));
    launch_gemm(ctx, whole(ctx, B));
    HIP_TRY(hipGetLastError());
    ctx->last_events = events_dev;
    ctx->prepared = true;
    return 0;
}

extern "C" int seir_eval_prepared_dev(seir_ctx *ctx, int32_t B, const double *u_dev, double *logp_dev,
                                      double *grad_dev) {
    int rc = check_batch(ctx, B);
    if (rc) return rc;
    if (!ctx->prepared) return fail(SEIR_ERR_STATE, "seir_prepare_events_dev has not been called");
    if (!u_dev || !logp_dev) return fail(SEIR_ERR_INVALID, "null u/logp pointer");
    launch_params(ctx, whole(ctx, B), u_dev);
    launch_se<0>(ctx, whole(ctx, B), grad_dev != nullptr);
    launch_finish(ctx, whole(ctx, B), u_dev, logp_dev, grad_dev);
    HIP_TRY(hipGetLastError());
    ctx->last_u = u_dev; ctx->last_logp = logp_dev; ctx->last_grad = grad_dev;
    return 0;
}

// The fused form of the full evaluation (default): [state part of the scan | parameter tables],
// [contraction tiles with the S->E term as epilogue | row constants | fold of the I->R partials], reduction.
static void launch_state_params(seir_ctx *ctx, const LaunchCfg &l, const double *u_dev, const double *events_dev) {
    const Dims &d = l.d;
    const size_t lds_a = (size_t)SCAN_WAVES * d.Tp * 2 * sizeof(double);
    static std::atomic<unsigned long long> attr_a{0ull};
    if (lds_a > 64 * 1024 && first_on_device(attr_a, ctx->device))
        (void)lds_attribute((const void *)k_state_params, lds_a);
    hipLaunchKernelGGL(k_state_params, dim3(d.nrb_scan + 1, l.nb), dim3(SCAN_WAVES * WAVE), lds_a, l.st, d, ctx->c, ctx->w,
                       events_dev, u_dev);
}
// the Dims of the tile launch and of the reduction after it: partial sums per 64 x TN tile
template <int TN>
static Dims fused_dims(const LaunchCfg &l) {
    Dims d = l.d;
    d.nmt = d.Mp / GEMM_TM;
    d.ntc = d.Tp / TN;
    return d;
}
// Do blocks with the same id mod 8 share an XCD on this GPU, eight different ones for the eight classes?  (XCC_ID of a
// probe grid; the XCD-local hand-offs inside a launch -- k_eval_all here, k_se_chunk and the band workgroups of
// k_move_pair in the sampler -- are used only then.)
static bool probe_xcd_local(hipStream_t st) {
    const int nblk = 8 * 144;
    DevBuf xcc;
    std::vector<unsigned> host(nblk, 99u);
    if (xcc.alloc(nblk * sizeof(unsigned))) return false;
    hipLaunchKernelGGL(k_xcc_probe, dim3(nblk), dim3(256), 0, st, xcc.as<unsigned>());
    hipError_t e = hipMemcpyAsync(host.data(), xcc.p, nblk * sizeof(unsigned), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    bool ok = e == hipSuccess;
    for (int L = 8; L < nblk && ok; ++L) ok = host[L] == host[L & 7] && host[L] < 16u;
    for (int a = 0; a < 8 && ok; ++a)
        for (int b2 = a + 1; b2 < 8; ++b2) ok = ok && host[a] != host[b2];
    return ok;
}

// which context may use the one-launch evaluation on each device (see seir_log_prob_dev)
static std::atomic<seir_ctx *> g_eval_all_owner[64];
static bool claim_eval_all(seir_ctx *ctx) {
    std::atomic<seir_ctx *> &slot = g_eval_all_owner[ctx->device & 63];
    seir_ctx *cur = slot.load();
    if (cur == ctx) return true;
    if (cur != nullptr) return false;
    return slot.compare_exchange_strong(cur, ctx) || cur == ctx;
}
static void release_eval_all(seir_ctx *ctx) {
    seir_ctx *me = ctx;
    (void)g_eval_all_owner[ctx->device & 63].compare_exchange_strong(me, nullptr);
}

template <int TN>
static void launch_finish_fused(seir_ctx *ctx, const LaunchCfg &l, const double *u_dev, double *logp_dev, double *grad_dev);
// The whole evaluation in one launch (k_eval_all): 8 chains, XCD-affine block ids, the GPU's XCD placement checked.
template <int TN>
static int launch_eval_all(seir_ctx *ctx, const LaunchCfg &l, const double *u_dev, const double *events_dev,
                           double *logp_dev, double *grad_dev) {
    const int nbv = (l.nb + 7) / 8 * 8;
    if (!ctx->eval_cnt) {
        int rc = dev_alloc(ctx, &ctx->eval_cnt, (size_t)((ctx->Bmax + 7) / 8 * 8) * EVC_STRIDE + 16);
        if (!rc) rc = dev_alloc(ctx, &ctx->eval_err, 1);
        if (rc) return rc;
    }
    Dims d = fused_dims<TN>(l);
    d.aff_nb = nbv;
    d.nlive = nbv != l.nb ? l.nb : 0;
    const int per = d.ntc * d.nmt, ncb = d.Tp / WAVE;
    if (ctx->eval_nb != l.nb) {
        // the counters are per chain and the targets one running total per context: a batch of another size leaves the
        // chains that sat out behind the target (they would wait for the time-out and go on without their producers'
        // data) -- start all of them from zero again, in stream order
        if (hipMemsetAsync(ctx->eval_cnt, 0, sizeof(unsigned long long) * ((size_t)((ctx->Bmax + 7) / 8 * 8) * EVC_STRIDE + 16),
                           l.st) != hipSuccess)
            return fail(SEIR_ERR_DEVICE, "resetting the evaluation hand-off counters failed");
        ctx->eval_a = ctx->eval_b = 0;
        ctx->eval_nb = l.nb;
    }
    ctx->eval_a += (unsigned long long)(per + 1);                       // per chain: the tiles' state parts + the parameter block
    ctx->eval_b += (unsigned long long)(per + d.nrb_scan + ncb);        //            tiles + row-constant blocks + I->R fold blocks
    const size_t lds = eval_all_lds_bytes<TN>(d);
    static std::atomic<unsigned long long> attr{0ull};
    if (lds > 64 * 1024 && first_on_device(attr, ctx->device)) {
        (void)lds_attribute((const void *)k_eval_all<true, TN>, lds);
        (void)lds_attribute((const void *)k_eval_all<false, TN>, lds);
    }
    const dim3 grid((unsigned)((1 + per + d.nrb_scan + ncb + 1) * nbv));
    // the reduction block runs inside the launch for value-only calls; with the gradient it is its own launch (measured:
    // the gradient assembly takes 12.7 us as the last block of this large kernel against 4.8 us in k_finish -- 59.2 us
    // per batch against 56.9)
#ifndef EVAL_FIN_GRAD
#define EVAL_FIN_GRAD 0
#endif
    const int fin = grad_dev ? EVAL_FIN_GRAD : 1;
    if (grad_dev)
        hipLaunchKernelGGL((k_eval_all<true, TN>), grid, dim3(512), lds, l.st, d, ctx->c, ctx->w, events_dev, u_dev, logp_dev,
                           grad_dev, ctx->eval_cnt, ctx->eval_a, ctx->eval_b, ctx->eval_err, fin);
    else
        hipLaunchKernelGGL((k_eval_all<false, TN>), grid, dim3(512), lds, l.st, d, ctx->c, ctx->w, events_dev, u_dev, logp_dev,
                           grad_dev, ctx->eval_cnt, ctx->eval_a, ctx->eval_b, ctx->eval_err, fin);
    if (!fin) launch_finish_fused<TN>(ctx, l, u_dev, logp_dev, grad_dev);
    return 0;
}

template <int TN>
static void launch_eval_tiles(seir_ctx *ctx, const LaunchCfg &l, const double *events_dev, bool grad) {
    Dims d = fused_dims<TN>(l);
    const int B = l.nb;
    const bool affinity = (l.affinity & 1) && xcd_affinity_applies(d.ntc * d.nmt, B);
    d.aff_nb = affinity ? B : 0;
    const size_t lds_b = eval_tiles_lds_bytes<TN>();
    static std::atomic<unsigned long long> attr_b{0ull};
    if (lds_b > 64 * 1024 && first_on_device(attr_b, ctx->device)) {
        (void)lds_attribute((const void *)k_eval_tiles<true, TN>, lds_b);
        (void)lds_attribute((const void *)k_eval_tiles<false, TN>, lds_b);
    }
    const dim3 grid((unsigned)((d.ntc * d.nmt + d.nrb_scan + d.Tp / WAVE) * B));
    if (grad) hipLaunchKernelGGL((k_eval_tiles<true, TN>), grid, dim3(512), lds_b, l.st, d, ctx->c, ctx->w, events_dev, B);
    else hipLaunchKernelGGL((k_eval_tiles<false, TN>), grid, dim3(512), lds_b, l.st, d, ctx->c, ctx->w, events_dev, B);
}
template <int TN>
static void launch_finish_fused(seir_ctx *ctx, const LaunchCfg &l, const double *u_dev, double *logp_dev, double *grad_dev) {
    const Dims d = fused_dims<TN>(l);
    const size_t lds_f = (size_t)d.Tp * sizeof(double);
    if (grad_dev) hipLaunchKernelGGL(k_finish<true>, dim3(l.nb), dim3(256), lds_f, l.st, d, ctx->c, ctx->w, u_dev, logp_dev, grad_dev, 1);
    else hipLaunchKernelGGL(k_finish<false>, dim3(l.nb), dim3(256), lds_f, l.st, d, ctx->c, ctx->w, u_dev, logp_dev, grad_dev, 1);
}
template <int TN>
static void launch_eval_fused(seir_ctx *ctx, const LaunchCfg &l, const double *u_dev, const double *events_dev,
                              double *logp_dev, double *grad_dev) {
    launch_state_params(ctx, l, u_dev, events_dev);
    launch_eval_tiles<TN>(ctx, l, events_dev, grad_dev != nullptr);
    launch_finish_fused<TN>(ctx, l, u_dev, logp_dev, grad_dev);
}

// The full evaluation.  Default: the fused form above.  SEIR_OPT_EVAL_FORM = 1 (and the fp32 contraction option)
// select the four-launch form: [state scan | parameter tables], mobility contraction,
// [S->E tiles | fold of the scan's I->R partials], reduction -- the tables depend on u only and the fold
// feeds the last launch only, so each rides along with the wide kernel next to it.
extern "C" int seir_log_prob_dev(seir_ctx *ctx, int32_t B, const double *u_dev, const double *events_dev,
                                 double *logp_dev, double *grad_dev) {
    int rc = check_batch(ctx, B);
    if (rc) return rc;
    if (!events_dev || !u_dev || !logp_dev) return fail(SEIR_ERR_INVALID, "null u/events/logp pointer");
    const LaunchCfg l = whole(ctx, B);
    Dims d = l.d;
    const bool f32 = ctx->opt_gemm_f32 && ctx->c.Cstar32 && ctx->w.Xn32;
    if (ctx->opt_eval_form != 1 && !f32) {
        bool one = false;
        if (ctx->opt_eval_form == 0 && B % 8 == 0 && (l.affinity & 1)) {
            // one launch for multiples of 8 chains (a single chain confined to one XCD loses more than the launches cost:
            // 46 / 54 us against 38 / 45, level at 4; 12 chains in the layout of 16 cost nearly what 16 do) while the parameter blocks and every tile workgroup
            // fit the chip at once (two workgroups of k_eval_all per CU: 128 VGPRs x 8 waves, <= 54 KB of LDS): UK-380
            // up to 16 chains (83 / 92 us against 87 / 93 in three launches)
            const int tn = d.Tp % 96 == 0 ? 96 : 64;
            const int per1 = (d.Tp / tn) * (d.Mp / GEMM_TM);
            const int nbv = (B + 7) / 8 * 8;
            // what the chip holds of this kernel at once: asked of the occupancy API with the launch's real dynamic LDS
            // (cached per instance), not assumed
            const int gi = grad_dev ? 1 : 0, ti = tn == 96 ? 1 : 0;
            if (ctx->eval_slots[ti][gi] < 0) {
                int occ = 0, cus = 0;
                const void *fn = tn == 96 ? (grad_dev ? (const void *)k_eval_all<true, 96> : (const void *)k_eval_all<false, 96>)
                                          : (grad_dev ? (const void *)k_eval_all<true, 64> : (const void *)k_eval_all<false, 64>);
                Dims dq = d;
                dq.nmt = d.Mp / GEMM_TM; dq.ntc = d.Tp / tn;
                const size_t lds = tn == 96 ? eval_all_lds_bytes<96>(dq) : eval_all_lds_bytes<64>(dq);
                (void)lds_attribute(fn, lds);
                if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, 512, lds) != hipSuccess) occ = 0;
                (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
                ctx->eval_slots[ti][gi] = occ * cus;
            }
            // ... and ONE context per device: the launch's tiles wait, holding their CUs, for workgroups of the same launch; two
            // such launches from two contexts' streams can each be placed in part and wait for the other's CUs (three
            // contexts used in turn: 45 - 152 us per launch, sigma 32 us, profiles/r03_bench_kernel_stats.csv).  The
            // first context to get here owns the one-launch form on its device until it is destroyed; the others run the
            // three launches, which wait for nothing and overlap freely.
            if ((1 + per1) * nbv <= ctx->eval_slots[ti][gi] && claim_eval_all(ctx)) {
                if (ctx->xcd_local < 0) ctx->xcd_local = probe_xcd_local(ctx->stream) ? 1 : 0;
                one = ctx->xcd_local == 1;
            }
        }
        if (one) {
            rc = d.Tp % 96 == 0 ? launch_eval_all<96>(ctx, l, u_dev, events_dev, logp_dev, grad_dev)
                                : launch_eval_all<64>(ctx, l, u_dev, events_dev, logp_dev, grad_dev);
            if (rc) return rc;
        } else if (d.Tp % 96 == 0) {
            launch_eval_fused<96>(ctx, l, u_dev, events_dev, logp_dev, grad_dev);
        } else {
            launch_eval_fused<64>(ctx, l, u_dev, events_dev, logp_dev, grad_dev);
        }
    } else {
        const size_t lds = scan_lds_bytes(d.Tp);
        (void)lds_attribute((const void *)k_scan_params, lds);
        hipLaunchKernelGGL(k_scan_params, dim3(d.nrb_scan + 1, B), dim3(SCAN_WAVES * WAVE), lds, l.st, d, ctx->c, ctx->w,
                           events_dev, u_dev);
        launch_gemm(ctx, l);
        const bool affinity = (l.affinity & 1) && xcd_affinity_applies(d.ntc * d.nmt, B) && (d.ntc * B) % 8 == 0;
        d.aff_nb = affinity ? B : 0;
        const dim3 grid((unsigned)(d.ntc * d.nmt * B + d.ntc * B));
        if (grad_dev) hipLaunchKernelGGL(k_se_colreduce<true>, grid, dim3(256), 0, l.st, d, ctx->c, ctx->w, B);
        else hipLaunchKernelGGL(k_se_colreduce<false>, grid, dim3(256), 0, l.st, d, ctx->c, ctx->w, B);
        launch_finish(ctx, l, u_dev, logp_dev, grad_dev);
    }
    HIP_TRY(hipGetLastError());
    ctx->last_events = events_dev;
    ctx->prepared = true;
    ctx->last_u = u_dev; ctx->last_logp = logp_dev; ctx->last_grad = grad_dev;
    return 0;
}

static int check_eval_handoffs(seir_ctx *ctx);
static int host_eval(seir_ctx *ctx, int B, const double *u, const double *events, double *logp, double *grad) {
    int rc = check_batch(ctx, B);
    if (rc) return rc;
    if (!u || !events || !logp) return fail(SEIR_ERR_INVALID, "null host pointer");
    const Dims &d = ctx->d;
    HIP_TRY(hipMemcpyAsync(ctx->u_stage, u, sizeof(double) * B * d.P, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->ev_stage, events, sizeof(double) * B * d.M * d.T * 3, hipMemcpyHostToDevice,
                           ctx->stream));
    rc = seir_log_prob_dev(ctx, B, ctx->u_stage, ctx->ev_stage, ctx->logp_stage, grad ? ctx->grad_stage : nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(logp, ctx->logp_stage, sizeof(double) * B, hipMemcpyDeviceToHost, ctx->stream));
    if (grad)
        HIP_TRY(hipMemcpyAsync(grad, ctx->grad_stage, sizeof(double) * B * d.P, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return check_eval_handoffs(ctx);
}

extern "C" int seir_log_prob(seir_ctx *ctx, int32_t B, const double *u, const double *events, double *logp) {
    return host_eval(ctx, B, u, events, logp, nullptr);
}

extern "C" int seir_log_prob_grad(seir_ctx *ctx, int32_t B, const double *u, const double *events, double *logp,
                                  double *grad) {
    if (!grad) return fail(SEIR_ERR_INVALID, "null grad pointer");
    return host_eval(ctx, B, u, events, logp, grad);
}

// k_eval_all's bounded waits: a time-out means a consumer block went on without its producers' data
static int check_eval_handoffs(seir_ctx *ctx) {
    if (!ctx->eval_err) return 0;
    int n = 0;
    HIP_TRY(hipMemcpy(&n, ctx->eval_err, sizeof(int), hipMemcpyDeviceToHost));
    if (n) {
        (void)hipMemset(ctx->eval_err, 0, sizeof(int));
        return fail(SEIR_ERR_HANDOFF, "%d in-launch hand-off(s) of the one-launch evaluation timed out: results since the last "
                    "synchronisation are unreliable (SEIR_OPT_EVAL_FORM 2 selects the three-launch form)", n);
    }
    return 0;
}

extern "C" int seir_sync(seir_ctx *ctx) {
    if (!ctx) return fail(SEIR_ERR_INVALID, "null context");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (int rc = check_eval_handoffs(ctx)) return rc;
    return 0;
}

extern "C" void *seir_stream(seir_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

extern "C" int seir_malloc(void **p, uint64_t bytes) {
    if (!p) return fail(SEIR_ERR_INVALID, "null pointer");
    HIP_TRY(hipMalloc(p, bytes ? bytes : 8));
    return 0;
}
extern "C" int seir_free(void *p) {
    HIP_TRY(hipFree(p));
    return 0;
}
extern "C" int seir_memcpy_h2d(void *dst, const void *src, uint64_t bytes) {
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return 0;
}
extern "C" int seir_memcpy_d2h(void *dst, const void *src, uint64_t bytes) {
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int seir_timer_start(seir_ctx *ctx) {
    if (!ctx) return fail(SEIR_ERR_INVALID, "null context");
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    return 0;
}
extern "C" int seir_timer_stop(seir_ctx *ctx, float *ms) {
    if (!ctx || !ms) return fail(SEIR_ERR_INVALID, "null argument");
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(hipEventSynchronize(ctx->ev1));
    HIP_TRY(hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    return 0;
}

extern "C" int seir_time_kernel(seir_ctx *ctx, int32_t which, int32_t B, int32_t iters, float *mean_ms) {
    int rc = check_batch(ctx, B);
    if (rc) return rc;
    if (!mean_ms || iters < 1) return fail(SEIR_ERR_INVALID, "bad iters/mean_ms");
    if (!ctx->last_events || !ctx->last_u || !ctx->last_logp)
        return fail(SEIR_ERR_STATE, "run one evaluation before timing a kernel");
    if ((which == SEIR_K_SE_GRAD || which == SEIR_K_TILES_GRAD) && !ctx->last_grad)
        return fail(SEIR_ERR_STATE, "last evaluation had no gradient buffer");
    auto once = [&]() {
        switch (which) {
            case SEIR_K_SCAN: launch_scan<0>(ctx, whole(ctx, B), ctx->last_events); break;
            case SEIR_K_GEMM: launch_gemm(ctx, whole(ctx, B)); break;
            case SEIR_K_SE_VALUE: launch_se<0>(ctx, whole(ctx, B), false); break;
            case SEIR_K_SE_GRAD: launch_se<0>(ctx, whole(ctx, B), true); break;
            case SEIR_K_STATE: launch_state_params(ctx, whole(ctx, B), ctx->last_u, ctx->last_events); break;
            case SEIR_K_TILES_VALUE:
            case SEIR_K_TILES_GRAD:
                if (ctx->d.Tp % 96 == 0) launch_eval_tiles<96>(ctx, whole(ctx, B), ctx->last_events, which == SEIR_K_TILES_GRAD);
                else launch_eval_tiles<64>(ctx, whole(ctx, B), ctx->last_events, which == SEIR_K_TILES_GRAD);
                break;
            case SEIR_K_FINISH_FUSED:
                if (ctx->d.Tp % 96 == 0) launch_finish_fused<96>(ctx, whole(ctx, B), ctx->last_u, ctx->last_logp, ctx->last_grad);
                else launch_finish_fused<64>(ctx, whole(ctx, B), ctx->last_u, ctx->last_logp, ctx->last_grad);
                break;
            default: launch_finish(ctx, whole(ctx, B), ctx->last_u, ctx->last_logp, ctx->last_grad); break;
        }
    };
    if (which < SEIR_K_SCAN || which > SEIR_K_FINISH_FUSED) return fail(SEIR_ERR_INVALID, "unknown kernel id %d", which);
    once();                                    // warm
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    for (int i = 0; i < iters; ++i) once();
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    HIP_TRY(hipGetLastError());
    *mean_ms = ms / iters;
    return 0;
}

__global__ void k_selftest_math(Consts c, int n, const double *x, double *L, double *inv, double *lf) {
    __shared__ double2 ltab[LDSTAB_N];
    log_table_to_lds(ltab, c.logtab);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        double a, b2;
        l1me_inv(x[i], a, b2, ltab);
        L[i] = a; inv[i] = b2;
        lf[i] = lfact(floor(x[i]), ltab);
    }
}

extern "C" int seir_selftest_math(seir_ctx *ctx, int32_t n, const double *x, double *L, double *inv, double *lf) {
    int rc = check_batch(ctx, 1);
    if (rc) return rc;
    if (n < 1 || !x || !L || !inv || !lf) return fail(SEIR_ERR_INVALID, "bad arguments");
    DevBuf buf;
    if ((rc = buf.alloc(sizeof(double) * 4 * n))) return rc;
    double *dx = buf.as<double>();
    HIP_TRY(hipMemcpy(dx, x, sizeof(double) * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_selftest_math, dim3(64), dim3(256), 0, ctx->stream, ctx->c, n, dx, dx + n, dx + 2 * n, dx + 3 * n);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(L, dx + n, sizeof(double) * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(inv, dx + 2 * n, sizeof(double) * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(lf, dx + 3 * n, sizeof(double) * n, hipMemcpyDeviceToHost));
    return 0;
}

template <int RT_TT>
static void launch_rt(seir_ctx *ctx, int nb, double *rit_dev) {
    const Dims &d = ctx->d;
    const size_t lds = k_rt_lds_bytes<RT_TT>(d.Mp);
    static std::atomic<unsigned long long> attr_set{0ull};
    if (lds > 64 * 1024 && first_on_device(attr_set, ctx->device))
        (void)lds_attribute((const void *)k_rt<RT_TT>, lds);
    hipLaunchKernelGGL(k_rt<RT_TT>, dim3((d.M + 63) / 64, (d.T + RT_TT - 1) / RT_TT, nb), dim3(256), lds, ctx->stream, d,
                       ctx->c, ctx->w, ctx->u_stage, rit_dev);
}

extern "C" int seir_reproduction_number(seir_ctx *ctx, int32_t n, const double *theta, const double *events,
                                        double *R_it) {
    int rc = check_batch(ctx, 1);
    if (rc) return rc;
    if (n < 1 || !theta || !events || !R_it) return fail(SEIR_ERR_INVALID, "bad arguments");
    const Dims &d = ctx->d;
    const int Bm = ctx->Bmax;
    DevBuf rit;
    if ((rc = rit.alloc(sizeof(double) * Bm * d.T * d.M))) return rc;
    double *rit_dev = rit.as<double>();
    for (int s0 = 0; s0 < n; s0 += Bm) {
        const int nb = std::min(Bm, n - s0);
        HIP_TRY(hipMemcpyAsync(ctx->u_stage, theta + (size_t)s0 * d.P, sizeof(double) * nb * d.P,
                               hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(ctx->ev_stage, events + (size_t)s0 * d.M * d.T * 3, sizeof(double) * nb * d.M * d.T * 3,
                               hipMemcpyHostToDevice, ctx->stream));
        launch_scan<0>(ctx, whole(ctx, nb), ctx->ev_stage);               // KS = (k_se, S - k_se): S_it
        hipLaunchKernelGGL(k_rt_tables, dim3(nb), dim3(256), 0, ctx->stream, d, ctx->w, ctx->u_stage);
        if (rt_days_per_block(d.Mp) == 16) launch_rt<16>(ctx, nb, rit_dev);
        else launch_rt<4>(ctx, nb, rit_dev);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(R_it + (size_t)s0 * d.T * d.M, rit_dev, sizeof(double) * nb * d.T * d.M,
                               hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    ctx->prepared = false;                     // the scan overwrote the prepared-events workspace
    return 0;
}

// ===========================================================================
// Forward simulation (see include/seir_hip.h, "Chain-binomial forward simulation")
// ===========================================================================
__global__ void k_selftest_math_wide(Consts c, int n, const double *x, double *L, double *inv) {
    __shared__ double2 ltab[LDSTAB_N];
    log_table_to_lds(ltab, c.logtab);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        double a, b2;
        l1me_inv_wide(x[i], a, b2, ltab);
        L[i] = a; inv[i] = b2;
    }
}

extern "C" int seir_selftest_math_wide(seir_ctx *ctx, int32_t n, const double *x, double *L, double *inv) {
    int rc = check_batch(ctx, 1);
    if (rc) return rc;
    if (n < 1 || !x || !L || !inv) return fail(SEIR_ERR_INVALID, "bad arguments");
    DevBuf dx, dL, di;
    if ((rc = dx.alloc(sizeof(double) * n)) || (rc = dL.alloc(sizeof(double) * n)) || (rc = di.alloc(sizeof(double) * n)))
        return rc;
    HIP_TRY(hipMemcpyAsync(dx.p, x, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_selftest_math_wide, dim3(64), dim3(256), 0, ctx->stream, ctx->c, n, dx.as<double>(), dL.as<double>(),
                       di.as<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(L, dL.p, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(inv, di.p, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---- self-tests of the device math by function (selftest_kernels.h; tests/test_devmath_gpu.py) ----
namespace {
bool st_finite(const double *v, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}
bool st_count(const double *v, int n, double lo, double hi) {      // integer-valued, lo <= v <= hi
    for (int i = 0; i < n; ++i)
        if (!(v[i] >= lo && v[i] <= hi) || v[i] != std::floor(v[i])) return false;
    return true;
}
}  // namespace

extern "C" int seir_selftest_fn(seir_ctx *ctx, int32_t op, int32_t n, const double *x, const double *y, double *out0,
                                double *out1) {
    int rc = check_batch(ctx, 1);
    if (rc) return rc;
    if (op < 0 || op >= SEIR_FN_COUNT) return fail(SEIR_ERR_INVALID, "unknown function %d", op);
    if (n < 1 || !x || !out0) return fail(SEIR_ERR_INVALID, "bad arguments");
    const bool two_in = op == SEIR_FN_LBINOM_TAB || op == SEIR_FN_LBINOM_CONST || op == SEIR_FN_LBINOM_BF ||
                        op == SEIR_FN_LOG1MEXP_DIFF_SLOW;
    const bool two_out = op == SEIR_FN_SOFTPLUS_SIGMOID_TAB || op == SEIR_FN_LOG1MEXP_SERIES ||
                         op == SEIR_FN_L1ME_INV_SERIES || op == SEIR_FN_L1ME_INV_K || op == SEIR_FN_L1ME_INV_SERIES_K;
    if (two_in && !y) return fail(SEIR_ERR_INVALID, "function %d takes two arguments", op);
    if (two_out && !out1) return fail(SEIR_ERR_INVALID, "function %d has two results", op);
    // the domains (include/seir_hip.h): a table is never indexed out of range, whatever the caller passes
    if (!st_finite(x, n) || (two_in && !st_finite(y, n))) return fail(SEIR_ERR_INVALID, "argument not finite");
    switch (op) {
        case SEIR_FN_FAST_LOG: case SEIR_FN_FAST_LOG_K: case SEIR_FN_MV_LOG: case SEIR_FN_FAST_RCP:
            for (int i = 0; i < n; ++i)
                if (!(x[i] > 0.0) || !std::isnormal(x[i])) return fail(SEIR_ERR_INVALID, "x[%d] is not a positive normal number", i);
            break;
        case SEIR_FN_LFACT_BF: case SEIR_FN_LBINOM_TAB: case SEIR_FN_LBINOM_CONST: case SEIR_FN_LBINOM_BF:
            if (!st_count(x, n, 0.0, 2147483647.0)) return fail(SEIR_ERR_INVALID, "n must be an integer in 0 .. 2^31 - 1");
            if (two_in && !st_count(y, n, -2147483648.0, 2147483648.0)) return fail(SEIR_ERR_INVALID, "k must be an integer of |k| <= 2^31");
            break;
        default: break;
    }
    DevBuf dx, dy, d0, d1;
    const size_t bytes = sizeof(double) * (size_t)n;
    if ((rc = dx.alloc(bytes)) || (rc = dy.alloc(two_in ? bytes : 8)) || (rc = d0.alloc(bytes)) ||
        (rc = d1.alloc(out1 ? bytes : 8)))
        return rc;
    HIP_TRY(hipMemcpyAsync(dx.p, x, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (two_in) HIP_TRY(hipMemcpyAsync(dy.p, y, bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_selftest_fn, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->c.logtab, (int)op, (int)n,
                       dx.as<double>(), two_in ? dy.as<double>() : (const double *)nullptr, d0.as<double>(),
                       out1 ? d1.as<double>() : (double *)nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out0, d0.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (out1) HIP_TRY(hipMemcpyAsync(out1, d1.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int seir_selftest_band_delta(seir_ctx *ctx, int32_t op, int32_t n, const double *S, const double *I,
                                        const double *K0, const double *F, const double *dF, const double *ee,
                                        const double *psiW, double rate_floor, double dt, double *out) {
    int rc = check_batch(ctx, 1);
    if (rc) return rc;
    if (op < SEIR_DELTA_BAND || op > SEIR_DELTA_OWN_SE) return fail(SEIR_ERR_INVALID, "unknown delta %d", op);
    if (n < 1 || !S || !I || !K0 || !F || !dF || !ee || !psiW || !out) return fail(SEIR_ERR_INVALID, "bad arguments");
    const double *in[7] = {S, I, K0, F, dF, ee, psiW};
    for (const double *v : in)
        if (!st_finite(v, n)) return fail(SEIR_ERR_INVALID, "argument not finite");
    if (!std::isfinite(rate_floor) || !std::isfinite(dt)) return fail(SEIR_ERR_INVALID, "argument not finite");
    DevBuf din, dout;
    const size_t bytes = sizeof(double) * (size_t)n;
    if ((rc = din.alloc(7 * bytes)) || (rc = dout.alloc(bytes))) return rc;
    double *p = din.as<double>();
    for (int a = 0; a < 7; ++a) HIP_TRY(hipMemcpyAsync(p + (size_t)a * n, in[a], bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_selftest_delta, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->c.logtab, (int)op, (int)n, p,
                       p + (size_t)n, p + (size_t)2 * n, p + (size_t)3 * n, p + (size_t)4 * n, p + (size_t)5 * n,
                       p + (size_t)6 * n, rate_floor, dt, dout.as<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, dout.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int seir_selftest_wave(seir_ctx *ctx, int32_t op, int32_t is_int, int32_t nblocks, const void *in, void *out,
                                  void *total) {
    int rc = check_batch(ctx, 1);
    if (rc) return rc;
    if (op < SEIR_WAVE_SUM || op > SEIR_BLOCK_SUM) return fail(SEIR_ERR_INVALID, "unknown primitive %d", op);
    if (is_int && op != SEIR_WAVE_SUM && op != SEIR_WAVE_INCL_SCAN && op != SEIR_BLOCK_EXCL_SCAN)
        return fail(SEIR_ERR_INVALID, "primitive %d has no int32 form", op);
    if (nblocks < 1 || nblocks > 1024 || !in || !out) return fail(SEIR_ERR_INVALID, "bad arguments");
    DevBuf din, dout, dtot;
    const size_t bytes = (is_int ? sizeof(int32_t) : sizeof(double)) * (size_t)nblocks * 256;
    if ((rc = din.alloc(bytes)) || (rc = dout.alloc(bytes)) || (rc = dtot.alloc(bytes))) return rc;
    HIP_TRY(hipMemcpyAsync(din.p, in, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (is_int)
        hipLaunchKernelGGL(k_selftest_wave<1>, dim3(nblocks), dim3(256), 0, ctx->stream, (int)op, din.as<int>(),
                           dout.as<int>(), total ? dtot.as<int>() : (int *)nullptr);
    else
        hipLaunchKernelGGL(k_selftest_wave<0>, dim3(nblocks), dim3(256), 0, ctx->stream, (int)op, din.as<double>(),
                           dout.as<double>(), total ? dtot.as<double>() : (double *)nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, dout.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (total) HIP_TRY(hipMemcpyAsync(total, dtot.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int seir_within_between(seir_ctx *ctx, int32_t n, const double *psi, const double *I_last, double W,
                                   double *within, double *between) {
    int rc = check_batch(ctx, 1);
    if (rc) return rc;
    if (n < 1 || !psi || !I_last || !within || !between) return fail(SEIR_ERR_INVALID, "bad arguments");
    const Dims &d = ctx->d;
    DevBuf dpsi, dI, dw, db;
    const size_t nm = sizeof(double) * (size_t)n * d.M;
    if ((rc = dpsi.alloc(sizeof(double) * n)) || (rc = dI.alloc(nm)) || (rc = dw.alloc(nm)) || (rc = db.alloc(nm)))
        return rc;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(dpsi.p, psi, sizeof(double) * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dI.p, I_last, nm, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_within_between, dim3(n), dim3(256), sizeof(double) * d.Mp, st, d, ctx->c, n, dpsi.as<double>(),
                       dI.as<double>(), W, dw.as<double>(), db.as<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(within, dw.p, nm, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(between, db.p, nm, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int seir_simulate(seir_ctx *ctx, const seir_sim_desc *sd) {
    int rc = check_batch(ctx, 1);
    if (rc) return rc;
    if (!sd || sd->num_draws < 1 || sd->num_steps < 1 || !sd->par || !sd->log_baseline || !sd->spatial || !sd->W ||
        !sd->weekday_c || !sd->init_state || !sd->events)
        return fail(SEIR_ERR_INVALID, "bad arguments");
    const Dims &d = ctx->d;
    const int M = d.M, S = sd->num_steps;
    if ((long long)S * M > 0x7fffffffLL) return fail(SEIR_ERR_INVALID, "num_steps * M overflows the cell counter");
    const size_t lds = k_simulate_lds_bytes(d);
    if (lds > 160 * 1024) return fail(SEIR_ERR_INVALID, "M=%d needs %zu B of LDS for the simulator", M, lds);
    HIP_TRY(lds_attribute((const void *)k_simulate, lds));
    // draws per batch: bound the device output buffer to ~512 MB
    const size_t per_draw = (size_t)M * S * 3 * sizeof(double);
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)sd->num_draws, ((size_t)512 << 20) / per_draw));
    DevBuf par, ap, sp, W, wd, init, ev;
    if ((rc = par.alloc(sizeof(double) * chunk * 5)) || (rc = ap.alloc(sizeof(double) * chunk * S)) ||
        (rc = sp.alloc(sizeof(double) * chunk * M)) || (rc = W.alloc(sizeof(double) * S)) ||
        (rc = wd.alloc(sizeof(double) * S)) || (rc = init.alloc(sizeof(double) * chunk * M * 4)) ||
        (rc = ev.alloc(per_draw * chunk)))
        return rc;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(W.p, sd->W, sizeof(double) * S, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(wd.p, sd->weekday_c, sizeof(double) * S, hipMemcpyHostToDevice, st));
    for (int s0 = 0; s0 < sd->num_draws; s0 += chunk) {
        const int nb = std::min(chunk, sd->num_draws - s0);
        HIP_TRY(hipMemcpyAsync(par.p, sd->par + (size_t)s0 * 5, sizeof(double) * nb * 5, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ap.p, sd->log_baseline + (size_t)s0 * S, sizeof(double) * nb * S, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(sp.p, sd->spatial + (size_t)s0 * M, sizeof(double) * nb * M, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(init.p, sd->init_state + (size_t)s0 * M * 4, sizeof(double) * nb * M * 4,
                               hipMemcpyHostToDevice, st));
        SimArgs a{};
        a.n = nb; a.S = S; a.first_draw = sd->first_draw_id + s0;
        a.k0 = (uint32_t)(sd->seed & 0xffffffffu); a.k1 = (uint32_t)(sd->seed >> 32);
        a.par = par.as<double>(); a.a_path = ap.as<double>(); a.spatial = sp.as<double>();
        a.W = W.as<double>(); a.wd = wd.as<double>(); a.init = init.as<double>(); a.events = ev.as<double>();
        hipLaunchKernelGGL(k_simulate, dim3(nb), dim3(SIM_THREADS), lds, st, d, ctx->c, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(sd->events + (size_t)s0 * M * S * 3, ev.p, per_draw * nb, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return 0;
}

__global__ void k_selftest_binomial(int count, const int *n, const double *p, uint32_t k0, uint32_t k1, int *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    RngKey key{k0, k1, 0u, (uint32_t)i};
    out[i] = sim_binomial(n[i], p[i], key, RS_SIM_BASE);
}

extern "C" int seir_selftest_binomial(seir_ctx *ctx, int32_t count, const int32_t *n, const double *p, uint64_t seed,
                                      int32_t *out) {
    int rc = check_batch(ctx, 1);
    if (rc) return rc;
    if (count < 1 || !n || !p || !out) return fail(SEIR_ERR_INVALID, "bad arguments");
    DevBuf dn, dp, dout;
    if ((rc = dn.alloc(sizeof(int) * count)) || (rc = dp.alloc(sizeof(double) * count)) ||
        (rc = dout.alloc(sizeof(int) * count)))
        return rc;
    HIP_TRY(hipMemcpyAsync(dn.p, n, sizeof(int) * count, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dp.p, p, sizeof(double) * count, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_selftest_binomial, dim3((count + 255) / 256), dim3(256), 0, ctx->stream, count, dn.as<int>(),
                       dp.as<double>(), (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), dout.as<int>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, dout.p, sizeof(int) * count, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// ===========================================================================
// Sampler (see include/seir_hip.h, "Device-resident Metropolis-within-Gibbs")
// ===========================================================================
// A device allocation that travels with the snapshots (seir_sampler_snapshot / _restore): its shadow copy for each of the two
// slots and whether that holds anything.  A shadow taken before the feature that owns the buffer was enabled or last reset
// holds nothing of it (valid = false): restoring that slot leaves the buffer alone.
struct Shadowed {
    DevBuf buf, snap[2];
    bool valid[2] = {false, false};
};
// One set of moment accumulators (MomentBufs' ref .. overflow) as ONE allocation, every part naturally aligned:
//     sum [cells] | sumsq [cells] | count [B, padded to 256 B] | ref [cells] | flag
// (the padding keeps count's length from moving ref off the cache lines that the 16 B x cells before it leave it on)
struct MomentAcc : Shadowed {
    size_t cells = 0, B = 0;
    size_t count_words() const { return (B + 31) / 32 * 32; }
};

static void acc_layout(const MomentAcc &a, MomentBufs &mb) {
    mb.sum = a.buf.as<int64_t>();
    mb.sumsq = (uint64_t *)(mb.sum + a.cells);
    mb.count = mb.sumsq + a.cells;
    mb.ref = (int32_t *)(mb.count + a.count_words());
    mb.overflow = (unsigned *)(mb.ref + a.cells);
}
static int acc_alloc(MomentAcc &a, size_t cells, size_t B, MomentBufs &mb) {
    a.cells = cells; a.B = B;
    if (int rc = a.buf.zeroed(cells * (sizeof(int64_t) + sizeof(uint64_t) + sizeof(int32_t)) + a.count_words() * sizeof(uint64_t) + 8))
        return rc;
    acc_layout(a, mb);
    return 0;
}
static int acc_zero(Shadowed &a, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(a.buf.p, 0, a.buf.bytes, st));
    return 0;
}
// save: the buffer into the slot's shadow; else the shadow back, if it holds anything.  In stream order.
static int acc_shadow(Shadowed &a, int slot, bool save, hipStream_t st) {
    if (!save && !a.valid[slot]) return 0;
    if (!a.snap[slot])
        if (int rc = a.snap[slot].alloc(a.buf.bytes)) return rc;
    HIP_TRY(hipMemcpyAsync(save ? a.snap[slot].p : a.buf.p, save ? a.buf.p : a.snap[slot].p, a.buf.bytes, hipMemcpyDeviceToDevice, st));
    if (save) a.valid[slot] = true;
    return 0;
}
static void acc_invalidate(Shadowed &a) { a.valid[0] = a.valid[1] = false; }
// Accumulators with the host's count of the draws per chain folded into them since the product's reset: the counter travels
// with the block, and a restore from a slot that holds nothing of the block leaves both alone.
template <typename Acc>
struct Counted : Acc {
    long long j = 0, snap_j[2] = {0, 0};                 // the count; what it was when each slot's shadow was taken
    void drop() { static_cast<Acc &>(*this) = Acc{}; }   // the block goes; j stays until the reset that follows
};
template <typename Acc>
static int counted_shadow(Counted<Acc> &a, int slot, bool save, hipStream_t st) {
    if (save) a.snap_j[slot] = a.j;
    else if (a.valid[slot]) a.j = a.snap_j[slot];
    return acc_shadow(a, slot, save, st);
}
// Blocking read of whichever parts are asked for, and of the sticky overflow flag.
static int acc_read(const MomentAcc &a, hipStream_t st, uint64_t *count, int32_t *ref, int64_t *sum, uint64_t *sumsq, unsigned *flag) {
    MomentBufs mb{};
    acc_layout(a, mb);
    HIP_TRY(hipMemcpyAsync(flag, mb.overflow, sizeof(*flag), hipMemcpyDeviceToHost, st));
    if (count) HIP_TRY(hipMemcpyAsync(count, mb.count, sizeof(uint64_t) * a.B, hipMemcpyDeviceToHost, st));
    if (ref) HIP_TRY(hipMemcpyAsync(ref, mb.ref, sizeof(int32_t) * a.cells, hipMemcpyDeviceToHost, st));
    if (sum) HIP_TRY(hipMemcpyAsync(sum, mb.sum, sizeof(int64_t) * a.cells, hipMemcpyDeviceToHost, st));
    if (sumsq) HIP_TRY(hipMemcpyAsync(sumsq, mb.sumsq, sizeof(uint64_t) * a.cells, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// The per-slot group sums of one source (seir_sampler_groups_set): ev [cap][B][G][L][3], st0 [cap][B][G][3] (null for the trace).
struct GroupOut {
    DevBuf ev, st0;                   // int64
    int L = 0;                        // day extent the arrays are sized for; 0: none (no table, or the source is off)
};

// One family of group curves (seir_sampler_group_rt: weighted; seir_sampler_group_wb), a plane per national curve of its
// Window: the switch, the per-slot outputs out [cap][B][G][D] and the cell planes [slots * B][D][Mp] of a batch.  D = 0: no
// outputs (the switch is off, there is no table, the product is off, or the outputs were refused) -- nothing is launched then.
struct GroupCurve {
    bool on = false;
    DevBuf weights;                   // double [nnz] aligned with the members (group R_t), or empty
    struct Bufs {                     // what the table and the window size; Bufs{}: none, the switch and the weights stay
        int D = 0, slots = 0;         // window days the buffers are sized for; trace slots per batch
        DevBuf offsets;               // device copy of the table's offsets [G + 1], int
        DevBuf cells[2], out[2];      // double
    } b;
};

// The group next-generation matrix of the kept draws (seir_sampler_group_ngm; ngm_kernels.h): the draw store
// out [cap][B][G][G][D], indexed by draw position since the rt reset, and the rows plane P [slots * B][G][D][Mp] of a batch.
// cap = 0: off, nothing is allocated and nothing is launched.
struct GroupNgm {
    long long cap = 0;                // draws per chain the store holds
    int D = 0, slots = 0;             // window days the buffers are sized for; trace slots per batch
    DevBuf offsets;                   // device copy of the table's offsets [G + 1], int
    DevBuf weights;                   // double [nnz] aligned with the members
    DevBuf P, out;                    // double
};

// The users of a trace range that have to be enabled first, in the words their refusals use: what they do with the events; that
// they are off; their name; what they have done to a draw; their reset, fold and draw-store entry points; their group curve off.
struct TraceUser { const char *verb, *not_enabled, *name, *done, *reset, *call, *keep, *no_curve; };
static const TraceUser SUMMARY_USER = {"summarise", "summaries are not enabled: call seir_sampler_summary_reset first"};
static const TraceUser RT_USER = {"form the reproduction number from",
                                   "the reproduction number is not enabled: call seir_sampler_rt_reset first", "rt", "folded",
                                   "seir_sampler_rt_reset", "seir_sampler_rt", "seir_sampler_rt_keep",
                                   "group R_t is not enabled: call seir_sampler_group_rt first"};
static const TraceUser WB_USER = {"form the within/between pressure shares from",
                                   "the within/between pressure shares are not enabled: call seir_sampler_wb_reset first",
                                   nullptr, nullptr, nullptr, nullptr, nullptr,
                                   "group within/between is not enabled: call seir_sampler_group_wb first"};
static const TraceUser FORECAST_USER = {"forecast from", "the forecast is not enabled: call seir_sampler_forecast_reset first", "forecast",
                                         "forecast", "seir_sampler_forecast_reset", "seir_sampler_forecast", "seir_sampler_forecast_keep"};
static const TraceUser CHECK_USER = {"check", "the in-sample check is not enabled: call seir_sampler_check_reset first", "check",
                                      "checked"};

// The host's half of a ForecastBufs that is rolled forward day by day from the kept draws (forecast_kernels.h): the forecast
// and the in-sample check each own one (rollout_*, below).
struct Rollout {
    bool on = false;                  // enabled by the user's first reset: buffers exist
    ForecastBufs fb{};
    int slots = 0;                    // trace slots per batch: min(cap, FC_JMAX)
    int ndmax = 0;                    // row stride the planes are allocated for: ceil64(slots * B)
    std::vector<DevBuf> allocs;       // device buffers sized by fb.H (allocated again when it changes)
    Counted<MomentAcc> acc;           // fb.mom's ref .. overflow; j: draws per chain rolled forward since the last reset (the draw id's j)
};

// The host's half of a product that folds a window of the last D days of the kept draws (rt_trace_kernels.h, wb_kernels.h):
// the reproduction number and the within/between pressure shares each own one (window_*, below).  The device's half, the
// kernel argument (RtBufs, WbBufs), stays with the product, as do its kernels and the layout of its block.
struct Window {
    const TraceUser &who;
    const int planes;                 // national curves per draw, and planes of the group curve: 1 (R_t) or 2 (within, between)
    bool on = false;                  // enabled by the user's first reset: buffers exist
    int D = 0;                        // window days everything below is sized for
    int slots = 0;                    // trace slots the batch planes are allocated for
    std::vector<DevBuf> allocs;       // device buffers sized by the window (allocated again when it changes)
    const double *draws[2] = {nullptr, nullptr};   // among them the national curves [cap][B][D] of every slot (Rt; Wn, Bn)
    Counted<Shadowed> acc;            // the product's block; j: the host's copy of its count (every chain's: calls take them all)
    GroupCurve curve;                 // the product's curves per group
    Window(const TraceUser &u, int np) : who(u), planes(np) {}
};

// The draws of every cell that a product keeps for order statistics (seir_sampler_forecast_keep, seir_sampler_rt_keep), or
// empty: off.  Position j of a cell's run is the chain's j-th draw since the product's reset, so a reset empties it.
struct DrawStore {
    DevBuf buf;                       // int [B][3][M][H][stride] (forecast), double [B][D][M][stride] (R_it)
    long long cap = 0, stride = 0;    // draws per chain it holds; a cell's run: cap, for R_it rounded up to RT_KEEP_RUN (aligned runs)
};

// The scenarios that ride on the forecast (seir_sampler_scenarios_set; scenario_kernels.h), or K = 0: off.  Everything is
// sized by the forecast's H and goes when that changes.  j is the forecast's (fc.acc.j): scenario and baseline are rolled
// forward together.
struct ScenarioSet {
    int K = 0;
    long long cap = 0;                // draws per chain the position stores hold
    std::vector<double> commute;      // [K][H] on the host: W_k is formed again from the calendar of every forecast reset
                                      //     (a local set: [K][M][H] as the caller gave it)
    std::vector<DevBuf> allocs;
    double *log_shift = nullptr, *Wk = nullptr;     // [K][H]
    int *St = nullptr;                // [3][Mp][K ndmax]
    double *X = nullptr, *F = nullptr;              // [Mp][K ndmax]
    double *base = nullptr;           // [K][H][ndmax]
    int *sev = nullptr;               // [K][fc.slots * B][M][H][3]
    MomentBufs mom[4]{};              // per scenario: the per-slot marginals (the accumulators' pointers come from acc's layout)
    int64_t *by_day = nullptr, *state_by_day = nullptr;   // [K][cap][B][H][3] by draw position since the forecast reset
    // ONE block, shadowed with the forecast's: per scenario the moments (sum | sumsq [c6], count [B, padded]) and the
    // differences (sum | sumsq [c4]), then the 32-bit parts per scenario (ref [c6]; ref | lt | eq [c4]; the two flags)
    Shadowed acc;
    size_t c6 = 0, c4 = 0, B = 0;
    size_t count_words() const { return (B + 31) / 32 * 32; }
    size_t words8() const { return 2 * c6 + count_words() + 2 * c4; }
    size_t words4() const { return c6 + 3 * c4 + 2; }
    // A local set (seir_sampler_scenarios_set_local; scenario_local_kernels.h): scenarios_batch launches the local kernels,
    // which read these two in the place of log_shift, Wk and base (not allocated then).
    // A triggered set (seir_sampler_scenarios_set_triggered; scenario_trigger_kernels.h): the local tensors are its off pair,
    // and it has the on pair, the rule and the rule's planes and products below.
    enum Mode { GLOBAL = 0, LOCAL = 1, TRIGGERED = 2 };
    Mode mode = GLOBAL;
    bool local() const { return mode != GLOBAL; }       // the operands are [K][H][M] tensors
    bool triggered() const { return mode == TRIGGERED; }
    double *log_shift_loc = nullptr, *Wk_loc = nullptr;   // [K][H][M]: the caller's tensors transposed
    std::vector<double> commute_on;   // [K][M][H] on the host, as commute is
    double *log_shift_on = nullptr, *Wk_on = nullptr;     // [K][H][M]
    int32_t *trig_on = nullptr, *trig_off = nullptr;      // [K][M] thresholds
    int32_t *trig_params = nullptr;   // [K][4] window, from_day, min_days, review_every
    int wmax = 0;                     // the largest window: hist's rows
    int32_t *hist = nullptr;          // [wmax][Mp][ndmax]
    int32_t *win = nullptr, *age = nullptr;               // [Mp][K ndmax]
    uint64_t *mask = nullptr;         // [2][Mp][K ndmax]
    int32_t *active_by_day = nullptr; // [K][cap][B][H] by draw position since the forecast reset; overwritten, no shadow
    Shadowed tacc;                    // active_count [K][B][M][H] uint32: shadowed, invalidated and zeroed where acc is
    // The per-draw region totals of the scenarios (seir_sampler_scenario_groups_set), by draw position since the forecast
    // reset like by_day: int64 [K][cap][B][G][H][3], or empty: off.  No shadow: a burst run again overwrites its positions.
    DevBuf gstore;
    int gG = 0;                       // groups the store is sized for; 0: none
};

// The truth the forecast is scored against (seir_sampler_verify_set; verify_kernels.h), or on = false.  Sized by the
// forecast's H and gone when that changes; the count of the accumulators is the forecast's j (fc.acc.j).
struct VerifySet {
    bool on = false;
    std::vector<DevBuf> allocs;
    int32_t *truth = nullptr;         // [M][H], < 0: missing
    int64_t *cum = nullptr;           // [M][H] its running total over the days, < 0 from a row's first missing day on
    size_t c2 = 0;                    // B x M x H x 2 cells
    Shadowed acc;                     // ONE block, shadowed with the forecast's: abs_sum [c2] uint64 | lt [c2] | eq [c2] uint32
};

struct seir_sampler {
    seir_ctx *ctx = nullptr;
    SamplerCfg cfg{};
    Chains ch{};
    int record_events = 1;
    // what the chip holds, asked once at creation (inputs of plan_sweep): compute units, workgroups per CU of the k_leap
    // instances the planner can choose (24-row / this shape's 32-row tiles), k_move_pairs allowed its LDS request
    int cus = 0, leap_occ[2] = {0, 0};
    bool pairs_lds_attr = false;
    std::vector<DevBuf> allocs;
    // chains are independent: they are split into groups that run on their own streams
    // so that one group's single-workgroup-per-chain kernels overlap another group's wide ones
    int ngroups = 1;
    std::vector<hipStream_t> gstream;
    std::vector<hipGraph_t> graph;
    std::vector<hipGraphExec_t> gexec;
    hipEvent_t ev_fork = nullptr;
    std::vector<hipEvent_t> ev_join;
    hipStream_t copy_stream = nullptr;    // overlapped egress (seir_sampler_read_trace_async)
    hipEvent_t ev_burst = nullptr, ev_copy = nullptr;
    bool copy_pending = false;
    bool use_graph = false;       // seir_sampler_desc::use_graph
    int leap_rows = 0;            // seir_sampler_desc::leap_rows: 0 auto, 24 / 32: only that tile shape (else the per-step form)
    // seir_sampler_time_leapfrog: HIP events around the inner leapfrog steps of each sweep while it is on
    std::vector<hipEvent_t> prof_ev;     // pairs (before, after)
    int prof_i = -1;              // next pair to record (-1: off)
    bool vt_dirty = true;         // Work::Vt does not match Chains::var (set_kernel / set_adaptation / creation)
    unsigned long long leap_rsteps = 0;  // steps the ROLES of k_leap have done over all launches (the tiles do one more per folded launch)
    unsigned long long leap_steps = 0;   // leapfrog steps done by all k_leap launches so far (what Chains::leap's flags show)
    bool xcd_local = false;       // blocks with the same id mod 8 share an XCD (k_xcc_probe at creation)
    unsigned long long tail_count = 0;   // tiles per chain counted in by all k_se_chunk launches so far (Chains::tail)
    unsigned pbar_count = 0;      // role arrivals every chain's step counter (Chains::pbar) has seen over all k_move_pairs launches
    int pair_debug = 0;           // debug_pair: test hooks of k_move_pair's handshake (1 late, 2 absent role 1; 16..128: delays per step, k_move_pairs)
    int moves_mode = 0;           // (moves_form: the mode in force) 0 = paired updates (k_move_pair) with the S->E-type proposal pre-drawn one pair ahead -- every pair of a
                                  //     sweep in one launch (k_move_pairs) where band workgroups can be part of it, else one launch per
                                  //     pair (4: always one launch per pair; 3: the same, never with band workgroups in the pair launch);
                                  // 1 = one proposal kernel per update (k_move_pa2); 2 = paired launches without the pre-draw
    int graph_skew = 0, graph_aff = 3, graph_mm = 0;   // context options the captured graph was built with (graph_mm: sampler_mm)
    bool have_state = false;
    double *ev_stage = nullptr;       // [B][M][T][3] fp64 staging for set/get_state
    // --- recovery from a failed in-launch hand-off (seir_sampler_snapshot / _restore) ---
    // Every device buffer of the sampler is one of: chain STATE (what the next sweep's draws are a function of: copied by a
    // snapshot), HAND-OFF scratch (tokens, counters, descriptors in flight inside a sweep: zeroed by a restore, together
    // with the host's running totals of the counters), or neither (trace, staging).
    enum { R_OTHER = 0, R_STATE = 1, R_HANDOFF = 2 };
    struct Region { void *p; size_t bytes; int kind; };
    std::vector<Region> regions;
    DevBuf snap[2];                       // shadow copies of the STATE regions, packed
    bool snap_valid[2] = {false, false};
    size_t snap_bytes = 0;
    bool poisoned = false;            // a fatal hand-off time-out was reported: no sweeps until set_state / refresh / restore
    int poison_chain = 0;
    unsigned poison_count = 0;
    int hmc_mode = 0;                 // the launch forms in force (seir_sampler_set_launch_form)
    int thin_pending = 1;             // seir_sampler_set_thin: becomes cfg.thin at the next trace reset (Chains::slot0 is encoded for cfg.thin)
    // --- summaries of the recorded events (seir_sampler_summary_reset ...; summary_kernels.h) ---
    bool sum_on = false;              // enabled by the first seir_sampler_summary_reset: buffers exist
    MomentBufs sum{};
    MomentAcc sum_acc;                // sum's ref .. overflow
    // --- convergence diagnostics (seir_sampler_diag_reset ...): ONE allocation of 64-bit words,
    //     bsum [n] | bsumsq [n] | nbatch [B] | mark 0: count [B] | sum [n] | sumsq [n] | mark 1: the same
    bool diag_on = false;
    SummaryDiag<1> diag{};
    Shadowed diag_buf;
    // --- forecast of the next H days (seir_sampler_forecast_reset ...; forecast_kernels.h) ---
    Rollout fc;
    PinnedBuf fc_steps_host;          // page-locked double [cap][B][H]: the caller's random-walk steps on their way to the device
    double *fc_steps_dev = nullptr;   // [fc.slots * B][H] (one of fc.allocs)
    hipEvent_t fc_ev_steps = nullptr; // behind the last upload from fc_steps_host
    bool fc_steps_pending = false;
    DrawStore keep_fc;                // int keep[B][3][M][H][cap]: position j of a cell is the draw with the forecast's j
    std::vector<double> fc_W_host;    // [H] the commuting volume of the last forecast reset (the scenarios' W_k come from it)
    ScenarioSet scen;                 // scenarios riding on the forecast (seir_sampler_scenarios_set, _set_local)
    bool scen_grp_on = false;         // seir_sampler_scenario_groups_set: the scenarios' region totals are wanted
    VerifySet ver;                    // the later data the forecast is scored against (seir_sampler_verify_set)
    // --- in-sample check of the last K days (seir_sampler_check_reset ...; check_kernels.h): a Rollout with H := K ---
    Rollout ck;                       // its j is not the forecast's
    CheckCmp ck_cmp{};
    Shadowed ck_cnt;                  // ck_cmp's arrays, 32-bit words: lt | eq | obs [B M K] | loc_lt | loc_eq [B M] |
                                      //     day_lt | day_eq [B K] | all_lt | all_eq | moved [B]
    // --- reproduction number of the kept draws (seir_sampler_rt_reset ...; rt_trace_kernels.h) ---
    Window rt{RT_USER, 1};            // batch planes ea, S, part; block sum | sumsq | ref [cells] | count [B, padded] | gt1 [cells]
    RtBufs rtb{};
    // The R_it draw store double keepR[B][D][M][stride].  It has no shadow: count comes back with the accumulators, and the
    // host's copy of it with them, so a burst run again overwrites its own positions of the store.
    DrawStore keep_rt;
    // --- within/between pressure shares of the kept draws (seir_sampler_wb_reset ...; wb_kernels.h) ---
    Window wb{WB_USER, 2};            // batch planes I, part; block sum_w | sumsq_w | ref_w | ref_b | sum_b [cells] | count [B, padded] | n | gt [cells]
    WbBufs wbb{};
    // --- region totals of the kept draws (seir_sampler_groups_set ...; group_kernels.h) ---
    bool grp_on = false;              // a table is set
    GroupTable grp{};                 // its device copy: segments and members, out of grp_seg and grp_members
    DevBuf grp_seg, grp_members;
    GroupOut grp_out[3];              // per-slot outputs of the trace, the forecast and the check (L = 0: that source is off)
    // --- group curves (seir_sampler_group_rt / _group_wb; group_curve_kernels.h): rt.curve (weighted) and wb.curve ---
    std::vector<int> grp_offsets;     // the table's offsets [G + 1] on the host (the device copy exists only with a curve on)
    // --- group next-generation matrix (seir_sampler_group_ngm; ngm_kernels.h) ---
    GroupNgm ngm;
    // --- stored draws into trace slots (seir_sampler_load_trace; trace_load_kernels.h): nothing of it exists before the first load ---
    double *load_stage = nullptr;     // [load_slots][M T 3 + P] fp64 rows as the file has them: events, then theta (one of allocs)
    unsigned long long *load_words = nullptr;   // the status words of trace_load.h (one of allocs)
    int load_slots = 0;               // draws per chunk: min(LOAD_JMAX, LOAD_STAGING_BYTES / a draw's bytes), at least 1
    hipEvent_t ev_load = nullptr;     // behind the last host-to-device copy of a call
    std::vector<std::pair<int, int>> load_calls;   // (chain, first) of the calls since the last clear, by tag
};

// Zeroed device memory (DevBuf::zeroed) owned by `list` (seir_sampler::allocs: freed with the sampler; Rollout::allocs: also when
// the length changes) and, when it is chain state or hand-off scratch, in the regions a snapshot / restore goes through.
template <typename T>
static int s_alloc(seir_sampler *s, std::vector<DevBuf> &list, T **p, size_t count, int kind = seir_sampler::R_OTHER) {
    DevBuf b;
    if (int rc = b.zeroed((count ? count : 1) * sizeof(T))) return rc;
    if (kind != seir_sampler::R_OTHER) s->regions.push_back({b.p, b.bytes, kind});
    *p = b.as<T>();
    list.push_back(std::move(b));
    return 0;
}
#define S_ALLOC(list, ptr, ...) if (!rc) rc = s_alloc(s, s->list, &(ptr), __VA_ARGS__)

static int gcurve_fit(seir_sampler *s, Window &w);   // with the rest of the group curves, behind the within/between shares

// No table: what was sized by it or weighted along its members goes with it -- the group next-generation matrix, group R_t
// (switch and weights), the buffers of group within / between (its switch stays), the sources' outputs.
static void groups_free(seir_sampler *s) {
    s->ngm = GroupNgm{};
    s->rt.curve = GroupCurve{};
    s->wb.curve.b = {};
    s->grp_offsets.clear();
    for (GroupOut &o : s->grp_out) o = GroupOut{};
    s->grp_seg.reset(); s->grp_members.reset();
    s->grp = GroupTable{};
    s->grp_on = false;
}

static void drop_graph(seir_sampler *s) {
    for (auto &g : s->gexec) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
    for (auto &g : s->graph) if (g) { (void)hipGraphDestroy(g); g = nullptr; }
}

extern "C" void seir_sampler_destroy(seir_sampler *s) {
    if (s) for (hipEvent_t e : s->prof_ev) (void)hipEventDestroy(e);
    if (s) s->prof_ev.clear();
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    drop_graph(s);
    for (auto st : s->gstream) if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    for (auto e : s->ev_join) if (e) (void)hipEventDestroy(e);
    if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
    if (s->copy_stream) { (void)hipStreamSynchronize(s->copy_stream); (void)hipStreamDestroy(s->copy_stream); }
    if (s->ev_burst) (void)hipEventDestroy(s->ev_burst);
    if (s->ev_copy) (void)hipEventDestroy(s->ev_copy);
    if (s->fc_ev_steps) (void)hipEventDestroy(s->fc_ev_steps);
    if (s->ev_load) (void)hipEventDestroy(s->ev_load);
    Work &w = s->ctx->w;
    for (int x = 0; x < 3; ++x) { w.K[x] = nullptr; w.St[x] = nullptr; }
    w.rowtot = w.rngtot = nullptr;
    w.TS = w.sp = w.gst = w.Vt = w.acur = w.rirc = w.CT = w.CG = w.Lpart0 = nullptr;
    delete s;                                        // every buffer goes with its owner (dev_mem.h), behind the waits above
}

// The kernel instances a sweep launches, for the numbers of its plan (sweep_plan.h).
// The persistent leapfrog kernel for (tile-scalar mode, day chunks, gradient tiles per workgroup)
// nst = 2: two 16-row gradient tiles per workgroup (32 rows); nst = 1: ONE 24-row tile per workgroup, six rows per wave -- the
// shape whose 96 workgroups per chain divide UK-380's XCD evenly (instantiated for that size class: M <= 512, six day chunks)
static const void *leap_fn(int ts_mode, int ntc, int nst) {
    if (nst == 1) return (const void *)k_leap<1, 6, 1, 6>;
#define LEAP_ROW(TSM_, NTC_) ((const void *)k_leap<TSM_, NTC_, 2>)
    if (ts_mode == 1) return ntc == 1 ? LEAP_ROW(1, 1) : ntc == 6 ? LEAP_ROW(1, 6) : LEAP_ROW(1, 12);
    return ntc == 1 ? LEAP_ROW(2, 1) : ntc == 6 ? LEAP_ROW(2, 6) : LEAP_ROW(2, 12);
#undef LEAP_ROW
}
static decltype(&k_se_chunk<1, 1>) se_chunk_fn(int ts_mode, int ntc) {
    if (ts_mode == 1) return ntc == 1 ? k_se_chunk<1, 1> : ntc == 6 ? k_se_chunk<1, 6> : k_se_chunk<1, 12>;
    return ntc == 1 ? k_se_chunk<2, 1> : ntc == 6 ? k_se_chunk<2, 6> : k_se_chunk<2, 12>;
}
static decltype(&k_hmc_final<1>) hmc_final_fn(int ntc) { return ntc == 1 ? k_hmc_final<1> : ntc == 6 ? k_hmc_final<6> : k_hmc_final<12>; }
// chunk count at compile time for the BASELINE sizes (NI, UK, SYN), rolled loops otherwise
static decltype(&k_hmc_chunk<0>) hmc_chunk_fn(int ntc) {
    return ntc == 1 ? k_hmc_chunk<1> : ntc == 6 ? k_hmc_chunk<6> : ntc == 12 ? k_hmc_chunk<12> : k_hmc_chunk<0>;
}
// HT / HM: 512-day / 512-row parts of the series and the rows (sampler_create caps T <= 1024, M <= 2048)
static decltype(&k_hmc_step<0, 1, 1>) hmc_step_fn(int stage, const Dims &d) {
    const int ht = (d.Tp + HB - 1) / HB, hm = (d.M + HB - 1) / HB;
#define HMC_STEP(S_) (ht <= 1 ? (hm <= 1 ? k_hmc_step<S_, 1, 1> : hm <= 2 ? k_hmc_step<S_, 1, 2> : k_hmc_step<S_, 1, 4>) \
                              : (hm <= 1 ? k_hmc_step<S_, 2, 1> : hm <= 2 ? k_hmc_step<S_, 2, 2> : k_hmc_step<S_, 2, 4>))
    return stage == 0 ? HMC_STEP(0) : stage == 1 ? HMC_STEP(1) : HMC_STEP(2);
#undef HMC_STEP
}
// The event-update kernels by the day chunks of a row (move_nch) and the sub-move bound of the instance (move_mm): the
// kernels' plain names are the MM_SMALL instances, `_m4` the ones for every m <= MMAX
#define MOVE_FN(K_, mm_, ...) ((mm_) == MM_SMALL ? K_<__VA_ARGS__> : K_##_m4<__VA_ARGS__>)
static decltype(&k_move_pair<6>) move_pair_fn(int nch, int mm) {
    return nch == 6 ? MOVE_FN(k_move_pair, mm, 6) : nch == 12 ? MOVE_FN(k_move_pair, mm, 12) : MOVE_FN(k_move_pair, mm, 16);
}
static decltype(&k_move_pairs<6>) move_pairs_fn(int nch, int mm) {
    return nch == 6 ? MOVE_FN(k_move_pairs, mm, 6) : nch == 12 ? MOVE_FN(k_move_pairs, mm, 12) : MOVE_FN(k_move_pairs, mm, 16);
}
static decltype(&k_move_pa2<6>) move_pa2_fn(int nch, int mm) {
    return nch == 6 ? MOVE_FN(k_move_pa2, mm, 6) : nch == 12 ? MOVE_FN(k_move_pa2, mm, 12) : MOVE_FN(k_move_pa2, mm, 16);
}
static decltype(&k_move_delta<true>) move_delta_fn(bool own, int mm) { return own ? MOVE_FN(k_move_delta, mm, true) : MOVE_FN(k_move_delta, mm, false); }
static decltype(&k_record) record_fn(int mm) { return mm == MM_SMALL ? k_record : k_record_m4; }
static decltype(&k_apply_fpend) apply_fpend_fn(int mm) { return mm == MM_SMALL ? k_apply_fpend : k_apply_fpend_m4; }
#undef MOVE_FN

// seir_sampler_desc::hmc_mode / moves_mode -> the form in force (plan_sweep reads it)
static void apply_launch_form(seir_sampler *s, int hmc_mode, int moves_mode) {
    s->hmc_mode = hmc_mode;
    s->moves_mode = moves_form(moves_mode, s->cfg.n_scans);
}

extern "C" int seir_sampler_create(seir_ctx *ctx, const seir_sampler_desc *ds, seir_sampler **out) {
    if (!ctx || !ds || !out) return fail(SEIR_ERR_INVALID, "null argument");
    *out = nullptr;
    const Dims &d = ctx->d;
    const int B = ds->num_chains;
    if (B < 1 || B > ctx->Bmax) return fail(SEIR_ERR_INVALID, "num_chains=%d outside [1, %d]", B, ctx->Bmax);
    if (ctx->w.K[0]) return fail(SEIR_ERR_STATE, "this context already has a sampler");
    if (d.Tp > 2 * HB || d.M > 4 * HB)
        return fail(SEIR_ERR_INVALID, "sampler supports T <= %d and M <= %d", 2 * HB, 4 * HB);
    if (ds->m < 1 || ds->m > MMAX) return fail(SEIR_ERR_INVALID, "m=%d outside [1, %d]", ds->m, MMAX);
    if (ds->dmax < 1 || ds->nmax < 0 || ds->occult_nmax < 0 || ds->num_event_time_updates < 0)
        return fail(SEIR_ERR_INVALID, "bad dmax/nmax/occult_nmax/num_event_time_updates");
    if (ds->t_range_lo < 0 || ds->t_range_hi > d.T || ds->t_range_lo >= ds->t_range_hi)
        return fail(SEIR_ERR_INVALID, "occult t_range [%d,%d) outside [0,%d)", ds->t_range_lo, ds->t_range_hi, d.T);
    if (ds->num_leapfrog_steps < 1) return fail(SEIR_ERR_INVALID, "num_leapfrog_steps must be >= 1");
    if (ds->trace_capacity < 1) return fail(SEIR_ERR_INVALID, "trace_capacity must be >= 1");
    if (ds->record_events < 0 || ds->record_events > 2) return fail(SEIR_ERR_INVALID, "record_events is 0, 1 or 2");
    if (ds->moves_mode < 0 || ds->moves_mode > 4 || ds->hmc_mode < 0 || ds->hmc_mode > 6)
        return fail(SEIR_ERR_INVALID, "moves_mode is 0..4, hmc_mode 0..6");
    if (ds->disable_mask < 0 || ds->disable_mask > 31) return fail(SEIR_ERR_INVALID, "disable_mask is a 5-bit mask");
    if (ds->leap_rows != 0 && ds->leap_rows != 24 && ds->leap_rows != 32) return fail(SEIR_ERR_INVALID, "leap_rows is 0 (auto), 24 or 32");
    if (ds->thin < 0) return fail(SEIR_ERR_INVALID, "thin must be >= 0 (0 or 1: every sweep is recorded)");
    HIP_TRY(hipSetDevice(ctx->device));
    seir_sampler *s = new (std::nothrow) seir_sampler();
    if (!s) return fail(SEIR_ERR_DEVICE, "out of host memory");
    s->ctx = ctx;
    SamplerCfg &c = s->cfg;
    c.B = B; c.dmax = ds->dmax; c.nmax = ds->nmax; c.mmax = ds->m; c.occult_nmax = ds->occult_nmax;
    c.n_scans = ds->num_event_time_updates; c.tr_lo = ds->t_range_lo; c.tr_hi = ds->t_range_hi;
    c.L = ds->num_leapfrog_steps;
    c.k0 = (uint32_t)(ds->seed & 0xffffffffu); c.k1 = (uint32_t)(ds->seed >> 32);
    c.chain0 = ds->first_chain_id;
    c.adapt_step = 0; c.adapt_mass = 0; c.n_adapt = 0; c.target_accept = 0.75;
    c.cap = ds->trace_capacity;
    c.nrb_d = (d.M + 7) / 8;        // row blocks of k_move_delta (4-row blocks measured slower, twice)
    s->record_events = ds->record_events;
    c.ev16 = ds->record_events == 2 ? 1 : 0;
    // Launch mode of a sweep's ~76 dependent kernels.  Measured on MI355X / ROCm 7.2 (UK-380, 8 chains):
    // stream launches 0.815 ms per sweep, replay of the captured hipGraph 0.872 ms -- the graph
    // executor costs ~0.75 us more per node than the stream path while the host (3-4 us per launch,
    // kernels of ~10 us) stays ahead either way.  Default: stream launches; seir_sampler_desc::use_graph selects the graph.
    s->use_graph = ds->use_graph != 0;
    s->pair_debug = ds->debug_pair;
    s->leap_rows = ds->leap_rows;
    apply_launch_form(s, ds->hmc_mode, ds->moves_mode);
    c.disable_mask = ds->disable_mask;
    c.thin = s->thin_pending = ds->thin < 1 ? 1 : ds->thin;
    {
        int g = ds->chain_groups;    // measured: concurrent chain groups on several streams do not overlap profitably
        if (g < 1) g = 1;
        if (g > B) g = B;
        s->ngroups = g;
        s->gstream.assign(g, nullptr); s->graph.assign(g, nullptr); s->gexec.assign(g, nullptr);
        s->ev_join.assign(g, nullptr);
    }

    int rc = 0;
    Work &w = ctx->w;
    const size_t cells = (size_t)ctx->Bmax * d.Mp * d.Tp;
    Chains &ch = s->ch;
#define S_STATE(ptr, n) S_ALLOC(allocs, ptr, (n), seir_sampler::R_STATE)
#define S_HAND(ptr, n) S_ALLOC(allocs, ptr, (n), seir_sampler::R_HANDOFF)
    for (int x = 0; x < 3; ++x) { S_STATE(w.K[x], cells); S_STATE(w.St[x], cells); }
    S_STATE(w.rowtot, (size_t)ctx->Bmax * 2 * d.Mp);
    S_STATE(w.rngtot, (size_t)ctx->Bmax * 2 * d.Mp);
    S_ALLOC(allocs, w.TS, (size_t)ctx->Bmax * d.nmt * d.ntc * 4);
    S_ALLOC(allocs, w.Lpart0, (size_t)ctx->Bmax * d.nmt * d.ntc);
    S_STATE(w.sp, (size_t)ctx->Bmax * 2 * d.Mp);
    S_STATE(w.gst, (size_t)ctx->Bmax * 2 * GST_N);
    S_STATE(w.Vt, (size_t)ctx->Bmax * d.Tp);
    S_STATE(w.acur, (size_t)ctx->Bmax * d.Tp);
    S_ALLOC(allocs, w.rirc, (size_t)ctx->Bmax * 2 * d.Tp);
    S_STATE(w.CT, (size_t)ctx->Bmax * 2 * CT_MAXC * 4);
    S_STATE(w.CG, (size_t)ctx->Bmax * 2 * CT_MAXC * 2);
    S_STATE(ch.q, (size_t)B * d.Pp); S_STATE(ch.p, (size_t)B * d.Pp); S_STATE(ch.q0, (size_t)B * d.Pp);
    S_STATE(ch.grad, (size_t)B * d.Pp); S_STATE(ch.var, (size_t)B * d.Pp);
    S_STATE(ch.rv_mean, (size_t)B * d.Pp); S_STATE(ch.rv_m2, (size_t)B * d.Pp);
    S_STATE(ch.hs, (size_t)B * NHS);
    S_HAND(ch.mv, (size_t)2 * B);
    S_HAND(ch.fpend, (size_t)B);
    S_HAND(ch.mvfix, (size_t)2 * B);
    S_HAND(ch.mvsel, (size_t)2 * B);
    S_HAND(ch.hand, (size_t)B);
    S_HAND(ch.late, (size_t)2 * B);
    ch.late_fatal = B;
    S_HAND(ch.tail, (size_t)B * TAIL_STRIDE + (size_t)B * TAIL_FLAG_STRIDE);
    S_HAND(ch.leap, (size_t)B * LEAP_CH);
    // k_leap's hand-off words (16 bytes per value, two step parities): the tiles' partial sums and the roles' tables
    S_HAND(ch.llK, (size_t)B * 2 * (d.Mp / 16) * d.Tp);
    S_HAND(ch.llR, (size_t)B * 2 * d.ntc * d.Mp);
    S_HAND(ch.llP, (size_t)B * 2 * d.ntc * (d.Mp / 16));
    S_HAND(ch.llTS, (size_t)B * 2 * d.ntc * (d.Mp / 16) * 4);
    S_HAND(ch.llT, (size_t)B * ((size_t)d.Tp + 2 * (size_t)d.Mp + 8));
    S_HAND(ch.llmv, (size_t)2 * B * 32);
    S_HAND(ch.k0part, (size_t)B * ROLE_SLOTS);
    S_HAND(ch.irl0, (size_t)B);
    S_ALLOC(allocs, ch.stamps, stamps::buffer_words(B));   // developer timelines (stamps.h): the largest family's region
    S_HAND(ch.done, (size_t)B * 2 * TAIL_STRIDE);
    S_HAND(ch.pbar, (size_t)B * PBAR_STRIDE);
    S_HAND(ch.finpart, (size_t)B * ROLE_SLOTS * 4);
    S_HAND(ch.hand2, (size_t)B);
    S_HAND(ch.mvs, (size_t)2 * B);
    S_HAND(ch.DownS, (size_t)2 * B * 2);
    S_HAND(ch.prev, (size_t)2 * B);
    S_HAND(ch.Dpart, (size_t)B * c.nrb_d * 2);
    S_HAND(ch.llD, (size_t)2 * B * c.nrb_d * 2);           // (band workgroups per chain <= nrb_d: plan_sweep)
    S_HAND(ch.Down, (size_t)2 * 2 * B * 2);
    S_STATE(ch.sweep, (size_t)B); S_STATE(ch.slot0, 1);
    S_ALLOC(allocs, ch.tr_theta, (size_t)c.cap * B * d.P);
    {
        char *tre = nullptr;                               // bytes: int32 or uint16 per count
        S_ALLOC(allocs, tre, s->record_events ? (size_t)c.cap * B * d.M * d.T * 3 * (c.ev16 ? 2 : 4) : 4);
        ch.tr_events = tre;
    }
    S_ALLOC(allocs, ch.ev_overflow, 1);
    S_ALLOC(allocs, ch.tr_hmc, (size_t)c.cap * B * 3);
    S_ALLOC(allocs, ch.tr_mv, (size_t)c.cap * B * 4 * NMVTR);
    S_ALLOC(allocs, s->ev_stage, (size_t)B * d.M * d.T * 3);
#undef S_STATE
#undef S_HAND
    if (!rc) {
        // chain state held in the context's own work arrays (written by accepted event updates and by the HMC roles):
        // part of a snapshot too.  Sizes as in create_impl (max_chains chains).
        const size_t Bm = (size_t)ctx->Bmax;
        auto st_ = [&](void *p_, size_t bytes_) { s->regions.push_back({p_, bytes_, seir_sampler::R_STATE}); };
        st_(w.F, cells * sizeof(double));
        st_(w.rowconst, Bm * d.Mp * sizeof(double));
        st_(w.ea, Bm * d.Tp * sizeof(double)); st_(w.eb, Bm * d.Mp * sizeof(double)); st_(w.rir, Bm * d.Tp * sizeof(double));
        st_(w.scal, Bm * NSCAL * sizeof(double)); st_(w.Qs, Bm * d.Mp * sizeof(double));
        st_(w.Kir, Bm * d.Tp * sizeof(double)); st_(w.Dir, Bm * d.Tp * sizeof(double));
        st_(w.constsum, Bm * sizeof(double));
    }
    if (!rc) {
        std::vector<double> ones((size_t)B * d.Pp, 1.0), hs((size_t)B * NHS, 0.0);
        for (int b = 0; b < B; ++b) hs[(size_t)b * NHS + HS_EPS] = 0.1;     // inference.py:325
        hipError_t e = hipMemcpy(ch.var, ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(ch.hs, hs.data(), hs.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = fail(SEIR_ERR_DEVICE, "sampler init copy failed: %s", hipGetErrorString(e));
    }
    if (!rc) {
        hipError_t e = hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_burst, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_copy, hipEventDisableTiming);
        for (int g = 0; g < s->ngroups && e == hipSuccess; ++g) {
            e = hipStreamCreateWithFlags(&s->gstream[g], hipStreamNonBlocking);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_join[g], hipEventDisableTiming);
        }
        if (e != hipSuccess) rc = fail(SEIR_ERR_DEVICE, "sampler stream setup failed: %s", hipGetErrorString(e));
    }
    if (!rc && (HMC_FORMS[ds->hmc_mode].roles || ds->moves_mode == 0 || ds->moves_mode == 2 || ds->moves_mode == 4)) {
        // Do blocks with the same id mod 8 share an XCD here?  (probe_xcd_local)
        if (ctx->xcd_local < 0) ctx->xcd_local = probe_xcd_local(ctx->stream) ? 1 : 0;
        const bool ok = ctx->xcd_local == 1;
        s->xcd_local = ok;
    }
    if (!rc) {
        // What the chip holds, asked once here: a sweep makes no HIP query (it may be under graph capture).  Workgroups
        // per CU of the k_leap instances plan_sweep can choose (a refused query: 0, the launch never fits)
        (void)hipDeviceGetAttribute(&s->cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
        for (int nst = 1; nst <= 2; ++nst)
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&s->leap_occ[nst - 1], leap_fn(chunk_ts_mode(d.Mp), d.ntc, nst), 256, 0) != hipSuccess)
                s->leap_occ[nst - 1] = 0;
        // k_move_pairs asks for more than half a CU's LDS (one workgroup per CU); the other event-update kernels only above
        // the default 64 KB
        // -- for every instance this sampler can come to launch: SEIR_OPT_GENERIC_MOVES may change between two sweeps
        const int nch = move_nch(d.Tp);
        const size_t plds = k_move_pa2_lds_bytes(d);
        s->pairs_lds_attr = true;
        for (int mm : {MM_SMALL, MMAX}) {
            if (mm < move_mm(c.mmax, false)) continue;            // (m > MM_SMALL: the generic instances only)
            s->pairs_lds_attr = lds_attribute((const void *)move_pairs_fn(nch, mm), k_move_pairs_lds_bytes(d)) == hipSuccess && s->pairs_lds_attr;
            for (const void *fn : {(const void *)move_pair_fn(nch, mm), (const void *)move_pa2_fn(nch, mm)})
                (void)lds_attribute(fn, plds);
        }
    }
    if (rc) { seir_sampler_destroy(s); return rc; }
    *out = s;
    return 0;
}

extern "C" int seir_sampler_xcd_local(seir_sampler *s) { return (s && s->xcd_local) ? 1 : 0; }

static int sampler_check(seir_sampler *s) {
    if (!s) return fail(SEIR_ERR_INVALID, "null sampler");
    HIP_TRY(hipSetDevice(s->ctx->device));
    return 0;
}

// Whatever is still queued on the context stream, and a pending copy of a burst.
static int drain(seir_sampler *s) {
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    if (s->copy_pending) { (void)hipEventSynchronize(s->ev_copy); s->copy_pending = false; }
    return 0;
}

// Hand-off scratch back to its initial state, in stream order: every token / counter / in-flight descriptor zero (0 is no
// launch's token) and the host's running totals of the counters with them.  Between two sweeps nothing of it is live
// (a sweep's first launch starts with have_prev = have_pre = 0), so this is always allowed there.
static int reset_handoffs(seir_sampler *s) {
    hipStream_t st = s->ctx->stream;
    for (const auto &r : s->regions)
        if (r.kind == seir_sampler::R_HANDOFF) HIP_TRY(hipMemsetAsync(r.p, 0, r.bytes, st));
    s->leap_rsteps = s->leap_steps = 0;
    s->tail_count = 0;
    s->pbar_count = 0;
    s->poisoned = false;
    return 0;
}

extern "C" int seir_sampler_set_launch_form(seir_sampler *s, int32_t hmc_mode, int32_t moves_mode) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if (moves_mode < 0 || moves_mode > 4 || hmc_mode < 0 || hmc_mode > 6)
        return fail(SEIR_ERR_INVALID, "moves_mode is 0..4, hmc_mode 0..6");
    if (hmc_mode != s->hmc_mode || moves_form(moves_mode, s->cfg.n_scans) != s->moves_mode) {
        HIP_TRY(hipStreamSynchronize(s->ctx->stream));
        drop_graph(s);                               // the captured sweep is one form's launches
        apply_launch_form(s, hmc_mode, moves_mode);
    }
    return 0;
}

extern "C" int seir_sampler_launch_form(seir_sampler *s, int32_t *hmc_mode, int32_t *moves_mode) {
    if (!s) return fail(SEIR_ERR_INVALID, "null sampler");
    if (hmc_mode) *hmc_mode = s->hmc_mode;
    if (moves_mode) *moves_mode = s->moves_mode;
    return 0;
}

static SweepInputs sweep_inputs(const seir_sampler *s, int g);

// the instances the next sweep launches: by the sampler's m and the context's option as they are now
static int sampler_mm(const seir_sampler *s) { return move_mm(s->cfg.mmax, s->ctx->opt_generic_moves != 0); }

extern "C" int seir_move_instance(int32_t m, int32_t generic_moves) {
    if (m < 1 || m > MMAX) return fail(SEIR_ERR_INVALID, "m=%d outside [1, %d]", m, MMAX);
    return move_mm(m, generic_moves != 0);
}

extern "C" int seir_sampler_move_instance(seir_sampler *s, int32_t *mm) {
    if (!s) return fail(SEIR_ERR_INVALID, "null sampler");
    if (!mm) return fail(SEIR_ERR_INVALID, "null pointer");
    *mm = sampler_mm(s);
    return 0;
}

// The plan enqueue_sweep executes for the first chain group, member for member (include/seir_hip.h): host fields only.
extern "C" int seir_sampler_sweep_plan(seir_sampler *s, seir_sweep_plan *out) {
    if (!s) return fail(SEIR_ERR_INVALID, "null sampler");
    if (!out) return fail(SEIR_ERR_INVALID, "null pointer");
    const SweepPlan p = plan_sweep(sweep_inputs(s, 0));
    seir_sweep_plan o{};
    o.hmc = p.hmc; o.inner = p.inner; o.ts_mode = p.ts_mode; o.per = p.per; o.nbv = p.nbv; o.nlive = p.nlive;
    o.end_in_leap = p.end_in_leap; o.chunk_aff = p.chunk_aff; o.final_aff = p.final_aff;
    o.leap_nst = p.leap_nst; o.leap_nmt = p.leap_nmt; o.leap_wgs = p.leap_wgs; o.leap_nbv = p.leap_nbv;
    o.leap_nlive = p.leap_nlive; o.leap_launches = p.leap_launches;
    o.section_launches = p.section_launches; o.section_evals = p.section_evals;
    o.moves = p.moves; o.nband = p.nband; o.nbk = p.nbk; o.pair_nlive = p.pair_nlive; o.nch = p.nch; o.fpend = p.fpend;
    o.pre = p.pre; o.move_aff = p.move_aff; o.record = p.record; o.advance = p.advance;
    *out = o;
    return 0;
}

// Test hook: what a timed-out wait leaves behind -- chain `chain`'s fatal counter raised, in stream order.  Every wait of
// that chain then gives up at its first look at the counter (a wait that is served within 256 polls still completes) and
// the next read of the trace reports the time-out.
extern "C" int seir_sampler_debug_fail_handoff(seir_sampler *s, int32_t chain) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if (chain < 0 || chain >= s->cfg.B) return fail(SEIR_ERR_INVALID, "chain %d outside [0, %d)", chain, s->cfg.B);
    static const uint32_t one = 1u;
    HIP_TRY(hipMemcpyAsync(s->ch.late + s->ch.late_fatal + chain, &one, sizeof(one), hipMemcpyHostToDevice, s->ctx->stream));
    return 0;
}

// While a feature is enabled a snapshot also holds its accumulators (device copies in stream order), so that a burst can
// be folded as soon as it is enqueued and a burst that is run again after a hand-off time-out is not counted twice: the
// moments, count and flag of the summaries; with them the diagnostics' batch sums and marks (a mark taken in a burst that is
// thrown away goes with it); the forecast's moments and its draw counter; the reproduction number's moments and count; the
// check's moments, comparison counts, obs, flags and its draw counter; the within/between shares' accumulators and count.
static size_t summary_cells(const seir_sampler *s) { return (size_t)s->cfg.B * s->ctx->d.M * s->ctx->d.T * seir::SUMMARY_Q; }
static size_t diag_words(const seir_sampler *s) { return 6 * summary_cells(s) + 3 * (size_t)s->cfg.B; }
static uint64_t *diag_mark(const seir_sampler *s, int which) {       // count [B] | sum [n] | sumsq [n]
    const size_t n = summary_cells(s), B = (size_t)s->cfg.B;
    return s->diag_buf.buf.as<uint64_t>() + 2 * n + B + (size_t)which * (B + 2 * n);
}
static int moments_shadow(seir_sampler *s, int slot, bool save) {
    hipStream_t st = s->ctx->stream;
    int rc = 0;
    if (s->sum_on) {
        if (s->diag_on) rc = acc_shadow(s->diag_buf, slot, save, st);
        if (!rc) rc = acc_shadow(s->sum_acc, slot, save, st);
    }
    if (!rc && s->fc.on) rc = counted_shadow(s->fc.acc, slot, save, st);
    if (!rc && s->fc.on && s->scen.K) rc = acc_shadow(s->scen.acc, slot, save, st);   // their count is the forecast's j
    if (!rc && s->fc.on && s->scen.K && s->scen.triggered()) rc = acc_shadow(s->scen.tacc, slot, save, st);
    if (!rc && s->fc.on && s->ver.on) rc = acc_shadow(s->ver.acc, slot, save, st);    // and so is the verification's
    if (!rc && s->rt.on) rc = counted_shadow(s->rt.acc, slot, save, st);
    if (!rc && s->ck.on) {
        rc = counted_shadow(s->ck.acc, slot, save, st);
        if (!rc) rc = acc_shadow(s->ck_cnt, slot, save, st);
    }
    if (!rc && s->wb.on) rc = counted_shadow(s->wb.acc, slot, save, st);
    return rc;
}

extern "C" int seir_sampler_snapshot(seir_sampler *s, int32_t slot) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if (slot < 0 || slot > 1) return fail(SEIR_ERR_INVALID, "snapshot slot is 0 or 1");
    if (!s->have_state) return fail(SEIR_ERR_STATE, "no chain state set");
    if (s->poisoned) return fail(SEIR_ERR_STATE, "the sampler's state is unreliable (hand-off time-out): nothing to snapshot");
    if (!s->snap_bytes)
        for (const auto &r : s->regions)
            if (r.kind == seir_sampler::R_STATE) s->snap_bytes += (r.bytes + 255) / 256 * 256;
    if (!s->snap[slot] && (rc = s->snap[slot].alloc(s->snap_bytes))) return rc;
    // in stream order: the snapshot is the state after everything queued so far
    size_t off = 0;
    for (const auto &r : s->regions)
        if (r.kind == seir_sampler::R_STATE) {
            HIP_TRY(hipMemcpyAsync(s->snap[slot].as<char>() + off, r.p, r.bytes, hipMemcpyDeviceToDevice, s->ctx->stream));
            off += (r.bytes + 255) / 256 * 256;
        }
    s->snap_valid[slot] = true;
    return moments_shadow(s, slot, true);
}

extern "C" int seir_sampler_restore(seir_sampler *s, int32_t slot) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if (slot < 0 || slot > 1) return fail(SEIR_ERR_INVALID, "snapshot slot is 0 or 1");
    if (!s->snap_valid[slot] || !s->snap[slot]) return fail(SEIR_ERR_STATE, "no snapshot in slot %d", slot);
    hipStream_t st = s->ctx->stream;
    // whatever is still queued (the rest of a failed burst: its waits give up at their first look at the chain's time-out
    // counter, so it drains quickly) and the copy of a burst that nobody wants any more
    if ((rc = drain(s))) return rc;
    size_t off = 0;
    for (const auto &r : s->regions)
        if (r.kind == seir_sampler::R_STATE) {
            HIP_TRY(hipMemcpyAsync(r.p, s->snap[slot].as<const char>() + off, r.bytes, hipMemcpyDeviceToDevice, st));
            off += (r.bytes + 255) / 256 * 256;
        }
    if ((rc = reset_handoffs(s))) return rc;
    if ((rc = moments_shadow(s, slot, false))) return rc;
    s->vt_dirty = true;                              // Work::Vt came back with the snapshot, the flag did not
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// What is on, how it is sized, how far it has counted (include/seir_hip.h): host fields only, a poisoned sampler answers too.
extern "C" int seir_sampler_product_state(seir_sampler *s, seir_product_state *out) {
    if (!s) return fail(SEIR_ERR_INVALID, "null sampler");
    if (!out) return fail(SEIR_ERR_INVALID, "null pointer");
    seir_product_state p{};
    p.summary_on = s->sum_on;
    p.diag_batch_len = s->diag_on ? (int32_t)s->diag.L : 0;
    p.forecast_H = s->fc.on ? s->fc.fb.H : 0;
    p.check_K = s->ck.on ? s->ck.fb.H : 0;
    p.rt_D = s->rt.on ? s->rt.D : 0;
    p.wb_D = s->wb.on ? s->wb.D : 0;
    p.groups_G = s->grp_on ? s->grp.G : 0;
    p.groups_nnz = s->grp_on && !s->grp_offsets.empty() ? s->grp_offsets.back() : 0;
    for (int which = 0; which < 3; ++which) p.group_L[which] = s->grp_out[which].L;
    p.group_rt_on = s->rt.curve.on;
    p.group_wb_on = s->wb.curve.on;
    p.group_rt_D = s->rt.curve.b.D;
    p.group_wb_D = s->wb.curve.b.D;
    p.ngm_D = s->ngm.D;
    p.fc_j = s->fc.acc.j;
    p.ck_j = s->ck.acc.j;
    p.rt_j = s->rt.acc.j;
    p.ngm_cap = s->ngm.cap;
    p.fc_keep_cap = s->keep_fc.cap;
    p.rt_keep_cap = s->keep_rt.cap;
    *out = p;
    return 0;
}

static void enqueue_refresh(seir_sampler *s) {
    seir_ctx *ctx = s->ctx;
    const Dims &d = ctx->d;
    const int B = s->cfg.B;
    launch_scan<1>(ctx, whole(ctx, B), nullptr);
    hipLaunchKernelGGL(k_range_totals, dim3((d.M + 3) / 4, B), dim3(256), 0, ctx->stream, d, ctx->w, s->cfg);
    launch_colreduce(ctx, whole(ctx, B));
    launch_gemm(ctx, whole(ctx, B));
    hipLaunchKernelGGL(k_chain_tables, dim3(B), dim3(256), 0, ctx->stream, d, ctx->c, ctx->w, s->ch);
    launch_se<1>(ctx, whole(ctx, B), false);
    hipLaunchKernelGGL(k_chain_refresh, dim3(B), dim3(256), (size_t)d.Tp * sizeof(double), ctx->stream, d, ctx->c,
                       ctx->w, s->ch);
}

extern "C" int seir_sampler_refresh(seir_sampler *s) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if (!s->have_state) return fail(SEIR_ERR_STATE, "no chain state set");
    if (s->poisoned) {
        HIP_TRY(hipStreamSynchronize(s->ctx->stream));
        if ((rc = reset_handoffs(s))) return rc;
    }
    enqueue_refresh(s);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int seir_sampler_set_state(seir_sampler *s, const double *u, const double *events) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if (!u || !events) return fail(SEIR_ERR_INVALID, "null pointer");
    seir_ctx *ctx = s->ctx;
    const Dims &d = ctx->d;
    const int B = s->cfg.B;
    for (size_t i = 0, n = (size_t)B * d.M * d.T * 3; i < n; ++i)
        if (!(events[i] >= 0.0 && events[i] < 2147483648.0 && events[i] == std::floor(events[i])))
            return fail(SEIR_ERR_INVALID, "events[%zu]=%g is not a non-negative integer count", i, events[i]);
    HIP_TRY(hipMemcpyAsync(s->ch.q, u, sizeof(double) * B * d.P, hipMemcpyHostToDevice, ctx->stream));
    // Chains::q0 = the position at the start of the next trajectory, kept equal to q between trajectories (k_hmc_step<2>
    // leaves it so): the folded first step reads the start point from it while its roles already write the next one to q
    HIP_TRY(hipMemcpyAsync(s->ch.q0, u, sizeof(double) * B * d.P, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(s->ev_stage, events, sizeof(double) * B * d.M * d.T * 3, hipMemcpyHostToDevice,
                           ctx->stream));
    hipLaunchKernelGGL(k_import_events, dim3(1024), dim3(256), 0, ctx->stream, d, ctx->w, s->ev_stage, B);
    s->have_state = true;
    if (s->poisoned && (rc = reset_handoffs(s))) return rc;
    enqueue_refresh(s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int seir_sampler_get_state(seir_sampler *s, double *u, double *events, double *logp) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if (!s->have_state) return fail(SEIR_ERR_STATE, "no chain state set");
    seir_ctx *ctx = s->ctx;
    const Dims &d = ctx->d;
    const int B = s->cfg.B;
    if (u) HIP_TRY(hipMemcpyAsync(u, s->ch.q, sizeof(double) * B * d.P, hipMemcpyDeviceToHost, ctx->stream));
    if (events) {
        hipLaunchKernelGGL(k_export_events, dim3(1024), dim3(256), 0, ctx->stream, d, ctx->w, s->ev_stage, B);
        HIP_TRY(hipMemcpyAsync(events, s->ev_stage, sizeof(double) * B * d.M * d.T * 3, hipMemcpyDeviceToHost,
                               ctx->stream));
    }
    std::vector<double> hs;
    if (logp) {
        hs.resize((size_t)B * NHS);
        HIP_TRY(hipMemcpyAsync(hs.data(), s->ch.hs, sizeof(double) * B * NHS, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (logp)
        for (int b = 0; b < B; ++b) logp[b] = hs[(size_t)b * NHS + HS_LP_THETA] + hs[(size_t)b * NHS + HS_LP_CONST];
    return 0;
}

static int hs_update(seir_sampler *s, const std::vector<std::pair<int, const double *>> &cols) {
    const int B = s->cfg.B;
    std::vector<double> hs((size_t)B * NHS);
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    HIP_TRY(hipMemcpy(hs.data(), s->ch.hs, sizeof(double) * B * NHS, hipMemcpyDeviceToHost));
    for (auto &c : cols)
        for (int b = 0; b < B; ++b) hs[(size_t)b * NHS + c.first] = c.second[b];
    HIP_TRY(hipMemcpy(s->ch.hs, hs.data(), sizeof(double) * B * NHS, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int seir_sampler_set_kernel(seir_sampler *s, const double *step_size, const double *variance) {
    int rc = sampler_check(s);
    if (rc) return rc;
    const Dims &d = s->ctx->d;
    const int B = s->cfg.B;
    if (step_size) {
        for (int b = 0; b < B; ++b)
            if (!(step_size[b] > 0.0)) return fail(SEIR_ERR_INVALID, "step_size[%d] must be positive", b);
        if ((rc = hs_update(s, {{HS_EPS, step_size}}))) return rc;
    }
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    if (variance) {
        for (size_t i = 0; i < (size_t)B * d.P; ++i)
            if (!(variance[i] > 0.0)) return fail(SEIR_ERR_INVALID, "variance[%zu] must be positive", i);
        HIP_TRY(hipMemcpy(s->ch.var, variance, sizeof(double) * B * d.P, hipMemcpyHostToDevice));
        s->vt_dirty = true;
    } else {
        std::vector<double> ones((size_t)B * d.P, 1.0);
        HIP_TRY(hipMemcpy(s->ch.var, ones.data(), sizeof(double) * B * d.P, hipMemcpyHostToDevice));
        s->vt_dirty = true;
    }
    return 0;
}

extern "C" int seir_sampler_get_kernel(seir_sampler *s, double *step_size, double *variance) {
    int rc = sampler_check(s);
    if (rc) return rc;
    const Dims &d = s->ctx->d;
    const int B = s->cfg.B;
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    if (step_size) {
        std::vector<double> hs((size_t)B * NHS);
        HIP_TRY(hipMemcpy(hs.data(), s->ch.hs, sizeof(double) * B * NHS, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b) step_size[b] = hs[(size_t)b * NHS + HS_EPS];
    }
    if (variance) HIP_TRY(hipMemcpy(variance, s->ch.var, sizeof(double) * B * d.P, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int seir_sampler_set_adaptation(seir_sampler *s, int32_t adapt_step, int32_t adapt_mass, int32_t n_adapt,
                                           double target, const double *rv_count, const double *rv_mean,
                                           const double *rv_var) {
    int rc = sampler_check(s);
    if (rc) return rc;
    const Dims &d = s->ctx->d;
    const int B = s->cfg.B;
    if (adapt_mass && (!rv_count || !rv_mean || !rv_var))
        return fail(SEIR_ERR_INVALID, "adapt_mass needs the initial running variance");
    if (adapt_step && !(target > 0.0 && target < 1.0)) return fail(SEIR_ERR_INVALID, "target_accept_prob in (0,1)");
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    std::vector<double> hs((size_t)B * NHS);
    HIP_TRY(hipMemcpy(hs.data(), s->ch.hs, sizeof(double) * B * NHS, hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b) {
        double *h = hs.data() + (size_t)b * NHS;
        // a fresh DualAveragingStepSizeAdaptation: error_sum 0, step 0, log_averaging_step 0,
        // shrinkage target log(10 * current step size)
        h[HS_DA_ERR] = 0.0; h[HS_DA_STEP] = 0.0; h[HS_DA_LOGAVG] = 0.0;
        h[HS_DA_MU] = std::log(10.0 * h[HS_EPS]);
        if (adapt_mass) h[HS_RV_N] = rv_count[b];
    }
    HIP_TRY(hipMemcpy(s->ch.hs, hs.data(), sizeof(double) * B * NHS, hipMemcpyHostToDevice));
    if (adapt_mass) {
        std::vector<double> m2((size_t)B * d.P);
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < d.P; ++i) {
                const double v = rv_var[(size_t)b * d.P + i];
                if (!(v > 0.0)) return fail(SEIR_ERR_INVALID, "running variance must be positive");
                m2[(size_t)b * d.P + i] = v * rv_count[b];
            }
        HIP_TRY(hipMemcpy(s->ch.rv_mean, rv_mean, sizeof(double) * B * d.P, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(s->ch.rv_m2, m2.data(), sizeof(double) * B * d.P, hipMemcpyHostToDevice));
        // momentum distribution at bootstrap: the initial running variance
        HIP_TRY(hipMemcpy(s->ch.var, rv_var, sizeof(double) * B * d.P, hipMemcpyHostToDevice));
    }
    SamplerCfg &c = s->cfg;
    if (c.adapt_step != adapt_step || c.adapt_mass != adapt_mass || c.n_adapt != n_adapt ||
        c.target_accept != target)
        drop_graph(s);                               // kernel arguments are baked into the graph
    c.adapt_step = adapt_step; c.adapt_mass = adapt_mass; c.n_adapt = n_adapt; c.target_accept = target;
    s->vt_dirty = true;                              // the variances may have moved since Work::Vt was last formed (k_vt)
    return 0;
}

// A thinning interval set since the last reset comes into force: the sweeps enqueued so far carry the old one in their
// kernel arguments, the ones enqueued from here on the new one, and slot0 is written for it by the caller
static int drop_graph_for_thin(seir_sampler *s) {
    bool captured = false;
    for (auto g : s->gexec) captured = captured || g != nullptr;
    if (!captured) return 0;
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));   // its replays have finished (as seir_sampler_set_launch_form waits)
    drop_graph(s);                                   // kernel arguments are baked into the graph
    return 0;
}
static int apply_pending_thin(seir_sampler *s) {
    if (s->cfg.thin == s->thin_pending) return 0;
    int rc = drop_graph_for_thin(s);
    if (rc) return rc;
    s->cfg.thin = s->thin_pending;
    return 0;
}

extern "C" int seir_sampler_set_thin(seir_sampler *s, int32_t thin) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if (thin < 0) return fail(SEIR_ERR_INVALID, "thin must be >= 0 (0 or 1: every sweep is recorded)");
    s->thin_pending = thin < 1 ? 1 : thin;
    return s->thin_pending != s->cfg.thin ? drop_graph_for_thin(s) : 0;
}

extern "C" int seir_sampler_thin(seir_sampler *s, int32_t *thin) {
    if (!s) return fail(SEIR_ERR_INVALID, "null sampler");
    if (thin) *thin = s->thin_pending;
    return 0;
}

extern "C" int seir_sampler_reset_trace(seir_sampler *s) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = apply_pending_thin(s))) return rc;
    // slot0 = sweep counter of chain 0 (all chains advance together): first slot 0, whatever the thinning interval
    HIP_TRY(hipMemcpyAsync(s->ch.slot0, s->ch.sweep, sizeof(unsigned), hipMemcpyDeviceToDevice, s->ctx->stream));
    return 0;
}

extern "C" int seir_sampler_reset_trace_at(seir_sampler *s, int32_t first_slot) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if (first_slot < 0 || first_slot >= s->cfg.cap)
        return fail(SEIR_ERR_INVALID, "first_slot %d outside [0, %d)", first_slot, s->cfg.cap);
    if ((rc = apply_pending_thin(s))) return rc;
    hipLaunchKernelGGL(k_set_slot0, dim3(1), dim3(1), 0, s->ctx->stream, s->ch, (unsigned)first_slot, (unsigned)s->cfg.thin);
    HIP_TRY(hipGetLastError());
    return 0;
}

static void launch_hmc(seir_ctx *ctx, const LaunchCfg &l, const SamplerCfg &c, const Chains &ch, int stage,
                       int gather_qs = 0) {
    hipLaunchKernelGGL(hmc_step_fn(stage, l.d), dim3(l.nb), dim3(HB), (size_t)l.d.Mp * sizeof(double), l.st, l.d, ctx->c, ctx->w, c, ch, gather_qs);
}

// chains [b0, b0+nb) of group g
static void group_range(const seir_sampler *s, int g, int &b0, int &nb) {
    const int B = s->cfg.B, G = s->ngroups;
    b0 = (int)((long long)B * g / G);
    nb = (int)((long long)B * (g + 1) / G) - b0;
}

// what plan_sweep reads for group g's sweep
static SweepInputs sweep_inputs(const seir_sampler *s, int g) {
    const Dims &d = s->ctx->d;
    const SamplerCfg &c = s->cfg;
    int b0, nb;
    group_range(s, g, b0, nb);
    return {d.M, d.Mp, d.Tp, d.ntc, d.nmt, c.nrb_d,
            nb, c.L, c.n_scans, s->record_events,
            s->hmc_mode, s->moves_mode, s->leap_rows,
            s->xcd_local, s->ngroups == 1, s->use_graph, s->ctx->opt_affinity,
            s->cus, s->leap_occ[0], s->leap_occ[1], s->pairs_lds_attr};
}

// Group g's sweep: the launches of its plan, with the hand-off counters the host keeps for them
static void enqueue_sweep(seir_sampler *s, int g) {
    seir_ctx *ctx = s->ctx;
    const SamplerCfg &c = s->cfg;
    const SweepPlan p = plan_sweep(sweep_inputs(s, g));
    int b0, nb;
    group_range(s, g, b0, nb);
    LaunchCfg l{ctx->d, s->gstream[g], nb, ctx->opt_affinity};
    l.d.b0 = b0;
    l.d.skew = ctx->opt_skew;
    const Dims d0 = l.d;
    hipStream_t st = l.st;
    const int ntile = d0.ntc * d0.nmt;
    // seir_sampler_time_leapfrog: HIP events around the leapfrog section (end = 1 closes the pair)
    const bool prof = s->prof_i >= 0 && (size_t)(2 * s->prof_i + 1) < s->prof_ev.size() && g == 0;
    auto prof_mark = [&](int end) {
        if (prof) (void)hipEventRecord(s->prof_ev[2 * s->prof_i + end], st);
        if (prof) s->prof_i += end;
    };
    auto vt = [&] {     // Work::Vt to Chains::var where it does not match (set_kernel / set_adaptation / creation, mass adaptation)
        if (s->vt_dirty || c.adapt_mass) hipLaunchKernelGGL(k_vt, dim3(nb), dim3(WAVE), 0, st, l.d, ctx->w, s->ch);
        s->vt_dirty = false;
    };
    auto launch_leap = [&](int par0, int nsteps, int fold) {
        Dims df = l.d;
        df.aff_nb = p.leap_nbv;
        df.nlive = p.leap_nlive;
        df.sp_par = 0;
        df.chunked = p.ts_mode;
        df.nmt = p.leap_nmt;                                     // the partial sums of this launch: one set per row tile of ITS shape
        const dim3 gf((unsigned)((p.leap_wgs + p.per) * p.leap_nbv));
        // (every chain's counters and hand-off words count its OWN launches: the sub-batches of a sweep share the step numbers)
        const unsigned long long step_base = s->leap_steps, role_base = s->leap_rsteps;
        s->leap_steps += (unsigned long long)nsteps;
        s->leap_rsteps += (unsigned long long)(nsteps - (((fold & 2) && !(fold & 4)) ? 1 : 0));
        for (int sub = 0; sub < p.leap_launches; ++sub) {
            df.b0 = l.d.b0 + sub * p.leap_nbv;
            void *args[] = {(void *)&df, (void *)&ctx->c, (void *)&ctx->w, (void *)&c, (void *)&s->ch, (void *)&par0, (void *)&nsteps,
                            (void *)&step_base, (void *)&role_base, (void *)&fold};
            (void)hipLaunchKernel(leap_fn(p.ts_mode, d0.ntc, p.leap_nst), gf, dim3(256), args, 0, st);
        }
    };
    // steps it0..it1 of the trajectory as k_se_chunk launches (tiles, then the chunk roles) from buffer par; with `ends`, the
    // roles also do the trajectory's first step (momentum draw, half kick: traj 1), the step after it (2) and the last half
    // kick (3).  Returns the buffer the last step wrote.
    auto se_chunk_steps = [&](int it0, int it1, int par, bool ends) {
        Dims df = l.d;
        df.aff_nb = p.nbv;
        df.nlive = p.nlive;
        df.chunked = p.ts_mode;
        for (int it = it0; it <= it1; ++it) {
            const int traj = !ends ? 0 : it == 0 ? 1 : it == 1 ? 2 : it == c.L ? 3 : 0;
            df.sp_par = par;
            Work wf = ctx->w;
            if (it == 0) wf.Lpart = wf.Lpart0;                    // the start point's value of the S->E term: kept for the accept test
            s->tail_count += (unsigned long long)ntile;           // what a chain's counter shows once this launch's tiles are in
            const unsigned long long target = s->tail_count;
            hipLaunchKernelGGL(se_chunk_fn(p.ts_mode, d0.ntc), dim3((unsigned)((ntile + p.per) * p.nbv)), dim3(256), 0, st, df, ctx->c, wf,
                               c, s->ch, par, target, traj);
            if (it < c.L) par ^= 1;
        }
        return par;
    };
    // [part 0] HMC on u | events: L+1 gradient evaluations
    l.d.sp_par = 0;
    if (p.hmc == SweepPlan::FOLD) {
        // The whole trajectory in ONE launch: gradient at the start point, the first step (momentum draw, half kick, drift:
        // k_hmc_step<0>'s work, by the chunk roles), the L-1 inner steps, gradient at the end point, and the end itself (half
        // kick, accept test, adaptation, trace: by the roles as well, or -- hmc_mode 5 -- by k_hmc_step<2> as a launch of its
        // own).  L+1 gradient evaluations, L (+1) role steps.
        vt();
        prof_mark(0);
        launch_leap(1, c.L + 1, p.end_in_leap ? 7 : 3);
        prof_mark(1);
        if (!p.end_in_leap) {
            l.d.sp_par = c.L & 1 ? 0 : 1;       // the buffer the last role step wrote: steps alternate from buffer 1
            l.d.chunked = 0;
            l.d.nmt = p.leap_nmt;               // the end point's partial sums are k_leap's: its row tiles
            launch_hmc(ctx, l, c, s->ch, 2, /*gather_qs=*/3);
            l.d.nmt = d0.nmt;
        }
    } else if (p.hmc == SweepPlan::TAILFOLD) {
        // The whole trajectory as L + 1 launches of k_se_chunk whose roles also do its first step and last half kick, then
        // the accept test, adaptation and trace by the roles' own launch (k_hmc_final): what k_se, k_hmc_step<0>, ..., k_se,
        // k_hmc_step<2> do in the stage form, and what k_leap's roles do inside the persistent launch.  Buffers alternate
        // from 1, as there.
        vt();
        int par = 1;
        if (p.ts_mode == 2) hipLaunchKernelGGL(k_sp_prep, dim3(nb), dim3(256), 0, st, l.d, ctx->w, s->ch, par);
        prof_mark(0);
        par = se_chunk_steps(0, c.L, par, true);
        Dims dz = l.d;
        dz.aff_nb = p.final_aff ? nb : 0;
        hipLaunchKernelGGL(hmc_final_fn(d0.ntc), p.final_aff ? dim3(p.per * nb) : dim3(p.per, nb), dim3(WAVE), 0, st, dz, ctx->c, ctx->w, c, s->ch, par);
        prof_mark(1);
    } else {
        l.d.chunked = 0;                       // k_se writes tile scalars only ahead of a chunked step
        launch_se<1>(ctx, l, true);
        l.d.chunked = p.ts_mode;               // stage 0 hands the trajectory over to the chunk kernel
        launch_hmc(ctx, l, c, s->ch, 0);
        s->vt_dirty = false;                   // (k_hmc_step<0> writes Work::Vt on its way)
        if (p.inner == SweepPlan::SINGLE) {
            for (int i = 1; i < c.L; ++i) {
                launch_se<1>(ctx, l, true);
                launch_hmc(ctx, l, c, s->ch, 1);
            }
        } else {
            // the inner steps 1..L-1 by the chunk roles; stage 2 then gathers (Q s) and computes the priors and the
            // Jacobian of the end point itself (gather_qs = 3)
            int par = 0;
            prof_mark(0);
            if (p.inner == SweepPlan::LEAP) {
                launch_leap(par, c.L - 1, 0);
                par = (c.L - 1) & 1;
            } else if (p.inner == SweepPlan::SE_CHUNK) {
                par = se_chunk_steps(1, c.L - 1, par, false);
            } else {
                for (int i = 1; i < c.L; ++i) {
                    l.d.sp_par = par;
                    launch_se<1>(ctx, l, true);
                    Dims dc = l.d;
                    dc.aff_nb = p.chunk_aff ? nb : 0;
                    hipLaunchKernelGGL(hmc_chunk_fn(d0.ntc), p.chunk_aff ? dim3(p.per * nb) : dim3(p.per, nb), dim3(WAVE), 0, st, dc, ctx->c, ctx->w, c, s->ch, par);
                    par ^= 1;
                }
            }
            l.d.sp_par = par;
            prof_mark(1);
        }
        l.d.chunked = 0;
        launch_se<1>(ctx, l, true);
        launch_hmc(ctx, l, c, s->ch, 2, /*gather_qs=*/p.inner == SweepPlan::SINGLE ? 0 : 3);
    }
    // [part 1] MultiScan(n_scans, Gibbs[move S->E, move E->I, occult S->E, occult E->I]):
    // per update [finalize previous | propose] then the log-ratio over the touched cells
    Dims d = l.d;
    d.aff_nb = p.move_aff ? nb : 0;
    const dim3 gm = p.move_aff ? dim3(c.nrb_d * nb) : dim3(c.nrb_d, nb);
    const size_t plds = k_move_pa2_lds_bytes(d);
    const int mm = sampler_mm(s);                                // the instances of every event-update kernel below
    int have_prev = 0, pbuf = 0;
    if (p.moves == SweepPlan::SPLIT_MOVES) {
        const auto pa2_fn = move_pa2_fn(p.nch, mm);
        for (int scan = 0; scan < c.n_scans; ++scan)
            for (int slot = 0; slot < 4; ++slot) {
                const MoveSpec spec{slot >= 2 ? 1 : 0, slot & 1, slot, scan};
                hipLaunchKernelGGL(pa2_fn, gm, dim3(MVB), plds, st, d, ctx->c, ctx->w, c, s->ch, spec,
                                   have_prev, pbuf);
                pbuf ^= 1;
                hipLaunchKernelGGL(move_delta_fn(true, mm), gm, dim3(DELTA_THREADS), 0, st, d, ctx->c, ctx->w, c, s->ch, pbuf, 0);
                have_prev = 1;
            }
        if (have_prev) {
            // closing launch: finalize the last proposal and advance the sweep counter
            const MoveSpec none{-2, 0, 0, 0};
            hipLaunchKernelGGL(pa2_fn, gm, dim3(MVB), plds, st, d, ctx->c, ctx->w, c, s->ch, none, 1, pbuf);
        }
    } else {
        // paired form: [finalize pending E->I-type | whole S->E-type update | propose E->I-type], then the log-ratio of the
        // E->I-type proposal over its band -- by k_move_delta, or by the band workgroups of the pair launch itself
        // (XCD-local hand-off, see pair_band_block)
        const int npairs = 2 * c.n_scans;
        const auto pair_fn = move_pair_fn(p.nch, mm);
        Dims dp = d;
        dp.nlive = p.pair_nlive;
        SamplerCfg cp = c;
        if (p.nband) cp.nrb_d = p.nband;                             // the band's partial sums: one pair per band workgroup
        if (p.moves == SweepPlan::PAIRS) {
            // every pair of the sweep and the closing step in ONE launch, resident for the whole sweep (its closing step
            // also does what k_apply_fpend / k_record are launched for in the other forms)
            hipLaunchKernelGGL(move_pairs_fn(p.nch, mm), dim3((3 + p.nband) * p.nbk), dim3(MVB), k_move_pairs_lds_bytes(d), st, dp, ctx->c, ctx->w, cp,
                               s->ch, npairs, 1, p.nbk, s->pair_debug, p.nband, band_rows(d.M, p.nband), s->pbar_count, s->record_events ? 3 : 1);
            s->pbar_count += (unsigned)(npairs * 3);                 // what every live chain's counter shows after this launch: the roles' arrivals
        } else {
            int have_pre = 0;
            for (int scan = 0; scan < c.n_scans; ++scan)
                for (int half = 0; half < 2; ++half) {
                    const int pair = 2 * scan + half;
                    const MoveSpec se{half, 0, 2 * half, scan}, nx{half, 1, 2 * half + 1, scan};
                    // a third role pre-draws the S->E-type proposal of the next pair (same sweep)
                    const bool pre = p.pre && pair + 1 < npairs;
                    const int nh = (half + 1) & 1, nscan = scan + (half == 1 ? 1 : 0);
                    const MoveSpec se_next = pre ? MoveSpec{nh, 0, 2 * nh, nscan} : MoveSpec{-1, 0, 0, 0};
                    hipLaunchKernelGGL(pair_fn, dim3(((pre ? 3 : 2) + p.nband) * p.nbk), dim3(MVB), plds, st, dp, ctx->c, ctx->w, cp,
                                       s->ch, se, nx, se_next, have_prev, have_pre, pbuf, p.nbk, pair, s->pair_debug, p.nband, band_rows(d.M, p.nband));
                    have_pre = pre ? 1 : 0;
                    pbuf ^= 1;
                    if (!p.nband)
                        hipLaunchKernelGGL(move_delta_fn(false, mm), gm, dim3(DELTA_THREADS), 0, st, d, ctx->c, ctx->w, c, s->ch, pbuf, 1);
                    have_prev = 1;
                }
            if (have_prev) {
                const MoveSpec none{-1, 0, 0, 0}, close{-2, 0, 0, 0};
                hipLaunchKernelGGL(pair_fn, dim3(nb), dim3(MVB), plds, st, d, ctx->c, ctx->w, cp, s->ch, none, close, none, 1,
                                   0, pbuf, nb, 62, 0, 0, 0);
                if (p.fpend == SweepPlan::F_APPLY) hipLaunchKernelGGL(apply_fpend_fn(mm), gm, dim3(256), 0, st, d, ctx->c, ctx->w, c, s->ch);
            }
        }
    }
    d.aff_nb = 0;
    if (p.record)
        hipLaunchKernelGGL(record_fn(mm), dim3((d.M + 3) / 4, nb), dim3(256), 0, st, d, ctx->c, ctx->w, c, s->ch, p.advance ? 0 : 1,
                           p.fpend == SweepPlan::F_RECORD ? 1 : 0);
    if (p.advance) hipLaunchKernelGGL(k_advance, dim3((nb + 63) / 64), dim3(64), 0, st, s->ch, b0, nb);
}

static int check_handoffs(seir_sampler *s);
extern "C" int seir_sampler_run(seir_sampler *s, int32_t n) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if (!s->have_state) return fail(SEIR_ERR_STATE, "no chain state set");
    if (n < 0) return fail(SEIR_ERR_INVALID, "num_sweeps must be >= 0");
    if (s->poisoned) return check_handoffs(s);       // sticky: see there
    hipStream_t main_st = s->ctx->stream;
    // fork: every group stream starts after what is already queued on the context stream
    HIP_TRY(hipEventRecord(s->ev_fork, main_st));
    for (int g = 0; g < s->ngroups; ++g) {
        hipStream_t st = s->gstream[g];
        HIP_TRY(hipStreamWaitEvent(st, s->ev_fork, 0));
        if (s->use_graph && (s->graph_skew != s->ctx->opt_skew || s->graph_aff != s->ctx->opt_affinity || s->graph_mm != sampler_mm(s))) {
            drop_graph(s);                           // launch options are baked into the captured kernels
            s->graph_skew = s->ctx->opt_skew; s->graph_aff = s->ctx->opt_affinity; s->graph_mm = sampler_mm(s);
        }
        if (s->use_graph && !s->gexec[g]) {
            HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
            enqueue_sweep(s, g);
            HIP_TRY(hipStreamEndCapture(st, &s->graph[g]));
            HIP_TRY(hipGraphInstantiate(&s->gexec[g], s->graph[g], nullptr, nullptr, 0));
        }
    }
    for (int i = 0; i < n; ++i)
        for (int g = 0; g < s->ngroups; ++g) {
            if (s->use_graph) HIP_TRY(hipGraphLaunch(s->gexec[g], s->gstream[g]));
            else enqueue_sweep(s, g);
        }
    // join: the context stream continues after every group has finished
    for (int g = 0; g < s->ngroups; ++g) {
        HIP_TRY(hipEventRecord(s->ev_join[g], s->gstream[g]));
        HIP_TRY(hipStreamWaitEvent(main_st, s->ev_join[g], 0));
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// 16-bit event trace: a count that did not fit was truncated on the device -- fail loudly
// A hand-off inside a launch that timed out (k_move_pair's handshakes and band tokens, k_se_chunk's tile counter) means
// a workgroup went on without what it waited for: never seen outside the test hooks, and then the draws are not to be
// trusted -- the next read of the trace fails loudly instead of delivering them.
static int check_handoffs(seir_sampler *s) {
    if ((s->pair_debug & 15) != 0) return 0;              // the hooks make roles late on purpose (16..128 only delay: checked)
    // only the waits a workgroup cannot recover from (band tokens, k_se_chunk's tile flag, k_leap's flags, k_move_pairs'
    // step barrier); a late speculative role of k_move_pair is benign -- role 0 draws the proposal itself, the traces
    // are the same -- and only counted
    if (!s->poisoned) {
        std::vector<uint32_t> late((size_t)s->cfg.B, 0u);
        uint32_t *fatal = s->ch.late + s->ch.late_fatal;
        HIP_TRY(hipMemcpy(late.data(), fatal, sizeof(uint32_t) * late.size(), hipMemcpyDeviceToHost));
        for (size_t b = 0; b < late.size(); ++b)
            if (late[b]) { s->poisoned = true; s->poison_chain = (int)b; s->poison_count = late[b]; break; }
    }
    if (s->poisoned)
        // STICKY: a workgroup that gave up a wait went on with stale data (a band workgroup with an old F-band descriptor:
        // Work::F is only ever updated incrementally and would stay out of step with the event planes), so nothing this
        // sampler produces is to be trusted until its state is rebuilt -- seir_sampler_restore (back to the last snapshot:
        // the failed burst can be run again, e.g. in the per-step launch forms), seir_sampler_set_state or
        // seir_sampler_refresh (F and every table recomputed from the planes as they are; the failed burst's draws are lost)
        return fail(SEIR_ERR_HANDOFF, "chain %d: %u in-launch hand-off(s) timed out -- the persistent launches could not get all "
                    "their workgroups on the GPU at once (another sampler or process holds part of it?).  Draws since the last "
                    "check are unreliable and the sampler refuses to go on until seir_sampler_restore / _set_state / _refresh; "
                    "hmc_mode 3 + moves_mode 4 (seir_sampler_set_launch_form) are the launch forms for a shared GPU",
                    s->poison_chain, s->poison_count);
    return 0;
}

static int check_ev_overflow(seir_sampler *s) {
    int rc = check_handoffs(s);
    if (rc) return rc;
    if (!s->cfg.ev16) return 0;
    unsigned flag = 0;
    HIP_TRY(hipMemcpy(&flag, s->ch.ev_overflow, sizeof(flag), hipMemcpyDeviceToHost));
    if (flag) return fail(SEIR_ERR_STATE, "an event count exceeded 65535: record_events=2 (uint16 trace) cannot hold this chain");
    return 0;
}

// What every reader of recorded events refuses first.  verb: what the caller wanted the events for (null: just to read them).
static int need_events(const seir_sampler *s, const char *verb) {
    if (s->record_events) return 0;
    if (!verb) return fail(SEIR_ERR_STATE, "sampler was created with record_events=0");
    return fail(SEIR_ERR_STATE, "sampler was created with record_events=0: there are no recorded events to %s", verb);
}

// Enqueue fn(copy stream) behind everything queued on the context stream so far (the burst); what is queued there afterwards
// overlaps it.  seir_sampler_trace_wait completes it.
template <typename F>
static int on_copy_stream(seir_sampler *s, F fn) {
    HIP_TRY(hipEventRecord(s->ev_burst, s->ctx->stream));
    HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_burst, 0));
    if (int rc = fn(s->copy_stream)) return rc;
    HIP_TRY(hipEventRecord(s->ev_copy, s->copy_stream));
    s->copy_pending = true;
    return 0;
}

// The tail of every read that has an _async form; copy(stream) enqueues the device-to-host copies.  Blocking: on the context
// stream, waited for, then the draws' own refusals (check_ev_overflow).  async: on the copy stream, as above.
template <typename F>
static int deliver(seir_sampler *s, bool async, F copy) {
    if (async) return on_copy_stream(s, copy);
    if (int rc = copy(s->ctx->stream)) return rc;
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    return check_ev_overflow(s);
}

static int copy_trace(seir_sampler *s, hipStream_t st, int32_t first, int32_t count, double *theta, void *events, double *hmc,
                      double *moves) {
    const Dims &d = s->ctx->d;
    const SamplerCfg &c = s->cfg;
    const size_t B = c.B;
    if (theta)
        HIP_TRY(hipMemcpyAsync(theta, s->ch.tr_theta + (size_t)first * B * d.P, sizeof(double) * count * B * d.P,
                               hipMemcpyDeviceToHost, st));
    if (events)
        HIP_TRY(hipMemcpyAsync(events, (const char *)s->ch.tr_events + (size_t)first * B * d.M * d.T * 3 * (c.ev16 ? 2 : 4),
                               (size_t)(c.ev16 ? 2 : 4) * count * B * d.M * d.T * 3, hipMemcpyDeviceToHost, st));
    if (hmc)
        HIP_TRY(hipMemcpyAsync(hmc, s->ch.tr_hmc + (size_t)first * B * 3, sizeof(double) * count * B * 3,
                               hipMemcpyDeviceToHost, st));
    if (moves)
        HIP_TRY(hipMemcpyAsync(moves, s->ch.tr_mv + (size_t)first * B * 4 * NMVTR,
                               sizeof(double) * count * B * 4 * NMVTR, hipMemcpyDeviceToHost, st));
    return 0;
}

static int read_trace(seir_sampler *s, bool async, int32_t first, int32_t count, double *theta, void *events, double *hmc,
                      double *moves) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if (first < 0 || count < 0 || first + count > s->cfg.cap)
        return fail(SEIR_ERR_INVALID, "trace range [%d,%d) outside capacity %d", first, first + count, s->cfg.cap);
    if (events && (rc = need_events(s, nullptr))) return rc;
    return deliver(s, async, [&](hipStream_t st) { return copy_trace(s, st, first, count, theta, events, hmc, moves); });
}

extern "C" int seir_sampler_read_trace(seir_sampler *s, int32_t first, int32_t count, double *theta,
                                       void *events, double *hmc, double *moves) {
    return read_trace(s, false, first, count, theta, events, hmc, moves);
}
extern "C" int seir_sampler_read_trace_async(seir_sampler *s, int32_t first, int32_t count, double *theta,
                                             void *events, double *hmc, double *moves) {
    return read_trace(s, true, first, count, theta, events, hmc, moves);
}

extern "C" int seir_sampler_trace_wait(seir_sampler *s) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if (s->copy_pending) {
        HIP_TRY(hipEventSynchronize(s->ev_copy));
        s->copy_pending = false;
        return check_ev_overflow(s);
    }
    return 0;
}

// ---------------------------------------------------------------------------
// Summaries of the recorded events (include/seir_hip.h; kernels: summary_kernels.h)
// ---------------------------------------------------------------------------
// What every user of a trace range (TraceUser) refuses first.
static int trace_range_check(seir_sampler *s, bool enabled, const TraceUser &what, int32_t first = 0, int32_t count = 0) {
    if (int rc = need_events(s, what.verb)) return rc;
    if (!enabled) return fail(SEIR_ERR_STATE, "%s", what.not_enabled);
    if (first < 0 || count < 0 || (long long)first + count > s->cfg.cap)
        return fail(SEIR_ERR_INVALID, "trace range [%d,%lld) outside capacity %d", first, (long long)first + count, s->cfg.cap);
    return 0;
}

// The per-draw marginals of a MomentBufs: E, the day extent, is T (summaries), H (forecast) or K (check).
static int copy_marginals(seir_sampler *s, hipStream_t st, int32_t first, int32_t count, const MomentBufs &m, size_t E,
                          int64_t *by_day, int64_t *by_loc, int64_t *state_by_day) {
    const size_t B = s->cfg.B, f = (size_t)first, n = (size_t)count, M = (size_t)s->ctx->d.M;
    if (by_day) HIP_TRY(hipMemcpyAsync(by_day, m.by_day + f * B * E * 3, sizeof(int64_t) * n * B * E * 3, hipMemcpyDeviceToHost, st));
    if (by_loc) HIP_TRY(hipMemcpyAsync(by_loc, m.by_loc + f * B * M * 3, sizeof(int64_t) * n * B * M * 3, hipMemcpyDeviceToHost, st));
    if (state_by_day)
        HIP_TRY(hipMemcpyAsync(state_by_day, m.state_by_day + f * B * E * 3, sizeof(int64_t) * n * B * E * 3, hipMemcpyDeviceToHost, st));
    return 0;
}
// What is behind every seir_sampler_read_*_marginals(_async), after the null-sampler refusal.
static int read_marginals(seir_sampler *s, bool enabled, const TraceUser &what, const MomentBufs &m, int day_extent, bool async,
                          int32_t first, int32_t count, int64_t *by_day, int64_t *by_loc, int64_t *state_by_day) {
    if (int rc = trace_range_check(s, enabled, what, first, count)) return rc;
    return deliver(s, async, [&](hipStream_t st) {
        return copy_marginals(s, st, first, count, m, (size_t)day_extent, by_day, by_loc, state_by_day);
    });
}

// ---------------------------------------------------------------------------
// Region totals on the device (include/seir_hip.h; kernel: group_kernels.h)
// ---------------------------------------------------------------------------
// The refusals of a table against M rows, and its cut into segments of at most GRP_SEG members (GroupTable::seg).
static int groups_parse(int32_t G, const int32_t *offsets, const int32_t *members, int M, std::vector<int> &seg) {
    if (G < 1 || G > GRP_MAX_G) return fail(SEIR_ERR_INVALID, "G=%d outside [1, %d]", G, GRP_MAX_G);
    if (!offsets || !members) return fail(SEIR_ERR_INVALID, "null group table pointer");
    if (offsets[0] != 0) return fail(SEIR_ERR_INVALID, "offsets[0]=%d: the table starts at 0", offsets[0]);
    for (int g = 0; g < G; ++g) {
        const int beg = offsets[g], end = offsets[g + 1];
        if (end < beg) return fail(SEIR_ERR_INVALID, "offsets[%d]=%d below offsets[%d]=%d: offsets must not decrease", g + 1, end, g, beg);
        if (end == beg) return fail(SEIR_ERR_INVALID, "group %d is empty", g);
        if (end - beg > M) return fail(SEIR_ERR_INVALID, "group %d has %d members of M=%d locations: a member is repeated", g, end - beg, M);
        for (int i = beg; i < end; ++i) {
            if (members[i] < 0 || members[i] >= M)
                return fail(SEIR_ERR_INVALID, "member %d of group %d outside [0, M=%d)", members[i], g, M);
            if (i > beg && members[i] <= members[i - 1])
                return fail(SEIR_ERR_INVALID, "group %d: member %d after %d: members must be ascending and unique", g, members[i],
                            members[i - 1]);
        }
        for (int b = beg; b < end; b += GRP_SEG) {
            seg.push_back(g); seg.push_back(b); seg.push_back(std::min(end, b + GRP_SEG));
        }
    }
    return 0;
}

// nd draws of ev [.][M][L][3] from draw ev_d0 onto out / state0 from draw out_d0, which the caller has zeroed (the kernel adds).
// Defined at the end of this file: it is the one place that names k_group_sums, and a kernel template is emitted where it is
// first named -- behind every kernel the parent had, whose places in the code object then stay what they were.
static void groups_launch(const Dims &d, hipStream_t st, const GroupTable &gt, bool ev16, const void *ev, int M, int L,
                          long long ev_d0, long long out_d0, long long nd, int64_t *out, const int *St0, long long plane, int ndp,
                          int64_t *state0);

// The scenarios' region totals (seir_sampler_scenario_groups_set; defined with the scenarios, at the end of this file): the
// bytes of the store for K scenarios, `cap` draws per chain, G groups and H days while the switch is on, else 0; and the
// store sized for what is in force -- at j = 0 made (or refused), behind the first forecast only ever turned off.  `held`: the
// caller has already held the store's bytes, in a sum of its own, against half of the free memory: they are not held again
// behind the caller's other allocations, where a second refusal would leave what the first one promised to keep undone.
static unsigned long long scenario_groups_bytes(const seir_sampler *s, int K, long long cap, int G, int H);
static int scenario_groups_fit(seir_sampler *s, bool held = false);

// The day extent of source `which` (0 trace, 1 forecast, 2 check) while it is on, else 0.
static int groups_source_len(const seir_sampler *s, int which) {
    if (which == 0) return s->sum_on ? s->ctx->d.T : 0;
    const Rollout &r = which == 1 ? s->fc : s->ck;
    return r.on ? r.fb.H : 0;
}

// Bytes of the outputs of source `which` at G groups and L days, and their refusal above half of the device's free memory.
static unsigned long long groups_bytes(const seir_sampler *s, int G, int which, int L) {
    const unsigned long long rows = (unsigned long long)s->cfg.cap * s->cfg.B * G;
    return rows * L * 3ull * 8ull + (which ? rows * 3ull * 8ull : 0ull);
}
static int groups_refuse_bytes(const seir_sampler *s, unsigned long long bytes, int G) {
    return refuse_above_half_free(bytes, "the group sums need %llu bytes (%d slots x %d chains x %d groups x 24 per day and per state)",
                                  bytes, s->cfg.cap, s->cfg.B, G);
}

// Size the outputs of source `which` for the table and the source's present length (none when either is off).
static int groups_fit(seir_sampler *s, int which) {
    GroupOut &o = s->grp_out[which];
    const int L = s->grp_on ? groups_source_len(s, which) : 0;
    if (L == o.L) return 0;
    if (int rc = drain(s)) return rc;
    o = GroupOut{};
    if (L == 0) return 0;
    const unsigned long long rows = (unsigned long long)s->cfg.cap * s->cfg.B * s->grp.G;
    const unsigned long long bytes = groups_bytes(s, s->grp.G, which, L);
    if (int rc = groups_refuse_bytes(s, bytes, s->grp.G)) return rc;
    // both arrays or neither: a source whose outputs could not be made has none (L = 0) and is not launched for
    GroupOut made;
    if (made.ev.zeroed((size_t)(rows * L * 3ull * 8ull)) || (which && made.st0.zeroed((size_t)(rows * 3ull * 8ull))))
        return alloc_failed(bytes, "group sums");
    made.L = L;
    o = std::move(made);
    return 0;
}

// Source `which` forms group sums: a table is set and the source's outputs exist (a refused or failed groups_fit leaves none).
static bool groups_live(const seir_sampler *s, int which) { return s->grp_on && s->grp_out[which].L != 0; }

// The kernel adds: the outputs of slots [first, first + count) of source `which` start from zero.  In stream order.
static int groups_zero(seir_sampler *s, int which, int32_t first, int32_t count) {
    const GroupOut &o = s->grp_out[which];
    const size_t row = (size_t)s->cfg.B * s->grp.G;
    HIP_TRY(hipMemsetAsync(o.ev.as<int64_t>() + (size_t)first * row * o.L * 3, 0, sizeof(int64_t) * count * row * o.L * 3, s->ctx->stream));
    if (o.st0) HIP_TRY(hipMemsetAsync(o.st0.as<int64_t>() + (size_t)first * row * 3, 0, sizeof(int64_t) * count * row * 3, s->ctx->stream));
    return 0;
}

extern "C" int seir_sampler_groups_set(seir_sampler *s, int32_t G, const int32_t *offsets, const int32_t *members) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if (G == 0) {
        if ((rc = drain(s))) return rc;
        groups_free(s);
        s->wb.curve.on = false;
        s->scen.gstore.reset(); s->scen.gG = 0;      // the scenarios' region totals go with the table
        return 0;
    }
    if ((rc = need_events(s, "sum over groups of locations"))) return rc;
    std::vector<int> seg;
    if ((rc = groups_parse(G, offsets, members, s->ctx->d.M, seg))) return rc;
    // what the sources that are on need, against the free memory as it is with the old table's outputs still there
    // (conservative), and the new table's device copy: a refusal or failure here leaves the table in force alone
    unsigned long long need = 0;
    for (int which = 0; which < 3; ++which)
        if (const int L = groups_source_len(s, which)) need += groups_bytes(s, G, which, L);
    // the scenarios' store by draw position is made again only before the first forecast; behind it a new table turns it off
    if (s->fc.on && s->fc.acc.j == 0) need += scenario_groups_bytes(s, s->scen.K, s->scen.cap, G, s->fc.fb.H);
    if ((rc = groups_refuse_bytes(s, need, G))) return rc;
    DevBuf dseg, dmem;
    if ((rc = dseg.upload(seg.data(), seg.size() * sizeof(int))) || (rc = dmem.upload(members, (size_t)offsets[G] * sizeof(int))))
        return rc;
    if ((rc = drain(s))) return rc;
    groups_free(s);
    s->scen.gstore.reset(); s->scen.gG = 0;
    s->grp_seg = std::move(dseg); s->grp_members = std::move(dmem);
    s->grp.seg = s->grp_seg.as<int>(); s->grp.members = s->grp_members.as<int>();
    s->grp.nseg = (int)(seg.size() / 3);
    s->grp.G = G;
    s->grp_on = true;
    for (int which = 0; which < 3; ++which)
        if ((rc = groups_fit(s, which))) { groups_free(s); return rc; }
    if ((rc = scenario_groups_fit(s, true))) { groups_free(s); return rc; }
    s->grp_offsets.assign(offsets, offsets + G + 1);
    // group R_t went off with the old table's weights (groups_free); group within / between has none and is sized again
    return s->wb.curve.on ? gcurve_fit(s, s->wb) : 0;
}

static int copy_group_marginals(seir_sampler *s, hipStream_t st, int which, int32_t first, int32_t count, int64_t *ev, int64_t *st0) {
    const GroupOut &o = s->grp_out[which];
    const size_t row = (size_t)s->cfg.B * s->grp.G, f = (size_t)first, n = (size_t)count;
    if (ev) HIP_TRY(hipMemcpyAsync(ev, o.ev.as<int64_t>() + f * row * o.L * 3, sizeof(int64_t) * n * row * o.L * 3, hipMemcpyDeviceToHost, st));
    if (st0) HIP_TRY(hipMemcpyAsync(st0, o.st0.as<int64_t>() + f * row * 3, sizeof(int64_t) * n * row * 3, hipMemcpyDeviceToHost, st));
    return 0;
}

static int read_group_marginals(seir_sampler *s, bool async, int32_t which, int32_t first, int32_t count, int64_t *ev, int64_t *st0) {
    if (int rc = sampler_check(s)) return rc;
    if (which < 0 || which > 2) return fail(SEIR_ERR_INVALID, "which=%d: 0 trace, 1 forecast, 2 check", which);
    if (int rc = need_events(s, "sum over groups of locations")) return rc;
    if (!s->grp_on) return fail(SEIR_ERR_STATE, "no group table is set: call seir_sampler_groups_set first");
    if (s->grp_out[which].L == 0)
        return fail(SEIR_ERR_STATE, "%s", which == 0 ? SUMMARY_USER.not_enabled : which == 1 ? FORECAST_USER.not_enabled
                                                                                             : CHECK_USER.not_enabled);
    if (first < 0 || count < 0 || (long long)first + count > s->cfg.cap)
        return fail(SEIR_ERR_INVALID, "trace range [%d,%lld) outside capacity %d", first, (long long)first + count, s->cfg.cap);
    if (which == 0 && st0)
        return fail(SEIR_ERR_INVALID, "the trace has no per-draw state0: it is the context's initial state summed over the members");
    return deliver(s, async, [&](hipStream_t st) { return copy_group_marginals(s, st, which, first, count, ev, st0); });
}

extern "C" int seir_sampler_read_group_marginals(seir_sampler *s, int32_t which, int32_t first, int32_t count,
                                                 int64_t *events_by_group, int64_t *state0_by_group) {
    return read_group_marginals(s, false, which, first, count, events_by_group, state0_by_group);
}

extern "C" int seir_sampler_read_group_marginals_async(seir_sampler *s, int32_t which, int32_t first, int32_t count,
                                                       int64_t *events_by_group, int64_t *state0_by_group) {
    return read_group_marginals(s, true, which, first, count, events_by_group, state0_by_group);
}

extern "C" int seir_group_sums(seir_ctx *ctx, const int32_t *events, int64_t n, int32_t M, int32_t L, int32_t G,
                               const int32_t *offsets, const int32_t *members, int64_t *out) {
    int rc = check_batch(ctx, 1);
    if (rc) return rc;
    if (!events || !out) return fail(SEIR_ERR_INVALID, "null pointer");
    if (n < 1 || M < 1 || L < 1 || n > 0x7fffffffll)
        return fail(SEIR_ERR_INVALID, "n=%lld, M=%d, L=%d: at least one of each, n below 2^31", (long long)n, M, L);
    std::vector<int> seg;
    if ((rc = groups_parse(G, offsets, members, M, seg))) return rc;
    const size_t nin = (size_t)n * M * L * 3, nout = (size_t)n * G * L * 3, nnz = (size_t)offsets[G];
    DevBuf dev, dout, dseg, dmem;
    if ((rc = dev.alloc(sizeof(int32_t) * nin)) || (rc = dout.alloc(sizeof(int64_t) * nout)) ||
        (rc = dseg.alloc(sizeof(int) * seg.size())) || (rc = dmem.alloc(sizeof(int) * nnz)))
        return rc;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(dev.p, events, sizeof(int32_t) * nin, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dseg.p, seg.data(), sizeof(int) * seg.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dmem.p, members, sizeof(int) * nnz, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(dout.p, 0, sizeof(int64_t) * nout, st));
    const GroupTable gt{dseg.as<int>(), dmem.as<int>(), (int)(seg.size() / 3), G};
    groups_launch(whole(ctx, 1).d, st, gt, false, dev.p, M, L, 0, 0, n, dout.as<int64_t>(), nullptr, 0, 0, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, dout.p, sizeof(int64_t) * nout, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// ---------------------------------------------------------------------------
// Summaries of the recorded events (include/seir_hip.h; kernels: summary_kernels.h)
// ---------------------------------------------------------------------------
extern "C" int seir_sampler_summary_reset(seir_sampler *s) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = need_events(s, SUMMARY_USER.verb))) return rc;
    const Dims &d = s->ctx->d;
    const size_t B = (size_t)s->cfg.B, cap = (size_t)s->cfg.cap;
    MomentBufs &sb = s->sum;
    if (!s->sum_on) {
        S_ALLOC(allocs, sb.by_day, cap * B * d.T * 3); S_ALLOC(allocs, sb.by_loc, cap * B * d.M * 3);
        S_ALLOC(allocs, sb.state_by_day, cap * B * d.T * 3);
        if (!rc) rc = acc_alloc(s->sum_acc, summary_cells(s), B, sb);
        if (rc) return rc;
        s->sum_on = true;
    }
    hipStream_t st = s->ctx->stream;
    if ((rc = acc_zero(s->sum_acc, st))) return rc;
    // the batch sums are about the same ref and the marks are copies of these accumulators: they start again with them
    if (s->diag_on && (rc = acc_zero(s->diag_buf, st))) return rc;
    return s->grp_on ? groups_fit(s, 0) : 0;
}

extern "C" int seir_sampler_summarize(seir_sampler *s, int32_t first, int32_t count, int32_t accumulate) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = trace_range_check(s, s->sum_on, SUMMARY_USER, first, count))) return rc;
    if (count == 0) return 0;
    seir_ctx *ctx = s->ctx;
    const LaunchCfg l = whole(ctx, s->cfg.B);
    const Dims &d = l.d;
    const int B = s->cfg.B;
    // events_by_day is summed with atomics: zero the call's slots first
    HIP_TRY(hipMemsetAsync(s->sum.by_day + (size_t)first * B * d.T * 3, 0, sizeof(int64_t) * count * B * d.T * 3, l.st));
    for (int j0 = 0; j0 < count; j0 += SUM_JMAX) {
        const int nj = std::min(SUM_JMAX, count - j0);
        const dim3 grid((d.M + SUM_ROWS - 1) / SUM_ROWS, B), block(64 * SUM_ROWS);
        // while the diagnostics are on, folding draws goes through the instance that carries the batch sums as well
        const bool diag = s->diag_on && accumulate != 0;
        if (s->cfg.ev16 && diag)
            hipLaunchKernelGGL((k_summarize<1, 1>), grid, block, 0, l.st, d, ctx->c, s->sum, (const void *)s->ch.tr_events, B,
                               first + j0, nj, 1, s->diag);
        else if (diag)
            hipLaunchKernelGGL((k_summarize<0, 1>), grid, block, 0, l.st, d, ctx->c, s->sum, (const void *)s->ch.tr_events, B,
                               first + j0, nj, 1, s->diag);
        else if (s->cfg.ev16)
            hipLaunchKernelGGL((k_summarize<1, 0>), grid, block, 0, l.st, d, ctx->c, s->sum, (const void *)s->ch.tr_events, B,
                               first + j0, nj, accumulate != 0, SummaryDiag<0>{});
        else
            hipLaunchKernelGGL((k_summarize<0, 0>), grid, block, 0, l.st, d, ctx->c, s->sum, (const void *)s->ch.tr_events, B,
                               first + j0, nj, accumulate != 0, SummaryDiag<0>{});
        hipLaunchKernelGGL(k_summary_finish, dim3(nj, B), dim3(64), 0, l.st, d, ctx->c, s->sum, B, first + j0, nj,
                           accumulate != 0);
    }
    if (groups_live(s, 0)) {                         // the region totals of the same slots
        if ((rc = groups_zero(s, 0, first, count))) return rc;
        groups_launch(d, l.st, s->grp, s->cfg.ev16 != 0, s->ch.tr_events, d.M, d.T, (long long)first * B, (long long)first * B,
                      (long long)count * B, s->grp_out[0].ev.as<int64_t>(), nullptr, 0, 0, nullptr);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int seir_sampler_read_marginals(seir_sampler *s, int32_t first, int32_t count, int64_t *events_by_day,
                                           int64_t *events_by_location, int64_t *state_by_day) {
    if (int rc = sampler_check(s)) return rc;
    return read_marginals(s, s->sum_on, SUMMARY_USER, s->sum, s->ctx->d.T, false, first, count, events_by_day, events_by_location,
                          state_by_day);
}

extern "C" int seir_sampler_read_marginals_async(seir_sampler *s, int32_t first, int32_t count, int64_t *events_by_day,
                                                 int64_t *events_by_location, int64_t *state_by_day) {
    if (int rc = sampler_check(s)) return rc;
    return read_marginals(s, s->sum_on, SUMMARY_USER, s->sum, s->ctx->d.T, true, first, count, events_by_day, events_by_location,
                          state_by_day);
}

// What is behind every seir_sampler_read_<moments>, after the null-sampler refusal: a blocking read of a set of moments;
// `whose` and `reset` word the refusal when an accumulator has overflowed.
static int read_moments(seir_sampler *s, bool enabled, const TraceUser &what, const MomentAcc &a, const char *whose,
                        const char *reset, uint64_t *count, int32_t *ref, int64_t *sum, uint64_t *sumsq) {
    int rc = trace_range_check(s, enabled, what);
    if (rc) return rc;
    unsigned flag = 0;
    rc = acc_read(a, s->ctx->stream, count, ref, sum, sumsq, &flag);
    if (!rc) rc = check_ev_overflow(s);
    if (rc) return rc;
    if (flag) return fail(SEIR_ERR_STATE, "a sum of squared deviations reached 2^63: the %smoment accumulators overflowed "
                          "(%s starts them again)", whose, reset);
    return 0;
}

extern "C" int seir_sampler_read_summary(seir_sampler *s, uint64_t *count, int32_t *ref, int64_t *sum, uint64_t *sumsq) {
    if (int rc = sampler_check(s)) return rc;
    return read_moments(s, s->sum_on, SUMMARY_USER, s->sum_acc, "", "seir_sampler_summary_reset", count, ref, sum, sumsq);
}

// ---------------------------------------------------------------------------
// Convergence diagnostics (include/seir_hip.h; the DIAG instance of k_summarize)
// ---------------------------------------------------------------------------
extern "C" int seir_sampler_diag_reset(seir_sampler *s, int32_t batch_len) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if (batch_len < 1) return fail(SEIR_ERR_INVALID, "batch_len=%d: a batch has at least one draw", batch_len);
    if ((rc = need_events(s, "diagnose"))) return rc;
    if (!s->diag_on) {
        if ((rc = s->diag_buf.buf.zeroed(diag_words(s) * sizeof(uint64_t)))) return rc;
        const size_t n = summary_cells(s);
        s->diag.bsum = s->diag_buf.buf.as<int64_t>();
        s->diag.bsumsq = s->diag_buf.buf.as<uint64_t>() + n;
        s->diag.nbatch = s->diag.bsumsq + n;
        s->diag_on = true;
    }
    s->diag.L = (uint64_t)batch_len;
    // a snapshot taken before this reset holds batch sums cut by another L (which is no part of it): restoring it from now
    // on leaves the moments, the batch sums and the marks alone, as a snapshot from before the summaries were enabled does
    acc_invalidate(s->sum_acc);
    acc_invalidate(s->diag_buf);
    return seir_sampler_summary_reset(s);            // zeroes the batch sums and the marks with the moments
}

static int diag_check(seir_sampler *s, int32_t which) {
    if (int rc = need_events(s, "diagnose")) return rc;
    if (!s->diag_on) return fail(SEIR_ERR_STATE, "diagnostics are not enabled: call seir_sampler_diag_reset first");
    if (which < 0 || which > 1) return fail(SEIR_ERR_INVALID, "mark %d: marks are numbered 0 and 1", which);
    return 0;
}

extern "C" int seir_sampler_diag_mark(seir_sampler *s, int32_t which) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = diag_check(s, which))) return rc;
    const size_t n = summary_cells(s), B = (size_t)s->cfg.B;
    uint64_t *mk = diag_mark(s, which);
    hipStream_t st = s->ctx->stream;
    HIP_TRY(hipMemcpyAsync(mk, s->sum.count, B * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(mk + B, s->sum.sum, n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(mk + B + n, s->sum.sumsq, n * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    return 0;
}

static int diag_read_end(seir_sampler *s, unsigned flag) {
    int rc = check_ev_overflow(s);
    if (rc) return rc;
    if (flag) return fail(SEIR_ERR_STATE, "a sum of squares reached 2^63 or a batch sum 2^32: the accumulators overflowed "
                          "(seir_sampler_diag_reset starts them again)");
    return 0;
}

extern "C" int seir_sampler_read_diag(seir_sampler *s, uint64_t *nbatch, int64_t *bsum, uint64_t *bsumsq) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = diag_check(s, 0))) return rc;
    hipStream_t st = s->ctx->stream;
    const size_t n = summary_cells(s);
    unsigned flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, s->sum.overflow, sizeof(flag), hipMemcpyDeviceToHost, st));
    if (nbatch) HIP_TRY(hipMemcpyAsync(nbatch, s->diag.nbatch, sizeof(uint64_t) * s->cfg.B, hipMemcpyDeviceToHost, st));
    if (bsum) HIP_TRY(hipMemcpyAsync(bsum, s->diag.bsum, sizeof(int64_t) * n, hipMemcpyDeviceToHost, st));
    if (bsumsq) HIP_TRY(hipMemcpyAsync(bsumsq, s->diag.bsumsq, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return diag_read_end(s, flag);
}

extern "C" int seir_sampler_read_diag_mark(seir_sampler *s, int32_t which, uint64_t *count, int64_t *sum, uint64_t *sumsq) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = diag_check(s, which))) return rc;
    hipStream_t st = s->ctx->stream;
    const size_t n = summary_cells(s), B = (size_t)s->cfg.B;
    const uint64_t *mk = diag_mark(s, which);
    unsigned flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, s->sum.overflow, sizeof(flag), hipMemcpyDeviceToHost, st));
    if (count) HIP_TRY(hipMemcpyAsync(count, mk, sizeof(uint64_t) * B, hipMemcpyDeviceToHost, st));
    if (sum) HIP_TRY(hipMemcpyAsync(sum, mk + B, sizeof(int64_t) * n, hipMemcpyDeviceToHost, st));
    if (sumsq) HIP_TRY(hipMemcpyAsync(sumsq, mk + B + n, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return diag_read_end(s, flag);
}

// ---------------------------------------------------------------------------
// Forecast on the device (include/seir_hip.h; kernels: forecast_kernels.h)
// ---------------------------------------------------------------------------
// One Rollout behind the forecast and the in-sample check: what the two resets and the two calls have in common.  Where the
// users differ (the range of the length, the prepare kernel, what follows the fold, their own buffers) the callers do it.
static int rollout_refuse(const seir_sampler *s, const TraceUser &who, const double *W, const double *weekday_c) {
    if (!W || !weekday_c) return fail(SEIR_ERR_INVALID, "null calendar pointer");
    const Dims &d = s->ctx->d;
    const size_t lds = k_simulate_lds_bytes(d);
    if (lds > 160 * 1024) return fail(SEIR_ERR_INVALID, "M=%d needs %zu B of LDS for the simulator", d.M, lds);
    if ((long long)s->cfg.chain0 + s->cfg.B > FC_MAX_CHAIN)
        return fail(SEIR_ERR_INVALID, "global chain id %d: the %s's draw ids need chain ids below %d", s->cfg.chain0 + s->cfg.B - 1,
                    who.name, FC_MAX_CHAIN);
    return 0;
}

// First reset, or another length: everything is sized by H.  The caller sets r.on once its own buffers exist as well.
static int rollout_resize(seir_sampler *s, Rollout &r, int H) {
    int rc = drain(s);
    if (rc) return rc;
    r.allocs.clear(); r.acc.drop(); r.fb = ForecastBufs{};       // everything sized by H; j stays until the reset that follows
    r.on = false;
    const Dims &d = s->ctx->d;
    const size_t B = (size_t)s->cfg.B, cap = (size_t)s->cfg.cap;
    ForecastBufs &fb = r.fb;
    r.slots = std::min(s->cfg.cap, FC_JMAX);
    r.ndmax = ceil_to(r.slots * s->cfg.B, 64);
    const size_t plane = (size_t)d.Mp * r.ndmax, ndm = (size_t)r.slots * B;
#define R_ALLOC(ptr, ...) if (!rc) rc = s_alloc(s, r.allocs, &(ptr), __VA_ARGS__)
    double *Wd = nullptr, *wdd = nullptr;
    R_ALLOC(Wd, H); R_ALLOC(wdd, H);
    R_ALLOC(fb.St0, 3 * plane); R_ALLOC(fb.St, 3 * plane);
    R_ALLOC(fb.X, plane); R_ALLOC(fb.F, plane); R_ALLOC(fb.eb, plane);
    R_ALLOC(fb.sc, 3 * (size_t)r.ndmax); R_ALLOC(fb.base, (size_t)H * r.ndmax);
    R_ALLOC(fb.fev, ndm * d.M * H * 3);              // the user's own staging tensor
    R_ALLOC(fb.mom.by_day, cap * B * H * 3); R_ALLOC(fb.mom.by_loc, cap * B * d.M * 3);
    R_ALLOC(fb.mom.state_by_day, cap * B * H * 3);
#undef R_ALLOC
    if (!rc) rc = acc_alloc(r.acc, B * d.M * H * seir::SUMMARY_Q, B, fb.mom);
    if (rc) return rc;
    fb.W = Wd; fb.wd = wdd;
    fb.H = H;
    (void)lds_attribute((const void *)k_gemm<64>, gemm_lds_bytes<64>());
    return 0;
}

// Begin again: seed, calendar, moments and j.  Synchronises the stream, so what the caller has queued before is done as well.
static int rollout_begin(seir_sampler *s, Rollout &r, const double *W, const double *weekday_c, uint64_t seed) {
    hipStream_t st = s->ctx->stream;
    ForecastBufs &fb = r.fb;
    fb.k0 = (uint32_t)(seed & 0xffffffffu); fb.k1 = (uint32_t)(seed >> 32);
    // the caller's arrays are not retained: blocking copies behind what is queued (a reset is not on the hot path)
    HIP_TRY(hipMemcpyAsync(const_cast<double *>(fb.W), W, sizeof(double) * fb.H, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(const_cast<double *>(fb.wd), weekday_c, sizeof(double) * fb.H, hipMemcpyHostToDevice, st));
    if (int rc = acc_zero(r.acc, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    r.acc.j = 0;
    // what the snapshots taken before this reset hold of the moments is dropped with them: restoring one of them restores
    // the chain and leaves the accumulators and j as they are
    acc_invalidate(r.acc);
    return 0;
}

static int rollout_ids_left(const Rollout &r, const TraceUser &who, int32_t count) {
    if (r.acc.j + count > (1ll << FC_ID_SHIFT))
        return fail(SEIR_ERR_INVALID, "%lld draws per chain %s since the reset and %d more: the draw id holds 2^%d", r.acc.j, who.done,
                    count, FC_ID_SHIFT);
    return 0;
}

// Before a fold of `count` more draws behind the j since the reset: a store of `cap` per chain (entry point `sized_by`) holds them.
static int store_holds(const TraceUser &who, long long j, int32_t count, long long cap, const char *sized_by) {
    if (j + count <= cap) return 0;
    return fail(SEIR_ERR_INVALID, "%lld draws per chain %s since the reset and %d more: the draw store holds %lld (%s)", j, who.done,
                count, cap, sized_by);
}

// Trace slots [first + j0, first + j0 + nj) of a call: ND = nj * B draws, the planes' row stride ndp = ceil64(ND).
struct RolloutBatch { int j0, nj, ND, ndp; };

// A batch of a Rollout (forecast: which = 1, check: 2) behind its fold: the staging tensor and the per-draw initial state.
static void groups_rollout_batch(seir_sampler *s, int which, const Dims &d, hipStream_t st, const ForecastBufs &fb, int32_t first,
                                 const RolloutBatch &bt) {
    const GroupOut &o = s->grp_out[which];
    groups_launch(d, st, s->grp, false, fb.fev, d.M, fb.H, 0, (long long)(first + bt.j0) * s->cfg.B, bt.ND, o.ev.as<int64_t>(),
                  fb.St0, (long long)d.Mp * bt.ndp, bt.ndp, o.st0.as<int64_t>());
}

// The draws of trace slots [first, first + count) rolled forward fb.H days, in batches of at most r.slots slots.  Per batch:
// prepare(fb, batch) -- the user's prepare kernel on the batch's copy of r.fb, which it may amend first -- then per day the
// contraction and k_forecast_day, then k_forecast_fold, then after_fold(fb, batch).  The draw of slot first + jj has
// j = r.acc.j + jj; adding count to r.acc.j is left to the caller, behind whatever else it enqueues.
// The H days of a batch, whoever rolls it: per day the contraction F = Cstar . X over `cols` columns (a multiple of 64: one
// "chain", the columns in the place of the day index) and day(h), the caller's day launch on those columns.
template <typename Day>
static void rollout_day_loop(seir_ctx *ctx, const LaunchCfg &l, double *X, double *F, int cols, int H, Day day) {
    Dims gd = l.d;
    gd.b0 = 0;
    gd.Tp = cols;
    Work gw{};
    gw.Xn = X; gw.F = F;
    for (int h = 0; h < H; ++h) {
        hipLaunchKernelGGL((k_gemm<64>), dim3(cols / 64, l.d.Mp / GEMM_TM, 1), dim3(gemm_threads<64>()), gemm_lds_bytes<64>(), l.st,
                           gd, ctx->c, gw);
        day(h);
    }
}

template <typename Prepare, typename AfterFold>
static int rollout_days(seir_sampler *s, const Rollout &r, int32_t first, int32_t count, Prepare prepare, AfterFold after_fold) {
    seir_ctx *ctx = s->ctx;
    const LaunchCfg l = whole(ctx, s->cfg.B);
    const Dims &d = l.d;
    const int B = s->cfg.B, H = r.fb.H;
    // by_day is summed with atomics: zero the call's slots first
    HIP_TRY(hipMemsetAsync(r.fb.mom.by_day + (size_t)first * B * H * 3, 0, sizeof(int64_t) * count * B * H * 3, l.st));
    for (int j0 = 0; j0 < count; j0 += r.slots) {
        const int nj = std::min(r.slots, count - j0), ND = nj * B, ndp = ceil_to(ND, 64);
        const RolloutBatch bt{j0, nj, ND, ndp};
        ForecastBufs fb = r.fb;
        if (int rc = prepare(fb, bt)) return rc;
        rollout_day_loop(ctx, l, r.fb.X, r.fb.F, ndp, H, [&](int h) {
            hipLaunchKernelGGL(k_forecast_day, dim3(ndp / 64, (d.M + FC_DAY_ROWS - 1) / FC_DAY_ROWS), dim3(64 * FC_DAY_ROWS), 0,
                               l.st, d, ctx->c, fb, B, s->cfg.chain0, (int)(r.acc.j + j0), ND, ndp, h);
        });
        hipLaunchKernelGGL(k_forecast_fold, dim3((d.M + FC_ROWS - 1) / FC_ROWS, B), dim3(64 * FC_ROWS), 0, l.st, d, fb, B,
                           first + j0, nj, ndp);
        after_fold(fb, bt);
    }
    return 0;
}

// Scenarios riding on the forecast (behind the rest of the library's kernels: scenario_kernels.h is included at the end)
static int scenarios_begin(seir_sampler *s);
static int scenarios_zero_slots(seir_sampler *s, int32_t first, int32_t count);
static int scenarios_batch(seir_sampler *s, const ForecastBufs &fb, const RolloutBatch &bt, int32_t first);
// The forecast scored against later data (verify_kernels.h, included behind scenario_kernels.h)
static int verify_begin(seir_sampler *s);
static void verify_batch(seir_sampler *s, const ForecastBufs &fb, const RolloutBatch &bt);

extern "C" int seir_sampler_forecast_reset(seir_sampler *s, int32_t horizon, const double *W, const double *weekday_c,
                                           uint64_t seed) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = need_events(s, FORECAST_USER.verb))) return rc;
    if (horizon < 1 || horizon > SEIR_FORECAST_MAX_H)
        return fail(SEIR_ERR_INVALID, "horizon=%d outside [1, %d]", horizon, SEIR_FORECAST_MAX_H);
    if ((rc = rollout_refuse(s, FORECAST_USER, W, weekday_c))) return rc;
    Rollout &r = s->fc;
    if (!r.on || r.fb.H != horizon) {
        if ((rc = rollout_resize(s, r, horizon))) return rc;
        // the steps' buffers and the draw store are sized by H as well; the stream is idle
        s->fc_steps_host.reset();
        s->keep_fc = DrawStore{};
        s->scen = ScenarioSet{};
        s->ver = VerifySet{};
        S_ALLOC(fc.allocs, s->fc_steps_dev, (size_t)r.slots * s->cfg.B * horizon);
        if (rc) return rc;
        if (!s->fc_ev_steps) HIP_TRY(hipEventCreate(&s->fc_ev_steps));
        r.on = true;
    }
    if ((rc = rollout_begin(s, r, W, weekday_c, seed))) return rc;   // j = 0 empties the draw store too: it holds draws [0, j)
    s->fc_W_host.assign(W, W + horizon);
    if (s->scen.K && (rc = scenarios_begin(s))) return rc;           // the scenarios stay; their accumulators start again
    if (s->ver.on && (rc = verify_begin(s))) return rc;              // the truth stays; its accumulators start again
    if (s->grp_on && (rc = groups_fit(s, 1))) return rc;
    return scenario_groups_fit(s);                                   // the scenarios' region totals, sized where the forecast's are
}

extern "C" int seir_sampler_forecast(seir_sampler *s, int32_t first, int32_t count, const double *log_baseline_steps) {
    int rc = sampler_check(s);
    if (rc) return rc;
    Rollout &r = s->fc;
    if ((rc = trace_range_check(s, r.on, FORECAST_USER, first, count))) return rc;
    if (count == 0) return 0;
    if ((rc = rollout_ids_left(r, FORECAST_USER, count))) return rc;
    const DrawStore &keep = s->keep_fc;
    if (keep.buf && (rc = store_holds(FORECAST_USER, r.acc.j, count, keep.cap, FORECAST_USER.keep))) return rc;
    if (s->scen.K && (rc = store_holds(FORECAST_USER, r.acc.j, count, s->scen.cap, "seir_sampler_scenarios_set"))) return rc;
    seir_ctx *ctx = s->ctx;
    const LaunchCfg l = whole(ctx, s->cfg.B);
    const Dims &d = l.d;
    const int B = s->cfg.B, H = r.fb.H;
    if (groups_live(s, 1) && (rc = groups_zero(s, 1, first, count))) return rc;
    if (s->scen.K && (rc = scenarios_zero_slots(s, first, count))) return rc;
    int sc_rc = 0;
    if (log_baseline_steps) {
        // through page-locked memory indexed by trace slot, so that the call stays asynchronous; a slot's steps are
        // overwritten only once the upload that read them last has been done
        if (!s->fc_steps_host.p) HIP_TRY(hipHostMalloc(&s->fc_steps_host.p, sizeof(double) * s->cfg.cap * B * H, hipHostMallocDefault));
        if (s->fc_steps_pending) { HIP_TRY(hipEventSynchronize(s->fc_ev_steps)); s->fc_steps_pending = false; }
        std::memcpy(s->fc_steps_host.as<double>() + (size_t)first * B * H, log_baseline_steps, sizeof(double) * count * B * H);
    }
    rc = rollout_days(s, r, first, count,
        [&](ForecastBufs &fb, const RolloutBatch &bt) {
            if (log_baseline_steps) {
                HIP_TRY(hipMemcpyAsync(s->fc_steps_dev, s->fc_steps_host.as<double>() + (size_t)(first + bt.j0) * B * H,
                                       sizeof(double) * bt.ND * H, hipMemcpyHostToDevice, l.st));
                fb.steps = s->fc_steps_dev;
            }
            hipLaunchKernelGGL(s->cfg.ev16 ? k_forecast_prepare<1> : k_forecast_prepare<0>, dim3(d.Mp / FC_ROWS, bt.ndp),
                               dim3(64 * FC_ROWS), 0, l.st, d, ctx->c, fb, (const double *)s->ch.tr_theta,
                               (const void *)s->ch.tr_events, B, first + bt.j0, bt.ND, bt.ndp);
            return 0;
        },
        [&](const ForecastBufs &fb, const RolloutBatch &bt) {
            if (keep.buf)
                hipLaunchKernelGGL(k_forecast_keep, dim3((d.M + KEEP_ROWS - 1) / KEEP_ROWS, B), dim3(64 * KEEP_ROWS), 0, l.st, d,
                                   (const int *)fb.fev, (const int *)(fb.St0 + 2 * (size_t)d.Mp * bt.ndp), keep.buf.as<int>(),
                                   keep.stride, r.acc.j + bt.j0, H, B, bt.nj, bt.ndp);
            hipLaunchKernelGGL(k_forecast_finish, dim3(bt.nj, B), dim3(64), 0, l.st, d, fb, B, first + bt.j0, bt.nj, bt.ndp);
            if (groups_live(s, 1)) groups_rollout_batch(s, 1, d, l.st, fb, first, bt);
            if (s->scen.K && !sc_rc) sc_rc = scenarios_batch(s, fb, bt, first);   // while the batch's planes and fev live
            if (s->ver.on) verify_batch(s, fb, bt);
        });
    if (rc || (rc = sc_rc)) return rc;
    if (log_baseline_steps) { HIP_TRY(hipEventRecord(s->fc_ev_steps, l.st)); s->fc_steps_pending = true; }
    HIP_TRY(hipGetLastError());
    r.acc.j += count;
    return 0;
}

extern "C" int seir_sampler_read_forecast_marginals(seir_sampler *s, int32_t first, int32_t count, int64_t *forecast_by_day,
                                                    int64_t *forecast_by_location, int64_t *forecast_state_by_day) {
    if (int rc = sampler_check(s)) return rc;
    return read_marginals(s, s->fc.on, FORECAST_USER, s->fc.fb.mom, s->fc.fb.H, false, first, count, forecast_by_day,
                          forecast_by_location, forecast_state_by_day);
}

extern "C" int seir_sampler_read_forecast_marginals_async(seir_sampler *s, int32_t first, int32_t count,
                                                          int64_t *forecast_by_day, int64_t *forecast_by_location,
                                                          int64_t *forecast_state_by_day) {
    if (int rc = sampler_check(s)) return rc;
    return read_marginals(s, s->fc.on, FORECAST_USER, s->fc.fb.mom, s->fc.fb.H, true, first, count, forecast_by_day,
                          forecast_by_location, forecast_state_by_day);
}

extern "C" int seir_sampler_read_forecast(seir_sampler *s, uint64_t *count, int32_t *ref, int64_t *sum, uint64_t *sumsq) {
    if (int rc = sampler_check(s)) return rc;
    return read_moments(s, s->fc.on, FORECAST_USER, s->fc.acc, "forecast's ", "seir_sampler_forecast_reset", count, ref, sum, sumsq);
}

// ---------------------------------------------------------------------------
// Forecast intervals on the device (include/seir_hip.h; kernels: k_forecast_keep, order_stats_kernels.h)
// ---------------------------------------------------------------------------
// A draw store (the forecast's keep, the R_it store keepR) is sized between its product's reset and the first draws: the
// one resize behind seir_sampler_forecast_keep / seir_sampler_rt_keep.  cap == 0 frees it.  Otherwise a resize is refused
// once j draws per chain have been taken since the reset (in the words of `who`), a store that already has the capacity
// stays (the reset has emptied it), and a new one of `bytes` (`shape` spells the product out for the refusal) may take half
// of what is free on the device; it is zeroed, and its stride is its cap until the caller says otherwise.
static int keep_resize(seir_sampler *s, DrawStore &store, const TraceUser &who, int64_t cap, long long j, unsigned long long bytes,
                       const char *shape) {
    if (cap != 0) {
        if (j != 0)
            return fail(SEIR_ERR_STATE, "%lld draws per chain have been %s since the reset: the draw store is sized between "
                        "%s and the first %s", j, who.done, who.reset, who.call);
        if (store.buf && store.cap == cap) return 0;
    }
    if (store.buf) {
        HIP_TRY(hipStreamSynchronize(s->ctx->stream));
        store = DrawStore{};
    }
    if (cap == 0) return 0;
    if (int rc = refuse_above_half_free(bytes, "the draw store needs %llu bytes (%s)", bytes, shape)) return rc;
    if (int rc = store.buf.zeroed((size_t)bytes)) return rc;
    store.cap = store.stride = cap;
    return 0;
}

extern "C" int seir_sampler_forecast_keep(seir_sampler *s, int64_t cap) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = trace_range_check(s, s->fc.on, FORECAST_USER))) return rc;
    if (cap < 0 || cap > (1ll << FC_ID_SHIFT))
        return fail(SEIR_ERR_INVALID, "cap=%lld outside [0, 2^%d]: the draws per chain between two resets", (long long)cap, FC_ID_SHIFT);
    const unsigned long long cells = 3ull * s->cfg.B * s->ctx->d.M * s->fc.fb.H;
    char shape[160];
    snprintf(shape, sizeof shape, "%d chains x 3 x %d locations x %d days x %lld draws x 4", s->cfg.B, s->ctx->d.M, s->fc.fb.H,
             (long long)cap);
    return keep_resize(s, s->keep_fc, FORECAST_USER, cap, s->fc.acc.j, cells * (unsigned long long)cap * 4ull, shape);
}

// ranks [R] strictly increasing in [0, n): into the launch's arguments, or the refusal.
template <typename V>
static int order_ranks(const int64_t *ranks, int32_t R, long long n, OrderStatsArgs<V> &a) {
    if (R < 1 || R > ORDER_MAX_RANKS) return fail(SEIR_ERR_INVALID, "R=%d outside [1, %d]", R, ORDER_MAX_RANKS);
    if (!ranks) return fail(SEIR_ERR_INVALID, "null ranks pointer");
    for (int r = 0; r < R; ++r) {
        if (ranks[r] < 0 || ranks[r] >= n)
            return fail(SEIR_ERR_INVALID, "rank %lld outside [0, n=%lld)", (long long)ranks[r], n);
        if (r && ranks[r] <= ranks[r - 1])
            return fail(SEIR_ERR_INVALID, "ranks must be strictly increasing: %lld after %lld", (long long)ranks[r], (long long)ranks[r - 1]);
        a.ranks[r] = (uint32_t)ranks[r];
    }
    a.R = R;
    return 0;
}

// V = int32_t: k_order_stats; V = uint64_t, the doubles' bit patterns: k_order_stats_f64.  One wave per cell up to
// ORDER_WAVE_N values, four above.
template <typename V>
static void order_launch(const OrderStatsArgs<V> &a, hipStream_t st) {
    const bool one = (long long)a.segs * a.seg_len <= ORDER_WAVE_N;
    const dim3 grid((unsigned)a.cells), block(one ? 64 : 256);
    if constexpr (sizeof(V) == 4) {
        if (one) hipLaunchKernelGGL(k_order_stats<1>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(k_order_stats<4>, grid, block, 0, st, a);
    } else {
        if (one) hipLaunchKernelGGL(k_order_stats_f64<1>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(k_order_stats_f64<4>, grid, block, 0, st, a);
    }
}

// Order statistics of a draw store [B][plane][stride] holding j draws per chain, behind seir_sampler_forecast_order_stats
// and seir_sampler_rt_order_stats, refusing in the words of `who`: every chain's count (count_dev [B]) must be j; out [R][cells].
template <typename V>
static int keep_order_stats(seir_sampler *s, const DrawStore &store, const TraceUser &who, long long j, const uint64_t *count_dev,
                            long long plane, const int64_t *ranks, int32_t R, int32_t pooled, V *out) {
    if (!store.buf) return fail(SEIR_ERR_STATE, "the draw store is not enabled: call %s first", who.keep);
    if (!out) return fail(SEIR_ERR_INVALID, "null output pointer");
    if (j < 1) return fail(SEIR_ERR_STATE, "no draws kept since the %s reset", who.name);
    const int B = s->cfg.B;
    hipStream_t st = s->ctx->stream;
    std::vector<uint64_t> cnt((size_t)B);
    HIP_TRY(hipMemcpyAsync(cnt.data(), count_dev, sizeof(uint64_t) * B, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int b = 0; b < B; ++b)
        if ((long long)cnt[b] != j)
            return fail(SEIR_ERR_STATE, "chain %d has %llu draws %s, the store %lld: the chains' counts differ", b,
                        (unsigned long long)cnt[b], who.done, j);
    int rc;
    OrderStatsArgs<V> a{};
    if ((rc = order_ranks(ranks, R, pooled ? j * B : j, a))) return rc;
    a.values = store.buf.as<const V>();
    a.cells = pooled ? plane : plane * B;
    a.segs = pooled ? B : 1;
    a.seg_len = j;
    a.seg_stride = plane * store.stride;
    a.cell_stride = store.stride;
    DevBuf dout;
    const size_t nout = (size_t)R * (size_t)a.cells;
    if ((rc = dout.alloc(sizeof(V) * nout))) return rc;
    a.out = dout.as<V>();
    order_launch(a, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, dout.p, sizeof(V) * nout, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int seir_sampler_forecast_order_stats(seir_sampler *s, const int64_t *ranks, int32_t R, int32_t pooled, int32_t *out) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = trace_range_check(s, s->fc.on, FORECAST_USER))) return rc;
    return keep_order_stats<int32_t>(s, s->keep_fc, FORECAST_USER, s->fc.acc.j, s->fc.fb.mom.count, 3ll * s->ctx->d.M * s->fc.fb.H,
                                     ranks, R, pooled, out);
}

// The stateless select behind seir_order_stats / seir_order_stats_f64: values up, out [R][cells] back.
template <typename V>
static int order_stats_host(seir_ctx *ctx, const V *values, int64_t cells, int32_t segs, int64_t seg_len, int64_t seg_stride,
                            int64_t cell_stride, const int64_t *ranks, int32_t R, V *out) {
    int rc = check_batch(ctx, 1);
    if (rc) return rc;
    if (!values || !out) return fail(SEIR_ERR_INVALID, "null pointer");
    if (cells < 1 || cells > 0x7fffffffll || segs < 1 || seg_len < 1 || (long long)segs * seg_len > 0x7fffffffll)
        return fail(SEIR_ERR_INVALID, "cells=%lld, segs=%d, seg_len=%lld: at least one of each, n = segs x seg_len and cells below 2^31",
                    (long long)cells, segs, (long long)seg_len);
    if (cell_stride < 0 || seg_stride < 0 || (segs > 1 && seg_stride < seg_len))
        return fail(SEIR_ERR_INVALID, "seg_stride=%lld, cell_stride=%lld: no negative stride, and segments do not overlap",
                    (long long)seg_stride, (long long)cell_stride);
    OrderStatsArgs<V> a{};
    if ((rc = order_ranks(ranks, R, (long long)segs * seg_len, a))) return rc;
    const size_t extent = (size_t)(cells - 1) * cell_stride + (size_t)(segs - 1) * seg_stride + (size_t)seg_len;
    const size_t nout = (size_t)R * (size_t)cells;
    DevBuf dv, dout;
    if ((rc = dv.alloc(sizeof(V) * extent)) || (rc = dout.alloc(sizeof(V) * nout))) return rc;
    HIP_TRY(hipMemcpyAsync(dv.p, values, sizeof(V) * extent, hipMemcpyHostToDevice, ctx->stream));
    a.values = dv.as<V>(); a.out = dout.as<V>();
    a.cells = cells; a.segs = segs; a.seg_len = seg_len; a.seg_stride = seg_stride; a.cell_stride = cell_stride;
    order_launch(a, ctx->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, dout.p, sizeof(V) * nout, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int seir_order_stats(seir_ctx *ctx, const int32_t *values, int64_t cells, int32_t segs, int64_t seg_len,
                                int64_t seg_stride, int64_t cell_stride, const int64_t *ranks, int32_t R, int32_t *out) {
    return order_stats_host<int32_t>(ctx, values, cells, segs, seg_len, seg_stride, cell_stride, ranks, R, out);
}

extern "C" int seir_order_stats_f64(seir_ctx *ctx, const double *values, int64_t cells, int32_t segs, int64_t seg_len,
                                    int64_t seg_stride, int64_t cell_stride, const int64_t *ranks, int32_t R, double *out) {
    return order_stats_host<uint64_t>(ctx, (const uint64_t *)values, cells, segs, seg_len, seg_stride, cell_stride, ranks, R,
                                      (uint64_t *)out);
}

// ---------------------------------------------------------------------------
// In-sample predictive check on the device (include/seir_hip.h; kernels: check_kernels.h)
// ---------------------------------------------------------------------------
static void check_layout(seir_sampler *s, int K) {
    const size_t B = (size_t)s->cfg.B, M = (size_t)s->ctx->d.M, cells = B * M * K;
    CheckCmp &cc = s->ck_cmp;
    uint32_t *w = s->ck_cnt.buf.as<uint32_t>();
    cc.lt = w; cc.eq = w + cells; cc.obs = (int32_t *)(w + 2 * cells);
    w += 3 * cells;
    cc.loc_lt = w; cc.loc_eq = w + B * M;
    w += 2 * B * M;
    cc.day_lt = w; cc.day_eq = w + B * K;
    w += 2 * B * K;
    cc.all_lt = w; cc.all_eq = w + B; cc.moved = w + 2 * B;
}
static size_t check_words(const seir_sampler *s, int K) {
    const size_t B = (size_t)s->cfg.B, M = (size_t)s->ctx->d.M;
    return 3 * B * M * K + 2 * B * M + 2 * B * K + 3 * B;
}

extern "C" int seir_sampler_check_reset(seir_sampler *s, int32_t days, const double *W, const double *weekday_c, uint64_t seed) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = need_events(s, CHECK_USER.verb))) return rc;
    const Dims &d = s->ctx->d;
    const int kmax = std::min(d.T, SEIR_CHECK_MAX_DAYS);
    if (days < 1 || days > kmax) return fail(SEIR_ERR_INVALID, "days=%d outside [1, min(T = %d, %d)]", days, d.T, SEIR_CHECK_MAX_DAYS);
    if ((rc = rollout_refuse(s, CHECK_USER, W, weekday_c))) return rc;
    Rollout &r = s->ck;
    if (!r.on || r.fb.H != days) {
        if ((rc = rollout_resize(s, r, days))) return rc;
        s->ck_cnt = Shadowed{};                      // sized by K as well; the stream is idle
        if ((rc = s->ck_cnt.buf.zeroed(check_words(s, days) * sizeof(uint32_t)))) return rc;
        check_layout(s, days);
        r.on = true;
    }
    if ((rc = acc_zero(s->ck_cnt, s->ctx->stream))) return rc;
    if ((rc = rollout_begin(s, r, W, weekday_c, seed))) return rc;
    acc_invalidate(s->ck_cnt);                       // dropped from the snapshots with the moments
    return s->grp_on ? groups_fit(s, 2) : 0;
}

extern "C" int seir_sampler_check(seir_sampler *s, int32_t first, int32_t count) {
    int rc = sampler_check(s);
    if (rc) return rc;
    Rollout &r = s->ck;
    if ((rc = trace_range_check(s, r.on, CHECK_USER, first, count))) return rc;
    if (count == 0) return 0;
    if ((rc = rollout_ids_left(r, CHECK_USER, count))) return rc;
    seir_ctx *ctx = s->ctx;
    const LaunchCfg l = whole(ctx, s->cfg.B);
    const Dims &d = l.d;
    const int B = s->cfg.B;
    const dim3 rgrid((d.M + FC_ROWS - 1) / FC_ROWS, B), rblock(64 * FC_ROWS);
    if (groups_live(s, 2) && (rc = groups_zero(s, 2, first, count))) return rc;
    rc = rollout_days(s, r, first, count,
        [&](ForecastBufs &fb, const RolloutBatch &bt) {
            hipLaunchKernelGGL(s->cfg.ev16 ? k_check_prepare<1> : k_check_prepare<0>, dim3(d.Mp / FC_ROWS, bt.ndp), rblock, 0,
                               l.st, d, ctx->c, fb, (const double *)s->ch.tr_theta, (const void *)s->ch.tr_events, B,
                               first + bt.j0, bt.ND, bt.ndp);
            return 0;
        },
        [&](const ForecastBufs &fb, const RolloutBatch &bt) {
            const int fresh = r.acc.j + bt.j0 == 0;
            hipLaunchKernelGGL(k_forecast_finish, dim3(bt.nj, B), dim3(64), 0, l.st, d, fb, B, first + bt.j0, bt.nj, bt.ndp);
            hipLaunchKernelGGL(s->cfg.ev16 ? k_check_compare<1> : k_check_compare<0>, rgrid, rblock, 0, l.st, d, fb, s->ck_cmp,
                               (const void *)s->ch.tr_events, B, first + bt.j0, bt.nj, fresh);
            hipLaunchKernelGGL(k_check_totals, dim3(B), dim3(CK_TOT_THREADS), 0, l.st, d, fb, s->ck_cmp, B, first + bt.j0, bt.nj);
            if (groups_live(s, 2)) groups_rollout_batch(s, 2, d, l.st, fb, first, bt);
        });
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    r.acc.j += count;
    return 0;
}

extern "C" int seir_sampler_read_check_marginals(seir_sampler *s, int32_t first, int32_t count, int64_t *check_by_day,
                                                 int64_t *check_by_location, int64_t *check_state_by_day) {
    if (int rc = sampler_check(s)) return rc;
    return read_marginals(s, s->ck.on, CHECK_USER, s->ck.fb.mom, s->ck.fb.H, false, first, count, check_by_day, check_by_location,
                          check_state_by_day);
}

extern "C" int seir_sampler_read_check_marginals_async(seir_sampler *s, int32_t first, int32_t count, int64_t *check_by_day,
                                                       int64_t *check_by_location, int64_t *check_state_by_day) {
    if (int rc = sampler_check(s)) return rc;
    return read_marginals(s, s->ck.on, CHECK_USER, s->ck.fb.mom, s->ck.fb.H, true, first, count, check_by_day, check_by_location,
                          check_state_by_day);
}

extern "C" int seir_sampler_read_check(seir_sampler *s, uint64_t *count, int32_t *ref, int64_t *sum, uint64_t *sumsq) {
    if (int rc = sampler_check(s)) return rc;
    return read_moments(s, s->ck.on, CHECK_USER, s->ck.acc, "check's ", "seir_sampler_check_reset", count, ref, sum, sumsq);
}

extern "C" int seir_sampler_read_check_counts(seir_sampler *s, int32_t *obs, uint32_t *lt, uint32_t *eq, uint32_t *loc_lt,
                                              uint32_t *loc_eq, uint32_t *day_lt, uint32_t *day_eq, uint32_t *all_lt,
                                              uint32_t *all_eq) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = trace_range_check(s, s->ck.on, CHECK_USER))) return rc;
    hipStream_t st = s->ctx->stream;
    const size_t B = (size_t)s->cfg.B, M = (size_t)s->ctx->d.M, K = (size_t)s->ck.fb.H;
    const CheckCmp &cc = s->ck_cmp;
    std::vector<unsigned> moved(B, 0u);
    HIP_TRY(hipMemcpyAsync(moved.data(), cc.moved, sizeof(unsigned) * B, hipMemcpyDeviceToHost, st));
    const struct { void *dst; const void *src; size_t n; } parts[] = {
        {obs, cc.obs, B * M * K}, {lt, cc.lt, B * M * K}, {eq, cc.eq, B * M * K}, {loc_lt, cc.loc_lt, B * M},
        {loc_eq, cc.loc_eq, B * M}, {day_lt, cc.day_lt, B * K}, {day_eq, cc.day_eq, B * K}, {all_lt, cc.all_lt, B},
        {all_eq, cc.all_eq, B}};
    for (const auto &p : parts)
        if (p.dst) HIP_TRY(hipMemcpyAsync(p.dst, p.src, sizeof(uint32_t) * p.n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = check_ev_overflow(s))) return rc;
    for (size_t b = 0; b < B; ++b)
        if (moved[b])
            return fail(SEIR_ERR_STATE, "chain %zu: a draw's recorded I->R counts in the check window differ from those of the first "
                        "draw checked: the observed removals moved (seir_sampler_check_reset starts the check again)", b);
    return 0;
}

// ---------------------------------------------------------------------------
// Reproduction number on the device (include/seir_hip.h; kernels: rt_trace_kernels.h)
// ---------------------------------------------------------------------------
// The launches of the group curves (defined at the end of this file, where group_curve_kernels.h is included: the one place
// that names its kernels, behind every kernel the parent had).  Slots [slot0, slot0 + nj) are one batch.
static void gcurve_rt_trace_cells(seir_sampler *s, const LaunchCfg &l, int slot0, int nj);
static void gcurve_rt_gather(seir_sampler *s, const LaunchCfg &l, long long pos0, int nj);
static void gcurve_wb_trace_cells(seir_sampler *s, const LaunchCfg &l, int slot0, int nj);
static void gcurve_sums(seir_sampler *s, const LaunchCfg &l, const Window &w, int slot0, int nj);
static void gcurve_lds_attributes(int Mp);
// The launches of the group next-generation matrix (likewise at the end of this file, where ngm_kernels.h is included): the
// batch's slots [slot0, slot0 + nj) into the store's positions [pos0, pos0 + nj).
static void ngm_launch(seir_sampler *s, const LaunchCfg &l, int slot0, long long pos0, int nj);

// One Window behind the reproduction number and the within/between shares: what the two resets and every entry point's
// first refusals have in common.  Where the products differ (R_t's weights, draw store and group next-generation matrix; the
// planes and the layout of the block; the kernels) the entry points do it.  The first refusals: need_events' as
// SEIR_ERR_INVALID (a sampler without recorded events is a bad argument to this feature), then trace_range_check's
static int window_check(seir_sampler *s, const Window &w, int32_t first = 0, int32_t count = 0) {
    if (need_events(s, w.who.verb)) return SEIR_ERR_INVALID;
    return trace_range_check(s, w.on, w.who, first, count);
}
static size_t window_cells(const seir_sampler *s, const Window &w) { return (size_t)s->cfg.B * w.D * s->ctx->d.M; }
static size_t count_words(const seir_sampler *s) { return ((size_t)s->cfg.B + 31) / 32 * 32; }

// First reset, or another window: everything is sized by D.  The integer plane of a batch (R_t's S, the shares' I) is bounded,
// so a call is cut into batches of at most w.slots slots.  The caller then allocates its planes, lays out its block, sets w.on.
static int window_resize(seir_sampler *s, Window &w, int D) {
    if (int rc = drain(s)) return rc;
    w.allocs.clear(); w.acc.drop();                  // j stays until the reset that follows
    w.draws[0] = w.draws[1] = nullptr;
    w.on = false; w.D = D;
    w.slots = staging_slots(s->ctx, s->cfg.cap, (size_t)s->cfg.B * s->ctx->d.Mp * D * sizeof(int));
    return 0;
}

// Begin again: the block and j from zero, then the group curve sized for the window.  also(stream) enqueues what else of the
// product starts from zero, behind the block.  Synchronises the stream, so what the caller has queued before is done as well.
template <typename Also>
static int window_begin(seir_sampler *s, Window &w, Also also) {
    hipStream_t st = s->ctx->stream;
    if (int rc = acc_zero(w.acc, st)) return rc;
    if (int rc = also(st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    w.acc.j = 0;
    acc_invalidate(w.acc);                           // restoring a snapshot from before this reset leaves the accumulators alone
    return w.curve.on ? gcurve_fit(s, w) : 0;
}

extern "C" int seir_sampler_rt_reset(seir_sampler *s, int32_t days, const double *weight) {
    int rc = sampler_check(s);
    if (rc) return rc;
    Window &w = s->rt;
    if (need_events(s, w.who.verb)) return SEIR_ERR_INVALID;
    const Dims &d = s->ctx->d;
    if (days < 1 || days > d.T) return fail(SEIR_ERR_INVALID, "days=%d outside [1, T = %d]", days, d.T);
    if (!weight) return fail(SEIR_ERR_INVALID, "null weight pointer");
    const int B = s->cfg.B, D = days;
    RtBufs &rb = s->rtb;
    if (!w.on || w.D != D) {
        if ((rc = window_resize(s, w, D))) return rc;
        s->keep_rt = DrawStore{};                    // sized by D
        s->ngm = GroupNgm{};                         // sized by D too
        rb = RtBufs{};
        rb.D = D; rb.t0 = d.T - D; rb.ncb = (d.M + 63) / 64;
        const size_t nd = (size_t)w.slots * B;
        double *wd = nullptr;
        S_ALLOC(rt.allocs, wd, (size_t)rb.ncb * 64);
        S_ALLOC(rt.allocs, rb.ea, nd * d.Tp); S_ALLOC(rt.allocs, rb.S, nd * d.Mp * D);
        S_ALLOC(rt.allocs, rb.part, nd * D * rb.ncb); S_ALLOC(rt.allocs, rb.Rt, (size_t)s->cfg.cap * B * D);
        rb.weight = wd;
        w.draws[0] = rb.Rt;
        const size_t cells = window_cells(s, w);
        if (!rc) rc = w.acc.buf.zeroed(cells * (3 * sizeof(double) + sizeof(uint32_t)) + count_words(s) * sizeof(uint64_t));
        if (rc) return rc;
        rb.sum = w.acc.buf.as<double>();
        rb.sumsq = rb.sum + cells;
        rb.ref = rb.sumsq + cells;
        rb.count = (uint64_t *)(rb.ref + cells);
        rb.gt1 = (uint32_t *)(rb.count + count_words(s));
        (void)lds_attribute((const void *)k_rt_trace<RT_DT>, k_rt_trace_lds_bytes<RT_DT>(d.Mp));
        w.on = true;
    }
    // the caller's array is not retained: a blocking copy behind what is queued (a reset is not on the hot path)
    HIP_TRY(hipMemcpyAsync(const_cast<double *>(rb.weight), weight, sizeof(double) * d.M, hipMemcpyHostToDevice, s->ctx->stream));
    // j = 0 empties the draw store and the group next-generation matrix too: they hold draws [0, count)
    return window_begin(s, w, [&](hipStream_t st) {
        if (s->keep_rt.buf) HIP_TRY(hipMemsetAsync(s->keep_rt.buf.p, 0, sizeof(double) * window_cells(s, w) * (size_t)s->keep_rt.stride, st));
        if (s->ngm.cap)
            HIP_TRY(hipMemsetAsync(s->ngm.out.p, 0, sizeof(double) * (size_t)s->ngm.cap * B * s->grp.G * s->grp.G * D, st));
        return 0;
    });
}

extern "C" int seir_sampler_rt(seir_sampler *s, int32_t first, int32_t count) {
    int rc = sampler_check(s);
    if (rc) return rc;
    Window &w = s->rt;
    if ((rc = window_check(s, w, first, count))) return rc;
    if (count == 0) return 0;
    const DrawStore &keep = s->keep_rt;
    long long &j = w.acc.j;
    if (keep.buf && (rc = store_holds(w.who, j, count, keep.cap, w.who.keep))) return rc;
    if (s->ngm.cap && (rc = store_holds(w.who, j, count, s->ngm.cap, "seir_sampler_group_ngm"))) return rc;
    seir_ctx *ctx = s->ctx;
    const LaunchCfg l = whole(ctx, s->cfg.B);
    const Dims &d = l.d;
    const int B = s->cfg.B, D = w.D;
    const RtBufs &rb = s->rtb;
    Work tw = ctx->w;                                 // k_rt_tables writes Work::ea: the feature's own buffer, not the sampler's
    tw.ea = rb.ea;
    const size_t lds = k_rt_trace_lds_bytes<RT_DT>(d.Mp);
    const bool curves = w.curve.b.D != 0;               // group R_t: the batch also fits the cell plane
    const int slots = std::min(curves ? w.curve.b.slots : w.slots, s->ngm.cap ? s->ngm.slots : w.slots);
    for (int j0 = 0; j0 < count; j0 += slots) {
        const int nj = std::min(slots, count - j0), ND = nj * B;
        hipLaunchKernelGGL(k_rt_tables, dim3(ND), dim3(256), 0, l.st, d, tw,
                           (const double *)s->ch.tr_theta + (size_t)(first + j0) * B * d.P);
        const dim3 pgrid((d.M + RT_PREP_ROWS - 1) / RT_PREP_ROWS, ND), pblock(64 * RT_PREP_ROWS);
        if (s->cfg.ev16)
            hipLaunchKernelGGL(k_rt_prepare<1>, pgrid, pblock, 0, l.st, d, ctx->c, rb, (const void *)s->ch.tr_events, B, first + j0);
        else
            hipLaunchKernelGGL(k_rt_prepare<0>, pgrid, pblock, 0, l.st, d, ctx->c, rb, (const void *)s->ch.tr_events, B, first + j0);
        if (s->ngm.cap) ngm_launch(s, l, first + j0, j + j0, nj);            // behind k_rt_prepare: ea and S of the batch lie there
        if (keep.buf)                                 // in place of k_rt_trace: R_it is formed once
            hipLaunchKernelGGL(k_rt_trace_keep<RT_DT>, dim3(rb.ncb, (D + RT_DT - 1) / RT_DT, B), dim3(256), lds, l.st, d, ctx->c, rb,
                               (const double *)s->ch.tr_theta, B, first + j0, nj, keep.buf.as<double>(), keep.stride);
        else if (curves)                              // in place of k_rt_trace: it also leaves every cell's r in the plane
            gcurve_rt_trace_cells(s, l, first + j0, nj);
        else
            hipLaunchKernelGGL(k_rt_trace<RT_DT>, dim3(rb.ncb, (D + RT_DT - 1) / RT_DT, B), dim3(256), lds, l.st, d, ctx->c, rb,
                               (const double *)s->ch.tr_theta, B, first + j0, nj);
        hipLaunchKernelGGL(k_rt_finish, dim3((unsigned)(((size_t)ND * D + 255) / 256)), dim3(256), 0, l.st, rb, B, first + j0, nj);
        if (curves) {
            if (keep.buf) gcurve_rt_gather(s, l, j + j0, nj);
            gcurve_sums(s, l, w, first + j0, nj);
        }
    }
    HIP_TRY(hipGetLastError());
    j += count;
    return 0;
}

// ---------------------------------------------------------------------------
// R_t intervals on the device (include/seir_hip.h; kernels: rt_keep_kernels.h, order_stats_kernels.h)
// ---------------------------------------------------------------------------
extern "C" int seir_sampler_rt_keep(seir_sampler *s, int64_t cap) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = window_check(s, s->rt))) return rc;
    if (cap < 0 || cap > (1ll << 20))
        return fail(SEIR_ERR_INVALID, "cap=%lld outside [0, 2^20]: the draws per chain between two resets", (long long)cap);
    const long long stride = (cap + RT_KEEP_RUN - 1) / RT_KEEP_RUN * RT_KEEP_RUN;
    char shape[160];
    snprintf(shape, sizeof shape, "%d chains x %d days x %d locations x %lld draws x 8", s->cfg.B, s->rt.D, s->ctx->d.M, stride);
    DrawStore &keep = s->keep_rt;
    rc = keep_resize(s, keep, RT_USER, cap, s->rt.acc.j, (unsigned long long)window_cells(s, s->rt) * (unsigned long long)stride * 8ull,
                     shape);
    if (keep.buf && !rc) keep.stride = stride;       // a refused resize leaves the store and its stride as they were
    if (keep.buf) (void)lds_attribute((const void *)k_rt_trace_keep<RT_DT>, k_rt_trace_lds_bytes<RT_DT>(s->ctx->d.Mp));
    return rc;
}

extern "C" int seir_sampler_rt_order_stats(seir_sampler *s, const int64_t *ranks, int32_t R, int32_t pooled, double *out) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = window_check(s, s->rt))) return rc;
    if ((rc = keep_order_stats<uint64_t>(s, s->keep_rt, RT_USER, s->rt.acc.j, s->rtb.count, (long long)s->rt.D * s->ctx->d.M, ranks, R,
                                         pooled, (uint64_t *)out)))
        return rc;
    return check_ev_overflow(s);
}

// Slots [first, first + count) of a Window's per-draw curves src, `row` doubles per slot in each plane, to a (and b).  Where
// there is one plane a null destination is refused; of two, either may be left out.
static int deliver_curves(seir_sampler *s, const Window &w, bool async, const double *const *src, size_t row, int32_t first,
                          int32_t count, double *a, double *b) {
    if (w.planes == 1 && !a) return fail(SEIR_ERR_INVALID, "null pointer");
    double *const dst[2] = {a, b};
    return deliver(s, async, [&](hipStream_t st) {
        for (int x = 0; x < w.planes; ++x)
            if (dst[x])
                HIP_TRY(hipMemcpyAsync(dst[x], src[x] + (size_t)first * row, sizeof(double) * count * row, hipMemcpyDeviceToHost, st));
        return 0;
    });
}

// What is behind the four readers of the national curves [cap][B][D] of seir_sampler::rt or ::wb.
static int read_draws(seir_sampler *s, Window seir_sampler::*which, bool async, int32_t first, int32_t count, double *a, double *b) {
    if (int rc = sampler_check(s)) return rc;
    const Window &w = s->*which;
    if (int rc = window_check(s, w, first, count)) return rc;
    return deliver_curves(s, w, async, w.draws, (size_t)s->cfg.B * w.D, first, count, a, b);
}

extern "C" int seir_sampler_read_rt_draws(seir_sampler *s, int32_t first, int32_t count, double *R_t) {
    return read_draws(s, &seir_sampler::rt, false, first, count, R_t, nullptr);
}
extern "C" int seir_sampler_read_rt_draws_async(seir_sampler *s, int32_t first, int32_t count, double *R_t) {
    return read_draws(s, &seir_sampler::rt, true, first, count, R_t, nullptr);
}

extern "C" int seir_sampler_read_rt(seir_sampler *s, uint64_t *count, double *ref, double *sum, double *sumsq, uint32_t *gt1) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = window_check(s, s->rt))) return rc;
    hipStream_t st = s->ctx->stream;
    const size_t n = window_cells(s, s->rt);
    const RtBufs &rb = s->rtb;
    if (count) HIP_TRY(hipMemcpyAsync(count, rb.count, sizeof(uint64_t) * s->cfg.B, hipMemcpyDeviceToHost, st));
    if (ref) HIP_TRY(hipMemcpyAsync(ref, rb.ref, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    if (sum) HIP_TRY(hipMemcpyAsync(sum, rb.sum, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    if (sumsq) HIP_TRY(hipMemcpyAsync(sumsq, rb.sumsq, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    if (gt1) HIP_TRY(hipMemcpyAsync(gt1, rb.gt1, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return check_ev_overflow(s);
}

// ---------------------------------------------------------------------------
// Within/between pressure shares on the device (include/seir_hip.h; kernels: wb_kernels.h)
// ---------------------------------------------------------------------------
extern "C" int seir_sampler_wb_reset(seir_sampler *s, int32_t days) {
    int rc = sampler_check(s);
    if (rc) return rc;
    Window &w = s->wb;
    if (need_events(s, w.who.verb)) return SEIR_ERR_INVALID;
    const Dims &d = s->ctx->d;
    if (days < 1 || days > d.T) return fail(SEIR_ERR_INVALID, "days=%d outside [1, T = %d]", days, d.T);
    const int B = s->cfg.B, D = days;
    WbBufs &wb = s->wbb;
    if (!w.on || w.D != D) {
        if ((rc = window_resize(s, w, D))) return rc;
        wb = WbBufs{};
        wb.D = D; wb.t0 = d.T - D; wb.ncb = (d.M + 63) / 64;
        const size_t nd = (size_t)w.slots * B;
        S_ALLOC(wb.allocs, wb.I, nd * D * d.Mp); S_ALLOC(wb.allocs, wb.part, nd * D * wb.ncb * 2);
        S_ALLOC(wb.allocs, wb.Wn, (size_t)s->cfg.cap * B * D); S_ALLOC(wb.allocs, wb.Bn, (size_t)s->cfg.cap * B * D);
        w.draws[0] = wb.Wn; w.draws[1] = wb.Bn;
        const size_t cells = window_cells(s, w), cw = count_words(s);
        if (!rc) rc = w.acc.buf.zeroed(cells * (5 * sizeof(double) + 2 * sizeof(uint32_t)) + cw * sizeof(uint64_t));
        if (rc) return rc;
        wb.sum_w = w.acc.buf.as<double>();
        wb.sumsq_w = wb.sum_w + cells;
        wb.ref_w = wb.sumsq_w + cells;
        wb.ref_b = wb.ref_w + cells;
        wb.sum_b = wb.ref_b + cells;
        wb.count = (uint64_t *)(wb.sum_b + cells);
        wb.n = (uint32_t *)(wb.count + cw);
        wb.gt = wb.n + cells;
        (void)lds_attribute((const void *)k_wb_trace<WB_DT>, k_wb_trace_lds_bytes<WB_DT>(d.Mp));
        w.on = true;
    }
    return window_begin(s, w, [](hipStream_t) { return 0; });
}

extern "C" int seir_sampler_wb(seir_sampler *s, int32_t first, int32_t count) {
    int rc = sampler_check(s);
    if (rc) return rc;
    Window &w = s->wb;
    if ((rc = window_check(s, w, first, count))) return rc;
    if (count == 0) return 0;
    seir_ctx *ctx = s->ctx;
    const LaunchCfg l = whole(ctx, s->cfg.B);
    const Dims &d = l.d;
    const int B = s->cfg.B, D = w.D;
    const WbBufs &wb = s->wbb;
    const size_t lds = k_wb_trace_lds_bytes<WB_DT>(d.Mp);
    const bool curves = w.curve.b.D != 0;               // group within / between: the batch also fits the two cell planes
    const int slots = curves ? w.curve.b.slots : w.slots;
    for (int j0 = 0; j0 < count; j0 += slots) {
        const int nj = std::min(slots, count - j0), ND = nj * B;
        const dim3 pgrid((d.M + WB_PREP_ROWS - 1) / WB_PREP_ROWS, ND), pblock(64 * WB_PREP_ROWS);
        if (s->cfg.ev16)
            hipLaunchKernelGGL(k_wb_prepare<1>, pgrid, pblock, 0, l.st, d, ctx->c, wb, (const void *)s->ch.tr_events, B, first + j0);
        else
            hipLaunchKernelGGL(k_wb_prepare<0>, pgrid, pblock, 0, l.st, d, ctx->c, wb, (const void *)s->ch.tr_events, B, first + j0);
        if (curves)                                   // in place of k_wb_trace: it also leaves every cell's wi and be
            gcurve_wb_trace_cells(s, l, first + j0, nj);
        else
            hipLaunchKernelGGL(k_wb_trace<WB_DT>, dim3(wb.ncb, (D + WB_DT - 1) / WB_DT, B), dim3(256), lds, l.st, d, ctx->c, wb,
                               (const double *)s->ch.tr_theta, B, first + j0, nj);
        hipLaunchKernelGGL(k_wb_finish, dim3((unsigned)(((size_t)ND * D + 255) / 256)), dim3(256), 0, l.st, wb, B, first + j0, nj);
        if (curves) gcurve_sums(s, l, w, first + j0, nj);
    }
    HIP_TRY(hipGetLastError());
    w.acc.j += count;
    return 0;
}

extern "C" int seir_sampler_read_wb_draws(seir_sampler *s, int32_t first, int32_t count, double *within_pressure,
                                          double *between_pressure) {
    return read_draws(s, &seir_sampler::wb, false, first, count, within_pressure, between_pressure);
}
extern "C" int seir_sampler_read_wb_draws_async(seir_sampler *s, int32_t first, int32_t count, double *within_pressure,
                                                double *between_pressure) {
    return read_draws(s, &seir_sampler::wb, true, first, count, within_pressure, between_pressure);
}

extern "C" int seir_sampler_read_wb(seir_sampler *s, uint64_t *count, uint32_t *n, double *ref_w, double *sum_w, double *sumsq_w,
                                    double *ref_b, double *sum_b, uint32_t *gt) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = window_check(s, s->wb))) return rc;
    hipStream_t st = s->ctx->stream;
    const size_t cells = window_cells(s, s->wb);
    const WbBufs &wb = s->wbb;
    if (count) HIP_TRY(hipMemcpyAsync(count, wb.count, sizeof(uint64_t) * s->cfg.B, hipMemcpyDeviceToHost, st));
    const struct { double *dst; const double *src; } dbl[] = {{ref_w, wb.ref_w}, {sum_w, wb.sum_w}, {sumsq_w, wb.sumsq_w},
                                                              {ref_b, wb.ref_b}, {sum_b, wb.sum_b}};
    for (const auto &p : dbl)
        if (p.dst) HIP_TRY(hipMemcpyAsync(p.dst, p.src, sizeof(double) * cells, hipMemcpyDeviceToHost, st));
    if (n) HIP_TRY(hipMemcpyAsync(n, wb.n, sizeof(uint32_t) * cells, hipMemcpyDeviceToHost, st));
    if (gt) HIP_TRY(hipMemcpyAsync(gt, wb.gt, sizeof(uint32_t) * cells, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return check_ev_overflow(s);
}

// ---------------------------------------------------------------------------
// Group curves on the device: R_t and within / between per group (include/seir_hip.h; kernels: group_curve_kernels.h)
// ---------------------------------------------------------------------------
// Size the buffers of a family for the table, the switch and the product's window as they are now (none when any is off).
// The batch shrinks so that the product's integer plane and the cell plane(s) stay within the staging bound together.
static int gcurve_fit(seir_sampler *s, Window &w) {
    GroupCurve &c = w.curve;
    const int D = (c.on && s->grp_on && w.on) ? w.D : 0;
    if (D == c.b.D) return 0;
    if (int rc = drain(s)) return rc;
    c.b = {};
    if (D == 0) return 0;
    const Dims &d = s->ctx->d;
    const int B = s->cfg.B, G = s->grp.G;
    const int slots = staging_slots(s->ctx, w.slots, (size_t)B * d.Mp * D * (sizeof(int) + w.planes * sizeof(double)));
    const unsigned long long out_bytes = (unsigned long long)s->cfg.cap * B * G * D * 8ull;
    const unsigned long long cell_bytes = (unsigned long long)slots * B * D * d.Mp * 8ull;
    const unsigned long long bytes = (unsigned long long)w.planes * (out_bytes + cell_bytes);
    if (int rc = refuse_above_half_free(bytes, "the group curves need %llu bytes (%d planes x (%d slots x %d chains x %d groups x %d "
                                        "days x 8 + %llu of a batch's cells))", bytes, w.planes, s->cfg.cap, B, G, D, cell_bytes))
        return rc;
    // every buffer or none: a family whose outputs could not be made has none (D = 0) and is not launched for
    GroupCurve::Bufs b;
    int rc = b.offsets.upload(s->grp_offsets.data(), sizeof(int) * (size_t)(G + 1));
    for (int x = 0; x < w.planes && !rc; ++x)
        if (!(rc = b.out[x].zeroed((size_t)out_bytes))) rc = b.cells[x].zeroed((size_t)cell_bytes);
    if (rc) return alloc_failed(bytes, "group curves");
    gcurve_lds_attributes(d.Mp);
    b.D = D; b.slots = slots;
    c.b = std::move(b);
    return 0;
}

extern "C" int seir_sampler_group_rt(seir_sampler *s, const double *weights) {
    int rc = sampler_check(s);
    if (rc) return rc;
    GroupCurve &c = s->rt.curve;
    if (!weights) {
        if (c.on && (rc = drain(s))) return rc;
        c = GroupCurve{};                            // off: the weights belonged to the table that was in force
        return 0;
    }
    if ((rc = need_events(s, RT_USER.verb))) return rc;
    if (!s->grp_on) return fail(SEIR_ERR_STATE, "no group table is set: call seir_sampler_groups_set first");
    const size_t nnz = (size_t)s->grp_offsets[s->grp.G];
    for (size_t k = 0; k < nnz; ++k)
        if (!(fabs(weights[k]) < __builtin_inf())) return fail(SEIR_ERR_INVALID, "weights[%zu] is not finite", k);
    if ((rc = drain(s))) return rc;
    if ((rc = c.weights.upload(weights, sizeof(double) * nnz))) return rc;
    c.on = true;
    if ((rc = gcurve_fit(s, s->rt))) { c = GroupCurve{}; return rc; }
    return 0;
}

extern "C" int seir_sampler_group_wb(seir_sampler *s, int32_t on) {
    int rc = sampler_check(s);
    if (rc) return rc;
    GroupCurve &c = s->wb.curve;
    if (!on) {
        if (c.on && (rc = drain(s))) return rc;
        c = GroupCurve{};
        return 0;
    }
    if ((rc = need_events(s, WB_USER.verb))) return rc;
    if (!s->grp_on) return fail(SEIR_ERR_STATE, "no group table is set: call seir_sampler_groups_set first");
    c.on = true;
    if ((rc = gcurve_fit(s, s->wb))) { c.on = false; return rc; }
    return 0;
}

// What is behind the four readers of the group curves out [cap][B][G][D] of seir_sampler::rt or ::wb.
static int read_group_curves(seir_sampler *s, Window seir_sampler::*which, bool async, int32_t first, int32_t count, double *a,
                             double *b) {
    if (int rc = sampler_check(s)) return rc;
    const Window &w = s->*which;
    if (int rc = window_check(s, w, first, count)) return rc;
    const GroupCurve &c = w.curve;
    if (c.b.D == 0)
        return fail(SEIR_ERR_STATE, "%s", !c.on ? w.who.no_curve
                                              : "the group curves have no outputs: no table is set, or they were refused");
    const double *const src[2] = {c.b.out[0].as<double>(), c.b.out[1].as<double>()};
    return deliver_curves(s, w, async, src, (size_t)s->cfg.B * s->grp.G * c.b.D, first, count, a, b);
}

extern "C" int seir_sampler_read_group_rt(seir_sampler *s, int32_t first, int32_t count, double *Rg) {
    return read_group_curves(s, &seir_sampler::rt, false, first, count, Rg, nullptr);
}
extern "C" int seir_sampler_read_group_rt_async(seir_sampler *s, int32_t first, int32_t count, double *Rg) {
    return read_group_curves(s, &seir_sampler::rt, true, first, count, Rg, nullptr);
}
extern "C" int seir_sampler_read_group_wb(seir_sampler *s, int32_t first, int32_t count, double *Wg, double *Bg) {
    return read_group_curves(s, &seir_sampler::wb, false, first, count, Wg, Bg);
}
extern "C" int seir_sampler_read_group_wb_async(seir_sampler *s, int32_t first, int32_t count, double *Wg, double *Bg) {
    return read_group_curves(s, &seir_sampler::wb, true, first, count, Wg, Bg);
}

static void gcurve_wsums_launch(const Dims &d, hipStream_t st, const int *offsets, const int *members, const double *weights,
                                const double *v, int G, int L, long long ld, long long v_d0, long long out_d0, long long nd,
                                double *out);

extern "C" int seir_group_wsums(seir_ctx *ctx, const double *v, int64_t nd, int32_t L, int32_t M, int32_t G, const int32_t *offsets,
                                const int32_t *members, const double *weights, double *out) {
    int rc = check_batch(ctx, 1);
    if (rc) return rc;
    if (!v || !out) return fail(SEIR_ERR_INVALID, "null pointer");
    if (nd < 1 || M < 1 || L < 1 || nd > 0x7fffffffll)
        return fail(SEIR_ERR_INVALID, "nd=%lld, M=%d, L=%d: at least one of each, nd below 2^31", (long long)nd, M, L);
    std::vector<int> seg;
    if ((rc = groups_parse(G, offsets, members, M, seg))) return rc;
    const size_t nin = (size_t)nd * L * M, nout = (size_t)nd * G * L, nnz = (size_t)offsets[G];
    DevBuf dv, dout, doff, dmem, dw;
    if ((rc = dv.alloc(sizeof(double) * nin)) || (rc = dout.alloc(sizeof(double) * nout)) ||
        (rc = doff.alloc(sizeof(int) * (size_t)(G + 1))) || (rc = dmem.alloc(sizeof(int) * nnz)) ||
        (weights && (rc = dw.alloc(sizeof(double) * nnz))))
        return rc;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(dv.p, v, sizeof(double) * nin, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(doff.p, offsets, sizeof(int) * (size_t)(G + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dmem.p, members, sizeof(int) * nnz, hipMemcpyHostToDevice, st));
    if (weights) HIP_TRY(hipMemcpyAsync(dw.p, weights, sizeof(double) * nnz, hipMemcpyHostToDevice, st));
    gcurve_wsums_launch(whole(ctx, 1).d, st, doff.as<int>(), dmem.as<int>(), dw.as<double>(), dv.as<double>(), G, L, M, 0, 0, nd,
                        dout.as<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, dout.p, sizeof(double) * nout, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int seir_host_alloc(void **p, uint64_t bytes) {
    if (!p) return fail(SEIR_ERR_INVALID, "null pointer");
    HIP_TRY(hipHostMalloc(p, bytes ? bytes : 8, hipHostMallocDefault));
    return 0;
}
extern "C" int seir_host_free(void *p) {
    HIP_TRY(hipHostFree(p));
    return 0;
}

extern "C" int seir_sampler_time_grad_kernel(seir_sampler *s, int32_t iters, float *mean_ms) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if (!s->have_state) return fail(SEIR_ERR_STATE, "no chain state set");
    if (!mean_ms || iters < 1) return fail(SEIR_ERR_INVALID, "bad iters/mean_ms");
    seir_ctx *ctx = s->ctx;
    LaunchCfg l = whole(ctx, s->cfg.B);
    l.d.chunked = plan_sweep(sweep_inputs(s, 0)).ts_mode;   // as in the sweep
    launch_se<1>(ctx, l, true);
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    for (int i = 0; i < iters; ++i) launch_se<1>(ctx, l, true);
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    HIP_TRY(hipGetLastError());
    *mean_ms = ms / iters;
    return 0;
}

extern "C" int seir_sampler_time_leapfrog(seir_sampler *s, int32_t sweeps, float *mean_ms, int32_t *launches, int32_t *evals) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if (!s->have_state) return fail(SEIR_ERR_STATE, "no chain state set");
    if (!mean_ms || sweeps < 1 || sweeps > 4096) return fail(SEIR_ERR_INVALID, "bad sweeps/mean_ms");
    if (s->use_graph || s->ngroups != 1) return fail(SEIR_ERR_STATE, "timing of the leapfrog section needs stream launches on one stream");
    while (s->prof_ev.size() < (size_t)2 * sweeps) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        s->prof_ev.push_back(e);
    }
    s->prof_i = 0;
    rc = seir_sampler_run(s, sweeps);
    const int recorded = s->prof_i;
    s->prof_i = -1;
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    if (recorded < 1) return fail(SEIR_ERR_STATE, "this sampler's sweep has no chunked leapfrog section (hmc_mode 1 or fewer than 3 leapfrog steps)");
    double sum = 0.0;
    for (int i = 0; i < recorded; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, s->prof_ev[2 * i], s->prof_ev[2 * i + 1]));
        sum += ms;
    }
    *mean_ms = (float)(sum / recorded);
    const SweepPlan p = plan_sweep(sweep_inputs(s, 0));
    if (launches) *launches = p.section_launches;
    if (evals) *evals = p.section_evals;
    return 0;
}

extern "C" int seir_sampler_pair_timeouts(seir_sampler *s, uint32_t *out) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if (!out) return fail(SEIR_ERR_INVALID, "null pointer");
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    std::vector<uint32_t> both((size_t)2 * s->cfg.B, 0u);
    HIP_TRY(hipMemcpy(both.data(), s->ch.late, sizeof(uint32_t) * both.size(), hipMemcpyDeviceToHost));
    for (int b = 0; b < s->cfg.B; ++b) out[b] = both[b] + both[(size_t)s->cfg.B + b];
    return 0;
}

#if STAMPS_ON
// The stamped developer builds (stamps.h; tools/dev/stamps.py): the build's family region, read once everything enqueued has
// finished.  reset: afterwards the region is rewritten by the table's pattern -- min-words ~0, every other word 0.
static void stamps_reset_pattern(std::vector<unsigned long long> &h, int B) {
    for (size_t i = 0; i < h.size(); ++i) h[i] = stamps::min_word(stamps::FAMILY, B, i) ? ~0ull : 0ull;
}
// the sampler's families (SEIR, PAIR, LEAP, TAIL): words [0, n_words) of Chains::stamps
extern "C" int seir_stamps_read(seir_sampler *s, unsigned long long *out, int64_t n_words, int reset) {
    constexpr bool mine = stamps::FAMILY == stamps::F_SEIR || stamps::FAMILY == stamps::F_PAIR || stamps::FAMILY == stamps::F_LEAP ||
                          stamps::FAMILY == stamps::F_TAIL;
    const size_t ext = stamps::extent(stamps::FAMILY, s->cfg.B);
    static_assert(stamps::extent(stamps::F_SEIR, 1) <= stamps::buffer_words(1), "the buffer holds every family");
    if (!mine) return fail(SEIR_ERR_STATE, "this build's stamp family belongs to the context: seir_stamps_read_ctx");
    if (!out || n_words < 0 || (size_t)n_words > ext || ext > stamps::buffer_words(s->cfg.B))
        return fail(SEIR_ERR_INVALID, "stamps: %lld words asked for, the family's region has %zu", (long long)n_words, ext);
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    HIP_TRY(hipMemcpy(out, s->ch.stamps, (size_t)n_words * 8, hipMemcpyDeviceToHost));
    if (reset) {
        std::vector<unsigned long long> h(ext);
        stamps_reset_pattern(h, s->cfg.B);
        HIP_TRY(hipMemcpy(s->ch.stamps, h.data(), ext * 8, hipMemcpyHostToDevice));
    }
    return 0;
}
// the context's families.  SE: the tile scalars [tiles][4] (words 2 and 3 of a tile are its stamps; every launch rewrites them:
// no reset); EVAL: the words behind the counters of the last launch's chains
extern "C" int seir_stamps_read_ctx(seir_ctx *ctx, unsigned long long *out, int64_t n_words, int reset) {
    if (!out || n_words < 0) return fail(SEIR_ERR_INVALID, "stamps: null pointer or negative count");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (stamps::FAMILY == stamps::F_SE) {
        if (!ctx->w.TS || (size_t)n_words > (size_t)ctx->Bmax * ctx->d.nmt * ctx->d.ntc * stamps::SE_NW)
            return fail(SEIR_ERR_INVALID, "stamps: the tile scalars hold %d x %d x %d tiles of 4 words", ctx->Bmax, ctx->d.nmt, ctx->d.ntc);
        HIP_TRY(hipMemcpy(out, ctx->w.TS, (size_t)n_words * 8, hipMemcpyDeviceToHost));
        return 0;
    }
    if (stamps::FAMILY != stamps::F_EVAL) return fail(SEIR_ERR_STATE, "this build's stamp family belongs to the sampler: seir_stamps_read");
    if (!ctx->eval_cnt || ctx->eval_nb < 1 || n_words > stamps::EVAL_WORDS)
        return fail(SEIR_ERR_INVALID, "stamps: no one-launch evaluation yet, or more than %d words", stamps::EVAL_WORDS);
    static_assert(stamps::EVAL_WORDS <= 16, "the spare words behind the counters (launch_eval_all)");
    unsigned long long *base = ctx->eval_cnt + (size_t)((ctx->eval_nb + 7) / 8 * 8) * EVC_STRIDE;
    HIP_TRY(hipMemcpy(out, base, (size_t)n_words * 8, hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(base, 0, stamps::EVAL_WORDS * 8));
    return 0;
}
#endif

// ===========================================================================
// Region totals: the launch (declared above, with the rest of seir_sampler_groups_*)
// ===========================================================================
static void groups_launch(const Dims &d, hipStream_t st, const GroupTable &gt, bool ev16, const void *ev, int M, int L,
                          long long ev_d0, long long out_d0, long long nd, int64_t *out, const int *St0, long long plane, int ndp,
                          int64_t *state0) {
    const int nchunk = (L + 63) / 64;
    for (long long off = 0; off < nd; off += GRP_NDMAX) {
        const dim3 grid((unsigned)(gt.nseg * nchunk), (unsigned)std::min<long long>(GRP_NDMAX, nd - off)), block(64 * GRP_WAVES);
        hipLaunchKernelGGL(ev16 ? k_group_sums<1> : k_group_sums<0>, grid, block, 0, st, d, gt, ev, M, L, nchunk, ev_d0 + off,
                           out_d0 + off, (unsigned long long *)out, St0, plane, ndp, (unsigned long long *)state0);
    }
}

// ===========================================================================
// Group curves: the launches (declared above, with seir_sampler_rt / _wb and the rest of seir_sampler_group_*).  The header
// is included here, so that its kernels lie behind every kernel the parent had.
// ===========================================================================
#include "group_curve_kernels.h"

static void gcurve_wsums_launch(const Dims &d, hipStream_t st, const int *offsets, const int *members, const double *weights,
                                const double *v, int G, int L, long long ld, long long v_d0, long long out_d0, long long nd,
                                double *out) {
    const int nchunk = (L + GC_WAVES - 1) / GC_WAVES;
    for (long long off = 0; off < nd; off += GRP_NDMAX) {
        const dim3 grid((unsigned)(G * nchunk), (unsigned)std::min<long long>(GRP_NDMAX, nd - off)), block(64 * GC_WAVES);
        hipLaunchKernelGGL(weights ? k_group_wsums<1> : k_group_wsums<0>, grid, block, 0, st, d, offsets, members, weights, v, G, L,
                           ld, nchunk, v_d0 + off, out_d0 + off, out);
    }
}

// The batch's cell planes [nj * B][D][Mp] onto out [.][B][G][D] from slot slot0.
static void gcurve_sums(seir_sampler *s, const LaunchCfg &l, const Window &w, int slot0, int nj) {
    const GroupCurve &c = w.curve;
    const int B = s->cfg.B;
    for (int x = 0; x < w.planes; ++x)
        gcurve_wsums_launch(l.d, l.st, c.b.offsets.as<int>(), s->grp.members, c.weights.as<double>(), c.b.cells[x].as<double>(),
                            s->grp.G, w.D, l.d.Mp, 0, (long long)slot0 * B, (long long)nj * B, c.b.out[x].as<double>());
}

static void gcurve_rt_trace_cells(seir_sampler *s, const LaunchCfg &l, int slot0, int nj) {
    const RtBufs &rb = s->rtb;
    const int B = s->cfg.B;
    hipLaunchKernelGGL(k_rt_trace_cells<RT_DT>, dim3(rb.ncb, (rb.D + RT_DT - 1) / RT_DT, B), dim3(256),
                       k_rt_trace_lds_bytes<RT_DT>(l.d.Mp), l.st, l.d, s->ctx->c, rb, (const double *)s->ch.tr_theta, B, slot0, nj,
                       s->rt.curve.b.cells[0].as<double>(), (long long)l.d.Mp);
}

static void gcurve_rt_gather(seir_sampler *s, const LaunchCfg &l, long long pos0, int nj) {
    const int B = s->cfg.B, D = s->rt.D;
    hipLaunchKernelGGL(k_rt_cells_from_keep, dim3((l.d.M + 255) / 256, D, B), dim3(256), 0, l.st, l.d, s->keep_rt.buf.as<const double>(),
                       s->keep_rt.stride, pos0, B, D, nj, s->rt.curve.b.cells[0].as<double>(), (long long)l.d.Mp);
}

static void gcurve_wb_trace_cells(seir_sampler *s, const LaunchCfg &l, int slot0, int nj) {
    const WbBufs &wb = s->wbb;
    const int B = s->cfg.B;
    hipLaunchKernelGGL(k_wb_trace_cells<WB_DT>, dim3(wb.ncb, (wb.D + WB_DT - 1) / WB_DT, B), dim3(256),
                       k_wb_trace_lds_bytes<WB_DT>(l.d.Mp), l.st, l.d, s->ctx->c, wb, (const double *)s->ch.tr_theta, B, slot0, nj,
                       s->wb.curve.b.cells[0].as<double>(), s->wb.curve.b.cells[1].as<double>(), (long long)l.d.Mp);
}

// Above 64 KiB of dynamic LDS a kernel needs the attribute (as k_rt_trace and k_wb_trace get theirs at their resets).
static void gcurve_lds_attributes(int Mp) {
    (void)lds_attribute((const void *)k_rt_trace_cells<RT_DT>, k_rt_trace_lds_bytes<RT_DT>(Mp));
    (void)lds_attribute((const void *)k_wb_trace_cells<WB_DT>, k_wb_trace_lds_bytes<WB_DT>(Mp));
}

// ===========================================================================
// Group next-generation matrix on the device (include/seir_hip.h; kernel: ngm_kernels.h).  The header is included here,
// behind the group curves' launches, so that its kernel lies behind every kernel the parent had.
// ===========================================================================
#include "ngm_kernels.h"

// nd draws of the planes rb.ea / rb.S (theta: trace slot first + nd / B, chain nd % B) into P [nd][G][D][ld].
static void ngm_rows_launch(const Dims &d, const Consts &c, hipStream_t st, const RtBufs &rb, const double *theta, int B, int first,
                            long long nd, const int *offsets, const int *members, int G, double *P, long long ld) {
    const size_t lds = k_rt_trace_lds_bytes<RT_DT>(d.Mp);
    for (long long off = 0; off < nd; off += NGM_NDMAX) {
        const dim3 grid((unsigned)rb.ncb, (unsigned)((rb.D + RT_DT - 1) / RT_DT), (unsigned)std::min<long long>(NGM_NDMAX, nd - off));
        hipLaunchKernelGGL(k_ngm_rows<RT_DT>, grid, dim3(256), lds, st, d, c, rb, theta, B, first, (int)off, offsets, members, G, P, ld);
    }
}

// Above 64 KiB of dynamic LDS the kernel needs the attribute (as k_rt_trace gets its own at the rt reset).
static void ngm_lds_attribute(int Mp) {
    (void)lds_attribute((const void *)k_ngm_rows<RT_DT>, k_rt_trace_lds_bytes<RT_DT>(Mp));
}

static void ngm_launch(seir_sampler *s, const LaunchCfg &l, int slot0, long long pos0, int nj) {
    const GroupNgm &n = s->ngm;
    const int B = s->cfg.B, G = s->grp.G;
    ngm_rows_launch(l.d, s->ctx->c, l.st, s->rtb, (const double *)s->ch.tr_theta, B, slot0, (long long)nj * B, n.offsets.as<int>(),
                    s->grp.members, G, n.P.as<double>(), (long long)l.d.Mp);
    // K [pos][b][g][h][t]: the group sums of P [nd][g][t][.] over the members of h, (draw, g) as the "draw" axis
    gcurve_wsums_launch(l.d, l.st, n.offsets.as<int>(), s->grp.members, n.weights.as<double>(), n.P.as<double>(), G, n.D, l.d.Mp, 0,
                        pos0 * B * G, (long long)nj * B * G, n.out.as<double>());
}

extern "C" int seir_sampler_group_ngm(seir_sampler *s, const double *weights, int64_t cap) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if (!weights || cap == 0) {
        if (s->ngm.cap && (rc = drain(s))) return rc;
        s->ngm = GroupNgm{};
        return 0;
    }
    if ((rc = need_events(s, RT_USER.verb))) return rc;
    if (cap < 0 || cap > (1ll << 20))
        return fail(SEIR_ERR_INVALID, "cap=%lld outside [0, 2^20]: the draws per chain between two resets", (long long)cap);
    if (!s->grp_on) return fail(SEIR_ERR_STATE, "no group table is set: call seir_sampler_groups_set first");
    if (!s->rt.on) return fail(SEIR_ERR_STATE, "%s", RT_USER.not_enabled);
    if (s->rt.acc.j != 0)
        return fail(SEIR_ERR_STATE, "%lld draws per chain have been folded since the reset: the draw store is sized between "
                    "seir_sampler_rt_reset and the first seir_sampler_rt", s->rt.acc.j);
    const Dims &d = s->ctx->d;
    const int B = s->cfg.B, G = s->grp.G, D = s->rt.D;
    const size_t nnz = (size_t)s->grp_offsets[G];
    for (size_t k = 0; k < nnz; ++k)
        if (!(fabs(weights[k]) < __builtin_inf())) return fail(SEIR_ERR_INVALID, "weights[%zu] is not finite", k);
    if ((rc = drain(s))) return rc;
    s->ngm = GroupNgm{};                             // a refusal or failure below leaves it off
    // the staging bound covers the S plane, the cell plane of group R_t and P together: the batch shrinks accordingly
    const int slots = staging_slots(s->ctx, s->rt.slots, (size_t)B * d.Mp * D * (sizeof(int) + sizeof(double) + (size_t)G * sizeof(double)));
    const unsigned long long out_bytes = (unsigned long long)cap * B * G * G * D * 8ull;
    const unsigned long long p_bytes = (unsigned long long)slots * B * G * D * d.Mp * 8ull;
    if ((rc = refuse_above_half_free(out_bytes + p_bytes, "the group next-generation matrix needs %llu bytes (%lld draws x %d chains x "
                                     "%d x %d groups x %d days x 8 + %llu of a batch's rows)", out_bytes + p_bytes, (long long)cap, B,
                                     G, G, D, p_bytes)))
        return rc;
    GroupNgm n;
    if (n.offsets.upload(s->grp_offsets.data(), sizeof(int) * (size_t)(G + 1)) || n.weights.upload(weights, sizeof(double) * nnz) ||
        n.out.zeroed((size_t)out_bytes) || n.P.zeroed((size_t)p_bytes))
        return alloc_failed(out_bytes + p_bytes, "the group next-generation matrix");
    ngm_lds_attribute(d.Mp);
    n.cap = cap; n.D = D; n.slots = slots;
    s->ngm = std::move(n);
    return 0;
}

extern "C" int seir_sampler_read_group_ngm(seir_sampler *s, int64_t first_draw, int64_t count, double *out) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = window_check(s, s->rt))) return rc;
    if (!s->ngm.cap)
        return fail(SEIR_ERR_STATE, "the group next-generation matrix is not enabled: call seir_sampler_group_ngm behind "
                    "seir_sampler_rt_reset (a new table, another window or a refusal switches it off)");
    if (first_draw < 0 || count < 0 || first_draw + count > s->rt.acc.j)
        return fail(SEIR_ERR_INVALID, "draws [%lld,%lld) outside the %lld folded since the reset", (long long)first_draw,
                    (long long)(first_draw + count), s->rt.acc.j);
    if (!out) return fail(SEIR_ERR_INVALID, "null pointer");
    const size_t row = (size_t)s->cfg.B * s->grp.G * s->grp.G * s->ngm.D;
    if (count)
        HIP_TRY(hipMemcpyAsync(out, s->ngm.out.as<double>() + (size_t)first_draw * row, sizeof(double) * (size_t)count * row, hipMemcpyDeviceToHost,
                               s->ctx->stream));
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    return check_ev_overflow(s);
}

extern "C" int seir_group_ngm_rows(seir_ctx *ctx, int32_t n, const double *theta, const int32_t *events, int32_t days, int32_t G,
                                   const int32_t *offsets, const int32_t *members, double *out) {
    int rc = check_batch(ctx, 1);
    if (rc) return rc;
    if (!theta || !events || !out) return fail(SEIR_ERR_INVALID, "null pointer");
    const Dims d = whole(ctx, 1).d;
    if (n < 1) return fail(SEIR_ERR_INVALID, "n=%d: at least one draw", n);
    if (days < 1 || days > d.T) return fail(SEIR_ERR_INVALID, "days=%d outside [1, T = %d]", days, d.T);
    std::vector<int> seg;
    if ((rc = groups_parse(G, offsets, members, d.M, seg))) return rc;
    const int D = days;
    const size_t nnz = (size_t)offsets[G];
    // a batch's planes (events, S, P) stay within the staging bound; at least one draw is always taken
    const size_t ev_draw = (size_t)d.M * d.T * 3, p_draw = (size_t)G * D * d.M;
    const int nb = staging_slots(ctx, std::min<size_t>((size_t)n, NGM_NDMAX),
                                 ev_draw * sizeof(int) + (size_t)d.Mp * D * sizeof(int) + p_draw * sizeof(double));
    RtBufs rb{};
    rb.D = D; rb.t0 = d.T - D; rb.ncb = (d.M + 63) / 64;
    DevBuf dth, dev, dea, dS, dP, doff, dmem;
    if ((rc = dth.alloc(sizeof(double) * nb * d.P)) || (rc = dev.alloc(sizeof(int) * nb * ev_draw)) ||
        (rc = dea.alloc(sizeof(double) * nb * d.Tp)) || (rc = dS.alloc(sizeof(int) * (size_t)nb * d.Mp * D)) ||
        (rc = dP.alloc(sizeof(double) * nb * p_draw)) || (rc = doff.alloc(sizeof(int) * (size_t)(G + 1))) ||
        (rc = dmem.alloc(sizeof(int) * nnz)))
        return rc;
    rb.ea = dea.as<double>(); rb.S = dS.as<int>();
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(doff.p, offsets, sizeof(int) * (size_t)(G + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dmem.p, members, sizeof(int) * nnz, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(dS.p, 0, sizeof(int) * (size_t)nb * d.Mp * D, st));
    ngm_lds_attribute(d.Mp);
    Work tw = ctx->w;                                 // k_rt_tables writes Work::ea: a buffer of this call's own
    tw.ea = rb.ea;
    for (int s0 = 0; s0 < n; s0 += nb) {
        const int nj = std::min(nb, n - s0);
        HIP_TRY(hipMemcpyAsync(dth.p, theta + (size_t)s0 * d.P, sizeof(double) * nj * d.P, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(dev.p, events + (size_t)s0 * ev_draw, sizeof(int) * nj * ev_draw, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_rt_tables, dim3(nj), dim3(256), 0, st, d, tw, dth.as<double>());
        hipLaunchKernelGGL(k_rt_prepare<0>, dim3((d.M + RT_PREP_ROWS - 1) / RT_PREP_ROWS, nj), dim3(64 * RT_PREP_ROWS), 0, st, d,
                           ctx->c, rb, (const void *)dev.p, 1, 0);
        ngm_rows_launch(d, ctx->c, st, rb, dth.as<double>(), 1, 0, nj, doff.as<int>(), dmem.as<int>(), G, dP.as<double>(), d.M);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out + (size_t)s0 * p_draw, dP.p, sizeof(double) * nj * p_draw, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return 0;
}

// ---------------------------------------------------------------------------
// Stored draws into trace slots (include/seir_hip.h; kernels: trace_load_kernels.h)
// ---------------------------------------------------------------------------
#include "trace_load_kernels.h"

static int load_words_clear(seir_sampler *s, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(s->load_words, 0, sizeof(unsigned long long) * LOAD_ST_FIRST_KEY, st));
    HIP_TRY(hipMemsetAsync(s->load_words + LOAD_ST_FIRST_KEY, 0xff, sizeof(unsigned long long), st));
    s->load_calls.clear();
    return 0;
}

extern "C" int seir_sampler_load_trace(seir_sampler *s, int32_t chain, int32_t first, int32_t count, const double *theta,
                                       const double *events) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if (!s->record_events)
        return fail(SEIR_ERR_STATE, "sampler was created with record_events=0: there is no event trace to load stored draws into");
    const int B = s->cfg.B;
    if (chain < 0 || chain >= B) return fail(SEIR_ERR_INVALID, "chain=%d outside [0, %d)", chain, B);
    if (first < 0 || count < 0 || (long long)first + count > s->cfg.cap)
        return fail(SEIR_ERR_INVALID, "trace range [%d,%lld) outside capacity %d", first, (long long)first + count, s->cfg.cap);
    if (count == 0) return 0;
    if (!theta || !events) return fail(SEIR_ERR_INVALID, "null pointer");
    seir_ctx *ctx = s->ctx;
    const LaunchCfg l = whole(ctx, B);
    const Dims &d = l.d;
    const size_t ev_draw = (size_t)d.M * d.T * 3, draw = ev_draw + (size_t)d.P;
    if ((unsigned long long)count * std::max(ev_draw, (size_t)d.P) >= (1ull << (LOAD_KEY_BITS - 3)))
        return fail(SEIR_ERR_INVALID, "count=%d: the call's %zu items per draw do not fit the key of the first bad item", count,
                    std::max(ev_draw, (size_t)d.P));
    if (!s->load_stage) {                              // the first load of this sampler
        const int slots = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min(LOAD_JMAX, s->cfg.cap),
                                                                    LOAD_STAGING_BYTES / (draw * sizeof(double))));
        if (!s->ev_load) HIP_TRY(hipEventCreateWithFlags(&s->ev_load, hipEventDisableTiming));
        double *stage = nullptr;
        S_ALLOC(allocs, stage, (size_t)slots * draw);
        const bool words = !s->load_words;
        if (words) S_ALLOC(allocs, s->load_words, (size_t)LOAD_ST_FIRST_KEY + 1);
        if (rc) return rc;
        if (words && (rc = load_words_clear(s, l.st))) return rc;
        s->load_stage = stage;
        s->load_slots = slots;
    }
    // the call's tag: the number of calls since the last clear; past 2^20 - 1 they share the last one
    const size_t tag = std::min<size_t>(s->load_calls.size(), ((size_t)1 << 20) - 1);
    if (tag == s->load_calls.size()) s->load_calls.emplace_back(chain, first);
    LoadArgs a{};
    a.status = s->load_words;
    a.tag = (unsigned long long)tag << LOAD_KEY_BITS;
    a.chain = chain;
    for (int j0 = 0; j0 < count; j0 += s->load_slots) {
        const int nj = std::min(s->load_slots, count - j0);
        double *st_ev = s->load_stage, *st_th = s->load_stage + (size_t)s->load_slots * ev_draw;
        HIP_TRY(hipMemcpyAsync(st_ev, events + (size_t)j0 * ev_draw, sizeof(double) * nj * ev_draw, hipMemcpyHostToDevice, l.st));
        HIP_TRY(hipMemcpyAsync(st_th, theta + (size_t)j0 * d.P, sizeof(double) * nj * d.P, hipMemcpyHostToDevice, l.st));
        HIP_TRY(hipEventRecord(s->ev_load, l.st));
        a.ev = st_ev; a.theta = st_th; a.first = first + j0; a.j0 = j0;
        const dim3 grid((d.M + LOAD_ROWS - 1) / LOAD_ROWS, nj), block(64 * LOAD_ROWS);
        if (s->cfg.ev16) hipLaunchKernelGGL(k_trace_load<1>, grid, block, 0, l.st, d, ctx->c, a, (void *)s->ch.tr_events, B);
        else hipLaunchKernelGGL(k_trace_load<0>, grid, block, 0, l.st, d, ctx->c, a, (void *)s->ch.tr_events, B);
        hipLaunchKernelGGL(k_trace_load_theta<LOAD_THETA_THREADS>, dim3(nj), dim3(LOAD_THETA_THREADS), 0, l.st, d, a, s->ch.tr_theta, s->ch.tr_hmc, s->ch.tr_mv, B);
        HIP_TRY(hipGetLastError());
    }
    // the host buffers may be reused once the last copy is done; the kernels behind it are not waited for
    HIP_TRY(hipEventSynchronize(s->ev_load));
    return 0;
}

extern "C" int seir_sampler_load_status(seir_sampler *s, uint64_t out[8], int32_t clear) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if (!out) return fail(SEIR_ERR_INVALID, "null pointer");
    for (int i = 0; i < LOAD_ST_WORDS; ++i) out[i] = 0;
    if (!s->load_words) return 0;                      // nothing was ever loaded
    hipStream_t st = s->ctx->stream;
    unsigned long long w[LOAD_ST_FIRST_KEY + 1];
    HIP_TRY(hipMemcpyAsync(w, s->load_words, sizeof(w), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < LOAD_ST_FIRST_KEY; ++i) out[i] = w[i];
    if (w[LOAD_ST_FIRST_KEY] != ~0ull) {
        const size_t tag = (size_t)(w[LOAD_ST_FIRST_KEY] >> LOAD_KEY_BITS);
        out[LOAD_ST_FIRST_KEY] = w[LOAD_ST_FIRST_KEY] & ((1ull << LOAD_KEY_BITS) - 1);
        if (tag < s->load_calls.size()) {
            out[LOAD_ST_CHAIN] = (uint64_t)s->load_calls[tag].first;
            out[LOAD_ST_FIRST] = (uint64_t)s->load_calls[tag].second;
        }
    }
    return clear ? load_words_clear(s, st) : 0;
}

// ---------------------------------------------------------------------------
// Scenario forecasts: the fold of the paired differences (include/seir_hip.h; kernel: scenario_kernels.h)
// ---------------------------------------------------------------------------
#include "scenario_kernels.h"

// Draws [j0, j0 + nj) per chain of the two staging tensors into a scenario's accumulators; nj <= SC_JMAX.
static void scenario_diff_launch(const Dims &d, hipStream_t st, const ScenarioDiffBufs &o, const int *fev, const int *sev, int M,
                                 int H, int B, int nj, bool fresh) {
    hipLaunchKernelGGL(k_scenario_diff<SC_U>, dim3((M + SC_ROWS - 1) / SC_ROWS, B), dim3(64 * SC_ROWS), 0, st, d, o, fev, sev, M,
                       H, B, nj, fresh ? 1 : 0);
}

extern "C" int seir_scenario_diffs(seir_ctx *ctx, const int32_t *base_events, const int32_t *scenario_events, int64_t n, int32_t B,
                                   int32_t M, int32_t H, uint64_t folded, int32_t *ref, int64_t *sum, uint64_t *sumsq,
                                   uint32_t *lt, uint32_t *eq, uint32_t *overflow) {
    int rc = check_batch(ctx, 1);
    if (rc) return rc;
    if (!base_events || !scenario_events || !ref || !sum || !sumsq || !lt || !eq || !overflow)
        return fail(SEIR_ERR_INVALID, "null pointer");
    if (n < 1 || B < 1 || M < 1 || B > 65535)
        return fail(SEIR_ERR_INVALID, "n=%lld, B=%d, M=%d: at least one of each, B at most 65535", (long long)n, B, M);
    if (H < 1 || H > SEIR_FORECAST_MAX_H) return fail(SEIR_ERR_INVALID, "H=%d outside [1, %d]", H, SEIR_FORECAST_MAX_H);
    if (folded > 0xffffffffull || folded + (uint64_t)n > 0xffffffffull)
        return fail(SEIR_ERR_INVALID, "%llu draws per chain folded and %lld more: the comparison counts hold 2^32 - 1",
                    (unsigned long long)folded, (long long)n);
    const size_t cells = (size_t)B * M * H * SCENARIO_Q, draw = (size_t)B * M * H * 3;
    const unsigned long long bytes = 2ull * (unsigned long long)n * draw * sizeof(int32_t) + cells * 28ull;
    if ((rc = refuse_above_half_free(bytes, "the scenario differences need %llu bytes (2 x %lld draws x %d chains x %d locations x "
                                            "%d days x 3 x 4)", bytes, (long long)n, B, M, H)))
        return rc;
    DevBuf dfev, dsev, dacc;
    if ((rc = dfev.alloc(sizeof(int32_t) * n * draw)) || (rc = dsev.alloc(sizeof(int32_t) * n * draw)) ||
        (rc = dacc.alloc(cells * 28 + 8)))
        return rc;
    // one block, the 64-bit arrays first: sum | sumsq | ref | lt | eq | overflow
    ScenarioDiffBufs o{};
    o.sum = dacc.as<int64_t>();
    o.sumsq = (uint64_t *)(o.sum + cells);
    o.ref = (int32_t *)(o.sumsq + cells);
    o.lt = (uint32_t *)(o.ref + cells);
    o.eq = o.lt + cells;
    o.overflow = (unsigned *)(o.eq + cells);
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(dfev.p, base_events, sizeof(int32_t) * n * draw, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dsev.p, scenario_events, sizeof(int32_t) * n * draw, hipMemcpyHostToDevice, st));
    if (folded) {
        HIP_TRY(hipMemcpyAsync(o.sum, sum, sizeof(int64_t) * cells, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(o.sumsq, sumsq, sizeof(uint64_t) * cells, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(o.ref, ref, sizeof(int32_t) * cells, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(o.lt, lt, sizeof(uint32_t) * cells, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(o.eq, eq, sizeof(uint32_t) * cells, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(o.overflow, overflow, sizeof(uint32_t), hipMemcpyHostToDevice, st));
    } else {
        HIP_TRY(hipMemsetAsync(o.overflow, 0, sizeof(uint32_t), st));
    }
    const Dims d = whole(ctx, 1).d;
    for (int64_t j0 = 0; j0 < n; j0 += SC_JMAX) {
        const int nj = (int)std::min<int64_t>(SC_JMAX, n - j0);
        scenario_diff_launch(d, st, o, dfev.as<int>() + (size_t)j0 * draw, dsev.as<int>() + (size_t)j0 * draw, M, H, B, nj,
                             folded == 0 && j0 == 0);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(sum, o.sum, sizeof(int64_t) * cells, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(sumsq, o.sumsq, sizeof(uint64_t) * cells, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(ref, o.ref, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(lt, o.lt, sizeof(uint32_t) * cells, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(eq, o.eq, sizeof(uint32_t) * cells, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(overflow, o.overflow, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// ---- scenarios riding on the sampler's forecast ----
// The begin and day launches of a local set (seir_sampler_scenarios_set_local).  Defined at the end of this file, behind
// scenario_local_kernels.h: a kernel template is emitted where it is first named, and its kernels lie behind every kernel the
// parent had.
static void scenarios_local_rollout(seir_sampler *s, const LaunchCfg &l, const ForecastBufs &fb, const ScenarioBufs &sb,
                                    const RolloutBatch &bt, int j);
// The same of a triggered set (seir_sampler_scenarios_set_triggered), and the fold of its masks behind the days: behind
// scenario_trigger_kernels.h, which is included behind scenario_local_kernels.h.
static void scenarios_trigger_rollout(seir_sampler *s, const LaunchCfg &l, const ForecastBufs &fb, const ScenarioBufs &sb,
                                      const RolloutBatch &bt, int32_t first, int j);
static void scenarios_trigger_fold(seir_sampler *s, const LaunchCfg &l, const RolloutBatch &bt, int k, long long j);

// The rollout of a batch's K column blocks, whichever set rolls it: `begin` over `elems` elements of every block's planes, then
// the H days over the K ndp columns with day(grid, block, h), the set's day launch.
// launch_begin(grid, block) is the set's begin launch: a triggered set's takes more than a ScenarioBegin's arguments.
using ScenarioBegin = void (*)(Dims, Consts, ForecastBufs, ScenarioBufs, int, int);
template <typename Begin, typename Day>
static void scenarios_rollout_with(seir_ctx *ctx, const LaunchCfg &l, const ForecastBufs &fb, const ScenarioBufs &sb,
                                   const RolloutBatch &bt, size_t elems, Begin launch_begin, Day day) {
    const int cols = sb.K * bt.ndp;
    launch_begin(dim3((unsigned)((elems + SC_BEGIN_THREADS - 1) / SC_BEGIN_THREADS), sb.K), dim3(SC_BEGIN_THREADS));
    const dim3 grid(cols / 64, (l.d.M + FC_DAY_ROWS - 1) / FC_DAY_ROWS), block(64 * FC_DAY_ROWS);
    rollout_day_loop(ctx, l, sb.X, sb.F, cols, fb.H, [&](int h) { day(grid, block, h); });
}
template <typename Day>
static void scenarios_rollout(seir_ctx *ctx, const LaunchCfg &l, const ForecastBufs &fb, const ScenarioBufs &sb,
                              const RolloutBatch &bt, ScenarioBegin begin, size_t elems, Day day) {
    scenarios_rollout_with(ctx, l, fb, sb, bt, elems, [&](dim3 grid, dim3 block) {
        hipLaunchKernelGGL(begin, grid, block, 0, l.st, l.d, ctx->c, fb, sb, bt.ND, bt.ndp);
    }, day);
}

// Scenario k's parts of the one block (ScenarioSet::acc): the moments into mb's accumulator pointers, the differences into df.
static void scenarios_layout(const ScenarioSet &sc, int k, MomentBufs &mb, ScenarioDiffBufs &df) {
    uint64_t *w8 = sc.acc.buf.as<uint64_t>() + (size_t)k * sc.words8();
    mb.sum = (int64_t *)w8;
    mb.sumsq = w8 + sc.c6;
    mb.count = w8 + 2 * sc.c6;
    df.sum = (int64_t *)(w8 + 2 * sc.c6 + sc.count_words());
    df.sumsq = w8 + 2 * sc.c6 + sc.count_words() + sc.c4;
    uint32_t *w4 = (uint32_t *)(sc.acc.buf.as<uint64_t>() + (size_t)sc.K * sc.words8()) + (size_t)k * sc.words4();
    mb.ref = (int32_t *)w4;
    df.ref = (int32_t *)(w4 + sc.c6);
    df.lt = w4 + sc.c6 + sc.c4;
    df.eq = w4 + sc.c6 + 2 * sc.c4;
    mb.overflow = w4 + sc.c6 + 3 * sc.c4;
    df.overflow = mb.overflow + 1;
}

// Behind a forecast reset (and the set itself): W_k from the reset's calendar, the accumulators zero, and what the snapshots
// hold of them dropped -- but for a slot whose snapshot holds the forecast's block: that was taken at j = 0, and so holds
// these zeros too.
static int scenarios_begin(seir_sampler *s) {
    ScenarioSet &sc = s->scen;
    const int H = s->fc.fb.H;
    hipStream_t st = s->ctx->stream;
    const size_t M = sc.local() ? (size_t)s->ctx->d.M : 1;
    std::vector<double> wk((size_t)sc.K * H * M), wk_on;
    if (sc.triggered()) {                             // the on pair's, by the same rounded multiply
        wk_on.resize(wk.size());
        for (int k = 0; k < sc.K; ++k)
            for (size_t m = 0; m < M; ++m)
                for (int h = 0; h < H; ++h)
                    wk_on[((size_t)k * H + h) * M + m] = s->fc_W_host[h] * sc.commute_on[((size_t)k * M + m) * H + h];
        HIP_TRY(hipMemcpyAsync(sc.Wk_on, wk_on.data(), sizeof(double) * wk_on.size(), hipMemcpyHostToDevice, st));
        if (int rc = acc_zero(sc.tacc, st)) return rc;
        acc_invalidate(sc.tacc);
        for (int slot = 0; slot < 2; ++slot)
            if (s->fc.acc.valid[slot])
                if (int rc = acc_shadow(sc.tacc, slot, true, st)) return rc;
    }
    if (sc.local()) {                                 // [K][H][M] out of the caller's [K][M][H]
        for (int k = 0; k < sc.K; ++k)
            for (size_t m = 0; m < M; ++m)
                for (int h = 0; h < H; ++h)
                    wk[((size_t)k * H + h) * M + m] = s->fc_W_host[h] * sc.commute[((size_t)k * M + m) * H + h];
    } else {
        for (int k = 0; k < sc.K; ++k)
            for (int h = 0; h < H; ++h) wk[(size_t)k * H + h] = s->fc_W_host[h] * sc.commute[(size_t)k * H + h];
    }
    HIP_TRY(hipMemcpyAsync(sc.local() ? sc.Wk_loc : sc.Wk, wk.data(), sizeof(double) * wk.size(), hipMemcpyHostToDevice, st));
    if (int rc = acc_zero(sc.acc, st)) return rc;
    acc_invalidate(sc.acc);
    for (int slot = 0; slot < 2; ++slot)
        if (s->fc.acc.valid[slot])
            if (int rc = acc_shadow(sc.acc, slot, true, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));                // wk is the host's
    return 0;
}

// by_day is summed with atomics: zero the call's slots of every scenario first.
static int scenarios_zero_slots(seir_sampler *s, int32_t first, int32_t count) {
    const ScenarioSet &sc = s->scen;
    const size_t row = (size_t)s->cfg.B * s->fc.fb.H * 3;
    for (int k = 0; k < sc.K; ++k)
        HIP_TRY(hipMemsetAsync(sc.mom[k].by_day + (size_t)first * row, 0, sizeof(int64_t) * count * row, s->ctx->stream));
    // k_group_sums adds: the call's draw positions [j, j + count) of the region totals start from zero, so a burst run again
    // behind a restore overwrites them
    if (sc.gG) {
        const size_t grow = row * sc.gG;
        for (int k = 0; k < sc.K; ++k)
            HIP_TRY(hipMemsetAsync(sc.gstore.as<int64_t>() + ((size_t)k * sc.cap + (size_t)s->fc.acc.j) * grow, 0,
                                   sizeof(int64_t) * count * grow, s->ctx->stream));
    }
    return 0;
}

// A batch of the forecast behind its fold: the K scenarios of the batch's draws rolled forward in one set of planes, then per
// scenario the forecast's fold and finish on its slice, the difference fold against the forecast's staging tensor, and the
// by-day curves into the position stores.
static int scenarios_batch(seir_sampler *s, const ForecastBufs &fb, const RolloutBatch &bt, int32_t first) {
    const ScenarioSet &sc = s->scen;
    seir_ctx *ctx = s->ctx;
    const LaunchCfg l = whole(ctx, s->cfg.B);
    const Dims &d = l.d;
    const int B = s->cfg.B, H = fb.H, K = sc.K, ND = bt.ND, ndp = bt.ndp;
    const long long j = s->fc.acc.j + bt.j0;        // the batch's first draw position
    const ScenarioBufs sb{K, sc.log_shift, sc.Wk, sc.St, sc.X, sc.F, sc.base, sc.sev};
    if (sc.triggered()) {
        scenarios_trigger_rollout(s, l, fb, sb, bt, first, (int)j);
    } else if (sc.local()) {
        scenarios_local_rollout(s, l, fb, sb, bt, (int)j);
    } else {
        // a variable, so that the begin is named -- and emitted -- in front of the day kernel; it also writes the base plane's H rows
        const ScenarioBegin begin = k_scenario_begin<SC_BEGIN_THREADS>;
        scenarios_rollout(ctx, l, fb, sb, bt, begin, (size_t)std::max(d.Mp, H) * ndp, [&](dim3 grid, dim3 block, int h) {
            hipLaunchKernelGGL(k_scenario_day<FC_DAY_ROWS>, grid, block, 0, l.st, d, ctx->c, fb, sb, B, s->cfg.chain0, (int)j, ND,
                               ndp, h);
        });
    }
    const size_t slice = (size_t)ND * d.M * H * 3, row = (size_t)B * H * 3, slot0 = (size_t)(first + bt.j0);
    for (int k = 0; k < K; ++k) {
        ForecastBufs fk = fb;
        ScenarioDiffBufs df{};
        fk.fev = sc.sev + (size_t)k * slice;
        fk.mom = sc.mom[k];
        scenarios_layout(sc, k, fk.mom, df);
        hipLaunchKernelGGL(k_forecast_fold, dim3((d.M + FC_ROWS - 1) / FC_ROWS, B), dim3(64 * FC_ROWS), 0, l.st, d, fk, B,
                           first + bt.j0, bt.nj, ndp);
        scenario_diff_launch(d, l.st, df, fb.fev, fk.fev, d.M, H, B, bt.nj, j == 0);
        hipLaunchKernelGGL(k_forecast_finish, dim3(bt.nj, B), dim3(64), 0, l.st, d, fk, B, first + bt.j0, bt.nj, ndp);
        const size_t at = ((size_t)k * sc.cap + (size_t)j) * row;
        HIP_TRY(hipMemcpyAsync(sc.by_day + at, fk.mom.by_day + slot0 * row, sizeof(int64_t) * bt.nj * row, hipMemcpyDeviceToDevice, l.st));
        HIP_TRY(hipMemcpyAsync(sc.state_by_day + at, fk.mom.state_by_day + slot0 * row, sizeof(int64_t) * bt.nj * row,
                               hipMemcpyDeviceToDevice, l.st));
        if (sc.gG)                                   // the region totals of the slice, by draw position (zeroed by the call)
            groups_launch(d, l.st, s->grp, false, fk.fev, d.M, H, 0, ((long long)k * sc.cap + j) * B, ND, sc.gstore.as<int64_t>(),
                          nullptr, 0, 0, nullptr);
        if (sc.triggered()) scenarios_trigger_fold(s, l, bt, k, j);
    }
    return 0;
}

static int scenarios_on(seir_sampler *s) {
    if (int rc = trace_range_check(s, s->fc.on, FORECAST_USER)) return rc;
    if (!s->scen.K) return fail(SEIR_ERR_STATE, "no scenarios are set: call seir_sampler_scenarios_set first");
    return 0;
}

// The on pair and the rule of seir_sampler_scenarios_set_triggered, next to the off pair that every face gives.
struct TriggerArgs {
    const double *log_shift_on, *commute_on;         // [K][M][H]
    const int32_t *on, *off;                         // [K][M]
    const int32_t *params;                           // [K][4] window, from_day, min_days, review_every
};

// What is behind seir_sampler_scenarios_set (GLOBAL: arrays [K][H]), seir_sampler_scenarios_set_local (LOCAL: [K][M][H]) and
// seir_sampler_scenarios_set_triggered (TRIGGERED: LOCAL's tensors as the off pair, and `trig`).
static int scenarios_set(seir_sampler *s, int32_t K, const double *log_shift, const double *commute, int64_t cap,
                         ScenarioSet::Mode mode, const TriggerArgs *trig = nullptr) {
    const bool local = mode != ScenarioSet::GLOBAL, triggered = mode == ScenarioSet::TRIGGERED;
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = trace_range_check(s, s->fc.on, FORECAST_USER))) return rc;
    if (K < 0 || K > SEIR_SCENARIO_MAX) return fail(SEIR_ERR_INVALID, "K=%d outside [0, %d]", K, SEIR_SCENARIO_MAX);
    if (cap < 0 || cap > (1ll << FC_ID_SHIFT))
        return fail(SEIR_ERR_INVALID, "cap=%lld outside [0, 2^%d]: the draws per chain between two resets", (long long)cap, FC_ID_SHIFT);
    if (K == 0 || cap == 0) {
        if ((rc = drain(s))) return rc;
        s->scen = ScenarioSet{};
        return 0;
    }
    if (s->fc.acc.j != 0)
        return fail(SEIR_ERR_STATE, "%lld draws per chain have been forecast since the reset: scenarios are set between "
                    "seir_sampler_forecast_reset and the first seir_sampler_forecast", s->fc.acc.j);
    if (!log_shift || !commute) return fail(SEIR_ERR_INVALID, "null pointer");
    if (triggered && (!trig->log_shift_on || !trig->commute_on || !trig->on || !trig->off || !trig->params))
        return fail(SEIR_ERR_INVALID, "null pointer");
    const Dims &d = s->ctx->d;
    const int H = s->fc.fb.H;
    const size_t Ml = local ? (size_t)d.M : 1, nop = (size_t)K * Ml * H;
    for (size_t i = 0; i < nop && local; ++i) {
        const int k = (int)(i / (Ml * H)), m = (int)(i / H % Ml), h = (int)(i % H);
        if (!std::isfinite(log_shift[i])) return fail(SEIR_ERR_INVALID, "log_shift[%d][%d][%d] is not finite", k, m, h);
        if (!std::isfinite(commute[i]) || commute[i] < 0.0)
            return fail(SEIR_ERR_INVALID, "commute[%d][%d][%d]=%g: finite and >= 0", k, m, h, commute[i]);
    }
    for (int i = 0; i < K * H && !local; ++i) {
        if (!std::isfinite(log_shift[i])) return fail(SEIR_ERR_INVALID, "log_shift[%d][%d] is not finite", i / H, i % H);
        if (!std::isfinite(commute[i]) || commute[i] < 0.0)
            return fail(SEIR_ERR_INVALID, "commute[%d][%d]=%g: finite and >= 0", i / H, i % H, commute[i]);
    }
    int wmax = 0;
    for (size_t i = 0; i < nop && triggered; ++i) {
        const int k = (int)(i / (Ml * H)), m = (int)(i / H % Ml), h = (int)(i % H);
        if (!std::isfinite(trig->log_shift_on[i])) return fail(SEIR_ERR_INVALID, "log_shift_on[%d][%d][%d] is not finite", k, m, h);
        if (!std::isfinite(trig->commute_on[i]) || trig->commute_on[i] < 0.0)
            return fail(SEIR_ERR_INVALID, "commute_on[%d][%d][%d]=%g: finite and >= 0", k, m, h, trig->commute_on[i]);
    }
    for (int k = 0; k < K && triggered; ++k) {
        const int32_t *p = trig->params + 4 * k;
        if (p[0] < 1 || p[0] > SEIR_TRIGGER_MAX_WINDOW)
            return fail(SEIR_ERR_INVALID, "params[%d][0]=%d: the window is in [1, %d]", k, p[0], SEIR_TRIGGER_MAX_WINDOW);
        if (p[1] < 0 || p[1] > H) return fail(SEIR_ERR_INVALID, "params[%d][1]=%d: from_day is in [0, %d]", k, p[1], H);
        if (p[2] < 0) return fail(SEIR_ERR_INVALID, "params[%d][2]=%d: min_days is >= 0", k, p[2]);
        if (p[3] < 1) return fail(SEIR_ERR_INVALID, "params[%d][3]=%d: review_every is >= 1", k, p[3]);
        wmax = std::max(wmax, (int)p[0]);
        for (int m = 0; m < d.M; ++m) {
            const int32_t on = trig->on[(size_t)k * d.M + m], off = trig->off[(size_t)k * d.M + m];
            if (off < 0 || off > on)
                return fail(SEIR_ERR_INVALID, "on[%d][%d]=%d, off[%d][%d]=%d: 0 <= off <= on", k, m, on, k, m, off);
        }
    }
    if ((rc = drain(s))) return rc;
    s->scen = ScenarioSet{};                         // what was set before goes first; a refusal leaves the forecast without scenarios
    const size_t B = (size_t)s->cfg.B, capT = (size_t)s->cfg.cap, Kz = (size_t)K, ndmax = (size_t)s->fc.ndmax;
    const size_t plane = (size_t)d.Mp * Kz * ndmax, ndm = (size_t)s->fc.slots * B;
    ScenarioSet sc;
    sc.K = K; sc.cap = cap; sc.B = B;
    sc.c6 = B * d.M * H * seir::SUMMARY_Q; sc.c4 = B * d.M * H * SCENARIO_Q;
    const size_t acc_bytes = Kz * (sc.words8() * 8 + sc.words4() * 4) + 8;
    // a local set has the two [K][H][M] tensors in the place of the two arrays and the base plane; the region totals' store
    // is part of the sum while its switch is on and a table is in force
    const unsigned long long gbytes = scenario_groups_bytes(s, K, cap, s->grp_on ? s->grp.G : 0, H);
    // a triggered set adds the on pair, the thresholds and parameters, hist, the three planes (win, age, the two mask words) and
    // its two outputs
    const size_t tacc_bytes = Kz * B * d.M * H * sizeof(uint32_t);
    const unsigned long long tbytes = !triggered ? 0ull :
        8ull * 2 * nop + 4ull * (2 * Kz * d.M + 4 * Kz) + 4ull * (size_t)wmax * d.Mp * ndmax + (4ull + 4ull + 16ull) * plane +
        tacc_bytes + 4ull * Kz * (unsigned long long)cap * B * H;
    const unsigned long long bytes = 8ull * (local ? 2 * nop + 2 * plane : 2 * Kz * H + 2 * plane + Kz * H * ndmax) +
                                     4ull * (3 * plane + Kz * ndm * d.M * H * 3) +
                                     8ull * Kz * capT * B * (2ull * H + d.M) * 3 + 16ull * Kz * (unsigned long long)cap * B * H * 3 +
                                     acc_bytes + gbytes + tbytes;
    if ((rc = refuse_above_half_free(bytes, "the scenarios need %llu bytes (%d scenarios x %zu chains x %d locations x %d days, stores of "
                                            "%lld draws)", bytes, K, B, d.M, H, (long long)cap)))
        return rc;
#define SC_ALLOC(ptr, ...) if (!rc) rc = s_alloc(s, sc.allocs, &(ptr), __VA_ARGS__)
    sc.mode = mode;
    if (local) {
        SC_ALLOC(sc.log_shift_loc, nop); SC_ALLOC(sc.Wk_loc, nop);
        if (triggered) {
            sc.wmax = wmax;
            SC_ALLOC(sc.log_shift_on, nop); SC_ALLOC(sc.Wk_on, nop);
            SC_ALLOC(sc.trig_on, Kz * d.M); SC_ALLOC(sc.trig_off, Kz * d.M); SC_ALLOC(sc.trig_params, 4 * Kz);
            SC_ALLOC(sc.hist, (size_t)wmax * d.Mp * ndmax);
            SC_ALLOC(sc.win, plane); SC_ALLOC(sc.age, plane); SC_ALLOC(sc.mask, 2 * plane);
            SC_ALLOC(sc.active_by_day, Kz * (size_t)cap * B * H);
        }
    } else {
        SC_ALLOC(sc.log_shift, Kz * H); SC_ALLOC(sc.Wk, Kz * H);
        SC_ALLOC(sc.base, Kz * H * ndmax);
    }
    SC_ALLOC(sc.St, 3 * plane); SC_ALLOC(sc.X, plane); SC_ALLOC(sc.F, plane);
    SC_ALLOC(sc.sev, Kz * ndm * d.M * H * 3);
    for (int k = 0; k < K; ++k) {
        SC_ALLOC(sc.mom[k].by_day, capT * B * H * 3); SC_ALLOC(sc.mom[k].by_loc, capT * B * d.M * 3);
        SC_ALLOC(sc.mom[k].state_by_day, capT * B * H * 3);
    }
    SC_ALLOC(sc.by_day, Kz * (size_t)cap * B * H * 3); SC_ALLOC(sc.state_by_day, Kz * (size_t)cap * B * H * 3);
#undef SC_ALLOC
    if (!rc) rc = sc.acc.buf.zeroed(acc_bytes);
    if (!rc && triggered) rc = sc.tacc.buf.zeroed(tacc_bytes);
    if (rc) return alloc_failed(bytes, "scenarios");
    sc.commute.assign(commute, commute + nop);
    if (local) {                                     // [K][H][M] out of the caller's [K][M][H]
        std::vector<double> ls(nop);
        for (int k = 0; k < K; ++k)
            for (size_t m = 0; m < Ml; ++m)
                for (int h = 0; h < H; ++h) ls[((size_t)k * H + h) * Ml + m] = log_shift[((size_t)k * Ml + m) * H + h];
        HIP_TRY(hipMemcpy(sc.log_shift_loc, ls.data(), sizeof(double) * nop, hipMemcpyHostToDevice));
        if (triggered) {
            sc.commute_on.assign(trig->commute_on, trig->commute_on + nop);
            for (int k = 0; k < K; ++k)
                for (size_t m = 0; m < Ml; ++m)
                    for (int h = 0; h < H; ++h) ls[((size_t)k * H + h) * Ml + m] = trig->log_shift_on[((size_t)k * Ml + m) * H + h];
            HIP_TRY(hipMemcpy(sc.log_shift_on, ls.data(), sizeof(double) * nop, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(sc.trig_on, trig->on, sizeof(int32_t) * Kz * d.M, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(sc.trig_off, trig->off, sizeof(int32_t) * Kz * d.M, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(sc.trig_params, trig->params, sizeof(int32_t) * 4 * Kz, hipMemcpyHostToDevice));
        }
    } else {
        HIP_TRY(hipMemcpy(sc.log_shift, log_shift, sizeof(double) * Kz * H, hipMemcpyHostToDevice));
    }
    s->scen = std::move(sc);
    if ((rc = scenarios_begin(s)) || (rc = scenario_groups_fit(s, true))) { s->scen = ScenarioSet{}; return rc; }
    return 0;
}

extern "C" int seir_sampler_scenarios_set(seir_sampler *s, int32_t K, const double *log_shift, const double *commute, int64_t cap) {
    return scenarios_set(s, K, log_shift, commute, cap, ScenarioSet::GLOBAL);
}

extern "C" int seir_sampler_scenarios_set_local(seir_sampler *s, int32_t K, const double *log_shift, const double *commute,
                                                int64_t cap) {
    return scenarios_set(s, K, log_shift, commute, cap, ScenarioSet::LOCAL);
}

extern "C" int seir_sampler_scenarios_set_triggered(seir_sampler *s, int32_t K, const double *log_shift, const double *commute,
                                                    const double *log_shift_on, const double *commute_on, const int32_t *on,
                                                    const int32_t *off, const int32_t *params, int64_t cap) {
    const TriggerArgs trig{log_shift_on, commute_on, on, off, params};
    return scenarios_set(s, K, log_shift, commute, cap, ScenarioSet::TRIGGERED, &trig);
}

static int scenario_triggers_on(seir_sampler *s) {
    if (int rc = scenarios_on(s)) return rc;
    if (!s->scen.triggered())
        return fail(SEIR_ERR_STATE, "the scenarios in force have no triggers: call seir_sampler_scenarios_set_triggered first");
    return 0;
}

extern "C" int seir_sampler_read_scenario_triggers(seir_sampler *s, uint32_t *active_count) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = scenario_triggers_on(s))) return rc;
    if (!active_count) return fail(SEIR_ERR_INVALID, "null output pointer");
    hipStream_t st = s->ctx->stream;
    HIP_TRY(hipMemcpyAsync(active_count, s->scen.tacc.buf.p, s->scen.tacc.buf.bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int seir_sampler_read_scenario_trigger_draws(seir_sampler *s, int64_t first, int64_t count, int32_t *active_by_day) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = scenario_triggers_on(s))) return rc;
    const ScenarioSet &sc = s->scen;
    if (first < 0 || count < 0 || first + count > s->fc.acc.j)
        return fail(SEIR_ERR_INVALID, "draw positions [%lld,%lld) outside the %lld draws per chain forecast since the reset",
                    (long long)first, (long long)(first + count), s->fc.acc.j);
    if (count && !active_by_day) return fail(SEIR_ERR_INVALID, "null output pointer");
    hipStream_t st = s->ctx->stream;
    const size_t row = sc.B * (size_t)s->fc.fb.H, n = (size_t)count * row;
    for (int k = 0; k < sc.K && n; ++k)
        HIP_TRY(hipMemcpyAsync(active_by_day + (size_t)k * n, sc.active_by_day + ((size_t)k * sc.cap + (size_t)first) * row,
                               sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// ---- the scenarios' region totals ----
static unsigned long long scenario_groups_bytes(const seir_sampler *s, int K, long long cap, int G, int H) {
    if (!s->scen_grp_on) return 0;
    return 8ull * (unsigned long long)K * (unsigned long long)cap * s->cfg.B * G * H * 3ull;
}

static int scenario_groups_fit(seir_sampler *s, bool held) {
    ScenarioSet &sc = s->scen;
    const int G = (s->scen_grp_on && s->grp_on && sc.K && s->fc.on) ? s->grp.G : 0;
    if (G == sc.gG) return 0;
    if (int rc = drain(s)) return rc;
    sc.gstore.reset(); sc.gG = 0;
    if (G == 0 || s->fc.acc.j != 0) return 0;         // behind the first forecast nothing is made: positions [0, j) would be missing
    const unsigned long long bytes = scenario_groups_bytes(s, sc.K, sc.cap, G, s->fc.fb.H);
    if (!held)
        if (int rc = refuse_above_half_free(bytes, "the scenarios' group sums need %llu bytes (%d scenarios x %lld draws x %d chains x "
                                                   "%d groups x %d days x 24)", bytes, sc.K, sc.cap, s->cfg.B, G, s->fc.fb.H))
            return rc;
    if (sc.gstore.zeroed((size_t)bytes)) return alloc_failed(bytes, "scenarios' group sums");
    sc.gG = G;
    return 0;
}

extern "C" int seir_sampler_scenario_groups_set(seir_sampler *s, int32_t on) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if (!on) {
        if ((rc = drain(s))) return rc;
        s->scen_grp_on = false;
        s->scen.gstore.reset(); s->scen.gG = 0;
        return 0;
    }
    if (!s->grp_on) return fail(SEIR_ERR_STATE, "no group table is set: call seir_sampler_groups_set first");
    s->scen_grp_on = true;
    if ((rc = scenario_groups_fit(s))) { s->scen_grp_on = false; return rc; }
    return 0;
}

extern "C" int seir_sampler_read_scenario_group_draws(seir_sampler *s, int64_t first, int64_t count, int64_t *by_group) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = scenarios_on(s))) return rc;
    const ScenarioSet &sc = s->scen;
    if (!sc.gG)
        return fail(SEIR_ERR_STATE, "the scenarios' group sums are off: seir_sampler_scenario_groups_set with a group table in "
                    "force, before the first seir_sampler_forecast (a new table behind it turns them off until the next reset)");
    if (first < 0 || count < 0 || first + count > s->fc.acc.j)
        return fail(SEIR_ERR_INVALID, "draw positions [%lld,%lld) outside the %lld draws per chain forecast since the reset",
                    (long long)first, (long long)(first + count), s->fc.acc.j);
    if (count && !by_group) return fail(SEIR_ERR_INVALID, "null output pointer");
    hipStream_t st = s->ctx->stream;
    const size_t row = sc.B * (size_t)sc.gG * s->fc.fb.H * 3, n = (size_t)count * row;
    for (int k = 0; k < sc.K && n; ++k)
        HIP_TRY(hipMemcpyAsync(by_group + (size_t)k * n, sc.gstore.as<int64_t>() + ((size_t)k * sc.cap + (size_t)first) * row,
                               sizeof(int64_t) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int seir_sampler_scenario_state(seir_sampler *s, int64_t out[4]) {
    if (!s) return fail(SEIR_ERR_INVALID, "null sampler");
    if (!out) return fail(SEIR_ERR_INVALID, "null pointer");
    out[0] = s->scen.K;
    out[1] = s->scen.K ? s->fc.fb.H : 0;
    out[2] = s->scen.cap;
    out[3] = s->scen.K ? s->fc.acc.j : 0;
    return 0;
}

extern "C" int seir_sampler_read_scenarios(seir_sampler *s, uint64_t *count, int32_t *ref, int64_t *sum, uint64_t *sumsq) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = scenarios_on(s))) return rc;
    const ScenarioSet &sc = s->scen;
    hipStream_t st = s->ctx->stream;
    unsigned flags[SEIR_SCENARIO_MAX] = {0, 0, 0, 0};
    for (int k = 0; k < sc.K; ++k) {
        MomentBufs mb{};
        ScenarioDiffBufs df{};
        scenarios_layout(sc, k, mb, df);
        HIP_TRY(hipMemcpyAsync(&flags[k], mb.overflow, sizeof(unsigned), hipMemcpyDeviceToHost, st));
        if (count) HIP_TRY(hipMemcpyAsync(count + (size_t)k * sc.B, mb.count, sizeof(uint64_t) * sc.B, hipMemcpyDeviceToHost, st));
        if (ref) HIP_TRY(hipMemcpyAsync(ref + (size_t)k * sc.c6, mb.ref, sizeof(int32_t) * sc.c6, hipMemcpyDeviceToHost, st));
        if (sum) HIP_TRY(hipMemcpyAsync(sum + (size_t)k * sc.c6, mb.sum, sizeof(int64_t) * sc.c6, hipMemcpyDeviceToHost, st));
        if (sumsq) HIP_TRY(hipMemcpyAsync(sumsq + (size_t)k * sc.c6, mb.sumsq, sizeof(uint64_t) * sc.c6, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < sc.K; ++k)
        if (flags[k])
            return fail(SEIR_ERR_STATE, "a sum of squared deviations reached 2^63: the moment accumulators of scenario %d overflowed "
                        "(seir_sampler_forecast_reset starts them again)", k);
    return 0;
}

extern "C" int seir_sampler_read_scenario_diffs(seir_sampler *s, int32_t *ref, int64_t *sum, uint64_t *sumsq, uint32_t *lt,
                                                uint32_t *eq) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = scenarios_on(s))) return rc;
    const ScenarioSet &sc = s->scen;
    hipStream_t st = s->ctx->stream;
    unsigned flags[SEIR_SCENARIO_MAX] = {0, 0, 0, 0};
    for (int k = 0; k < sc.K; ++k) {
        MomentBufs mb{};
        ScenarioDiffBufs df{};
        scenarios_layout(sc, k, mb, df);
        const size_t at = (size_t)k * sc.c4;
        HIP_TRY(hipMemcpyAsync(&flags[k], df.overflow, sizeof(unsigned), hipMemcpyDeviceToHost, st));
        if (ref) HIP_TRY(hipMemcpyAsync(ref + at, df.ref, sizeof(int32_t) * sc.c4, hipMemcpyDeviceToHost, st));
        if (sum) HIP_TRY(hipMemcpyAsync(sum + at, df.sum, sizeof(int64_t) * sc.c4, hipMemcpyDeviceToHost, st));
        if (sumsq) HIP_TRY(hipMemcpyAsync(sumsq + at, df.sumsq, sizeof(uint64_t) * sc.c4, hipMemcpyDeviceToHost, st));
        if (lt) HIP_TRY(hipMemcpyAsync(lt + at, df.lt, sizeof(uint32_t) * sc.c4, hipMemcpyDeviceToHost, st));
        if (eq) HIP_TRY(hipMemcpyAsync(eq + at, df.eq, sizeof(uint32_t) * sc.c4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < sc.K; ++k)
        if (flags[k])
            return fail(SEIR_ERR_STATE, "a sum of squared deviations reached 2^63: the difference accumulators of scenario %d "
                        "overflowed (seir_sampler_forecast_reset starts them again)", k);
    return 0;
}

extern "C" int seir_sampler_read_scenario_draws(seir_sampler *s, int64_t first, int64_t count, int64_t *by_day, int64_t *state_by_day) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = scenarios_on(s))) return rc;
    const ScenarioSet &sc = s->scen;
    if (first < 0 || count < 0 || first + count > s->fc.acc.j)
        return fail(SEIR_ERR_INVALID, "draw positions [%lld,%lld) outside the %lld draws per chain forecast since the reset",
                    (long long)first, (long long)(first + count), s->fc.acc.j);
    hipStream_t st = s->ctx->stream;
    const size_t row = sc.B * (size_t)s->fc.fb.H * 3, n = (size_t)count * row;
    for (int k = 0; k < sc.K && n; ++k) {
        const size_t at = ((size_t)k * sc.cap + (size_t)first) * row;
        if (by_day) HIP_TRY(hipMemcpyAsync(by_day + (size_t)k * n, sc.by_day + at, sizeof(int64_t) * n, hipMemcpyDeviceToHost, st));
        if (state_by_day)
            HIP_TRY(hipMemcpyAsync(state_by_day + (size_t)k * n, sc.state_by_day + at, sizeof(int64_t) * n, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// ---------------------------------------------------------------------------
// Scoring the forecast against later data (include/seir_hip.h; kernels: verify_kernels.h)
// ---------------------------------------------------------------------------
#include "verify_kernels.h"

static_assert(VF_JMAX == FC_JMAX, "a batch of the forecast is one launch of the verification fold");
static_assert(PAIR_CHUNK == SEIR_PAIR_ABS_CHUNK && PAIR_ABS_MAX_N == SEIR_PAIR_ABS_MAX_N, "the header's limits are the kernel's");

static void verify_layout(const VerifySet &v, VerifyBufs &vb) {
    vb.truth = v.truth;
    vb.cum = v.cum;
    vb.abs_sum = v.acc.buf.as<uint64_t>();
    vb.lt = (uint32_t *)(vb.abs_sum + v.c2);
    vb.eq = vb.lt + v.c2;
}

// Behind a forecast reset (and the set itself): the accumulators zero and what the snapshots hold of them dropped -- but for a
// slot whose snapshot holds the forecast's block: that was taken at j = 0, and so holds these zeros too (as scenarios_begin).
static int verify_begin(seir_sampler *s) {
    VerifySet &v = s->ver;
    hipStream_t st = s->ctx->stream;
    if (int rc = acc_zero(v.acc, st)) return rc;
    acc_invalidate(v.acc);
    for (int slot = 0; slot < 2; ++slot)
        if (s->fc.acc.valid[slot])
            if (int rc = acc_shadow(v.acc, slot, true, st)) return rc;
    return 0;
}

// A batch of the forecast behind its fold, while its staging tensor lives: an ordinary launch on the context stream.
static void verify_batch(seir_sampler *s, const ForecastBufs &fb, const RolloutBatch &bt) {
    const LaunchCfg l = whole(s->ctx, s->cfg.B);
    VerifyBufs vb{};
    verify_layout(s->ver, vb);
    hipLaunchKernelGGL(k_verify_fold<VF_ROWS>, dim3((l.d.M + VF_ROWS - 1) / VF_ROWS, s->cfg.B), dim3(64 * VF_ROWS), 0, l.st, l.d, vb,
                       (const int *)fb.fev, fb.H, s->cfg.B, bt.nj);
}

extern "C" int seir_sampler_verify_set(seir_sampler *s, const int32_t *truth) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if (!truth) {                                    // off: with or without a forecast
        if ((rc = drain(s))) return rc;
        s->ver = VerifySet{};
        return 0;
    }
    if ((rc = trace_range_check(s, s->fc.on, FORECAST_USER))) return rc;
    if (s->fc.acc.j != 0)
        return fail(SEIR_ERR_STATE, "%lld draws per chain have been forecast since the reset: the truth is set between "
                    "seir_sampler_forecast_reset and the first seir_sampler_forecast", s->fc.acc.j);
    const int M = s->ctx->d.M, H = s->fc.fb.H;
    const size_t B = (size_t)s->cfg.B, mh = (size_t)M * H;
    if ((rc = drain(s))) return rc;
    s->ver = VerifySet{};                            // what was set before goes first; a refusal leaves the forecast unscored
    VerifySet v;
    v.c2 = B * mh * 2;
    const size_t acc_bytes = v.c2 * 16;
    const unsigned long long bytes = 12ull * mh + 3ull * acc_bytes;    // the block and its two shadows
    if ((rc = refuse_above_half_free(bytes, "the verification needs %llu bytes (%zu chains x %d locations x %d days x 2 x 16, "
                                            "three times)", bytes, B, M, H)))
        return rc;
    if (!rc) rc = s_alloc(s, v.allocs, &v.truth, mh);
    if (!rc) rc = s_alloc(s, v.allocs, &v.cum, mh);
    if (!rc) rc = v.acc.buf.zeroed(acc_bytes);
    if (rc) return alloc_failed(bytes, "verification");
    // the running total per row, -1 from the first missing day on
    std::vector<int64_t> cum(mh);
    for (int m = 0; m < M; ++m) {
        int64_t run = 0;
        bool ok = true;
        for (int h = 0; h < H; ++h) {
            const int32_t y = truth[(size_t)m * H + h];
            ok = ok && y >= 0;
            if (ok) run += y;
            cum[(size_t)m * H + h] = ok ? run : -1;
        }
    }
    HIP_TRY(hipMemcpy(v.truth, truth, sizeof(int32_t) * mh, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(v.cum, cum.data(), sizeof(int64_t) * mh, hipMemcpyHostToDevice));
    v.on = true;
    s->ver = std::move(v);
    if ((rc = verify_begin(s))) { s->ver = VerifySet{}; return rc; }
    return 0;
}

extern "C" int seir_sampler_verify_state(seir_sampler *s, int64_t out[4]) {
    if (!s) return fail(SEIR_ERR_INVALID, "null sampler");
    if (!out) return fail(SEIR_ERR_INVALID, "null pointer");
    out[0] = s->ver.on ? 1 : 0;
    out[1] = s->ver.on ? s->fc.fb.H : 0;
    out[2] = s->ver.on ? s->fc.acc.j : 0;
    out[3] = s->ver.on && s->keep_fc.buf ? 1 : 0;
    return 0;
}

extern "C" int seir_sampler_read_verify(seir_sampler *s, uint64_t *count, uint32_t *lt, uint32_t *eq, uint64_t *abs_sum) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = trace_range_check(s, s->fc.on, FORECAST_USER))) return rc;
    if (!s->ver.on) return fail(SEIR_ERR_STATE, "no truth is set: call seir_sampler_verify_set first");
    VerifyBufs vb{};
    verify_layout(s->ver, vb);
    const size_t c2 = s->ver.c2;
    hipStream_t st = s->ctx->stream;
    if (count) HIP_TRY(hipMemcpyAsync(count, s->fc.fb.mom.count, sizeof(uint64_t) * s->cfg.B, hipMemcpyDeviceToHost, st));
    if (lt) HIP_TRY(hipMemcpyAsync(lt, vb.lt, sizeof(uint32_t) * c2, hipMemcpyDeviceToHost, st));
    if (eq) HIP_TRY(hipMemcpyAsync(eq, vb.eq, sizeof(uint32_t) * c2, hipMemcpyDeviceToHost, st));
    if (abs_sum) HIP_TRY(hipMemcpyAsync(abs_sum, vb.abs_sum, sizeof(uint64_t) * c2, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// Cells of n = segs x seg_len values on the device into out [cells] on the host.
static int pair_abs_run(seir_ctx *ctx, PairAbsArgs a, int64_t *out, uint32_t *overflow) {
    const long long n = (long long)a.segs * a.seg_len;
    if (n > SEIR_PAIR_ABS_MAX_N)
        return fail(SEIR_ERR_INVALID, "n = %d x %lld = %lld values per cell: above %d the sum of pairwise differences can reach 2^63",
                    a.segs, a.seg_len, n, SEIR_PAIR_ABS_MAX_N);
    DevBuf dout;
    if (int rc = dout.zeroed(sizeof(int64_t) * (size_t)a.cells + 8)) return rc;
    a.out = dout.as<int64_t>();
    a.overflow = (unsigned *)(a.out + a.cells);
    hipStream_t st = ctx->stream;
    uint32_t flag = 0;
    hipLaunchKernelGGL(k_pair_abs<PAIR_THREADS>, dim3((unsigned)a.cells), dim3(PAIR_THREADS), 0, st, whole(ctx, 1).d, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, a.out, sizeof(int64_t) * (size_t)a.cells, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&flag, a.overflow, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (overflow) *overflow = flag;
    if (flag) return fail(SEIR_ERR_STATE, "a cell above %d values reached the pair-sum kernel", SEIR_PAIR_ABS_MAX_N);
    return 0;
}

extern "C" int seir_sampler_forecast_pair_sums(seir_sampler *s, int32_t pooled, int64_t *out) {
    int rc = sampler_check(s);
    if (rc) return rc;
    if ((rc = trace_range_check(s, s->fc.on, FORECAST_USER))) return rc;
    const DrawStore &store = s->keep_fc;
    const TraceUser &who = FORECAST_USER;
    if (!store.buf) return fail(SEIR_ERR_STATE, "the draw store is not enabled: call %s first", who.keep);
    if (!out) return fail(SEIR_ERR_INVALID, "null output pointer");
    const long long j = s->fc.acc.j;
    if (j < 1) return fail(SEIR_ERR_STATE, "no draws kept since the %s reset", who.name);
    const int B = s->cfg.B;
    hipStream_t st = s->ctx->stream;
    std::vector<uint64_t> cnt((size_t)B);
    HIP_TRY(hipMemcpyAsync(cnt.data(), s->fc.fb.mom.count, sizeof(uint64_t) * B, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int b = 0; b < B; ++b)
        if ((long long)cnt[b] != j)
            return fail(SEIR_ERR_STATE, "chain %d has %llu draws %s, the store %lld: the chains' counts differ", b,
                        (unsigned long long)cnt[b], who.done, j);
    // planes 0 and 1 of keep[B][3][M][H][cap]: per chain (or once, pooled) two launches of M x H cells
    const long long mh = (long long)s->ctx->d.M * s->fc.fb.H, plane3 = 3 * mh;
    const int nb = pooled ? 1 : B;
    for (int b = 0; b < nb; ++b) {
        PairAbsArgs a{};
        a.values = store.buf.as<const int32_t>() + (size_t)b * (size_t)plane3 * (size_t)store.stride;
        a.cells = 2 * mh;                            // planes 0 and 1 are neighbours
        a.segs = pooled ? B : 1;
        a.seg_len = j;
        a.seg_stride = plane3 * store.stride;
        a.cell_stride = store.stride;
        if ((rc = pair_abs_run(s->ctx, a, out + (size_t)b * 2 * (size_t)mh, nullptr))) return rc;
    }
    return 0;
}

extern "C" int seir_pair_abs_sums(seir_ctx *ctx, const int32_t *values, int64_t cells, int32_t segs, int64_t seg_len,
                                  int64_t seg_stride, int64_t cell_stride, int64_t *out, uint32_t *overflow) {
    int rc = check_batch(ctx, 1);
    if (rc) return rc;
    if (!values || !out || !overflow) return fail(SEIR_ERR_INVALID, "null pointer");
    *overflow = 0;
    if (cells < 1 || cells > 0x7fffffffll || segs < 1 || seg_len < 1)
        return fail(SEIR_ERR_INVALID, "cells=%lld, segs=%d, seg_len=%lld: at least one of each, cells below 2^31", (long long)cells, segs,
                    (long long)seg_len);
    // each factor against the bound before the product is formed: it then fits 64 bits whatever the caller passed
    if (segs > SEIR_PAIR_ABS_MAX_N || seg_len > SEIR_PAIR_ABS_MAX_N || (long long)segs * seg_len > SEIR_PAIR_ABS_MAX_N)
        return fail(SEIR_ERR_INVALID, "n = %d x %lld values per cell: above %d the sum of pairwise differences can reach 2^63", segs,
                    (long long)seg_len, SEIR_PAIR_ABS_MAX_N);
    if (cell_stride < 0 || seg_stride < 0 || (segs > 1 && seg_stride < seg_len))
        return fail(SEIR_ERR_INVALID, "seg_stride=%lld, cell_stride=%lld: no negative stride, and segments do not overlap",
                    (long long)seg_stride, (long long)cell_stride);
    const size_t extent = (size_t)(cells - 1) * cell_stride + (size_t)(segs - 1) * seg_stride + (size_t)seg_len;
    DevBuf dv;
    if ((rc = dv.alloc(sizeof(int32_t) * extent))) return rc;
    HIP_TRY(hipMemcpyAsync(dv.p, values, sizeof(int32_t) * extent, hipMemcpyHostToDevice, ctx->stream));
    PairAbsArgs a{};
    a.values = dv.as<int32_t>();
    a.cells = cells; a.segs = segs; a.seg_len = seg_len; a.seg_stride = seg_stride; a.cell_stride = cell_stride;
    return pair_abs_run(ctx, a, out, overflow);
}

// ---------------------------------------------------------------------------
// Triggered scenarios: the launches of a triggered set and the fold of its masks (declared above, with the scenarios;
// kernels: scenario_trigger_kernels.h).  The header is included here, so that its kernels lie behind every kernel the parent had
// but the local set's pair: those two stay the last of the code object (they are emitted where scenarios_local_rollout, below,
// names them), and every other kernel keeps its address.
// ---------------------------------------------------------------------------
#include "scenario_trigger_kernels.h"

static_assert(TRIGGER_MAX_WINDOW == SEIR_TRIGGER_MAX_WINDOW, "the header's bound is the kernels'");

static void scenarios_trigger_rollout(seir_sampler *s, const LaunchCfg &l, const ForecastBufs &fb, const ScenarioBufs &sb,
                                      const RolloutBatch &bt, int32_t first, int j) {
    const ScenarioSet &sc = s->scen;
    const ScenarioLocalBufs lb{sc.log_shift_loc, sc.Wk_loc};
    const ScenarioTriggerBufs tb{sc.log_shift_on, sc.Wk_on, sc.trig_on, sc.trig_off, sc.trig_params, sc.wmax,
                                 sc.hist,         sc.win,   sc.age,     sc.mask};
    scenarios_rollout_with(s->ctx, l, fb, sb, bt, (size_t)l.d.Mp * bt.ndp, [&](dim3 grid, dim3 block) {
        hipLaunchKernelGGL(s->cfg.ev16 ? k_trigger_begin<1> : k_trigger_begin<0>, grid, block, 0, l.st, l.d, s->ctx->c, fb, sb, tb,
                           (const void *)s->ch.tr_events, s->cfg.B, first + bt.j0, bt.ND, bt.ndp);
    }, [&](dim3 grid, dim3 block, int h) {
        hipLaunchKernelGGL(k_scenario_trigger_day<FC_DAY_ROWS>, grid, block, 0, l.st, l.d, s->ctx->c, fb, sb, lb, tb, s->cfg.B,
                           s->cfg.chain0, j, bt.ND, bt.ndp, h);
    });
}

// The masks of nj draws per chain into a count block [B][M][H] and the curves of nj draw positions [nj][B][H].
static void trigger_fold_launch(const Dims &d, hipStream_t st, const uint64_t *mask, size_t plane, size_t stride, size_t col0,
                                uint32_t *count, int32_t *by_day, int M, int H, int B, int nj, bool fresh) {
    hipLaunchKernelGGL(k_trigger_fold<TRIG_U>, dim3((M + TRIG_ROWS - 1) / TRIG_ROWS + (nj + TRIG_ROWS - 1) / TRIG_ROWS, B),
                       dim3(64 * TRIG_ROWS), 0, st, d, mask, plane, stride, col0, count, by_day, M, H, B, nj, fresh ? 1 : 0);
}

static void scenarios_trigger_fold(seir_sampler *s, const LaunchCfg &l, const RolloutBatch &bt, int k, long long j) {
    const ScenarioSet &sc = s->scen;
    const Dims &d = l.d;
    const int B = s->cfg.B, H = s->fc.fb.H;
    const size_t ndk = (size_t)sc.K * bt.ndp;
    trigger_fold_launch(d, l.st, sc.mask, (size_t)d.Mp * ndk, ndk, (size_t)k * bt.ndp,
                        sc.tacc.buf.as<uint32_t>() + (size_t)k * B * d.M * H,
                        sc.active_by_day + ((size_t)k * sc.cap + (size_t)j) * B * H, d.M, H, B, bt.nj, j == 0);
}

extern "C" int seir_trigger_counts(seir_ctx *ctx, const uint64_t *masks, int64_t n, int32_t B, int32_t M, int32_t H, uint64_t folded,
                                   uint32_t *active_count, int32_t *active_by_day) {
    int rc = check_batch(ctx, 1);
    if (rc) return rc;
    if (!masks || !active_count || !active_by_day) return fail(SEIR_ERR_INVALID, "null pointer");
    if (n < 1 || B < 1 || M < 1 || B > 65535)
        return fail(SEIR_ERR_INVALID, "n=%lld, B=%d, M=%d: at least one of each, B at most 65535", (long long)n, B, M);
    if (H < 1 || H > SEIR_FORECAST_MAX_H) return fail(SEIR_ERR_INVALID, "H=%d outside [1, %d]", H, SEIR_FORECAST_MAX_H);
    if (folded > 0xffffffffull || folded + (uint64_t)n > 0xffffffffull)
        return fail(SEIR_ERR_INVALID, "%llu draws per chain folded and %lld more: the counts hold 2^32 - 1",
                    (unsigned long long)folded, (long long)n);
    // a launch's planes [2][M][ndp], the draw index nd = jj B + b contiguous as in the sampler's batches
    const int njmax = (int)std::min<int64_t>(n, SC_JMAX);
    const size_t ndp = (size_t)ceil_to(njmax * B, 64), plane = (size_t)M * ndp, cells = (size_t)B * M * H;
    const unsigned long long bytes = 16ull * plane + 4ull * cells + 4ull * (unsigned long long)n * B * H;
    if ((rc = refuse_above_half_free(bytes, "the trigger counts need %llu bytes (%lld draws x %d chains x %d locations x %d days)",
                                     bytes, (long long)n, B, M, H)))
        return rc;
    DevBuf dmask, dcount, dby;
    if ((rc = dmask.alloc(16 * plane)) || (rc = dcount.alloc(4 * cells)) || (rc = dby.alloc(4 * (size_t)n * B * H))) return rc;
    hipStream_t st = ctx->stream;
    if (folded) HIP_TRY(hipMemcpyAsync(dcount.p, active_count, 4 * cells, hipMemcpyHostToDevice, st));
    const Dims d = whole(ctx, 1).d;
    std::vector<uint64_t> host(2 * plane);
    for (int64_t j0 = 0; j0 < n; j0 += SC_JMAX) {
        const int nj = (int)std::min<int64_t>(SC_JMAX, n - j0);
        std::fill(host.begin(), host.end(), 0ull);
        for (int jj = 0; jj < nj; ++jj)                // [n][B][M][2] into [2][M][ndp]
            for (int b = 0; b < B; ++b)
                for (int m = 0; m < M; ++m)
                    for (int x = 0; x < 2; ++x)
                        host[(size_t)x * plane + (size_t)m * ndp + (size_t)jj * B + b] = masks[((((size_t)j0 + jj) * B + b) * M + m) * 2 + x];
        HIP_TRY(hipMemcpyAsync(dmask.p, host.data(), 16 * plane, hipMemcpyHostToDevice, st));
        trigger_fold_launch(d, st, dmask.as<uint64_t>(), plane, ndp, 0, dcount.as<uint32_t>(), dby.as<int32_t>() + (size_t)j0 * B * H, M,
                            H, B, nj, folded == 0 && j0 == 0);
        HIP_TRY(hipStreamSynchronize(st));             // host is filled again
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(active_count, dcount.p, 4 * cells, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(active_by_day, dby.p, 4 * (size_t)n * B * H, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// ---------------------------------------------------------------------------
// Targeted scenarios: the launches of a local set (declared above, with the scenarios; kernels: scenario_local_kernels.h).  The
// header is included here, so that its kernels lie behind every kernel the parent had.
// ---------------------------------------------------------------------------
#include "scenario_local_kernels.h"

static void scenarios_local_rollout(seir_sampler *s, const LaunchCfg &l, const ForecastBufs &fb, const ScenarioBufs &sb,
                                    const RolloutBatch &bt, int j) {
    const ScenarioLocalBufs lb{s->scen.log_shift_loc, s->scen.Wk_loc};
    const ScenarioBegin begin = k_scenario_local_begin<SC_BEGIN_THREADS>;   // in front of the day kernel, as in scenarios_batch
    scenarios_rollout(s->ctx, l, fb, sb, bt, begin, (size_t)l.d.Mp * bt.ndp, [&](dim3 grid, dim3 block, int h) {
        hipLaunchKernelGGL(k_scenario_local_day<FC_DAY_ROWS>, grid, block, 0, l.st, l.d, s->ctx->c, fb, sb, lb, s->cfg.B,
                           s->cfg.chain0, j, bt.ND, bt.ndp, h);
    });
}

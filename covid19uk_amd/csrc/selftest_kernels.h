// Self-test kernels: each scalar function of device_math.h, the delta log-ratios of the event updates and the wave / block
// primitives, one call per thread, so that a test can hold every one of them to a high-precision reference by itself
// (tests/test_devmath_gpu.py).  Off the hot path: nothing here is launched by the sampler or the evaluation.
// The op codes are those of include/seir_hip.h (SEIR_FN_*, SEIR_DELTA_*, SEIR_WAVE_*).
#pragma once
#include "../../include/seir_hip.h"
#include "device_math.h"
#include "sampler_kernels.h"
#include "moves_kernel.h"

namespace seir {

// One element per thread, 256-thread blocks, the LDS table filled as every kernel fills it: the lanes of a wave hold
// different arguments and take different branches.
__global__ __launch_bounds__(256) void k_selftest_fn(const double2 *__restrict__ logtab, int op, int n, const double *x,
                                                    const double *y, double *out0, double *out1) {
    __shared__ double2 ltab[LDSTAB_N];
    log_table_to_lds(ltab, logtab);
    SeK sk;
    sk.load();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double a = x[i], b = y ? y[i] : 0.0;
    double r0 = 0.0, r1 = 0.0;
    switch (op) {
        case SEIR_FN_FAST_LOG: r0 = fast_log(a, ltab); break;
        case SEIR_FN_FAST_LOG_K: r0 = fast_log_k(a, ltab, sk); break;
        case SEIR_FN_FAST_RCP: r0 = fast_rcp(a); break;
        case SEIR_FN_MV_LOG: r0 = mv_log(a, ltab); break;
        case SEIR_FN_SOFTPLUS_TAB: r0 = softplus_tab(a, ltab); break;
        case SEIR_FN_SOFTPLUS_SIGMOID_TAB: r0 = softplus_sigmoid_tab(a, ltab, r1); break;
        case SEIR_FN_SOFTPLUS: r0 = softplus(a); break;
        case SEIR_FN_LFACT_BF: r0 = lfact_bf(a, ltab); break;
        case SEIR_FN_LBINOM_TAB: r0 = lbinom(a, b, ltab); break;
        case SEIR_FN_LBINOM_CONST: r0 = lbinom(a, b); break;
        case SEIR_FN_LBINOM_BF: r0 = lbinom_bf(a, b, ltab); break;
        case SEIR_FN_LOG1MEXP_TAB: r0 = log1mexp(a, ltab); break;
        case SEIR_FN_LOG1MEXP: r0 = log1mexp(a); break;
        case SEIR_FN_LOG1MEXP_SERIES: {
            bool odd = false;
            r0 = log1mexp_series(a, ltab, odd);
            r1 = odd ? 1.0 : 0.0;
            break;
        }
        case SEIR_FN_L1ME_INV_SERIES: l1me_inv_series(a, r0, r1, ltab); break;
        case SEIR_FN_L1ME_INV_K: l1me_inv_k(a, r0, r1, ltab, sk); break;
        case SEIR_FN_L1ME_INV_SERIES_K: l1me_inv_series_k(a, r0, r1, ltab, sk); break;
        case SEIR_FN_LOG1MEXP_DIFF_SLOW: r0 = log1mexp_diff_slow(a, b, ltab); break;
        default: break;
    }
    out0[i] = r0;
    if (out1) out1[i] = r1;
}

// The S->E piece of own_rows_delta, RESTATED: the same expressions in the same order as the two cases of own_rows_delta
// (sampler_kernels.h, "only the terms the update changes").  As inline helpers that own_rows_delta called too, every kernel
// kept its resource record, but the instruction streams of k_move_pair, k_move_pairs and k_move_delta<true> moved by one to
// four instructions; the event-update kernels stay as they were, and a change there has to be repeated here.
//   S->E-type update: k_se goes from kse to k1 and S - k_se moves by dsk; the rate rr0 stays
__device__ __forceinline__ double own_se_delta_se(double kse, double k1, double dsk, double rr0, const double2 *ltab) {
    bool odd = false;
    double L0 = log1mexp_series(rr0, ltab, odd);
    if (odd) L0 = log1mexp(rr0, ltab);
    return ((k1 != 0.0 ? k1 * L0 : 0.0) - (kse != 0.0 ? kse * L0 : 0.0)) - dsk * rr0;
}
//   E->I-type update: the rate goes from rr0 to rr1 (I and F move); S and k_se stay
__device__ __forceinline__ double own_se_delta_ei(double S, double kse, double rr0, double rr1, const double2 *ltab) {
    bool odd = false;
    double L1 = log1mexp_series(rr1, ltab, odd), L0 = log1mexp_series(rr0, ltab, odd);
    if (odd) { L1 = log1mexp(rr1, ltab); L0 = log1mexp(rr0, ltab); }
    return (kse != 0.0 ? kse * (L1 - L0) : 0.0) - (S - kse) * (rr1 - rr0);
}

// band_delta and the S->E piece of own_rows_delta (own_se_delta_*: the restatement above), per element.
// SEIR_DELTA_OWN_SE: `S` holds dS and `dF` holds dk0 (see include/seir_hip.h).
__global__ __launch_bounds__(256) void k_selftest_delta(const double2 *__restrict__ logtab, int op, int n, const double *S,
                                                       const double *I, const double *K0, const double *F, const double *dF,
                                                       const double *ee, const double *psiW, double rate_floor, double dt,
                                                       double *out) {
    __shared__ double2 ltab[LDSTAB_N];
    log_table_to_lds(ltab, logtab);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double r;
    if (op == SEIR_DELTA_BAND) {
        r = band_delta(S[i], I[i], K0[i], F[i], dF[i], ee[i], psiW[i], rate_floor * dt, dt, ltab);
    } else {
        // the rates as own_rows_delta forms them
        const double rr0 = (ee[i] * (I[i] + psiW[i] * F[i]) + rate_floor) * dt;
        if (op == SEIR_DELTA_OWN_EI) {
            const double rr1 = (ee[i] * (I[i] + psiW[i] * (F[i] + dF[i])) + rate_floor) * dt;
            r = own_se_delta_ei(S[i], K0[i], rr0, rr1, ltab);
        } else {
            r = own_se_delta_se(K0[i], K0[i] + dF[i], S[i] - dF[i], rr0, ltab);
        }
    }
    out[i] = r;
}

// The wave and block primitives: thread tid of block b feeds in[b * 256 + tid] and stores what it gets back (and, for the
// block forms, the `total` it was handed).
template <int IS_INT> struct SelftestWaveT { using type = double; };
template <> struct SelftestWaveT<1> { using type = int; };
template <int IS_INT>
__global__ __launch_bounds__(256) void k_selftest_wave(int op, const typename SelftestWaveT<IS_INT>::type *in,
                                                      typename SelftestWaveT<IS_INT>::type *out,
                                                      typename SelftestWaveT<IS_INT>::type *total) {
    using T = typename SelftestWaveT<IS_INT>::type;
    __shared__ T sh[4];
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const T v = in[i];
    T r = 0, tot = 0;
    if (op == SEIR_WAVE_SUM) r = wave_sum(v);
    else if (op == SEIR_WAVE_INCL_SCAN) r = wave_incl_scan(v, lane);
    else if (op == SEIR_BLOCK_EXCL_SCAN) r = block_excl_scan_256(v, sh, tot);
    if constexpr (!IS_INT) {
        if (op == SEIR_WAVE_MIN) r = wave_min(v);
        else if (op == SEIR_WAVE_INCL_SUFFIX_SCAN) r = wave_incl_suffix_scan(v, lane);
        else if (op == SEIR_BLOCK_INCL_SUFFIX_SCAN) r = block_incl_suffix_scan_256(v, sh, tot);
        else if (op == SEIR_BLOCK_SUM) r = block_sum_256(v, sh);
    }
    out[i] = r;
    if (total) total[i] = tot;
}

}  // namespace seir

"""ctypes binding of libseirhip.so (C-ABI: include/seir_hip.h).

There is no CPU fallback: if the shared library has not been built
(`python -c "import __graft_entry__ as g; g.build()"` or `make -C
covid19uk_amd/csrc`) or no HIP device is usable, the calls raise.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libseirhip.so")

c_double_p = ctypes.POINTER(ctypes.c_double)
c_void_pp = ctypes.POINTER(ctypes.c_void_p)
c_int64_p = ctypes.POINTER(ctypes.c_int64)


class SeirDesc(ctypes.Structure):
    """Mirror of `seir_desc` (include/seir_hip.h)."""
    _fields_ = [
        ("M", ctypes.c_int32), ("T", ctypes.c_int32),
        ("max_chains", ctypes.c_int32), ("device", ctypes.c_int32),
        ("Cstar", c_double_p), ("N", c_double_p), ("W", c_double_p),
        ("weekday_c", c_double_p), ("log_area_c", c_double_p),
        ("car_Q", c_double_p), ("car_half_logdet", ctypes.c_double),
        ("init_state", c_double_p),
        ("nu", ctypes.c_double), ("time_delta", ctypes.c_double),
        ("rate_floor", ctypes.c_double),
    ]


class SeirSamplerDesc(ctypes.Structure):
    """Mirror of `seir_sampler_desc` (include/seir_hip.h)."""
    _fields_ = [
        ("num_chains", ctypes.c_int32),
        ("dmax", ctypes.c_int32), ("nmax", ctypes.c_int32), ("m", ctypes.c_int32),
        ("occult_nmax", ctypes.c_int32), ("num_event_time_updates", ctypes.c_int32),
        ("t_range_lo", ctypes.c_int32), ("t_range_hi", ctypes.c_int32),
        ("num_leapfrog_steps", ctypes.c_int32), ("trace_capacity", ctypes.c_int32),
        ("first_chain_id", ctypes.c_int32), ("record_events", ctypes.c_int32),
        ("seed", ctypes.c_uint64),
        # ABI v2: launch form and test hooks, all-zero = defaults
        ("moves_mode", ctypes.c_int32), ("hmc_mode", ctypes.c_int32), ("use_graph", ctypes.c_int32),
        ("chain_groups", ctypes.c_int32), ("disable_mask", ctypes.c_int32), ("debug_pair", ctypes.c_int32),
        ("leap_rows", ctypes.c_int32), ("thin", ctypes.c_int32),
    ]


class SeirSimDesc(ctypes.Structure):
    """Mirror of `seir_sim_desc` (include/seir_hip.h)."""
    _fields_ = [
        ("num_draws", ctypes.c_int32), ("num_steps", ctypes.c_int32),
        ("first_draw_id", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("seed", ctypes.c_uint64),
        ("par", ctypes.POINTER(ctypes.c_double)), ("log_baseline", ctypes.POINTER(ctypes.c_double)),
        ("spatial", ctypes.POINTER(ctypes.c_double)), ("W", ctypes.POINTER(ctypes.c_double)),
        ("weekday_c", ctypes.POINTER(ctypes.c_double)), ("init_state", ctypes.POINTER(ctypes.c_double)),
        ("events", ctypes.POINTER(ctypes.c_double)),
    ]


class SeirProductState(ctypes.Structure):
    """Mirror of `seir_product_state` (include/seir_hip.h)."""
    _fields_ = [(k, ctypes.c_int32) for k in ("summary_on", "diag_batch_len", "forecast_H", "check_K", "rt_D", "wb_D", "groups_G",
                                              "groups_nnz")] + [("group_L", ctypes.c_int32 * 3)] + \
        [(k, ctypes.c_int32) for k in ("group_rt_on", "group_wb_on", "group_rt_D", "group_wb_D", "ngm_D")] + \
        [(k, ctypes.c_int64) for k in ("fc_j", "ck_j", "rt_j", "ngm_cap", "fc_keep_cap", "rt_keep_cap")] + \
        [("reserved", ctypes.c_uint64 * 2)]


class SeirSweepPlan(ctypes.Structure):
    """Mirror of `seir_sweep_plan` (include/seir_hip.h)."""
    _fields_ = [(k, ctypes.c_int32) for k in (
        "hmc", "inner", "ts_mode", "per", "nbv", "nlive", "end_in_leap", "chunk_aff", "final_aff", "leap_nst", "leap_nmt",
        "leap_wgs", "leap_nbv", "leap_nlive", "leap_launches", "section_launches", "section_evals", "moves", "nband", "nbk",
        "pair_nlive", "nch", "fpend", "pre", "move_aff", "record", "advance")] + [("reserved", ctypes.c_int32 * 5)]


# the enums of SweepPlan (csrc/sweep_plan.h), by the names tests/test_sweep_plan.py gives them
PLAN_HMC = ("fold", "tailfold", "stage")
PLAN_INNER = ("single", "leap", "se_chunk", "split")
PLAN_MOVES = ("pairs", "pair", "split")
PLAN_FPEND = (None, "k_move_pairs", "k_record", "k_apply_fpend")

ABI_VERSION = 4               # SEIR_ABI_VERSION
OPT_DEBUG_SKEW, OPT_XCD_AFFINITY, OPT_GEMM_F32, OPT_EVAL_FORM, OPT_RT_STAGING_KIB, OPT_GENERIC_MOVES = 0, 1, 2, 3, 4, 5
ERR_INVALID, ERR_STATE = -1, -3   # SEIR_ERR_INVALID, SEIR_ERR_STATE
ERR_HANDOFF = -4              # SEIR_ERR_HANDOFF
MMAX = 4                      # SEIR_MMAX
MM_SMALL = 2                  # csrc/sampler_kernels.h: the sub-moves the event-update kernels have instances of their own for
MOVE_TRACE = 2 + 4 * MMAX     # SEIR_MOVE_TRACE
FORECAST_MAX_H = 128          # SEIR_FORECAST_MAX_H
FORECAST_ID_SHIFT, FORECAST_MAX_CHAIN = 20, 2048   # draw id = (global chain id << 20) + j
CHECK_MAX_DAYS = 128          # SEIR_CHECK_MAX_DAYS
PAIR_ABS_CHUNK = 4096         # SEIR_PAIR_ABS_CHUNK
PAIR_ABS_MAX_N = 92681        # SEIR_PAIR_ABS_MAX_N
ORDER_STATS_MAX_RANKS = 16    # SEIR_ORDER_STATS_MAX_RANKS
GROUPS_MAX = 256              # SEIR_GROUPS_MAX
# csrc/trace_load.h: the codes of a loaded item (LOAD_OK = 0 ...; out[code - 1] of seir_sampler_load_status counts them)
LOAD_CODES = ("ok", "not an integer", "negative", "over the trace's width", "state below zero", "theta not finite")
# SEIR_FN_*: the functions of seir_selftest_fn, name -> (op, takes y, has out1)
SELFTEST_FN = {"fast_log": (0, False, False), "fast_rcp": (1, False, False), "mv_log": (2, False, False),
               "softplus_tab": (3, False, False), "softplus_sigmoid_tab": (4, False, True), "softplus": (5, False, False),
               "lfact_bf": (6, False, False), "lbinom_tab": (7, True, False), "lbinom_const": (8, True, False),
               "lbinom_bf": (9, True, False), "log1mexp_tab": (10, False, False), "log1mexp": (11, False, False),
               "log1mexp_series": (12, False, True), "l1me_inv_series": (13, False, True), "l1me_inv_k": (14, False, True),
               "l1me_inv_series_k": (15, False, True), "log1mexp_diff_slow": (16, True, False), "fast_log_k": (17, False, False)}
SELFTEST_DELTA = {"band": 0, "own_ei": 1, "own_se": 2}                        # SEIR_DELTA_*
# SEIR_WAVE_* / SEIR_BLOCK_*: name -> (op, has an int32 form)
SELFTEST_WAVE = {"wave_sum": (0, True), "wave_min": (1, False), "wave_incl_scan": (2, True),
                 "wave_incl_suffix_scan": (3, False), "block_excl_scan_256": (4, True),
                 "block_incl_suffix_scan_256": (5, False), "block_sum_256": (6, False)}


class SeirError(RuntimeError):
    def __init__(self, msg, code=0):
        super().__init__(msg)
        self.code = code


class HandoffTimeout(SeirError):
    """A wait inside one of the persistent launches gave up (SEIR_ERR_HANDOFF from a read of the trace): its
    workgroups were not all resident -- something else holds part of the GPU.  `ChainSampler` recovers from it by
    itself (snapshot, restore, per-step launch forms)."""


# name -> (restype, argtypes); every symbol include/seir_hip.h declares
_SIGNATURES = {
    "seir_abi_version": (ctypes.c_int, []),
    "seir_last_error": (ctypes.c_char_p, []),
    "seir_create": (ctypes.c_int, [ctypes.POINTER(SeirDesc), c_void_pp]),
    "seir_destroy": (None, [ctypes.c_void_p]),
    "seir_num_params": (ctypes.c_int, [ctypes.c_void_p]),
    "seir_set_initial_state": (ctypes.c_int, [ctypes.c_void_p, c_double_p]),
    "seir_log_prob": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_double_p, c_double_p, c_double_p]),
    "seir_log_prob_grad": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_double_p, c_double_p,
                                          c_double_p, c_double_p]),
    "seir_log_prob_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_void_p] * 4),
    "seir_prepare_events_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]),
    "seir_eval_prepared_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_void_p] * 3),
    "seir_sync": (ctypes.c_int, [ctypes.c_void_p]),
    "seir_stream": (ctypes.c_void_p, [ctypes.c_void_p]),
    "seir_set_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]),
    "seir_malloc": (ctypes.c_int, [c_void_pp, ctypes.c_uint64]),
    "seir_free": (ctypes.c_int, [ctypes.c_void_p]),
    "seir_memcpy_h2d": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "seir_memcpy_d2h": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "seir_timer_start": (ctypes.c_int, [ctypes.c_void_p]),
    "seir_timer_stop": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]),
    "seir_time_kernel": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                        ctypes.POINTER(ctypes.c_float)]),
    "seir_selftest_math": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32] + [c_double_p] * 4),
    "seir_selftest_math_wide": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32] + [c_double_p] * 3),
    # the device math by function, the delta log-ratios and the wave primitives (csrc/selftest_kernels.h)
    "seir_selftest_fn": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32] + [c_double_p] * 4),
    "seir_selftest_band_delta": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32] + [c_double_p] * 7 +
                                 [ctypes.c_double, ctypes.c_double, c_double_p]),
    "seir_selftest_wave": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32] +
                           [ctypes.c_void_p] * 3),
    "seir_reproduction_number": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_double_p, c_double_p, c_double_p]),
    "seir_within_between": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_double_p, c_double_p, ctypes.c_double,
                                           c_double_p, c_double_p]),
    "seir_simulate": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(SeirSimDesc)]),
    "seir_selftest_binomial": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                              c_double_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_int32)]),
    "seir_sampler_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(SeirSamplerDesc), c_void_pp]),
    "seir_sampler_destroy": (None, [ctypes.c_void_p]),
    "seir_sampler_set_state": (ctypes.c_int, [ctypes.c_void_p, c_double_p, c_double_p]),
    "seir_sampler_get_state": (ctypes.c_int, [ctypes.c_void_p, c_double_p, c_double_p, c_double_p]),
    "seir_sampler_set_kernel": (ctypes.c_int, [ctypes.c_void_p, c_double_p, c_double_p]),
    "seir_sampler_get_kernel": (ctypes.c_int, [ctypes.c_void_p, c_double_p, c_double_p]),
    "seir_sampler_set_adaptation": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                                   ctypes.c_int32, ctypes.c_double, c_double_p, c_double_p,
                                                   c_double_p]),
    "seir_sampler_refresh": (ctypes.c_int, [ctypes.c_void_p]),
    "seir_sampler_reset_trace": (ctypes.c_int, [ctypes.c_void_p]),
    "seir_sampler_reset_trace_at": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "seir_sampler_set_thin": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "seir_sampler_thin": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]),
    "seir_sampler_read_trace_async": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, c_double_p,
                                                     ctypes.c_void_p, c_double_p, c_double_p]),
    "seir_sampler_trace_wait": (ctypes.c_int, [ctypes.c_void_p]),
    "seir_host_alloc": (ctypes.c_int, [c_void_pp, ctypes.c_uint64]),
    "seir_host_free": (ctypes.c_int, [ctypes.c_void_p]),
    "seir_sampler_run": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "seir_sampler_read_trace": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, c_double_p,
                                               ctypes.c_void_p, c_double_p, c_double_p]),
    "seir_sampler_time_grad_kernel": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32,
                                                     ctypes.POINTER(ctypes.c_float)]),
    "seir_sampler_time_leapfrog": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_float),
                                                  ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "seir_sampler_pair_timeouts": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]),
    "seir_sampler_xcd_local": (ctypes.c_int, [ctypes.c_void_p]),
    "seir_sampler_snapshot": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "seir_sampler_restore": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "seir_sampler_debug_fail_handoff": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "seir_sampler_set_launch_form": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]),
    "seir_sampler_launch_form": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32),
                                                ctypes.POINTER(ctypes.c_int32)]),
    "seir_sampler_sweep_plan": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(SeirSweepPlan)]),
    "seir_move_instance": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32]),
    "seir_sampler_move_instance": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]),
    # summaries of the recorded events on the device: moments and marginals
    "seir_sampler_summary_reset": (ctypes.c_int, [ctypes.c_void_p]),
    "seir_sampler_summarize": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "seir_sampler_read_marginals": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                                   c_int64_p, c_int64_p, c_int64_p]),
    "seir_sampler_read_marginals_async": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                                         c_int64_p, c_int64_p, c_int64_p]),
    "seir_sampler_read_summary": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64),
                                                 ctypes.POINTER(ctypes.c_int32), c_int64_p,
                                                 ctypes.POINTER(ctypes.c_uint64)]),
    # convergence diagnostics: batch sums and marks next to the moments
    "seir_sampler_diag_reset": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "seir_sampler_diag_mark": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "seir_sampler_read_diag": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), c_int64_p,
                                              ctypes.POINTER(ctypes.c_uint64)]),
    "seir_sampler_read_diag_mark": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64),
                                                   c_int64_p, ctypes.POINTER(ctypes.c_uint64)]),
    # forecast of the next H days from the burst buffer: moments and marginals of the simulated counts
    "seir_sampler_forecast_reset": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_double_p, c_double_p, ctypes.c_uint64]),
    "seir_sampler_forecast": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, c_double_p]),
    "seir_sampler_read_forecast_marginals": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                                            c_int64_p, c_int64_p, c_int64_p]),
    "seir_sampler_read_forecast_marginals_async": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                                                  c_int64_p, c_int64_p, c_int64_p]),
    "seir_sampler_read_forecast": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64),
                                                  ctypes.POINTER(ctypes.c_int32), c_int64_p,
                                                  ctypes.POINTER(ctypes.c_uint64)]),
    # forecast intervals: the draw store and exact order statistics of its cells; the selection alone on host arrays
    "seir_sampler_forecast_keep": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64]),
    "seir_sampler_forecast_order_stats": (ctypes.c_int, [ctypes.c_void_p, c_int64_p, ctypes.c_int32, ctypes.c_int32,
                                                         ctypes.POINTER(ctypes.c_int32)]),
    "seir_order_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int64, ctypes.c_int32,
                                        ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_int64_p, ctypes.c_int32,
                                        ctypes.POINTER(ctypes.c_int32)]),
    # in-sample check of the last K days from the burst buffer: moments, marginals and the comparison with the data
    "seir_sampler_check_reset": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_double_p, c_double_p, ctypes.c_uint64]),
    "seir_sampler_check": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]),
    "seir_sampler_read_check": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64),
                                               ctypes.POINTER(ctypes.c_int32), c_int64_p, ctypes.POINTER(ctypes.c_uint64)]),
    "seir_sampler_read_check_marginals": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                                         c_int64_p, c_int64_p, c_int64_p]),
    "seir_sampler_read_check_marginals_async": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                                               c_int64_p, c_int64_p, c_int64_p]),
    "seir_sampler_read_check_counts": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)] +
                                       [ctypes.POINTER(ctypes.c_uint32)] * 8),
    # reproduction number of the kept draws from the burst buffer: R_it moments and the national curve per draw
    "seir_sampler_rt_reset": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_double_p]),
    "seir_sampler_rt": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]),
    "seir_sampler_read_rt_draws": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, c_double_p]),
    "seir_sampler_read_rt_draws_async": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, c_double_p]),
    "seir_sampler_read_rt": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), c_double_p, c_double_p,
                                            c_double_p, ctypes.POINTER(ctypes.c_uint32)]),
    # R_t intervals: the R_it draw store and exact order statistics of its cells; the fp64 selection alone on host arrays
    "seir_sampler_rt_keep": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64]),
    "seir_sampler_rt_order_stats": (ctypes.c_int, [ctypes.c_void_p, c_int64_p, ctypes.c_int32, ctypes.c_int32, c_double_p]),
    "seir_order_stats_f64": (ctypes.c_int, [ctypes.c_void_p, c_double_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64,
                                            ctypes.c_int64, ctypes.c_int64, c_int64_p, ctypes.c_int32, c_double_p]),
    # within/between pressure shares of the kept draws from the burst buffer: moments per cell, national pressures per draw
    "seir_sampler_wb_reset": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "seir_sampler_wb": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]),
    "seir_sampler_read_wb": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32),
                                            c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                            ctypes.POINTER(ctypes.c_uint32)]),
    "seir_sampler_read_wb_draws": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, c_double_p, c_double_p]),
    "seir_sampler_read_wb_draws_async": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, c_double_p,
                                                        c_double_p]),
    # region totals: per-draw sums over groups of locations (trace, forecast, check); the kernel alone on host arrays
    "seir_sampler_groups_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                               ctypes.POINTER(ctypes.c_int32)]),
    "seir_sampler_read_group_marginals": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                         c_int64_p, c_int64_p]),
    "seir_sampler_read_group_marginals_async": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                               c_int64_p, c_int64_p]),
    "seir_group_sums": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int64, ctypes.c_int32,
                                       ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                       ctypes.POINTER(ctypes.c_int32), c_int64_p]),
    # group curves: R_t and within / between per group of every kept draw; the kernel alone on host arrays
    "seir_sampler_group_rt": (ctypes.c_int, [ctypes.c_void_p, c_double_p]),
    "seir_sampler_group_wb": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "seir_sampler_read_group_rt": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, c_double_p]),
    "seir_sampler_read_group_rt_async": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, c_double_p]),
    "seir_sampler_read_group_wb": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, c_double_p, c_double_p]),
    "seir_sampler_read_group_wb_async": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, c_double_p, c_double_p]),
    "seir_group_wsums": (ctypes.c_int, [ctypes.c_void_p, c_double_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                        ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                        c_double_p, c_double_p]),
    # group next-generation matrix of every kept draw (rides on seir_sampler_rt); the rows kernel alone on host arrays
    "seir_sampler_group_ngm": (ctypes.c_int, [ctypes.c_void_p, c_double_p, ctypes.c_int64]),
    "seir_sampler_read_group_ngm": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, c_double_p]),
    "seir_group_ngm_rows": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_double_p, ctypes.POINTER(ctypes.c_int32),
                                           ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                           ctypes.POINTER(ctypes.c_int32), c_double_p]),
    # stored draws into trace slots: the rows of a posterior file behind every product; the counters of what was wrong in them
    "seir_sampler_load_trace": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, c_double_p,
                                               c_double_p]),
    "seir_sampler_load_status": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int32]),
    # the state of the products, from the sampler's host fields: the binding keeps no copy of it
    "seir_sampler_product_state": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(SeirProductState)]),
    # scenario forecasts riding on the sampler's forecast; the fold of the paired differences alone on host arrays
    "seir_sampler_scenarios_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_double_p, c_double_p, ctypes.c_int64]),
    "seir_sampler_scenario_state": (ctypes.c_int, [ctypes.c_void_p, c_int64_p]),
    "seir_sampler_read_scenarios": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64),
                                                   ctypes.POINTER(ctypes.c_int32), c_int64_p, ctypes.POINTER(ctypes.c_uint64)]),
    "seir_sampler_read_scenario_diffs": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), c_int64_p,
                                                        ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32),
                                                        ctypes.POINTER(ctypes.c_uint32)]),
    "seir_sampler_read_scenario_draws": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, c_int64_p, c_int64_p]),
    "seir_scenario_diffs": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                           ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64,
                                           ctypes.POINTER(ctypes.c_int32), c_int64_p, ctypes.POINTER(ctypes.c_uint64),
                                           ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                           ctypes.POINTER(ctypes.c_uint32)]),
    # targeted scenarios: per-location operands, and the scenarios' per-draw region totals
    "seir_sampler_scenarios_set_local": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_double_p, c_double_p, ctypes.c_int64]),
    "seir_sampler_scenario_groups_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "seir_sampler_read_scenario_group_draws": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, c_int64_p]),
    # triggered scenarios: two operand pairs and a rule on the draw's own case counts; the fold of the rule's record alone
    "seir_sampler_scenarios_set_triggered": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_double_p, c_double_p, c_double_p,
                                                            c_double_p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                                            ctypes.POINTER(ctypes.c_int32), ctypes.c_int64]),
    "seir_sampler_read_scenario_triggers": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]),
    "seir_sampler_read_scenario_trigger_draws": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                                                ctypes.POINTER(ctypes.c_int32)]),
    "seir_trigger_counts": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int64, ctypes.c_int32,
                                           ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32),
                                           ctypes.POINTER(ctypes.c_int32)]),
    # the forecast scored against later data; the sum of pairwise absolute differences alone on host arrays
    "seir_sampler_verify_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]),
    "seir_sampler_verify_state": (ctypes.c_int, [ctypes.c_void_p, c_int64_p]),
    "seir_sampler_read_verify": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32),
                                                ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)]),
    "seir_sampler_forecast_pair_sums": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, c_int64_p]),
    "seir_pair_abs_sums": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int64, ctypes.c_int32,
                                          ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_int64_p,
                                          ctypes.POINTER(ctypes.c_uint32)]),
}

_lib = None


def exported_symbols():
    return sorted(_SIGNATURES)


def load():
    """Load libseirhip.so (once).  Raises SeirError if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SeirError(
                f"{LIB_PATH} not found: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()'). "
                "This package has no CPU fallback.")
        # PyTorch bundles its own libamdhip64; two HIP runtimes in one process break whichever
        # initialises second (torch.cuda.is_available() turns False).  Importing torch first makes
        # libseirhip's libamdhip64 dependency resolve to the runtime torch already loaded.
        try:
            import torch  # noqa: F401
        except ImportError:                           # pragma: no cover - torch-free hosts
            pass
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)       # AttributeError if the .so is stale
            fn.restype = res
            fn.argtypes = args
        if lib.seir_abi_version() != ABI_VERSION:
            raise SeirError(f"{LIB_PATH} has ABI {lib.seir_abi_version()}, this binding needs {ABI_VERSION}: rebuild it")
        _lib = lib
    return _lib


def check(rc):
    if rc != 0:
        msg = load().seir_last_error()
        text = msg.decode() if msg else "?"
        cls = HandoffTimeout if rc == ERR_HANDOFF else SeirError
        raise cls(f"libseirhip call failed ({rc}): {text}", rc)

"""`ChainSampler`: host handle on the device-resident Metropolis-within-Gibbs
sampler of libseirhip (C-ABI section "Device-resident Metropolis-within-Gibbs
sampler" of include/seir_hip.h).

It plays the role of the `GibbsKernel` + `tfp.mcmc.sample_chain` pair the
reference builds per window (covid19uk/inference/inference.py:60-242): the host
chooses the window mode (fixed / dual-averaging / dual-averaging + diagonal
mass adaptation), asks for `n` sweeps, and reads draws and kernel-result
traces back.  All sampling arithmetic runs in HIP kernels.
"""
from __future__ import annotations

import ctypes
import dataclasses
import sys

import numpy as np

from . import _lib
from .posterior.diagnostics import Diagnostics
from .seir import SeirModel, _dptr

MOVE_KEYS = ("move/S->E", "move/E->I", "occult/S->E", "occult/E->I")   # inference.py:277-280
MOVES_MODES = {"paired": 0, "split": 1, "paired-nopre": 2, "paired-delta": 3, "paired-launch": 4}
HMC_MODES = {"chunk": 0, "single": 1, "chunk-split": 2, "chunk-launch": 3, "chunk-leap": 4, "chunk-stage": 5,
             "chunk-launch-fold": 6}
# Launch forms to fall back on when a hand-off inside a persistent launch times out (the GPU is shared with something):
# first the per-step forms, whose waiting workgroups are always placed behind the ones they wait for, then the forms
# without any hand-off inside a launch.  What is sampled is the same in all of them.
FALLBACK_FORMS = (("chunk-launch", "paired-launch"), ("chunk-split", "paired-delta"))


@dataclasses.dataclass
class Trace:
    """Draws and kernel results of `count` kept sweeps for B chains (leading axes [count, B])."""
    theta: np.ndarray        # [n,B,P] constrained parameter draws
    events: np.ndarray       # [n,B,M,T,3] int32 or uint16 (or None)
    hmc: dict                # is_accepted, target_log_prob, step_size  -> [n,B]
    moves: dict              # MOVE_KEYS -> dict(is_accepted [n,B], target_log_prob [n,B], proposed_delta [n,B,4,m])
    marginals: dict = None   # MARGINAL_KEYS -> int64 [n,B,T,3] / [n,B,M,3] / [n,B,T,3]; None unless asked for
    forecast: dict = None    # FORECAST_KEYS -> int64 [n,B,H,3] / [n,B,M,3] / [n,B,H,3]; None unless the draws were forecast
    rt: np.ndarray = None    # [n,B,D] national R_t of every kept draw over the window; None unless asked for
    check: dict = None       # CHECK_KEYS -> int64 [n,B,K,3] / [n,B,M,3] / [n,B,K,3]; None unless the draws were checked
    wb: dict = None          # WB_KEYS -> float64 [n,B,D] national within / between pressure; None unless asked for
    groups: dict = None      # GROUP_KEYS of the sources that ran -> int64 [n,B,G,L,3] / [n,B,G,3]; None unless asked for
    group_curves: dict = None  # GROUP_CURVE_KEYS of the curves that are on -> float64 [n,B,G,D]; None unless one is on


MARGINAL_KEYS = ("events_by_day", "events_by_location", "state_by_day")
FORECAST_KEYS = ("forecast_by_day", "forecast_by_location", "forecast_state_by_day")
FORECAST_QUANTILE_PLANES = ("cases", "cum_cases", "prevalence")   # the planes of the draw store (keep_forecast_draws)
CHECK_KEYS = ("check_by_day", "check_by_location", "check_state_by_day")
WB_KEYS = ("within_pressure", "between_pressure")
# region totals (set_groups): source -> (which of the C-ABI, events_by_group key, state0_by_group key or None)
GROUP_SOURCES = {"trace": (0, "seir_by_group", None), "forecast": (1, "forecast_by_group", "forecast_group_state0"),
                 "check": (2, "check_by_group", "check_group_state0")}
GROUP_KEYS = tuple(k for _, ev, st in GROUP_SOURCES.values() for k in (ev, st) if k)
# group curves (set_group_rt / set_group_within_between): R_t and the within / between pressures of a draw per group
GROUP_CURVE_KEYS = ("rt_by_group", "within_by_group", "between_by_group")
SUMMARY_QUANTITIES = ("k_se", "k_ei", "k_ir", "S", "E", "I")


@dataclasses.dataclass
class Summary:
    """Moments of the recorded events and of the state over the kept draws folded since the last `reset_summary`
    (include/seir_hip.h, "Summaries of samples/seir on the device"): exact integers, per chain.  The last axis is
    `SUMMARY_QUANTITIES`; the state is the one at the start of the day (`model_spec.compute_state`)."""
    count: np.ndarray        # [B] uint64 draws folded
    ref: np.ndarray          # [B,M,T,6] int32: the value in the first draw folded
    sum: np.ndarray          # [B,M,T,6] int64: sum_j (x_j - ref)
    sumsq: np.ndarray        # [B,M,T,6] uint64: sum_j (x_j - ref)^2

    @property
    def mean(self) -> np.ndarray:
        """ref + sum / n, float64 [B,M,T,6]; NaN for a chain with no draw."""
        return summary_mean(self.count, self.ref, self.sum)

    @property
    def var(self) -> np.ndarray:
        """Unbiased variance (sumsq - sum^2 / n) / (n - 1), float64 [B,M,T,6]; NaN where n < 2."""
        return summary_var(self.count, self.sum, self.sumsq)


@dataclasses.dataclass
class RtSummary:
    """Moments of R_it over the kept draws folded since the last `reset_rt` (include/seir_hip.h, "Reproduction number on
    the device"), per chain, day of the window [T - D, T) and location: the device's accumulators as they are, and what
    the host forms from them."""
    count: np.ndarray        # [B] uint64 draws folded
    ref: np.ndarray          # [B,D,M] float64: R_it of the first draw folded
    sum: np.ndarray          # [B,D,M] float64: sum_j (r_j - ref)
    sumsq: np.ndarray        # [B,D,M] float64: sum_j (r_j - ref)^2
    gt1: np.ndarray          # [B,D,M] uint32: draws with r_j > 1

    @property
    def mean(self) -> np.ndarray:
        """ref + sum / n, [B,D,M]; NaN for a chain with no draw."""
        return summary_mean(self.count, self.ref, self.sum)

    @property
    def var(self) -> np.ndarray:
        """Unbiased variance (sumsq - sum^2 / n) / (n - 1), [B,D,M]; NaN (no warning) where n < 2."""
        return summary_var(self.count, self.sum, self.sumsq)

    @property
    def prob_gt1(self) -> np.ndarray:
        """gt1 / n, the posterior probability of R_it > 1, [B,D,M]; NaN for a chain with no draw."""
        return rt_prob_gt1(self.count, self.gt1)


@dataclasses.dataclass
class WbSummary:
    """The within/between pressure shares folded since the last `reset_within_between` (include/seir_hip.h, "Within/between
    pressure shares on the device"), per chain, day of the window [T - D, T) and location: the device's accumulators as they
    are, and what the host forms from them.  A draw whose shares are not finite for a cell (no infective anywhere) is counted
    in `count` and in no cell."""
    count: np.ndarray        # [B] uint64 draws folded, defined or not
    defined: np.ndarray      # [B,D,M] uint32: draws with finite shares in the cell
    ref_w: np.ndarray        # [B,D,M] float64: the within share of the cell's first defined draw
    sum_w: np.ndarray        # [B,D,M] float64: sum_j (within_j - ref_w)
    sumsq_w: np.ndarray      # [B,D,M] float64: sum_j (within_j - ref_w)^2
    ref_b: np.ndarray        # [B,D,M] float64: the between share of the cell's first defined draw
    sum_b: np.ndarray        # [B,D,M] float64: sum_j (between_j - ref_b)
    gt: np.ndarray           # [B,D,M] uint32: draws with within_j > between_j

    @property
    def within_mean(self) -> np.ndarray:
        """ref_w + sum_w / defined, [B,D,M]; NaN (no warning) where defined = 0."""
        return wb_mean(self.defined, self.ref_w, self.sum_w)

    @property
    def within_var(self) -> np.ndarray:
        """Unbiased variance (sumsq_w - sum_w^2 / defined) / (defined - 1), [B,D,M]; NaN (no warning) where defined < 2."""
        return summary_var(self.defined, self.sum_w, self.sumsq_w)

    @property
    def between_mean(self) -> np.ndarray:
        """ref_b + sum_b / defined, [B,D,M]; NaN (no warning) where defined = 0."""
        return wb_mean(self.defined, self.ref_b, self.sum_b)

    @property
    def p_within_gt_between(self) -> np.ndarray:
        """gt / defined, [B,D,M]; NaN (no warning) where defined = 0."""
        return wb_mean(self.defined, 0.0, self.gt)


def wb_mean(defined, ref, sum_):
    """ref + sum / n per cell; NaN, without a warning, where n = 0."""
    n = np.asarray(defined, np.float64)
    ok = n > 0
    return np.where(ok, np.asarray(ref, np.float64) + np.asarray(sum_, np.float64) / np.where(ok, n, 1.0), np.nan)


@dataclasses.dataclass
class CheckSummary:
    """The in-sample check folded since the last `reset_check` (include/seir_hip.h, "In-sample predictive check on the
    device"), per chain: the moments of the re-simulated last K days (a `Summary` over [B,M,K,6]) and the integer counts
    of the comparison with the observed removals.  gt is count - lt - eq; the mid-p values are formed by `mid_p`."""
    moments: Summary
    observed: np.ndarray     # [B,M,K] int32: the recorded I->R counts of the window
    lt: np.ndarray           # [B,M,K] uint32: draws whose simulated I->R count is < observed
    eq: np.ndarray           # [B,M,K] uint32: ... == observed
    location_lt: np.ndarray  # [B,M]: the location's total over the window
    location_eq: np.ndarray
    day_lt: np.ndarray       # [B,K]: the day's total over the locations
    day_eq: np.ndarray
    total_lt: np.ndarray     # [B]: the whole window, all locations
    total_eq: np.ndarray

    @property
    def count(self) -> np.ndarray:
        return self.moments.count

    @property
    def pit(self) -> np.ndarray:
        return mid_p(self.count, self.lt, self.eq)

    @property
    def location_pit(self) -> np.ndarray:
        return mid_p(self.count, self.location_lt, self.location_eq)

    @property
    def day_pit(self) -> np.ndarray:
        return mid_p(self.count, self.day_lt, self.day_eq)

    @property
    def total_pit(self) -> np.ndarray:
        return mid_p(self.count, self.total_lt, self.total_eq)


def mid_p(count, lt, eq):
    """The mid-p value (lt + eq / 2) / count of an observed value among `count` simulated ones (count broadcast over the
    leading axes); NaN, without a warning, where count = 0.  2 lt + eq < 2^22 is exact in float64 and so is the halving:
    the result is the correctly rounded quotient (2 lt + eq) / (2 count)."""
    n = _per_chain(count, lt)
    num = 2.0 * np.asarray(lt, np.float64) + np.asarray(eq, np.float64)
    ok = n > 0
    return np.where(ok, num / np.where(ok, 2.0 * n, 1.0), np.nan)


def rt_prob_gt1(count, gt1):
    """gt1 / n (count broadcast over the leading axes); NaN where n = 0."""
    n = _per_chain(count, gt1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n > 0, np.asarray(gt1, np.float64) / n, np.nan)


def forecast_draw_id(global_chain_id: int, j: int) -> int:
    """The Philox draw id of the forecast of a chain's j-th draw since the last `reset_forecast`
    (include/seir_hip.h, "Forecast on the device"): (global chain id << 20) + j, with both limits."""
    c, j = int(global_chain_id), int(j)
    if not 0 <= c < _lib.FORECAST_MAX_CHAIN:
        raise ValueError(f"global chain id {c}: the forecast's draw ids need chain ids in [0, {_lib.FORECAST_MAX_CHAIN})")
    if not 0 <= j < (1 << _lib.FORECAST_ID_SHIFT):
        raise ValueError(f"draw number {j}: fewer than 2^{_lib.FORECAST_ID_SHIFT} draws per chain between two forecast resets")
    return (c << _lib.FORECAST_ID_SHIFT) + j


def _per_chain(count, like):
    n = np.asarray(count).astype(np.float64)
    return n.reshape(n.shape + (1,) * (np.ndim(like) - n.ndim))


def summary_mean(count, ref, sum_):
    """mean = ref + sum / n from the integer accumulators (count broadcast over the leading axes); NaN where n = 0."""
    n = _per_chain(count, ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n > 0, np.asarray(ref, np.float64) + np.asarray(sum_, np.float64) / n, np.nan)


def summary_var(count, sum_, sumsq):
    """Unbiased variance (sumsq - sum^2 / n) / (n - 1) from the integer accumulators; NaN (no warning) where n < 2."""
    n = _per_chain(count, sum_)
    s1, s2 = np.asarray(sum_, np.float64), np.asarray(sumsq, np.float64)
    ok = n > 1
    nn = np.where(ok, n, 2.0)
    return np.where(ok, (s2 - s1 * s1 / nn) / (nn - 1.0), np.nan)


class PinnedTrace:
    """Page-locked host arrays for `count` sweeps of the burst buffer (seir_host_alloc): the target of
    `ChainSampler.read_trace_async`.  Views are valid until close()."""

    def __init__(self, sampler: "ChainSampler", count: int, events: bool = True, marginals: bool = False,
                 forecast: int = 0, rt: int = 0, check: int = 0, wb: int = 0, groups=None, group_curves=None):
        self._lib = sampler._lib
        self.count = int(count)
        B, P, M, T = sampler.B, sampler.P, sampler.M, sampler.T
        self._ptrs = []
        self.theta = self._alloc((count, B, P), np.float64)
        self.events = self._alloc((count, B, M, T, 3), sampler.events_dtype) if (events and sampler.record_events) else None
        self.hmc = self._alloc((count, B, 3), np.float64)
        self.moves = self._alloc((count, B, 4, _lib.MOVE_TRACE), np.float64)
        self.marginals = None
        if marginals:
            self.marginals = dict(events_by_day=self._alloc((count, B, T, 3), np.int64),
                                  events_by_location=self._alloc((count, B, M, 3), np.int64),
                                  state_by_day=self._alloc((count, B, T, 3), np.int64))
        self.forecast = None
        if forecast:
            H = int(forecast)
            self.forecast = dict(forecast_by_day=self._alloc((count, B, H, 3), np.int64),
                                 forecast_by_location=self._alloc((count, B, M, 3), np.int64),
                                 forecast_state_by_day=self._alloc((count, B, H, 3), np.int64))
        self.rt = self._alloc((count, B, int(rt)), np.float64) if rt else None
        self.check = None
        if check:
            K = int(check)
            self.check = dict(check_by_day=self._alloc((count, B, K, 3), np.int64),
                              check_by_location=self._alloc((count, B, M, 3), np.int64),
                              check_state_by_day=self._alloc((count, B, K, 3), np.int64))
        self.wb = {k: self._alloc((count, B, int(wb)), np.float64) for k in WB_KEYS} if wb else None
        # groups: (G, {source: day extent}) -- the group sums of the sources that run with the burst
        self.groups = None
        if groups:
            G, lens = groups
            self.groups = {}
            for src, L in lens.items():
                _, ev_key, st_key = GROUP_SOURCES[src]
                self.groups[ev_key] = self._alloc((count, B, G, int(L), 3), np.int64)
                if st_key:
                    self.groups[st_key] = self._alloc((count, B, G, 3), np.int64)
        # group_curves: (G, {key of GROUP_CURVE_KEYS: window days}) -- the curves that run with the burst
        self.group_curves = None
        if group_curves:
            G, days = group_curves
            self.group_curves = {k: self._alloc((count, B, G, int(D)), np.float64) for k, D in days.items()}

    def _alloc(self, shape, dtype):
        nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        p = ctypes.c_void_p()
        _lib.check(self._lib.seir_host_alloc(ctypes.byref(p), max(nbytes, 8)))
        self._ptrs.append(p)
        buf = (ctypes.c_char * max(nbytes, 8)).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape, dtype=np.int64))).reshape(shape)

    def close(self):
        self.theta = self.events = self.hmc = self.moves = self.marginals = self.forecast = self.rt = self.check = self.wb = None
        self.groups = self.group_curves = None
        for p in self._ptrs:
            self._lib.seir_host_free(p)
        self._ptrs = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ChainSampler:
    # thinning interval in force for the next burst (subclasses that never run __init__ sample every sweep)
    _thin = 1
    _summary_on = False           # reset_summary has been called: the device holds accumulators and marginal arrays
    _diag_L = 0                   # batch length of the diagnostics in force (0: reset_diagnostics was never called)
    _forecast_H = 0               # horizon of the forecast in force (0: reset_forecast was never called)
    _fc_j = 0                     # draws per chain forecast since the last reset_forecast (the library's counter, mirrored)
    _rt_D = 0                     # window of the reproduction number in force (0: reset_rt was never called)
    _check_K = 0                  # window of the in-sample check in force (0: reset_check was never called)
    _wb_D = 0                     # window of the within/between shares in force (0: reset_within_between was never called)
    _groups_G = 0                 # groups of the table in force (0: none set)
    _groups_nnz = 0               # members of the table in force
    _group_rt_on = False          # set_group_rt: group R_t rides on rt
    _group_wb_on = False          # set_group_within_between: group within / between rides on within_between
    _group_rt_refused = False     # the last reset_rt could not size the group outputs: rt is on without them
    _group_wb_refused = False
    first_chain_id = 0

    def __init__(self, model: SeirModel, config: dict, num_chains: int, seed: int = 0,
                 t_range=None, num_leapfrog_steps: int = 16, trace_capacity: int = 100,
                 first_chain_id: int = 0, record_events: bool = True, moves: str = "paired",
                 hmc: str = "chunk", use_graph: bool = False, chain_groups: int = 1,
                 disable: tuple = (), debug_pair: int = 0, auto_recover: bool = True, log=sys.stderr,
                 leap_rows: int = 0, thin: int = 1):
        """`config` is the reference's config["Mcmc"] dict: dmax, nmax, m,
        occult_nmax, num_event_time_updates (mcmc_kernel_factory.py:79-81,106,123).

        Launch form (seir_sampler_desc, ABI v2; none of it changes what is sampled):
        `moves` "paired" (k_move_pair with pre-drawn S->E-type proposals, default) | "paired-nopre" |
        "split" (one proposal kernel per update, cross-check);
        `hmc` "chunk" (default) | "single"; `use_graph`; `chain_groups`.
        `disable`: sub-kernels that draw their proposal but always reject, any of
        "hmc", "move/S->E", "move/E->I", "occult/S->E", "occult/E->I" (invariant-distribution tests).

        `auto_recover`: `sample` and `sample_bursts` snapshot the chain state at the start of every burst and, should a
        hand-off inside a persistent launch time out (`_lib.HandoffTimeout`: the launch could not get all its workgroups on
        the GPU -- another sampler or process holds part of it), restore it, switch to the per-step launch forms
        (`FALLBACK_FORMS`), run the burst again and carry on; after `retry_after` clean bursts the preferred forms are tried
        again (twice as many after every further failure).  Every recovery is logged and kept in `self.recoveries`.

        `thin`: thinning interval k >= 1, the reference's Mcmc.thin (example_config.yaml:33).  The device records the last
        sweep of every group of k (`tfp.mcmc.sample_chain(num_steps_between_results=k - 1)`) and skips the trace writes of
        the others; chain, random streams and adaptation see every sweep.  `sample(n)` / `sample_bursts(nb, n, ...)` keep
        meaning n KEPT draws (n * k sweeps), `trace_capacity` counts kept draws, `run(num_sweeps)` counts sweeps."""
        if int(thin) < 1:
            raise ValueError(f"thin={thin}: the thinning interval is >= 1")
        names = ("hmc",) + MOVE_KEYS
        mask = 0
        for name in disable:
            mask |= 1 << names.index(name)
        self._lib = _lib.load()
        self.model = model
        self.B = int(num_chains)
        self.P, self.M, self.T = model.P, model.M, model.T
        self.mmax = int(config["m"])
        if t_range is None:                       # inference.py:336-339
            t_range = (max(self.T - 21, 0), self.T)
        self.cap = int(trace_capacity)
        # record_events: False, True (int32 counts) or "u16" (uint16 counts: half the burst buffer and half the
        # bytes over PCIe; the read fails loudly if a count exceeds 65535)
        self.record_events = bool(record_events)
        self.events_dtype = np.uint16 if record_events == "u16" else np.int32
        desc = _lib.SeirSamplerDesc(
            num_chains=self.B, dmax=int(config["dmax"]), nmax=int(config["nmax"]), m=self.mmax,
            occult_nmax=int(config["occult_nmax"]),
            num_event_time_updates=int(config["num_event_time_updates"]),
            t_range_lo=int(t_range[0]), t_range_hi=int(t_range[1]),
            num_leapfrog_steps=int(num_leapfrog_steps), trace_capacity=self.cap,
            first_chain_id=int(first_chain_id), record_events=(2 if record_events == "u16" else int(self.record_events)),
            seed=int(seed) & (2 ** 64 - 1),
            moves_mode=MOVES_MODES[moves], hmc_mode=HMC_MODES[hmc],
            use_graph=int(bool(use_graph)), chain_groups=int(chain_groups), disable_mask=mask,
            debug_pair=int(debug_pair), leap_rows=int(leap_rows), thin=int(thin))
        self._s = ctypes.c_void_p()
        _lib.check(self._lib.seir_sampler_create(model._ctx, ctypes.byref(desc), ctypes.byref(self._s)))
        self._thin = int(thin)
        self.first_chain_id = int(first_chain_id)
        self._fc_j_snap = {}
        self.auto_recover = bool(auto_recover) and debug_pair == 0
        self.preferred_form = (hmc, moves)
        self.recoveries = []              # one dict per recovery: burst form that failed, form it was re-run in, message
        self.retry_after = 8              # clean bursts in a fall-back form before the preferred one is tried again
        self._fallback_level = 0          # 0: preferred form; k: FALLBACK_FORMS[k-1]
        self._clean_bursts = 0
        self._log = log

    def close(self):
        for bf in getattr(self, "_pinned", []):
            bf.close()
        self._pinned, self._pinned_key = [], None
        if getattr(self, "_s", None) is not None and self._s:
            self._lib.seir_sampler_destroy(self._s)
            self._s = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- state ---------------------------------------------------------------
    def set_state(self, u, events):
        u = np.ascontiguousarray(u, dtype=np.float64)
        ev = np.ascontiguousarray(events, dtype=np.float64)
        if u.shape != (self.B, self.P) or ev.shape != (self.B, self.M, self.T, 3):
            raise ValueError(f"need u [{self.B},{self.P}] and events [{self.B},{self.M},{self.T},3]")
        _lib.check(self._lib.seir_sampler_set_state(self._s, _dptr(u), _dptr(ev)))

    def get_state(self):
        u = np.empty((self.B, self.P))
        ev = np.empty((self.B, self.M, self.T, 3))
        lp = np.empty(self.B)
        _lib.check(self._lib.seir_sampler_get_state(self._s, _dptr(u), _dptr(ev), _dptr(lp)))
        return u, ev, lp

    def log_prob(self):
        lp = np.empty(self.B)
        _lib.check(self._lib.seir_sampler_get_state(self._s, None, None, _dptr(lp)))
        return lp

    def refresh(self):
        _lib.check(self._lib.seir_sampler_refresh(self._s))

    # -- surviving a placement failure of the persistent launches (include/seir_hip.h) ----------------
    def snapshot(self, slot: int = 0):
        """Copy the chain state (everything the next sweep's draws are a function of; not the trace) to shadow slot 0 / 1,
        in stream order."""
        _lib.check(self._lib.seir_sampler_snapshot(self._s, int(slot)))
        if self._forecast_H:
            self._fc_j_snap[int(slot)] = self._fc_j

    def restore(self, slot: int = 0):
        """Back to the snapshot in `slot`; clears a hand-off time-out."""
        _lib.check(self._lib.seir_sampler_restore(self._s, int(slot)))
        if self._forecast_H and int(slot) in self._fc_j_snap:
            self._fc_j = self._fc_j_snap[int(slot)]

    def set_launch_form(self, hmc: str, moves: str):
        _lib.check(self._lib.seir_sampler_set_launch_form(self._s, HMC_MODES[hmc], MOVES_MODES[moves]))

    def launch_form(self):
        h, m = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(self._lib.seir_sampler_launch_form(self._s, ctypes.byref(h), ctypes.byref(m)))
        inv_h = {v: k for k, v in HMC_MODES.items()}
        inv_m = {v: k for k, v in MOVES_MODES.items()}
        return inv_h[h.value], inv_m[m.value]

    def _recover(self, slot: int, err: Exception):
        """A burst failed with a hand-off time-out: back to the snapshot taken at its start, one step down the ladder of
        launch forms.  Raises `err` when there is nothing further down."""
        if self._fallback_level >= len(FALLBACK_FORMS):
            raise err
        failed = self.launch_form()
        self.restore(slot)
        self._fallback_level += 1
        form = FALLBACK_FORMS[self._fallback_level - 1]
        self.set_launch_form(*form)
        self._clean_bursts = 0
        self.retry_after = min(2 * self.retry_after, 4096) if self.recoveries else self.retry_after
        self.recoveries.append(dict(failed_form=failed, rerun_form=form, error=str(err)))
        if self._log is not None:
            print(f"[seir] hand-off time-out in launch form {failed}: the burst's draws are discarded, the chain state is "
                  f"restored from the snapshot taken at its start and the burst runs again as {form}; the preferred form is "
                  f"tried again after {self.retry_after} clean bursts ({err})", file=self._log, flush=True)

    def _burst_ok(self):
        """A burst was delivered: after enough clean ones in a fall-back form, try the preferred form again."""
        if self._fallback_level == 0:
            return
        self._clean_bursts += 1
        if self._clean_bursts >= self.retry_after:
            self._fallback_level = 0
            self._clean_bursts = 0
            self.set_launch_form(*self.preferred_form)
            if self._log is not None:
                print(f"[seir] back to launch form {self.preferred_form}", file=self._log, flush=True)

    # -- kernel parameters -----------------------------------------------------
    def set_kernel(self, step_size=None, variance=None):
        ss = None if step_size is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(step_size, dtype=np.float64), (self.B,)))
        var = None if variance is None else np.ascontiguousarray(
            np.broadcast_to(np.asarray(variance, dtype=np.float64), (self.B, self.P)))
        _lib.check(self._lib.seir_sampler_set_kernel(
            self._s, None if ss is None else _dptr(ss), None if var is None else _dptr(var)))

    def get_kernel(self):
        ss, var = np.empty(self.B), np.empty((self.B, self.P))
        _lib.check(self._lib.seir_sampler_get_kernel(self._s, _dptr(ss), _dptr(var)))
        return ss, var

    def set_adaptation(self, adapt_step_size=False, adapt_mass=False, num_adaptation_steps=0,
                       target_accept_prob=0.75, running_variance=None):
        """running_variance = (count [B], mean [B,P], variance [B,P])."""
        if adapt_mass:
            cnt, mean, var = (np.ascontiguousarray(x, dtype=np.float64) for x in running_variance)
            args = (_dptr(cnt), _dptr(mean), _dptr(var))
        else:
            args = (None, None, None)
        _lib.check(self._lib.seir_sampler_set_adaptation(
            self._s, int(bool(adapt_step_size)), int(bool(adapt_mass)), int(num_adaptation_steps),
            float(target_accept_prob), *args))

    # -- sampling ---------------------------------------------------------------
    @property
    def thin(self) -> int:
        """Thinning interval: sweeps per kept draw."""
        return self._thin

    def set_thin(self, k: int):
        """Thinning interval from the next `reset_trace` on -- i.e. from the next `sample` / `sample_bursts` burst (sweeps
        already enqueued are recorded by the old rule).  `run_mcmc` keeps the warm-up windows at 1 and sets Mcmc.thin for
        the sampling bursts."""
        k = int(k)
        if k < 1:
            raise ValueError(f"thin={k}: the thinning interval is >= 1")
        _lib.check(self._lib.seir_sampler_set_thin(self._s, k))
        self._thin = k

    def reset_trace(self, at: int = 0):
        """The next sweep opens a group of `thin` sweeps whose last one is recorded in trace slot `at` (0: start of the
        burst buffer)."""
        if at:
            _lib.check(self._lib.seir_sampler_reset_trace_at(self._s, int(at)))
        else:
            _lib.check(self._lib.seir_sampler_reset_trace(self._s))

    def run(self, num_sweeps: int):
        """Enqueue sweeps (asynchronous)."""
        _lib.check(self._lib.seir_sampler_run(self._s, int(num_sweeps)))

    def _as_trace(self, n, theta, ev, hmc, mv) -> Trace:
        hmc_d = dict(is_accepted=hmc[..., 0] != 0, target_log_prob=hmc[..., 1], step_size=hmc[..., 2])
        moves = {}
        for i, key in enumerate(MOVE_KEYS):
            delta = mv[:, :, i, 2:].reshape(n, self.B, 4, _lib.MMAX)[..., :self.mmax]
            moves[key] = dict(is_accepted=mv[:, :, i, 0] != 0, target_log_prob=mv[:, :, i, 1],
                              proposed_delta=delta.astype(np.int64))
        return Trace(theta=theta, events=ev, hmc=hmc_d, moves=moves)

    def read_trace(self, count: int, first: int = 0, events: bool = True) -> Trace:
        n = int(count)
        theta = np.empty((n, self.B, self.P))
        ev = np.empty((n, self.B, self.M, self.T, 3), dtype=self.events_dtype) if (events and self.record_events) else None
        hmc = np.empty((n, self.B, 3))
        mv = np.empty((n, self.B, 4, _lib.MOVE_TRACE))
        _lib.check(self._lib.seir_sampler_read_trace(
            self._s, int(first), n, _dptr(theta),
            None if ev is None else ev.ctypes.data_as(ctypes.c_void_p), _dptr(hmc), _dptr(mv)))
        return self._as_trace(n, theta, ev, hmc, mv)

    def read_trace_async(self, count: int, first: int, into: PinnedTrace):
        """Enqueue the device->host copy of trace slots [first, first+count) behind the sweeps queued so far;
        returns at once.  `trace_wait()` then `trace_view(into, count)` give the burst."""
        n = int(count)
        if n > into.count:
            raise ValueError("pinned buffer too small")
        _lib.check(self._lib.seir_sampler_read_trace_async(
            self._s, int(first), n, _dptr(into.theta),
            None if into.events is None else into.events.ctypes.data_as(ctypes.c_void_p),
            _dptr(into.hmc), _dptr(into.moves)))

    def trace_wait(self):
        _lib.check(self._lib.seir_sampler_trace_wait(self._s))

    def trace_view(self, buf: PinnedTrace, count: int) -> Trace:
        n = int(count)
        tr = self._as_trace(n, buf.theta[:n], None if buf.events is None else buf.events[:n], buf.hmc[:n],
                            buf.moves[:n])
        if buf.marginals is not None:
            tr.marginals = {k: v[:n] for k, v in buf.marginals.items()}
        if buf.forecast is not None:
            tr.forecast = {k: v[:n] for k, v in buf.forecast.items()}
        if buf.rt is not None:
            tr.rt = buf.rt[:n]
        if getattr(buf, "check", None) is not None:
            tr.check = {k: v[:n] for k, v in buf.check.items()}
        if getattr(buf, "wb", None) is not None:
            tr.wb = {k: v[:n] for k, v in buf.wb.items()}
        if getattr(buf, "groups", None) is not None:
            tr.groups = {k: v[:n] for k, v in buf.groups.items()}
        if getattr(buf, "group_curves", None) is not None:
            tr.group_curves = {k: v[:n] for k, v in buf.group_curves.items()}
        return tr

    # -- summaries of the recorded events on the device (include/seir_hip.h) --------------------------
    def reset_summary(self):
        """Enable the summaries (first call) and zero the moment accumulators, `count` and the overflow flag, in stream
        order: the next draw folded becomes `ref`."""
        _lib.check(self._lib.seir_sampler_summary_reset(self._s))
        self._summary_on = True

    def summarize(self, first: int, count: int, accumulate: bool = True):
        """Enqueue the summary of trace slots [first, first+count) behind the sweeps that fill them: their marginals are
        written, and with `accumulate` the draws are folded into the moments."""
        _lib.check(self._lib.seir_sampler_summarize(self._s, int(first), int(count), int(bool(accumulate))))

    def _read_marginal_set(self, fn, keys, days, count, first, into=None):
        """The three per-draw marginals `keys` (by day, by location, state by day; `days` = T or H) of trace slots
        [first, first+count) through the reader `fn`: into fresh arrays (blocking `fn`), or into the pinned arrays `into`
        (asynchronous `fn`, completed by `trace_wait()`)."""
        n = int(count)
        if into is None:
            into = {k: np.empty((n, self.B, e, 3), np.int64) for k, e in zip(keys, (days, self.M, days))}
        _lib.check(fn(self._s, int(first), n, *(into[k].ctypes.data_as(_lib.c_int64_p) for k in keys)))
        return into

    def _read_moments(self, fn, days) -> Summary:
        """(count, ref, sum, sumsq) over [B,M,days,6] through the blocking reader `fn`."""
        shape = (self.B, self.M, days, len(SUMMARY_QUANTITIES))
        cnt = np.zeros(self.B, np.uint64)
        ref, sm, sq = np.empty(shape, np.int32), np.empty(shape, np.int64), np.empty(shape, np.uint64)
        _lib.check(fn(self._s, cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ref.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                      sm.ctypes.data_as(_lib.c_int64_p), sq.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return Summary(count=cnt, ref=ref, sum=sm, sumsq=sq)

    def read_marginals(self, count: int, first: int = 0) -> dict:
        """Blocking read of the marginals of trace slots [first, first+count): MARGINAL_KEYS -> int64 arrays with
        leading axes [count, B]."""
        return self._read_marginal_set(self._lib.seir_sampler_read_marginals, MARGINAL_KEYS, self.T, count, first)

    def read_marginals_async(self, count: int, first: int, into: PinnedTrace):
        """As `read_trace_async`, for the marginals; completed by `trace_wait()`."""
        if int(count) > into.count or into.marginals is None:
            raise ValueError("pinned buffer too small or without marginals")
        self._read_marginal_set(self._lib.seir_sampler_read_marginals_async, MARGINAL_KEYS, self.T, count, first, into.marginals)

    def summary(self) -> Summary:
        """The moments folded since the last `reset_summary` (blocking).  Raises `SeirError` (SEIR_ERR_STATE) if an
        accumulator overflowed."""
        return self._read_moments(self._lib.seir_sampler_read_summary, self.T)

    # -- convergence diagnostics: batch sums and marks next to the moments (include/seir_hip.h) -----------
    def reset_diagnostics(self, batch_len: int):
        """Enable the diagnostics (first call), set the batch length and do what `reset_summary` does, zeroing the batch
        sums and the marks with the moments.  From now on every draw folded into the moments is folded into the batch
        sums too."""
        if int(batch_len) < 1:
            raise ValueError(f"batch_len={batch_len}: a batch has at least one draw")
        _lib.check(self._lib.seir_sampler_diag_reset(self._s, int(batch_len)))
        self._summary_on = True
        self._diag_L = int(batch_len)

    def mark(self, which: int):
        """Copy (count, sum, sumsq) into mark 0 / 1 on the device, in stream order behind everything queued so far."""
        _lib.check(self._lib.seir_sampler_diag_mark(self._s, int(which)))

    def diagnostics(self) -> Diagnostics:
        """The moments, the batch sums and both marks (blocking): `covid19uk_amd.posterior.diagnostics.Diagnostics`, whose
        `.ess`, `.half_mean`, `.half_var` and `.rhat` apply that module's formulas.  Raises `SeirError` (SEIR_ERR_STATE)
        if an accumulator overflowed or before `reset_diagnostics`."""
        shape = (self.B, self.M, self.T, len(SUMMARY_QUANTITIES))
        u64p, i64p = ctypes.POINTER(ctypes.c_uint64), _lib.c_int64_p
        nbatch = np.zeros(self.B, np.uint64)
        bsum, bsumsq = np.empty(shape, np.int64), np.empty(shape, np.uint64)
        _lib.check(self._lib.seir_sampler_read_diag(self._s, nbatch.ctypes.data_as(u64p), bsum.ctypes.data_as(i64p),
                                                    bsumsq.ctypes.data_as(u64p)))
        mc = np.zeros((2, self.B), np.uint64)
        ms, mq = np.empty((2,) + shape, np.int64), np.empty((2,) + shape, np.uint64)
        for w in (0, 1):
            _lib.check(self._lib.seir_sampler_read_diag_mark(self._s, w, mc[w].ctypes.data_as(u64p), ms[w].ctypes.data_as(i64p),
                                                             mq[w].ctypes.data_as(u64p)))
        sm = self.summary()
        return Diagnostics(batch_length=self._diag_L, count=sm.count, ref=sm.ref, sum=sm.sum, sumsq=sm.sumsq, bsum=bsum,
                           bsumsq=bsumsq, nbatch=nbatch, mark_count=mc, mark_sum=ms, mark_sumsq=mq)

    # -- forecast of the next H days from the burst buffer (include/seir_hip.h, "Forecast on the device") ----------
    def reset_forecast(self, horizon: int, W, weekday_c, seed: int = 0):
        """Enable the forecast (first call), zero its moments, count and flag, set the horizon, the calendar of the H
        forecast days (`W`, `weekday_c`: [H], `posterior.predict.forecast_calendar`) and the seed of its Philox stream, and
        start the draw counter j at 0."""
        H = int(horizon)
        if not 1 <= H <= _lib.FORECAST_MAX_H:
            raise ValueError(f"forecast horizon {H}: 1 <= H <= {_lib.FORECAST_MAX_H}")
        W = np.ascontiguousarray(W, dtype=np.float64).reshape(-1)
        wd = np.ascontiguousarray(weekday_c, dtype=np.float64).reshape(-1)
        if W.shape != (H,) or wd.shape != (H,):
            raise ValueError(f"need W [{H}] and weekday_c [{H}]")
        _lib.check(self._lib.seir_sampler_forecast_reset(self._s, H, _dptr(W), _dptr(wd), int(seed) & (2 ** 64 - 1)))
        self._forecast_H, self._fc_j, self._fc_j_snap = H, 0, {}

    def forecast(self, first: int, count: int, steps=None):
        """Enqueue the forecast of trace slots [first, first+count) behind the sweeps that fill them and fold it.  `steps`
        [count,B,H] (optional): random-walk steps of the log baseline; None holds the baseline at its last value."""
        n = int(count)
        if steps is not None:
            steps = np.ascontiguousarray(steps, dtype=np.float64)
            if steps.shape != (n, self.B, self._forecast_H):
                raise ValueError(f"need steps [{n},{self.B},{self._forecast_H}]")
        _lib.check(self._lib.seir_sampler_forecast(self._s, int(first), n, None if steps is None else _dptr(steps)))
        self._fc_j += n

    def read_forecast_marginals(self, count: int, first: int = 0) -> dict:
        """Blocking read of the forecast marginals of trace slots [first, first+count): FORECAST_KEYS -> int64 arrays with
        leading axes [count, B]."""
        return self._read_marginal_set(self._lib.seir_sampler_read_forecast_marginals, FORECAST_KEYS, self._forecast_H, count, first)

    def read_forecast_marginals_async(self, count: int, first: int, into: PinnedTrace):
        """As `read_marginals_async`, for the forecast marginals; completed by `trace_wait()`."""
        if int(count) > into.count or into.forecast is None:
            raise ValueError("pinned buffer too small or without forecast arrays")
        self._read_marginal_set(self._lib.seir_sampler_read_forecast_marginals_async, FORECAST_KEYS, self._forecast_H, count,
                                first, into.forecast)

    def forecast_summary(self) -> Summary:
        """The forecast moments folded since the last `reset_forecast` (blocking): a `Summary` whose day axis is the H
        forecast days, [B,M,H,6].  Raises `SeirError` (SEIR_ERR_STATE) if an accumulator overflowed or before a reset."""
        return self._read_moments(self._lib.seir_sampler_read_forecast, self._forecast_H)

    # -- forecast intervals: the draw store and exact order statistics (include/seir_hip.h, "Forecast intervals") ----
    def keep_forecast_draws(self, cap: int):
        """Keep cases, cumulative cases and prevalence of every forecast draw on the device, for up to `cap` draws per
        chain: between `reset_forecast` and the first `forecast`.  0 frees the store.  B x 3 x M x H x cap x 4 bytes; the
        library refuses a store above half of the device's free memory."""
        cap = int(cap)
        if cap < 0:
            raise ValueError(f"cap={cap}: the number of draws per chain to keep")
        _lib.check(self._lib.seir_sampler_forecast_keep(self._s, cap))

    def forecast_order_stats(self, ranks, pooled: bool = False) -> np.ndarray:
        """Exact order statistics `ranks` (strictly increasing, at most 16) of every cell over the draws kept since the
        reset (blocking): int32 [R, B, 3, M, H] -- planes `FORECAST_QUANTILE_PLANES` -- or, `pooled`, [R, 3, M, H] over the
        B x count values of all chains of this sampler.  Equal to np.sort(draws, axis=0)[ranks]."""
        ranks = np.ascontiguousarray(ranks, dtype=np.int64).reshape(-1)
        shape = (len(ranks),) + (() if pooled else (self.B,)) + (3, self.M, self._forecast_H)
        out = np.empty(shape, np.int32)
        _lib.check(self._lib.seir_sampler_forecast_order_stats(self._s, ranks.ctypes.data_as(_lib.c_int64_p), len(ranks),
                                                               1 if pooled else 0,
                                                               out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return out

    def forecast_quantiles(self, probs, pooled: bool = False) -> np.ndarray:
        """Quantiles `probs` (NumPy's default rule, `posterior.quantiles`) of every cell over the draws kept since the
        reset (blocking): float64 [K, B, 3, M, H], or [K, 3, M, H] when `pooled`."""
        from .posterior import quantiles as Q
        n = self._fc_j * (self.B if pooled else 1)
        ranks = Q.quantile_ranks(n, probs)
        return Q.interpolate(self.forecast_order_stats(ranks, pooled=pooled), ranks, n, probs)

    def _forecast_burst(self, first, count, forecast):
        """`forecast` of sample / sample_bursts: True (held baseline) or a callable (j0, count) -> steps [count,B,H], j0
        being the number of draws per chain forecast since the reset -- after a re-run of a burst it is the same again."""
        if not self._forecast_H:
            raise ValueError("forecast asked for before reset_forecast")
        self.forecast(first, count, forecast(self._fc_j, count) if callable(forecast) else None)

    # -- reproduction number of the kept draws (include/seir_hip.h, "Reproduction number on the device") ----------
    def reset_rt(self, days: int, weight):
        """Enable the reproduction number (first call), zero its accumulators and count, set the window to the last `days`
        days of the series (1 <= days <= T) and the national weights `weight` [M] (N / N.sum(), as the reference)."""
        D = int(days)
        if not 1 <= D <= self.T:
            raise ValueError(f"rt days {D}: 1 <= D <= T = {self.T}")
        w = np.ascontiguousarray(weight, dtype=np.float64).reshape(-1)
        if w.shape != (self.M,):
            raise ValueError(f"need weight [{self.M}]")
        try:
            _lib.check(self._lib.seir_sampler_rt_reset(self._s, D, _dptr(w)))
        except _lib.SeirError as e:
            if self._group_rt_on and "group curves" in str(e):   # the reset is done; the group outputs were refused
                self._rt_D, self._group_rt_refused = D, True
            raise
        self._rt_D, self._group_rt_refused = D, False

    def rt(self, first: int, count: int):
        """Enqueue R_it of trace slots [first, first+count) behind the sweeps that fill them: folded into the moments,
        and the national curve of every draw written."""
        _lib.check(self._lib.seir_sampler_rt(self._s, int(first), int(count)))

    def read_rt_draws(self, count: int, first: int = 0) -> np.ndarray:
        """Blocking read of R_t [count,B,D] of trace slots [first, first+count)."""
        out = np.empty((int(count), self.B, self._rt_D))
        _lib.check(self._lib.seir_sampler_read_rt_draws(self._s, int(first), int(count), _dptr(out)))
        return out

    def read_rt_draws_async(self, count: int, first: int, into: PinnedTrace):
        """As `read_marginals_async`, for the national curves; completed by `trace_wait()`."""
        if int(count) > into.count or into.rt is None:
            raise ValueError("pinned buffer too small or without R_t")
        _lib.check(self._lib.seir_sampler_read_rt_draws_async(self._s, int(first), int(count), _dptr(into.rt)))

    def rt_summary(self) -> RtSummary:
        """The R_it accumulators folded since the last `reset_rt` (blocking): `RtSummary`, whose `.mean`, `.var` and
        `.prob_gt1` are formed here.  Raises `SeirError` (SEIR_ERR_STATE) before a reset."""
        shape = (self.B, self._rt_D, self.M)
        cnt = np.zeros(self.B, np.uint64)
        ref, sm, sq, g1 = np.empty(shape), np.empty(shape), np.empty(shape), np.empty(shape, np.uint32)
        _lib.check(self._lib.seir_sampler_read_rt(self._s, cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), _dptr(ref),
                                                  _dptr(sm), _dptr(sq), g1.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
        return RtSummary(count=cnt, ref=ref, sum=sm, sumsq=sq, gt1=g1)

    # -- R_t intervals: the R_it draw store and exact order statistics (include/seir_hip.h, "R_t intervals") ----------
    def keep_rt_draws(self, cap: int):
        """Keep R_it of every draw that `rt` folds on the device, for up to `cap` draws per chain: between `reset_rt` and
        the first `rt`.  0 frees the store.  B x D x M x cap x 8 bytes; the library refuses a store above half of the
        device's free memory."""
        cap = int(cap)
        if cap < 0:
            raise ValueError(f"cap={cap}: the number of draws per chain to keep")
        _lib.check(self._lib.seir_sampler_rt_keep(self._s, cap))

    def rt_order_stats(self, ranks, pooled: bool = False) -> np.ndarray:
        """Exact order statistics `ranks` (strictly increasing, at most 16) of every cell's R_it over the draws kept since
        the reset (blocking): float64 [R, B, D, M] or, `pooled`, [R, D, M] over the B x count values of all chains of this
        sampler.  Equal to np.sort(draws, axis=0)[ranks], bit for bit."""
        ranks = np.ascontiguousarray(ranks, dtype=np.int64).reshape(-1)
        out = np.empty((len(ranks),) + (() if pooled else (self.B,)) + (self._rt_D, self.M))
        _lib.check(self._lib.seir_sampler_rt_order_stats(self._s, ranks.ctypes.data_as(_lib.c_int64_p), len(ranks),
                                                         1 if pooled else 0, _dptr(out)))
        return out

    def rt_quantiles(self, probs, pooled: bool = False) -> np.ndarray:
        """Quantiles `probs` (NumPy's default rule, `posterior.quantiles`) of every cell's R_it over the draws kept since
        the reset (blocking): float64 [K, B, D, M], or [K, D, M] when `pooled`."""
        from .posterior import quantiles as Q
        cnt = np.zeros(self.B, np.uint64)
        _lib.check(self._lib.seir_sampler_read_rt(self._s, cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), None, None,
                                                  None, None))
        n = int(cnt[0]) * (self.B if pooled else 1)         # the library refuses chains whose counts differ
        ranks = Q.quantile_ranks(n, probs)
        return Q.interpolate(self.rt_order_stats(ranks, pooled=pooled), ranks, n, probs)

    def _rt_burst(self, first, count):
        if not self._rt_D:
            raise ValueError("rt asked for before reset_rt")
        self.rt(first, count)

    # -- in-sample check of the last K days (include/seir_hip.h, "In-sample predictive check on the device") ----------
    def reset_check(self, days: int, W, weekday_c, seed: int = 0):
        """Enable the check (first call), zero its moments, comparison counts, observed counts and flags, set the window
        to the last `days` days (1 <= days <= min(T, 128)), its calendar (`W`, `weekday_c`: [days],
        `posterior.predict.check_calendar`) and the seed of its Philox stream, and start its draw counter at 0."""
        K = int(days)
        if not 1 <= K <= min(self.T, _lib.CHECK_MAX_DAYS):
            raise ValueError(f"check days {K}: 1 <= K <= min(T = {self.T}, {_lib.CHECK_MAX_DAYS})")
        W = np.ascontiguousarray(W, dtype=np.float64).reshape(-1)
        wd = np.ascontiguousarray(weekday_c, dtype=np.float64).reshape(-1)
        if W.shape != (K,) or wd.shape != (K,):
            raise ValueError(f"need W [{K}] and weekday_c [{K}]")
        _lib.check(self._lib.seir_sampler_check_reset(self._s, K, _dptr(W), _dptr(wd), int(seed) & (2 ** 64 - 1)))
        self._check_K = K

    def check(self, first: int, count: int):
        """Enqueue the check of trace slots [first, first+count) behind the sweeps that fill them: the window is simulated
        again from every draw, folded, and counted against the draw's recorded removals."""
        _lib.check(self._lib.seir_sampler_check(self._s, int(first), int(count)))

    def read_check_marginals(self, count: int, first: int = 0) -> dict:
        """Blocking read of the check's marginals of trace slots [first, first+count): CHECK_KEYS -> int64 arrays with
        leading axes [count, B]."""
        return self._read_marginal_set(self._lib.seir_sampler_read_check_marginals, CHECK_KEYS, self._check_K, count, first)

    def read_check_marginals_async(self, count: int, first: int, into: PinnedTrace):
        """As `read_marginals_async`, for the check's marginals; completed by `trace_wait()`."""
        if int(count) > into.count or into.check is None:
            raise ValueError("pinned buffer too small or without check arrays")
        self._read_marginal_set(self._lib.seir_sampler_read_check_marginals_async, CHECK_KEYS, self._check_K, count, first,
                                into.check)

    def check_summary(self) -> CheckSummary:
        """Moments and comparison counts folded since the last `reset_check` (blocking).  Raises `SeirError`
        (SEIR_ERR_STATE) if an accumulator overflowed, if the observed removals differed between draws, or before a reset."""
        B, M, K = self.B, self.M, self._check_K
        u32 = ctypes.POINTER(ctypes.c_uint32)
        obs = np.empty((B, M, K), np.int32)
        shapes = ((B, M, K), (B, M, K), (B, M), (B, M), (B, K), (B, K), (B,), (B,))
        arrs = [np.empty(sh, np.uint32) for sh in shapes]
        _lib.check(self._lib.seir_sampler_read_check_counts(self._s, obs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                            *(a.ctypes.data_as(u32) for a in arrs)))
        mom = self._read_moments(self._lib.seir_sampler_read_check, K)
        return CheckSummary(mom, obs, *arrs)

    def _check_burst(self, first, count):
        if not self._check_K:
            raise ValueError("check asked for before reset_check")
        self.check(first, count)

    # -- within/between pressure shares (include/seir_hip.h, "Within/between pressure shares on the device") ----------
    def reset_within_between(self, days: int):
        """Enable the within/between shares (first call), zero their accumulators and count and set the window to the last
        `days` days of the series (1 <= days <= T)."""
        D = int(days)
        if not 1 <= D <= self.T:
            raise ValueError(f"within_between days {D}: 1 <= D <= T = {self.T}")
        try:
            _lib.check(self._lib.seir_sampler_wb_reset(self._s, D))
        except _lib.SeirError as e:
            if self._group_wb_on and "group curves" in str(e):   # the reset is done; the group outputs were refused
                self._wb_D, self._group_wb_refused = D, True
            raise
        self._wb_D, self._group_wb_refused = D, False

    def within_between(self, first: int, count: int):
        """Enqueue the shares of trace slots [first, first+count) behind the sweeps that fill them: folded into the
        accumulators, and the national pressures of every draw written."""
        _lib.check(self._lib.seir_sampler_wb(self._s, int(first), int(count)))

    def read_wb_draws(self, count: int, first: int = 0) -> dict:
        """Blocking read of the national pressures of trace slots [first, first+count): WB_KEYS -> [count,B,D]."""
        out = {k: np.empty((int(count), self.B, self._wb_D)) for k in WB_KEYS}
        _lib.check(self._lib.seir_sampler_read_wb_draws(self._s, int(first), int(count), *(_dptr(out[k]) for k in WB_KEYS)))
        return out

    def read_wb_draws_async(self, count: int, first: int, into: PinnedTrace):
        """As `read_marginals_async`, for the national pressures; completed by `trace_wait()`."""
        if int(count) > into.count or getattr(into, "wb", None) is None:
            raise ValueError("pinned buffer too small or without within/between arrays")
        _lib.check(self._lib.seir_sampler_read_wb_draws_async(self._s, int(first), int(count),
                                                              *(_dptr(into.wb[k]) for k in WB_KEYS)))

    def within_between_summary(self) -> WbSummary:
        """The accumulators folded since the last `reset_within_between` (blocking): `WbSummary`, whose `.within_mean`,
        `.within_var`, `.between_mean` and `.p_within_gt_between` are formed here.  Raises `SeirError` (SEIR_ERR_STATE)
        before a reset."""
        shape = (self.B, self._wb_D, self.M)
        u32 = ctypes.POINTER(ctypes.c_uint32)
        cnt = np.zeros(self.B, np.uint64)
        n, gt = np.empty(shape, np.uint32), np.empty(shape, np.uint32)
        ref_w, sum_w, sumsq_w, ref_b, sum_b = (np.empty(shape) for _ in range(5))
        _lib.check(self._lib.seir_sampler_read_wb(self._s, cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                                  n.ctypes.data_as(u32), _dptr(ref_w), _dptr(sum_w), _dptr(sumsq_w),
                                                  _dptr(ref_b), _dptr(sum_b), gt.ctypes.data_as(u32)))
        return WbSummary(count=cnt, defined=n, ref_w=ref_w, sum_w=sum_w, sumsq_w=sumsq_w, ref_b=ref_b, sum_b=sum_b, gt=gt)

    def _wb_burst(self, first, count):
        if not self._wb_D:
            raise ValueError("within_between asked for before reset_within_between")
        self.within_between(first, count)

    # -- region totals: per-draw sums over groups of locations (include/seir_hip.h, "Region totals on the device") ------
    def set_groups(self, offsets, members):
        """Set the table of groups (CSR: `offsets` [G+1], `members` [nnz], ascending and unique within a group;
        `posterior.groups.parse_groups`), or free it with `set_groups(None, None)`.  While a table is set, `summarize`,
        `forecast` and `check` also form every kept draw's sums over each group's members (`read_group_marginals`)."""
        i32p = ctypes.POINTER(ctypes.c_int32)
        if offsets is None:
            _lib.check(self._lib.seir_sampler_groups_set(self._s, 0, None, None))
            self._groups_G = self._groups_nnz = 0
            self._group_rt_on = self._group_wb_on = False
            return
        off = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
        mem = np.ascontiguousarray(members, dtype=np.int32).reshape(-1)
        G = off.size - 1
        if G < 1 or mem.size < int(off.max()):              # what the library cannot check: it reads members up to the offsets
            raise ValueError(f"offsets [{off.size}] reach {int(off.max()) if off.size else 0}, members holds {mem.size}: not a "
                             "CSR pair of at least one group")
        if G > _lib.GROUPS_MAX:
            raise ValueError(f"G={G}: at most {_lib.GROUPS_MAX} groups")
        try:
            _lib.check(self._lib.seir_sampler_groups_set(self._s, G, off.ctypes.data_as(i32p), mem.ctypes.data_as(i32p)))
        except _lib.SeirError as e:
            if "group curves" not in str(e):
                raise
            # the table is in force; group within / between could not be sized for it
            self._groups_G, self._groups_nnz, self._group_rt_on, self._group_wb_refused = G, int(off[G]), False, True
            raise
        self._groups_G, self._groups_nnz = G, int(off[G])
        self._group_rt_on = False                           # its weights belonged to the old table
        self._group_wb_refused = False

    # -- group curves: R_t and within / between per group (include/seir_hip.h, "Group curves on the device") ------------
    def set_group_rt(self, weights):
        """Group R_t on: while a table is set and `rt` runs, every draw it folds also leaves, per group and window day, the
        sum over the members of weights[k] * R_it (`weights` [nnz] float64 aligned with the table's `members`; for a
        population-weighted curve N[members] / the group's population) in the fixed order of
        `posterior.groups.weighted_sum_rows`.  None switches it off.  A later `set_groups` switches it off too."""
        if weights is None:
            _lib.check(self._lib.seir_sampler_group_rt(self._s, None))
            self._group_rt_on = False
            return
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if self._groups_G and w.size != self._groups_nnz:
            raise ValueError(f"need weights [{self._groups_nnz}], aligned with the table's members")
        try:
            _lib.check(self._lib.seir_sampler_group_rt(self._s, _dptr(w)))   # SEIR_ERR_STATE without a table
        except _lib.SeirError as e:
            if "group curves" in str(e):                    # outputs refused: the switch is off; any other refusal left it alone
                self._group_rt_on = False
            raise
        self._group_rt_on, self._group_rt_refused = True, False

    def set_group_within_between(self, on: bool):
        """Group within / between on or off: while a table is set and `within_between` runs, every draw it folds also
        leaves the members' sums of the within and the between pressure per group and window day ("between": from outside
        each member location, as in the national figure)."""
        try:
            _lib.check(self._lib.seir_sampler_group_wb(self._s, 1 if on else 0))
        except _lib.SeirError as e:
            if "group curves" in str(e):                    # outputs refused: the switch is off; any other refusal left it alone
                self._group_wb_on = False
            raise
        self._group_wb_on, self._group_wb_refused = bool(on), False

    def _group_curve_days(self, do_rt, do_wb):
        """{key of GROUP_CURVE_KEYS: window days} of the curves that leave outputs with a burst that runs rt / within_between."""
        days = {}
        if do_rt and self._group_rt_on and self._groups_G and not self._group_rt_refused:
            days["rt_by_group"] = self._rt_D
        if do_wb and self._group_wb_on and self._groups_G and not self._group_wb_refused:
            days["within_by_group"] = days["between_by_group"] = self._wb_D
        return days

    def read_group_rt(self, count: int, first: int = 0) -> np.ndarray:
        """Blocking read of the group R_t of trace slots [first, first+count): float64 [count,B,G,D]."""
        out = np.empty((int(count), self.B, self._groups_G, self._rt_D))
        _lib.check(self._lib.seir_sampler_read_group_rt(self._s, int(first), int(count), _dptr(out)))
        return out

    def read_group_wb(self, count: int, first: int = 0) -> dict:
        """Blocking read of the group pressures of trace slots [first, first+count): within_by_group, between_by_group
        -> float64 [count,B,G,D]."""
        out = {k: np.empty((int(count), self.B, self._groups_G, self._wb_D)) for k in GROUP_CURVE_KEYS[1:]}
        _lib.check(self._lib.seir_sampler_read_group_wb(self._s, int(first), int(count), *(_dptr(out[k]) for k in GROUP_CURVE_KEYS[1:])))
        return out

    def _read_group_curves(self, days, count, first=0, into=None):
        """The curves of `_group_curve_days` of slots [first, first+count): blocking into new arrays, or on the copy stream
        `into` the arrays of a PinnedTrace (completed by `trace_wait()`)."""
        if into is None:
            out = {}
            if "rt_by_group" in days:
                out["rt_by_group"] = self.read_group_rt(count, first)
            if "within_by_group" in days:
                out.update(self.read_group_wb(count, first))
            return out
        if int(count) > into.count or getattr(into, "group_curves", None) is None or any(k not in into.group_curves for k in days):
            raise ValueError("pinned buffer too small or without group curves")
        g = into.group_curves
        if "rt_by_group" in days:
            _lib.check(self._lib.seir_sampler_read_group_rt_async(self._s, int(first), int(count), _dptr(g["rt_by_group"])))
        if "within_by_group" in days:
            _lib.check(self._lib.seir_sampler_read_group_wb_async(self._s, int(first), int(count), _dptr(g["within_by_group"]),
                                                                  _dptr(g["between_by_group"])))
        return g

    def _group_len(self, source):
        return {"trace": self.T if self._summary_on else 0, "forecast": self._forecast_H, "check": self._check_K}[source]

    def _read_groups(self, fn, source, count, first, into=None):
        which, ev_key, st_key = GROUP_SOURCES[source]
        n, G = int(count), self._groups_G
        if into is None:
            into = {ev_key: np.empty((n, self.B, G, self._group_len(source), 3), np.int64)}
            if st_key:
                into[st_key] = np.empty((n, self.B, G, 3), np.int64)
        _lib.check(fn(self._s, which, int(first), n, into[ev_key].ctypes.data_as(_lib.c_int64_p),
                      into[st_key].ctypes.data_as(_lib.c_int64_p) if st_key else None))
        return into

    def read_group_marginals(self, source: str, count: int, first: int = 0) -> dict:
        """Blocking read of the group sums of trace slots [first, first+count) of `source` ("trace", "forecast", "check"):
        its keys of `GROUP_SOURCES` -> int64 [count,B,G,L,3] (L = T, H, K) and, for the forecast and the check, the
        members' sum of S, E, I at the window's start [count,B,G,3]."""
        return self._read_groups(self._lib.seir_sampler_read_group_marginals, source, count, first)

    def read_group_marginals_async(self, source: str, count: int, first: int, into: PinnedTrace):
        """As `read_marginals_async`, for the group sums of `source`; completed by `trace_wait()`."""
        if int(count) > into.count or getattr(into, "groups", None) is None or GROUP_SOURCES[source][1] not in into.groups:
            raise ValueError("pinned buffer too small or without group arrays")
        self._read_groups(self._lib.seir_sampler_read_group_marginals_async, source, count, first, into.groups)

    def _group_sources(self, groups, do_sum, do_fc, do_ck):
        """`groups` of sample / sample_bursts: the sources whose group sums cross with the trace -- True: every one of
        "trace", "forecast", "check" that runs with the burst; or a tuple of those names, each of which must run."""
        if not groups:
            return ()
        if not self._groups_G:
            raise ValueError("groups asked for before set_groups")
        on = dict(trace=do_sum, forecast=do_fc, check=do_ck)
        if groups is True:
            src = tuple(k for k in GROUP_SOURCES if on[k])
        else:
            src = tuple(groups)
            bad = [k for k in src if not on.get(k)]
            if bad:
                raise ValueError(f"groups={groups!r}: {bad[0]!r} is not one of summarize, forecast, check run with this burst")
        if not src:
            raise ValueError("groups needs one of summarize, forecast, check")
        return src

    def _summarize_mode(self, summarize):
        """`summarize` of sample / sample_bursts: False, True (marginals + moments) or "marginals" (accumulate = 0)."""
        if summarize not in (False, True, "marginals"):
            raise ValueError(f"summarize={summarize!r}: False, True or 'marginals'")
        if summarize and not self._summary_on:
            self.reset_summary()
        return bool(summarize), summarize is True

    def sample_bursts(self, num_bursts: int, burst: int, consume, events: bool = True, summarize=False, marks=None,
                      forecast=False, rt=False, check=False, within_between=False, groups=False):
        """`num_bursts` x `burst` kept draws (`burst * thin` sweeps each) with the burst buffer used as two halves:
        while burst k+1 runs on the device, burst k crosses PCIe into page-locked memory on a copy stream and `consume(trace, k)`
        (e.g. the HDF5 writer) runs on a worker thread -- the sampler only waits when the consumer is
        the slower side.  Needs trace_capacity >= 2 * burst.  The trace handed to `consume` is a view of a
        pinned buffer that is re-used two bursts later: copy what must outlive the call.

        `summarize` (True, or "marginals" for the marginals without folding the draws into the moments): every burst is
        summarised on the device right behind its sweeps (snapshot -> reset_trace -> run -> summarize, in stream order) and
        its marginals cross with the trace (`trace.marginals`); with `events=False` the event tensors never leave the
        device.  A burst that is run again after a hand-off time-out is not counted twice: the snapshot taken at its start
        holds the accumulators.

        `marks` ({burst index: 0 | 1}, with the diagnostics on): `mark(which)` is enqueued right behind the summary of that
        burst, so the mark holds the accumulators over bursts 0 .. index.  A burst that is run again is marked again: the
        restored snapshot holds the marks as they were before it.

        `forecast` (True, or a callable giving random-walk steps, see `_forecast_burst`; needs `reset_forecast`): every
        burst's draws are forecast on the device right behind its summary and the forecast marginals cross with the trace
        (`trace.forecast`).

        `rt` (needs `reset_rt`): R_it of every burst's draws is formed and folded on the device right behind its summary
        and forecast, and the national curves cross with the trace (`trace.rt`).

        `check` (needs `reset_check`): the last K days of every burst's draws are simulated again and set against the data
        on the device, behind the summary, the forecast and R_t; the check's marginals cross with the trace
        (`trace.check`).

        `within_between` (needs `reset_within_between`): the within/between pressure shares of every burst's draws are
        formed and folded on the device, behind the summary, the forecast, R_t and the check; the national pressures cross
        with the trace (`trace.wb`).

        `groups` (True, or a tuple of "trace", "forecast", "check"; needs `set_groups` and the matching `summarize`,
        `forecast`, `check`): the group sums that the summary, the forecast and the check of every burst form while a table
        is set cross with the trace (`trace.groups`), all of them or the named ones.

        The group curves have no keyword: while `set_group_rt` / `set_group_within_between` is on, the curves that `rt` /
        `within_between` leave per group cross with the trace (`trace.group_curves`)."""
        from concurrent.futures import ThreadPoolExecutor
        do_sum, accumulate = self._summarize_mode(summarize)
        burst, num_bursts = int(burst), int(num_bursts)
        if 2 * burst > self.cap:
            raise ValueError(f"sample_bursts needs trace_capacity >= 2 * burst = {2 * burst}, have {self.cap}")
        # page-locking GBs of host memory takes tenths of a second: the two buffers are kept for the next call
        do_fc = bool(forecast)
        do_rt = bool(rt)
        do_ck = bool(check)
        do_wb = bool(within_between)
        grp_src = self._group_sources(groups, do_sum, do_fc, do_ck)
        grp_lens = {k: self._group_len(k) for k in grp_src}
        gc_days = self._group_curve_days(do_rt, do_wb)
        key = (burst, bool(events), do_sum, self._forecast_H if do_fc else 0) + ((self._rt_D,) if do_rt else ()) + \
            ((("check", self._check_K),) if do_ck else ()) + ((("wb", self._wb_D),) if do_wb else ()) + \
            ((("groups", self._groups_G, tuple(grp_lens.items())),) if grp_src else ()) + \
            ((("group_curves", self._groups_G, tuple(gc_days.items())),) if gc_days else ())
        if getattr(self, "_pinned_key", None) != key:
            for bf in getattr(self, "_pinned", []):
                bf.close()
            mk = dict(marginals=True) if do_sum else {}
            if do_fc:
                mk["forecast"] = self._forecast_H
            if do_rt:
                mk["rt"] = self._rt_D
            if do_ck:
                mk["check"] = self._check_K
            if do_wb:
                mk["wb"] = self._wb_D
            if grp_src:
                mk["groups"] = (self._groups_G, grp_lens)
            if gc_days:
                mk["group_curves"] = (self._groups_G, gc_days)
            self._pinned = [PinnedTrace(self, burst, events, **mk), PinnedTrace(self, burst, events, **mk)]
            self._pinned_key = key
        bufs = self._pinned
        futs = [None, None]
        # i: next burst to enqueue; prev: the burst whose copy is in flight (-1: none).  A hand-off time-out surfaces at
        # trace_wait (or at the next call after it): the oldest burst not yet handed to `consume` is then run again from
        # the snapshot taken at its start, in the next launch form down the ladder (_recover) -- and so is everything
        # enqueued after it, which ran from a state that cannot be trusted.
        i, prev, retried = 0, -1, -1
        try:
            with ThreadPoolExecutor(max_workers=1) as pool:
                while i < num_bursts or prev >= 0:
                    try:
                        h = i & 1
                        if i < num_bursts:
                            if futs[h] is not None:
                                futs[h].result()                 # the consumer is done with host buffer h
                                futs[h] = None
                            if self.auto_recover:
                                self.snapshot(h)                 # stream order: the state burst i starts from
                            self.reset_trace(at=h * burst)
                            self.run(burst * self._thin)         # asynchronous; a re-run after _recover passes here again
                            if do_sum:
                                self.summarize(h * burst, burst, accumulate)
                            if marks and i in marks:
                                self.mark(marks[i])
                            if do_fc:
                                self._forecast_burst(h * burst, burst, forecast)
                            if do_rt:
                                self._rt_burst(h * burst, burst)
                            if do_ck:
                                self._check_burst(h * burst, burst)
                            if do_wb:
                                self._wb_burst(h * burst, burst)
                        if prev >= 0:
                            self.trace_wait()                    # burst prev has landed (it crossed while burst i ran)
                            futs[prev & 1] = pool.submit(consume, self.trace_view(bufs[prev & 1], burst), prev)
                            prev = -1
                            self._burst_ok()
                        if i < num_bursts:
                            self.read_trace_async(burst, h * burst, bufs[h])
                            if do_sum:
                                self.read_marginals_async(burst, h * burst, bufs[h])
                            if do_fc:
                                self.read_forecast_marginals_async(burst, h * burst, bufs[h])
                            if do_rt:
                                self.read_rt_draws_async(burst, h * burst, bufs[h])
                            if do_ck:
                                self.read_check_marginals_async(burst, h * burst, bufs[h])
                            if do_wb:
                                self.read_wb_draws_async(burst, h * burst, bufs[h])
                            for src in grp_src:
                                self.read_group_marginals_async(src, burst, h * burst, bufs[h])
                            if gc_days:
                                self._read_group_curves(gc_days, burst, h * burst, bufs[h])
                            prev = i
                            i += 1
                    except _lib.HandoffTimeout as e:
                        bad = prev if prev >= 0 else i
                        if not self.auto_recover or bad >= num_bursts:
                            raise
                        if bad == retried and self._fallback_level >= len(FALLBACK_FORMS):
                            raise
                        retried = bad
                        self._recover(bad & 1, e)
                        i, prev = bad, -1
                for f in futs:
                    if f is not None:
                        f.result()
        finally:
            try:
                self.trace_wait()
            except _lib.HandoffTimeout:
                pass

    def sample(self, num_sweeps: int, events: bool = True, summarize=False, forecast=False, rt=False, check=False,
               within_between=False, groups=False) -> Trace:
        """reset_trace + run + read: the analogue of one `sample_chain` call with `num_sweeps` results, each the last of
        `thin` sweeps.  `summarize` as in `sample_bursts`: the burst is summarised on the device and `trace.marginals`
        filled; `forecast` likewise (`trace.forecast`), `rt` (`trace.rt`), `check` (`trace.check`), `within_between` (`trace.wb`)
        and `groups` (`trace.groups`); the group curves that are on (`set_group_rt`, `set_group_within_between`) ride on
        `rt` / `within_between` (`trace.group_curves`)."""
        do_sum, accumulate = self._summarize_mode(summarize)
        grp_src = self._group_sources(groups, do_sum, bool(forecast), bool(check))
        gc_days = self._group_curve_days(bool(rt), bool(within_between))
        if num_sweeps > self.cap:
            raise ValueError(f"num_sweeps={num_sweeps} exceeds trace_capacity={self.cap}")
        while True:
            if self.auto_recover:
                self.snapshot(0)
            self.reset_trace()
            self.run(num_sweeps * self._thin)
            try:
                if do_sum:
                    self.summarize(0, num_sweeps, accumulate)
                if forecast:
                    self._forecast_burst(0, num_sweeps, forecast)
                if rt:
                    self._rt_burst(0, num_sweeps)
                if check:
                    self._check_burst(0, num_sweeps)
                if within_between:
                    self._wb_burst(0, num_sweeps)
                tr = self.read_trace(num_sweeps, events=events)
                if do_sum:
                    tr.marginals = self.read_marginals(num_sweeps)
                if forecast:
                    tr.forecast = self.read_forecast_marginals(num_sweeps)
                if rt:
                    tr.rt = self.read_rt_draws(num_sweeps)
                if check:
                    tr.check = self.read_check_marginals(num_sweeps)
                if within_between:
                    tr.wb = self.read_wb_draws(num_sweeps)
                if grp_src:
                    tr.groups = {}
                    for src in grp_src:
                        tr.groups.update(self.read_group_marginals(src, num_sweeps))
                if gc_days:
                    tr.group_curves = self._read_group_curves(gc_days, num_sweeps)
            except _lib.HandoffTimeout as e:
                if not self.auto_recover:
                    raise
                self._recover(0, e)          # raises e again when no launch form is left to fall back on
                continue
            self._burst_ok()
            return tr

    def xcd_local(self) -> bool:
        """True if workgroups with ids congruent mod 8 share an XCD on this GPU (probed at creation): the condition for
        the chunk roles of an HMC step to run inside the gradient launch (hmc="chunk") and the band workgroups inside
        the pair launch (moves="paired")."""
        return bool(self._lib.seir_sampler_xcd_local(self._s))

    def pair_timeouts(self) -> np.ndarray:
        """Per chain: k_move_pair launches whose authoritative workgroup gave up on the speculative one."""
        out = np.zeros(self.B, dtype=np.uint32)
        _lib.check(self._lib.seir_sampler_pair_timeouts(self._s, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
        return out

    def time_leapfrog(self, sweeps: int = 50):
        """(mean ms, launches, gradient evaluations) of the inner leapfrog steps of a sweep -- HIP events around that
        section of `sweeps` ordinary sweeps, on the stream the kernels run on (seir_sampler_time_leapfrog)."""
        ms_, nl, ne = ctypes.c_float(), ctypes.c_int32(), ctypes.c_int32()
        _lib.check(self._lib.seir_sampler_time_leapfrog(self._s, int(sweeps), ctypes.byref(ms_), ctypes.byref(nl), ctypes.byref(ne)))
        return float(ms_.value), int(nl.value), int(ne.value)

    def time_grad_kernel(self, iters: int = 100) -> float:
        """Mean duration (ms) of the sweep's gradient kernel, HIP events on the context stream."""
        ms_ = ctypes.c_float()
        _lib.check(self._lib.seir_sampler_time_grad_kernel(self._s, int(iters), ctypes.byref(ms_)))
        return float(ms_.value)

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

import collections
import ctypes
import dataclasses
import sys
import typing

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


# What is on, how it is sized and how far it has counted: `seir_product_state` member for member (include/seir_hip.h says what
# each one is), as `ChainSampler._state()` reads it from the library, which owns it.  The defaults: nothing is on.
_STATE_KEYS = tuple(k for k, _ in _lib.SeirProductState._fields_ if k != "reserved")
ProductState = collections.namedtuple("ProductState", _STATE_KEYS,
                                      defaults=[(0, 0, 0) if k == "group_L" else 0 for k in _STATE_KEYS])


class BurstProduct(typing.NamedTuple):
    """A device product that rides on a burst of kept draws: one row of `BURST_PRODUCTS`."""
    field: str          # the Trace / PinnedTrace field it fills; PinnedTrace's keyword has the same name
    request: str        # the keyword of sample / sample_bursts that asks for it; None: the sampler's own switches decide
    size: object        # (sampler, request, {field: size} of the rows above) -> the value that sizes its arrays, falsy when
    #                     it is off; ValueError when it is asked for before its reset
    arrays: object      # (sampler, size) -> {key: (trailing shape, dtype)} behind the leading [count, B]; one pair for rt
    enqueue: str        # the method (first, count, *args) that enqueues it behind the sweeps; None: it rides on rows above
    read: str           # the blocking reader (count) -> arrays; for a row without `enqueue`: (size, count)
    read_async: str     # the reader on the copy stream (count, first, into); for a row without `enqueue`: (size, count, first, into)
    args: object = lambda sampler, request, count: ()   # what `enqueue` takes beyond (first, count)
    marks_behind: bool = False                          # the diagnostics' marks are enqueued right behind this row


def _after_reset(key, name):
    """The size of a product whose reset leaves its extent in member `key` of the `ProductState` (0: never reset)."""
    def size(sampler, request, sizes):
        if not request:
            return 0
        extent = getattr(sampler._state(), key)
        if not extent:
            raise ValueError(f"{name} asked for before reset_{name}")
        return extent
    return size


def _marginal_arrays(keys, whole=False):
    """By day, by location, state by day: int64 [days,3], [M,3], [days,3]; `whole`: the size is a switch, the days are T."""
    def arrays(sampler, days):
        d = sampler.T if whole else int(days)
        return {k: ((e, 3), np.int64) for k, e in zip(keys, (d, sampler.M, d))}
    return arrays


def _group_arrays(sampler, size):
    out = {}
    for src, L in size[1].items():
        _, ev_key, st_key = GROUP_SOURCES[src]
        out.update({ev_key: ((size[0], int(L), 3), np.int64)}, **({st_key: ((size[0], 3), np.int64)} if st_key else {}))
    return out


# The burst protocol, stated once ("The burst protocol"): per burst the products that are on are enqueued in this
# order behind the sweeps, then read in this order behind the trace.  PinnedTrace, trace_view, sample and sample_bursts loop
# over it and reach the sampler's methods by name, at call time.
BURST_PRODUCTS = (
    BurstProduct("marginals", "summarize", lambda s, req, sizes: s._summarize_mode(req),
                 _marginal_arrays(MARGINAL_KEYS, whole=True), "summarize", "read_marginals", "read_marginals_async",
                 args=lambda s, req, n: (req is True,), marks_behind=True),   # "marginals": written, not folded
    # forecast=True holds the baseline; a callable (j0, count) -> steps [count,B,H] is asked with j0 = the draws per chain
    # forecast since the reset, as they stand at enqueue time -- after a re-run of a burst it is the same again
    BurstProduct("forecast", "forecast", _after_reset("forecast_H", "forecast"), _marginal_arrays(FORECAST_KEYS),
                 "forecast", "read_forecast_marginals", "read_forecast_marginals_async",
                 args=lambda s, req, n: (req(s._state().fc_j, n) if callable(req) else None,)),
    BurstProduct("rt", "rt", _after_reset("rt_D", "rt"), lambda s, D: ((int(D),), np.float64),
                 "rt", "read_rt_draws", "read_rt_draws_async"),
    BurstProduct("check", "check", _after_reset("check_K", "check"), _marginal_arrays(CHECK_KEYS),
                 "check", "read_check_marginals", "read_check_marginals_async"),
    BurstProduct("wb", "within_between", _after_reset("wb_D", "within_between"),
                 lambda s, D: {k: ((int(D),), np.float64) for k in WB_KEYS},
                 "within_between", "read_wb_draws", "read_wb_draws_async"),
    # (G, {source: day extent}): the group sums of the sources that run with the burst
    BurstProduct("groups", "groups", lambda s, req, sizes: s._group_sources(req, sizes), _group_arrays,
                 None, "_read_group_sums", "_read_group_sums"),
    # (G, {key of GROUP_CURVE_KEYS: window days}): the curves that run with the burst
    BurstProduct("group_curves", None, lambda s, req, sizes: s._group_curve_days(sizes),
                 lambda s, size: {k: ((size[0], int(D)), np.float64) for k, D in size[1].items()},
                 None, "_read_group_curves", "_read_group_curves"),
)
PRODUCTS = {p.field: p for p in BURST_PRODUCTS}


def _allocate(spec, alloc):
    """`alloc(trailing shape, dtype)` for the one pair or for every entry of a row's `arrays`."""
    return alloc(*spec) if isinstance(spec, tuple) else {k: alloc(*v) for k, v in spec.items()}


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
        sizes = locals()                                    # first statement: the keywords, read by the rows' field names
        self._lib = sampler._lib
        self.count = int(count)
        B, P, M, T = sampler.B, sampler.P, sampler.M, sampler.T
        self._ptrs = []
        self.theta = self._alloc((count, B, P), np.float64)
        self.events = self._alloc((count, B, M, T, 3), sampler.events_dtype) if (events and sampler.record_events) else None
        self.hmc = self._alloc((count, B, 3), np.float64)
        self.moves = self._alloc((count, B, 4, _lib.MOVE_TRACE), np.float64)
        for p in BURST_PRODUCTS:                            # a row that is off leaves None
            setattr(self, p.field, _allocate(p.arrays(sampler, sizes[p.field]), lambda sh, dt: self._alloc((count, B) + sh, dt))
                    if sizes[p.field] else None)

    def _alloc(self, shape, dtype):
        nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        p = ctypes.c_void_p()
        _lib.check(self._lib.seir_host_alloc(ctypes.byref(p), max(nbytes, 8)))
        self._ptrs.append(p)
        buf = (ctypes.c_char * max(nbytes, 8)).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape, dtype=np.int64))).reshape(shape)

    def close(self):
        for field in ("theta", "events", "hmc", "moves") + tuple(PRODUCTS):
            setattr(self, field, None)
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
    _s = None                     # the library's handle; without one (a subclass that never runs __init__) nothing is on
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
        if self._s:
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
    def _state(self) -> ProductState:
        """The state of the products as the library holds it now (`seir_sampler_product_state`: host fields only, no device
        call; a sampler with a hand-off time-out pending answers too).  This class keeps no copy: what a reset, a switch, a
        refusal, a snapshot or a restore did to it is read here ("Who owns the product state")."""
        if not self._s:
            return ProductState()
        st = _lib.SeirProductState()
        _lib.check(self._lib.seir_sampler_product_state(self._s, ctypes.byref(st)))
        return ProductState(*(tuple(v) if isinstance(v, ctypes.Array) else v for v in (getattr(st, k) for k in _STATE_KEYS)))

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

    def restore(self, slot: int = 0):
        """Back to the snapshot in `slot`; clears a hand-off time-out."""
        _lib.check(self._lib.seir_sampler_restore(self._s, int(slot)))

    def set_launch_form(self, hmc: str, moves: str):
        _lib.check(self._lib.seir_sampler_set_launch_form(self._s, HMC_MODES[hmc], MOVES_MODES[moves]))

    def launch_form(self):
        h, m = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(self._lib.seir_sampler_launch_form(self._s, ctypes.byref(h), ctypes.byref(m)))
        inv_h = {v: k for k, v in HMC_MODES.items()}
        inv_m = {v: k for k, v in MOVES_MODES.items()}
        return inv_h[h.value], inv_m[m.value]

    def sweep_plan(self) -> dict:
        """The launch plan in force (`seir_sampler_sweep_plan`: csrc/sweep_plan.h's plan for the first chain group, host
        fields only).  `launch_form()` is the form that was asked for; this is what the shape, the chains and the chip made
        of it: "hmc" is "fold" / "tailfold" / "stage", "inner" "single" / "leap" / "se_chunk" / "split", "moves" "pairs" /
        "pair" / "split", "fpend" None or the kernel's name; every other member is an int."""
        p = _lib.SeirSweepPlan()
        _lib.check(self._lib.seir_sampler_sweep_plan(self._s, ctypes.byref(p)))
        out = {k: int(getattr(p, k)) for k, _ in _lib.SeirSweepPlan._fields_ if k != "reserved"}
        out["hmc"], out["inner"] = _lib.PLAN_HMC[out["hmc"]], _lib.PLAN_INNER[out["inner"]]
        out["moves"], out["fpend"] = _lib.PLAN_MOVES[out["moves"]], _lib.PLAN_FPEND[out["fpend"]]
        return out

    def move_instance(self) -> int:
        """The sub-move bound of the event-update instances the next sweep launches (`seir_sampler_move_instance`): 2 --
        the kernels under their plain names, for m <= 2 -- or 4, the `_m4` kernels (m > 2, or
        `SeirModel.set_option(generic_moves=True)`).  `kernel_resources.move_instance_names` spells the kernels."""
        mm = ctypes.c_int32()
        _lib.check(self._lib.seir_sampler_move_instance(self._s, ctypes.byref(mm)))
        return int(mm.value)

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

    def read_move_columns(self, count: int, first: int = 0) -> np.ndarray:
        """The move results of trace slots [first, first+count) as they are stored: [count, B, 4, 2 + 4 * MMAX] --
        is_accepted, target_log_prob, then m, t, delta_t, x_star for all MMAX sub-moves, those beyond `m` included
        (zeros), which `Trace.moves[...]["proposed_delta"]` cuts off."""
        n = int(count)
        theta, hmc = np.empty((n, self.B, self.P)), np.empty((n, self.B, 3))
        mv = np.empty((n, self.B, 4, _lib.MOVE_TRACE))
        _lib.check(self._lib.seir_sampler_read_trace(self._s, int(first), n, _dptr(theta), None, _dptr(hmc), _dptr(mv)))
        return mv

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
        for field in PRODUCTS:                              # a stand-in buffer may lack the newer fields
            v = getattr(buf, field, None)
            if v is not None:
                setattr(tr, field, {k: a[:n] for k, a in v.items()} if isinstance(v, dict) else v[:n])
        return tr

    def _fresh(self, field, size, count):
        """Unpinned arrays for `count` draws of the product `field`, shaped by its row of `BURST_PRODUCTS`."""
        return _allocate(PRODUCTS[field].arrays(self, size), lambda sh, dt: np.empty((int(count), self.B) + sh, dt))

    def _pinned_arrays(self, into, field, count, what):
        """The arrays of `field` in the pinned buffer `into`, which must hold `count` draws of them."""
        arrays = getattr(into, field, None)
        if int(count) > into.count or arrays is None:
            raise ValueError(f"pinned buffer too small or without {what}")
        return arrays

    # -- summaries of the recorded events on the device (include/seir_hip.h) --------------------------
    def reset_summary(self):
        """Enable the summaries (first call) and zero the moment accumulators, `count` and the overflow flag, in stream
        order: the next draw folded becomes `ref`."""
        _lib.check(self._lib.seir_sampler_summary_reset(self._s))

    def summarize(self, first: int, count: int, accumulate: bool = True):
        """Enqueue the summary of trace slots [first, first+count) behind the sweeps that fill them: their marginals are
        written, and with `accumulate` the draws are folded into the moments."""
        _lib.check(self._lib.seir_sampler_summarize(self._s, int(first), int(count), int(bool(accumulate))))

    def _read_product(self, fn, field, size, count, first, into=None, what=None):
        """The arrays of the product `field` (the three per-draw marginals by day, by location, state by day; the national
        curves) of trace slots [first, first+count) through its C reader `fn`, in the order of its row: into fresh arrays
        (blocking `fn`), or into those of the PinnedTrace `into` (asynchronous `fn`, completed by `trace_wait()`)."""
        out = self._fresh(field, size, count) if into is None else self._pinned_arrays(into, field, count, what)
        arrays = [out[k] for k in PRODUCTS[field].arrays(self, size)] if isinstance(out, dict) else [out]
        _lib.check(fn(self._s, int(first), int(count),
                      *(a.ctypes.data_as(_lib.c_int64_p) if a.dtype == np.int64 else _dptr(a) for a in arrays)))
        return out

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
        return self._read_product(self._lib.seir_sampler_read_marginals, "marginals", True, count, first)

    def read_marginals_async(self, count: int, first: int, into: PinnedTrace):
        """As `read_trace_async`, for the marginals; completed by `trace_wait()`."""
        self._read_product(self._lib.seir_sampler_read_marginals_async, "marginals", True, count, first, into, "marginals")

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
        return Diagnostics(batch_length=self._state().diag_batch_len, count=sm.count, ref=sm.ref, sum=sm.sum, sumsq=sm.sumsq, bsum=bsum,
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

    def forecast(self, first: int, count: int, steps=None):
        """Enqueue the forecast of trace slots [first, first+count) behind the sweeps that fill them and fold it.  `steps`
        [count,B,H] (optional): random-walk steps of the log baseline; None holds the baseline at its last value."""
        n = int(count)
        if steps is not None:
            steps = np.ascontiguousarray(steps, dtype=np.float64)
            H = self._state().forecast_H
            if steps.shape != (n, self.B, H):
                raise ValueError(f"need steps [{n},{self.B},{H}]")
        _lib.check(self._lib.seir_sampler_forecast(self._s, int(first), n, None if steps is None else _dptr(steps)))

    def read_forecast_marginals(self, count: int, first: int = 0) -> dict:
        """Blocking read of the forecast marginals of trace slots [first, first+count): FORECAST_KEYS -> int64 arrays with
        leading axes [count, B]."""
        return self._read_product(self._lib.seir_sampler_read_forecast_marginals, "forecast", self._state().forecast_H, count, first)

    def read_forecast_marginals_async(self, count: int, first: int, into: PinnedTrace):
        """As `read_marginals_async`, for the forecast marginals; completed by `trace_wait()`."""
        self._read_product(self._lib.seir_sampler_read_forecast_marginals_async, "forecast", self._state().forecast_H, count, first, into,
                           "forecast arrays")

    def forecast_summary(self) -> Summary:
        """The forecast moments folded since the last `reset_forecast` (blocking): a `Summary` whose day axis is the H
        forecast days, [B,M,H,6].  Raises `SeirError` (SEIR_ERR_STATE) if an accumulator overflowed or before a reset."""
        return self._read_moments(self._lib.seir_sampler_read_forecast, self._state().forecast_H)

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
        shape = (len(ranks),) + (() if pooled else (self.B,)) + (3, self.M, self._state().forecast_H)
        out = np.empty(shape, np.int32)
        _lib.check(self._lib.seir_sampler_forecast_order_stats(self._s, ranks.ctypes.data_as(_lib.c_int64_p), len(ranks),
                                                               1 if pooled else 0,
                                                               out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return out

    def forecast_quantiles(self, probs, pooled: bool = False) -> np.ndarray:
        """Quantiles `probs` (NumPy's default rule, `posterior.quantiles`) of every cell over the draws kept since the
        reset (blocking): float64 [K, B, 3, M, H], or [K, 3, M, H] when `pooled`."""
        from .posterior import quantiles as Q
        n = self._state().fc_j * (self.B if pooled else 1)
        ranks = Q.quantile_ranks(n, probs)
        return Q.interpolate(self.forecast_order_stats(ranks, pooled=pooled), ranks, n, probs)

    # -- the forecast scored against later data (include/seir_hip.h, "Scoring the forecast against later data") ----
    def set_verify(self, truth):
        """The forecast is scored against `truth` from now on: int32 [M, H], -1 where nothing was observed
        (`posterior.verify.extract_truth`).  Between `reset_forecast` and the first `forecast`; None turns it off."""
        if truth is None:
            _lib.check(self._lib.seir_sampler_verify_set(self._s, None))
            return
        H = self._state().forecast_H
        y = np.ascontiguousarray(truth)
        if y.dtype.kind not in "iu" or (H and y.shape != (self.M, H)) or (y.size and (y.min() < -2 ** 31 or y.max() >= 2 ** 31)):
            raise ValueError(f"truth {y.dtype} {y.shape}: need integers within int32 [{self.M}, {H}]")
        y = np.ascontiguousarray(y, dtype=np.int32)
        _lib.check(self._lib.seir_sampler_verify_set(self._s, y.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))

    def verify_state(self) -> dict:
        """on, H, j (the draws per chain folded since the forecast reset) and whether the draw store is on, as the library
        holds them; zeros while no truth is set.  No device call."""
        out = np.zeros(4, np.int64)
        _lib.check(self._lib.seir_sampler_verify_state(self._s, out.ctypes.data_as(_lib.c_int64_p)))
        return dict(on=bool(out[0]), H=int(out[1]), j=int(out[2]), store=bool(out[3]))

    def verify_summary(self) -> dict:
        """The accumulators against the truth folded since the last `reset_forecast` (blocking): `count` uint64 [B], `lt`,
        `eq` uint32 and `abs_sum` uint64 [B, M, H, 2] -- cases, cum_cases (`posterior.verify.scores` forms PIT, MAE and
        CRPS from them)."""
        st = self.verify_state()
        shape = (self.B, self.M, st["H"], 2)
        out = dict(count=np.zeros(self.B, np.uint64), lt=np.empty(shape, np.uint32), eq=np.empty(shape, np.uint32),
                   abs_sum=np.empty(shape, np.uint64))
        u32, u64 = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
        _lib.check(self._lib.seir_sampler_read_verify(self._s, out["count"].ctypes.data_as(u64), out["lt"].ctypes.data_as(u32),
                                                      out["eq"].ctypes.data_as(u32), out["abs_sum"].ctypes.data_as(u64)))
        return out

    def forecast_pair_sums(self, pooled: bool = False) -> np.ndarray:
        """The sum of pairwise absolute differences of every cell's kept forecast draws (blocking; needs the draw store):
        int64 [B, 2, M, H] -- planes cases, cum_cases -- or, `pooled`, [2, M, H] over the B x count values of all chains
        of this sampler.  Equal to `posterior.verify.pair_sum` of the draws."""
        H = self._state().forecast_H
        out = np.empty((() if pooled else (self.B,)) + (2, self.M, H), np.int64)
        _lib.check(self._lib.seir_sampler_forecast_pair_sums(self._s, 1 if pooled else 0, out.ctypes.data_as(_lib.c_int64_p)))
        return out

    # -- scenarios riding on the forecast (include/seir_hip.h, "Scenario forecasts on the device") ----------------
    def set_scenarios(self, log_shift, commute, cap: int, triggers=None):
        """K scenarios ride on the forecast from now on: `log_shift` and `commute` float64 [K, H] (`posterior.scenarios`),
        `cap` the draws per chain the per-draw stores hold.  Between `reset_forecast` and the first `forecast`; K = 0 or
        cap = 0 frees everything.  The library refuses what it cannot hold; the forecast then runs on without scenarios.
        Arrays [K, M, H] are targeted scenarios, whose operands differ by location (include/seir_hip.h, "Targeted scenarios
        on the device"; `posterior.scenarios.local_inputs`): they go through `seir_sampler_scenarios_set_local`.
        `triggers`: a mapping that makes the [K, M, H] arrays the off pair of triggered scenarios (include/seir_hip.h,
        "Triggered scenarios on the device"; `posterior.scenarios.trigger_states`) -- `log_shift_on`, `commute_on` [K, M, H],
        the thresholds `on`, `off` int32 [K, M] and `window`, `from_day`, `min_days`, `review_every` [K] -- through
        `seir_sampler_scenarios_set_triggered`."""
        H = self._state().forecast_H
        ls = np.zeros((0, H)) if log_shift is None else np.ascontiguousarray(log_shift, dtype=np.float64)
        cm = np.ones((0, H)) if commute is None else np.ascontiguousarray(commute, dtype=np.float64)
        if triggers is not None and ls.ndim != 3:
            raise ValueError(f"log_shift {ls.shape}: triggered scenarios take the off pair as [K, {self.M}, {H}]")
        if ls.ndim == 3:
            if ls.shape != cm.shape or ls.shape[1] != self.M or (ls.shape[0] and H and ls.shape[2] != H):
                raise ValueError(f"log_shift {ls.shape} and commute {cm.shape}: need two of [K, {self.M}, {H}]")
            if int(cap) < 0:
                raise ValueError(f"cap={cap}: the number of draws per chain to keep")
            if triggers is not None:
                K = ls.shape[0]
                lo = np.ascontiguousarray(triggers["log_shift_on"], dtype=np.float64)
                co = np.ascontiguousarray(triggers["commute_on"], dtype=np.float64)
                if lo.shape != ls.shape or co.shape != ls.shape:
                    raise ValueError(f"log_shift_on {lo.shape} and commute_on {co.shape}: need two of {ls.shape}")
                th = []
                for key in ("on", "off"):
                    v = np.asarray(triggers[key])
                    if v.shape != (K, self.M) or (v.size and (v.min() < -2 ** 31 or v.max() > 2 ** 31 - 1)):
                        raise ValueError(f"triggers[{key!r}] {v.shape}: int32 [{K}, {self.M}]")
                    th.append(np.ascontiguousarray(v, dtype=np.int32))
                par = np.empty((K, 4), np.int32)
                for i, key in enumerate(("window", "from_day", "min_days", "review_every")):
                    v = np.asarray(triggers[key])
                    if v.shape != (K,) or (v.size and (v.min() < -2 ** 31 or v.max() > 2 ** 31 - 1)):
                        raise ValueError(f"triggers[{key!r}] {v.shape}: int32 [{K}]")
                    par[:, i] = v
                ip = ctypes.POINTER(ctypes.c_int32)
                _lib.check(self._lib.seir_sampler_scenarios_set_triggered(
                    self._s, K, _dptr(ls), _dptr(cm), _dptr(lo), _dptr(co), th[0].ctypes.data_as(ip), th[1].ctypes.data_as(ip),
                    par.ctypes.data_as(ip), int(cap)))
                return
            _lib.check(self._lib.seir_sampler_scenarios_set_local(self._s, ls.shape[0], _dptr(ls), _dptr(cm), int(cap)))
            return
        if ls.ndim != 2 or ls.shape != cm.shape or (ls.shape[0] and H and ls.shape[1] != H):   # H = 0: the library refuses
            raise ValueError(f"log_shift {ls.shape} and commute {cm.shape}: need two of [K, {H}]")
        if int(cap) < 0:
            raise ValueError(f"cap={cap}: the number of draws per chain to keep")
        _lib.check(self._lib.seir_sampler_scenarios_set(self._s, ls.shape[0], _dptr(ls), _dptr(cm), int(cap)))

    def set_scenario_groups(self, on: bool = True):
        """Switch the scenarios' per-draw region totals on or off: with a group table in force (`set_groups`) and scenarios
        set, every `forecast` also sums each scenario's counts over the groups, by draw position since the forecast reset.
        Refused without a table; off frees the store."""
        _lib.check(self._lib.seir_sampler_scenario_groups_set(self._s, 1 if on else 0))

    def read_scenario_group_draws(self, count: int = None, first: int = 0) -> np.ndarray:
        """The scenarios' region totals by draw position since the forecast reset (blocking): int64 [K, count, B, G, H, 3];
        `count` None: every draw from `first` on."""
        st, G = self.scenario_state(), self._state().groups_G
        n = st["j"] - int(first) if count is None else int(count)
        out = np.empty((st["K"], max(n, 0), self.B, G, st["H"], 3), np.int64)
        _lib.check(self._lib.seir_sampler_read_scenario_group_draws(self._s, int(first), n, out.ctypes.data_as(_lib.c_int64_p)))
        return out

    def scenario_triggers(self) -> dict:
        """The record of the triggered scenarios' rules folded since the last `reset_forecast` (blocking): `count` (draws per
        chain) and `active_count` uint32 [K, B, M, H], the draws of chain b in which location m is under the measure on day s.
        Refused unless the set in force is a triggered one."""
        st = self.scenario_state()
        out = np.empty((st["K"], self.B, self.M, st["H"]), np.uint32)
        _lib.check(self._lib.seir_sampler_read_scenario_triggers(self._s, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
        return dict(count=st["j"], active_count=out)

    def read_scenario_trigger_draws(self, count: int = None, first: int = 0) -> np.ndarray:
        """The number of locations under the measure by draw position since the forecast reset (blocking): int32
        [K, count, B, H]; `count` None: every draw from `first` on."""
        st = self.scenario_state()
        n = st["j"] - int(first) if count is None else int(count)
        out = np.empty((st["K"], max(n, 0), self.B, st["H"]), np.int32)
        _lib.check(self._lib.seir_sampler_read_scenario_trigger_draws(self._s, int(first), n,
                                                                      out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return out

    def scenario_state(self) -> dict:
        """K, H, cap and j (the draws per chain rolled forward since the forecast reset) as the library holds them; zeros
        while no scenarios are set.  No device call."""
        out = np.zeros(4, np.int64)
        _lib.check(self._lib.seir_sampler_scenario_state(self._s, out.ctypes.data_as(_lib.c_int64_p)))
        return dict(K=int(out[0]), H=int(out[1]), cap=int(out[2]), j=int(out[3]))

    def scenario_summary(self) -> list:
        """The scenarios' moments folded since the last `reset_forecast` (blocking): one `Summary` [B,M,H,6] per scenario."""
        st = self.scenario_state()
        K, shape = st["K"], (st["K"], self.B, self.M, st["H"], len(SUMMARY_QUANTITIES))
        cnt = np.zeros((K, self.B), np.uint64)
        ref, sm, sq = np.empty(shape, np.int32), np.empty(shape, np.int64), np.empty(shape, np.uint64)
        u64 = ctypes.POINTER(ctypes.c_uint64)
        _lib.check(self._lib.seir_sampler_read_scenarios(self._s, cnt.ctypes.data_as(u64), ref.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                         sm.ctypes.data_as(_lib.c_int64_p), sq.ctypes.data_as(u64)))
        return [Summary(count=cnt[k], ref=ref[k], sum=sm[k], sumsq=sq[k]) for k in range(K)]

    def scenario_diffs(self) -> dict:
        """The accumulators of the paired differences, scenario minus forecast (blocking): `count` (draws per chain), `ref`
        int32, `sum` int64, `sumsq` uint64, `lt`, `eq` uint32, each [K,B,M,H,4] -- cases, cum_cases, prevalence,
        cum_infections (`posterior.scenarios.statistics` forms mean, variance and P(below) from them)."""
        st = self.scenario_state()
        shape = (st["K"], self.B, self.M, st["H"], 4)
        out = dict(ref=np.empty(shape, np.int32), sum=np.empty(shape, np.int64), sumsq=np.empty(shape, np.uint64),
                   lt=np.empty(shape, np.uint32), eq=np.empty(shape, np.uint32))
        u32 = ctypes.POINTER(ctypes.c_uint32)
        _lib.check(self._lib.seir_sampler_read_scenario_diffs(
            self._s, out["ref"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), out["sum"].ctypes.data_as(_lib.c_int64_p),
            out["sumsq"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), out["lt"].ctypes.data_as(u32), out["eq"].ctypes.data_as(u32)))
        out["count"] = st["j"]
        return out

    def read_scenario_draws(self, count: int = None, first: int = 0) -> dict:
        """The scenarios' per-draw curves by draw position since the forecast reset (blocking): `by_day` and `state_by_day`
        int64 [K, count, B, H, 3]; `count` None: every draw from `first` on."""
        st = self.scenario_state()
        n = st["j"] - int(first) if count is None else int(count)
        shape = (st["K"], max(n, 0), self.B, st["H"], 3)
        out = dict(by_day=np.empty(shape, np.int64), state_by_day=np.empty(shape, np.int64))
        _lib.check(self._lib.seir_sampler_read_scenario_draws(self._s, int(first), n, out["by_day"].ctypes.data_as(_lib.c_int64_p),
                                                              out["state_by_day"].ctypes.data_as(_lib.c_int64_p)))
        return out

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
        _lib.check(self._lib.seir_sampler_rt_reset(self._s, D, _dptr(w)))

    def rt(self, first: int, count: int):
        """Enqueue R_it of trace slots [first, first+count) behind the sweeps that fill them: folded into the moments,
        and the national curve of every draw written."""
        _lib.check(self._lib.seir_sampler_rt(self._s, int(first), int(count)))

    def read_rt_draws(self, count: int, first: int = 0) -> np.ndarray:
        """Blocking read of R_t [count,B,D] of trace slots [first, first+count)."""
        return self._read_product(self._lib.seir_sampler_read_rt_draws, "rt", self._state().rt_D, count, first)

    def read_rt_draws_async(self, count: int, first: int, into: PinnedTrace):
        """As `read_marginals_async`, for the national curves; completed by `trace_wait()`."""
        self._read_product(self._lib.seir_sampler_read_rt_draws_async, "rt", self._state().rt_D, count, first, into, "R_t")

    def rt_summary(self) -> RtSummary:
        """The R_it accumulators folded since the last `reset_rt` (blocking): `RtSummary`, whose `.mean`, `.var` and
        `.prob_gt1` are formed here.  Raises `SeirError` (SEIR_ERR_STATE) before a reset."""
        shape = (self.B, self._state().rt_D, self.M)
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
        out = np.empty((len(ranks),) + (() if pooled else (self.B,)) + (self._state().rt_D, self.M))
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

    def check(self, first: int, count: int):
        """Enqueue the check of trace slots [first, first+count) behind the sweeps that fill them: the window is simulated
        again from every draw, folded, and counted against the draw's recorded removals."""
        _lib.check(self._lib.seir_sampler_check(self._s, int(first), int(count)))

    def read_check_marginals(self, count: int, first: int = 0) -> dict:
        """Blocking read of the check's marginals of trace slots [first, first+count): CHECK_KEYS -> int64 arrays with
        leading axes [count, B]."""
        return self._read_product(self._lib.seir_sampler_read_check_marginals, "check", self._state().check_K, count, first)

    def read_check_marginals_async(self, count: int, first: int, into: PinnedTrace):
        """As `read_marginals_async`, for the check's marginals; completed by `trace_wait()`."""
        self._read_product(self._lib.seir_sampler_read_check_marginals_async, "check", self._state().check_K, count, first, into,
                           "check arrays")

    def check_summary(self) -> CheckSummary:
        """Moments and comparison counts folded since the last `reset_check` (blocking).  Raises `SeirError`
        (SEIR_ERR_STATE) if an accumulator overflowed, if the observed removals differed between draws, or before a reset."""
        B, M, K = self.B, self.M, self._state().check_K
        u32 = ctypes.POINTER(ctypes.c_uint32)
        obs = np.empty((B, M, K), np.int32)
        shapes = ((B, M, K), (B, M, K), (B, M), (B, M), (B, K), (B, K), (B,), (B,))
        arrs = [np.empty(sh, np.uint32) for sh in shapes]
        _lib.check(self._lib.seir_sampler_read_check_counts(self._s, obs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                            *(a.ctypes.data_as(u32) for a in arrs)))
        mom = self._read_moments(self._lib.seir_sampler_read_check, K)
        return CheckSummary(mom, obs, *arrs)

    # -- within/between pressure shares (include/seir_hip.h, "Within/between pressure shares on the device") ----------
    def reset_within_between(self, days: int):
        """Enable the within/between shares (first call), zero their accumulators and count and set the window to the last
        `days` days of the series (1 <= days <= T)."""
        D = int(days)
        if not 1 <= D <= self.T:
            raise ValueError(f"within_between days {D}: 1 <= D <= T = {self.T}")
        _lib.check(self._lib.seir_sampler_wb_reset(self._s, D))

    def within_between(self, first: int, count: int):
        """Enqueue the shares of trace slots [first, first+count) behind the sweeps that fill them: folded into the
        accumulators, and the national pressures of every draw written."""
        _lib.check(self._lib.seir_sampler_wb(self._s, int(first), int(count)))

    def read_wb_draws(self, count: int, first: int = 0) -> dict:
        """Blocking read of the national pressures of trace slots [first, first+count): WB_KEYS -> [count,B,D]."""
        return self._read_product(self._lib.seir_sampler_read_wb_draws, "wb", self._state().wb_D, count, first)

    def read_wb_draws_async(self, count: int, first: int, into: PinnedTrace):
        """As `read_marginals_async`, for the national pressures; completed by `trace_wait()`."""
        self._read_product(self._lib.seir_sampler_read_wb_draws_async, "wb", self._state().wb_D, count, first, into, "within/between arrays")

    def within_between_summary(self) -> WbSummary:
        """The accumulators folded since the last `reset_within_between` (blocking): `WbSummary`, whose `.within_mean`,
        `.within_var`, `.between_mean` and `.p_within_gt_between` are formed here.  Raises `SeirError` (SEIR_ERR_STATE)
        before a reset."""
        shape = (self.B, self._state().wb_D, self.M)
        u32 = ctypes.POINTER(ctypes.c_uint32)
        cnt = np.zeros(self.B, np.uint64)
        n, gt = np.empty(shape, np.uint32), np.empty(shape, np.uint32)
        ref_w, sum_w, sumsq_w, ref_b, sum_b = (np.empty(shape) for _ in range(5))
        _lib.check(self._lib.seir_sampler_read_wb(self._s, cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                                  n.ctypes.data_as(u32), _dptr(ref_w), _dptr(sum_w), _dptr(sumsq_w),
                                                  _dptr(ref_b), _dptr(sum_b), gt.ctypes.data_as(u32)))
        return WbSummary(count=cnt, defined=n, ref_w=ref_w, sum_w=sum_w, sumsq_w=sumsq_w, ref_b=ref_b, sum_b=sum_b, gt=gt)

    # -- region totals: per-draw sums over groups of locations (include/seir_hip.h, "Region totals on the device") ------
    def set_groups(self, offsets, members):
        """Set the table of groups (CSR: `offsets` [G+1], `members` [nnz], ascending and unique within a group;
        `posterior.groups.parse_groups`), or free it with `set_groups(None, None)`.  While a table is set, `summarize`,
        `forecast` and `check` also form every kept draw's sums over each group's members (`read_group_marginals`)."""
        i32p = ctypes.POINTER(ctypes.c_int32)
        if offsets is None:
            _lib.check(self._lib.seir_sampler_groups_set(self._s, 0, None, None))
            return
        off = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
        mem = np.ascontiguousarray(members, dtype=np.int32).reshape(-1)
        G = off.size - 1
        if G < 1 or mem.size < int(off.max()):              # what the library cannot check: it reads members up to the offsets
            raise ValueError(f"offsets [{off.size}] reach {int(off.max()) if off.size else 0}, members holds {mem.size}: not a "
                             "CSR pair of at least one group")
        if G > _lib.GROUPS_MAX:
            raise ValueError(f"G={G}: at most {_lib.GROUPS_MAX} groups")
        _lib.check(self._lib.seir_sampler_groups_set(self._s, G, off.ctypes.data_as(i32p), mem.ctypes.data_as(i32p)))

    def _check_group_weights(self, w):
        st = self._state()
        if st.groups_G and w.size != st.groups_nnz:
            raise ValueError(f"need weights [{st.groups_nnz}], aligned with the table's members")

    # -- group curves: R_t and within / between per group (include/seir_hip.h, "Group curves on the device") ------------
    def set_group_rt(self, weights):
        """Group R_t on: while a table is set and `rt` runs, every draw it folds also leaves, per group and window day, the
        sum over the members of weights[k] * R_it (`weights` [nnz] float64 aligned with the table's `members`; for a
        population-weighted curve N[members] / the group's population) in the fixed order of
        `posterior.groups.weighted_sum_rows`.  None switches it off.  A later `set_groups` switches it off too."""
        if weights is None:
            _lib.check(self._lib.seir_sampler_group_rt(self._s, None))
            return
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        self._check_group_weights(w)
        _lib.check(self._lib.seir_sampler_group_rt(self._s, _dptr(w)))   # SEIR_ERR_STATE without a table

    def set_group_within_between(self, on: bool):
        """Group within / between on or off: while a table is set and `within_between` runs, every draw it folds also
        leaves the members' sums of the within and the between pressure per group and window day ("between": from outside
        each member location, as in the national figure)."""
        _lib.check(self._lib.seir_sampler_group_wb(self._s, 1 if on else 0))

    # -- group next-generation matrix (include/seir_hip.h, "Group next-generation matrix on the device") ----------------
    def set_group_ngm(self, weights, cap: int):
        """Group next-generation matrix on: while a table is set, every draw that `rt` folds also leaves K[g][h][t], the
        expected infections in group g caused by one typical infective of group h on window day t, in a store of `cap`
        draws per chain (`read_group_ngm`).  `weights` [nnz] float64 aligned with the table's `members`
        (`posterior.groups.rt_weights`: the array group R_t uses).  Between `reset_rt` and the first `rt`, as
        `keep_rt_draws`.  None or cap = 0 switches it off and frees the store; so do a later `set_groups` and a `reset_rt`
        with another window.  Not a burst product: `sample` / `sample_bursts` carry nothing of it."""
        cap = int(cap)
        if cap < 0:
            raise ValueError(f"cap={cap}: the number of draws per chain to keep")
        if weights is None or cap == 0:
            _lib.check(self._lib.seir_sampler_group_ngm(self._s, None, 0))
            return
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        self._check_group_weights(w)
        _lib.check(self._lib.seir_sampler_group_ngm(self._s, _dptr(w), cap))   # SEIR_ERR_STATE without a table or an rt reset

    def read_group_ngm(self, count: int, first: int = 0) -> np.ndarray:
        """Blocking read of K of draws [first, first+count) since the last `reset_rt`: float64 [count,B,G,G,D]
        (destination group, source group, window day)."""
        count, st = int(count), self._state()
        out = np.empty((max(count, 0), self.B, st.groups_G, st.groups_G, st.ngm_D), dtype=np.float64)
        _lib.check(self._lib.seir_sampler_read_group_ngm(self._s, int(first), count, _dptr(out)))
        return out

    def _group_curve_days(self, sizes):
        """(G, {key of GROUP_CURVE_KEYS: window days}) of the curves that leave outputs with a burst that runs the rt /
        within_between of `sizes` ({field: size} of the burst's products); () when there is none."""
        days, st = {}, self._state()
        if sizes["rt"] and st.group_rt_D:                  # the library's own condition for forming the curves
            days["rt_by_group"] = st.group_rt_D
        if sizes["wb"] and st.group_wb_D:
            days["within_by_group"] = days["between_by_group"] = st.group_wb_D
        return (st.groups_G, days) if days else ()

    def read_group_rt(self, count: int, first: int = 0) -> np.ndarray:
        """Blocking read of the group R_t of trace slots [first, first+count): float64 [count,B,G,D]."""
        st = self._state()
        out = self._fresh("group_curves", (st.groups_G, {"rt_by_group": st.group_rt_D}), count)["rt_by_group"]
        _lib.check(self._lib.seir_sampler_read_group_rt(self._s, int(first), int(count), _dptr(out)))
        return out

    def read_group_wb(self, count: int, first: int = 0) -> dict:
        """Blocking read of the group pressures of trace slots [first, first+count): within_by_group, between_by_group
        -> float64 [count,B,G,D]."""
        st = self._state()
        out = self._fresh("group_curves", (st.groups_G, dict.fromkeys(GROUP_CURVE_KEYS[1:], st.group_wb_D)), count)
        _lib.check(self._lib.seir_sampler_read_group_wb(self._s, int(first), int(count), *(_dptr(out[k]) for k in GROUP_CURVE_KEYS[1:])))
        return out

    def _read_group_curves(self, size, count, first=0, into=None):
        """The curves of `size` (`_group_curve_days`) of slots [first, first+count): blocking into new arrays, or on the copy
        stream `into` the arrays of a PinnedTrace (completed by `trace_wait()`)."""
        days = size[1]
        if into is None:
            out = {}
            if "rt_by_group" in days:
                out["rt_by_group"] = self.read_group_rt(count, first)
            if "within_by_group" in days:
                out.update(self.read_group_wb(count, first))
            return out
        g = self._pinned_arrays(into, "group_curves", count, "group curves")
        if any(k not in g for k in days):
            raise ValueError("pinned buffer too small or without group curves")
        if "rt_by_group" in days:
            _lib.check(self._lib.seir_sampler_read_group_rt_async(self._s, int(first), int(count), _dptr(g["rt_by_group"])))
        if "within_by_group" in days:
            _lib.check(self._lib.seir_sampler_read_group_wb_async(self._s, int(first), int(count), _dptr(g["within_by_group"]),
                                                                  _dptr(g["between_by_group"])))
        return g

    def _read_groups(self, fn, source, count, first, into=None):
        which, ev_key, st_key = GROUP_SOURCES[source]
        if into is None:
            st = self._state()
            into = self._fresh("groups", (st.groups_G, {source: st.group_L[which]}), count)
        _lib.check(fn(self._s, which, int(first), int(count), into[ev_key].ctypes.data_as(_lib.c_int64_p),
                      into[st_key].ctypes.data_as(_lib.c_int64_p) if st_key else None))
        return into

    def read_group_marginals(self, source: str, count: int, first: int = 0) -> dict:
        """Blocking read of the group sums of trace slots [first, first+count) of `source` ("trace", "forecast", "check"):
        its keys of `GROUP_SOURCES` -> int64 [count,B,G,L,3] (L = T, H, K) and, for the forecast and the check, the
        members' sum of S, E, I at the window's start [count,B,G,3]."""
        return self._read_groups(self._lib.seir_sampler_read_group_marginals, source, count, first)

    def read_group_marginals_async(self, source: str, count: int, first: int, into: PinnedTrace):
        """As `read_marginals_async`, for the group sums of `source`; completed by `trace_wait()`."""
        g = self._pinned_arrays(into, "groups", count, "group arrays")
        if GROUP_SOURCES[source][1] not in g:
            raise ValueError("pinned buffer too small or without group arrays")
        self._read_groups(self._lib.seir_sampler_read_group_marginals_async, source, count, first, g)

    def _read_group_sums(self, size, count, first=0, into=None):
        """The group sums of every source of `size` (`_group_sources`) of slots [first, first+count): blocking into one new
        dict, or on the copy stream into the arrays of the PinnedTrace `into` (completed by `trace_wait()`)."""
        if into is None:
            return {k: v for src in size[1] for k, v in self.read_group_marginals(src, count, first).items()}
        for src in size[1]:
            self.read_group_marginals_async(src, count, first, into)

    def _group_sources(self, groups, sizes):
        """`groups` of sample / sample_bursts: (G, {source: day extent}) of the sources whose group sums cross with the trace
        -- True: every one of "trace", "forecast", "check" that runs with the burst (`sizes`: {field: size} of the burst's
        products); or a tuple of those names, each of which must run.  () when `groups` is off."""
        if not groups:
            return ()
        st = self._state()
        if not st.groups_G:
            raise ValueError("groups asked for before set_groups")
        # a source is on when it runs with the burst and its group outputs exist (none: the library refused them)
        runs = dict(trace=sizes["marginals"], forecast=sizes["forecast"], check=sizes["check"])
        on = {k: st.group_L[which] if runs[k] else 0 for k, (which, _, _) in GROUP_SOURCES.items()}
        if groups is True:
            src = tuple(k for k in GROUP_SOURCES if on[k])
        else:
            src = tuple(groups)
            bad = [k for k in src if not on.get(k)]
            if bad:
                raise ValueError(f"groups={groups!r}: {bad[0]!r} is not one of summarize, forecast, check run with this burst")
        if not src:
            raise ValueError("groups needs one of summarize, forecast, check")
        return st.groups_G, {k: on[k] for k in src}

    def _summarize_mode(self, summarize):
        """`summarize` of sample / sample_bursts: False, True (marginals + moments) or "marginals" (accumulate = 0)."""
        if summarize not in (False, True, "marginals"):
            raise ValueError(f"summarize={summarize!r}: False, True or 'marginals'")
        if summarize and not self._state().summary_on:
            self.reset_summary()
        return bool(summarize)

    def _burst_products(self, keywords):
        """{field: (row, size, request)} of the rows of `BURST_PRODUCTS` that the requests -- those of `keywords`, the locals
        of sample / sample_bursts, that a row names -- and the sampler's switches turn on, in table order.  Refuses what is
        asked for too early."""
        requests = {p.request: keywords[p.request] for p in BURST_PRODUCTS if p.request}
        sizes = {}
        for p in BURST_PRODUCTS:
            sizes[p.field] = p.size(self, requests.get(p.request), sizes)
        return {p.field: (p, sizes[p.field], requests.get(p.request)) for p in BURST_PRODUCTS if sizes[p.field]}

    def _enqueue_products(self, on, first, count, mark=None):
        """Enqueue the products `on` for trace slots [first, first+count) behind the sweeps that fill them, in table order;
        `mark` (0 | 1): the diagnostics' mark, right behind the summary's place."""
        for p in BURST_PRODUCTS:
            if p.enqueue and p.field in on:
                getattr(self, p.enqueue)(first, count, *p.args(self, on[p.field][2], count))
            if p.marks_behind and mark is not None:
                self.mark(mark)

    # -- stored draws into trace slots (include/seir_hip.h, "Stored draws into trace slots") --------------------------
    def _per_chain_draws(self, theta, events, chains):
        """`theta` [n,B',P] / `events` [n,B',M,T,3] or per-chain lists of [n,P] / [n,M,T,3] as (chain, theta, events) with
        contiguous float64 arrays, one per chain of `chains` (default 0 .. B'-1)."""
        if isinstance(theta, (list, tuple)) != isinstance(events, (list, tuple)):
            raise ValueError("theta and events: both arrays [n,B',...] or both per-chain lists")
        if isinstance(theta, (list, tuple)):
            th, ev = list(theta), list(events)
        else:
            theta, events = np.asarray(theta), np.asarray(events)
            if theta.ndim != 3 or events.ndim != 5:
                raise ValueError(f"need theta [n,B',{self.P}] and events [n,B',{self.M},{self.T},3]")
            th, ev = [theta[:, c] for c in range(theta.shape[1])], [events[:, c] for c in range(events.shape[1])]
        chains = list(range(len(th))) if chains is None else [int(c) for c in chains]
        if not len(th) == len(ev) == len(chains):
            raise ValueError(f"{len(th)} theta array(s), {len(ev)} event array(s) and {len(chains)} chain(s)")
        if len(set(chains)) != len(chains) or any(not 0 <= c < self.B for c in chains):
            raise ValueError(f"chains={chains}: distinct chains of [0, {self.B})")
        out = []
        for c, t, e in zip(chains, th, ev):
            t = np.ascontiguousarray(t, dtype=np.float64)
            e = np.ascontiguousarray(e, dtype=np.float64)       # integer events, as Trace.events holds them, become fp64 here
            n = t.shape[0]
            if t.shape != (n, self.P) or e.shape != (n, self.M, self.T, 3):
                raise ValueError(f"chain {c}: need theta [n,{self.P}] and events [n,{self.M},{self.T},3], have {t.shape} and {e.shape}")
            out.append((c, t, e))
        if len({t.shape[0] for _, t, _ in out}) > 1:
            raise ValueError("every chain is loaded with the same number of draws")
        return out

    def load_status(self, clear: bool = False) -> np.ndarray:
        """The counters of what was wrong in the draws loaded since creation or the last `clear` (blocking): uint64 [8] --
        cells that are not an integer, negative, over the trace's width; states below zero; theta entries that are not
        finite; the key of the first bad item, its call's chain and first slot.  All zeros: every loaded slot is a draw the
        products may be run on."""
        out = np.zeros(8, np.uint64)
        _lib.check(self._lib.seir_sampler_load_status(self._s, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), int(bool(clear))))
        return out

    def _load_error(self, status, n):
        """The ValueError for a status that is not all zeros: the counts, and the first bad item by category, chain and
        (draw, location, day, transition)."""
        key, chain, first = int(status[5]), int(status[6]), int(status[7])
        flat, code = key >> 3, key & 7
        names = _lib.LOAD_CODES
        counts = ", ".join(f"{int(status[q - 1])} {names[q]}" for q in range(1, 6) if status[q - 1])
        if code == 5:
            where = f"(draw {flat // self.P}, parameter {flat % self.P})"
        else:
            j, r = divmod(flat, self.M * self.T * 3)
            m, r = divmod(r, self.T * 3)
            t, x = divmod(r, 3)
            what = ("S", "E", "I")[x] + f" behind day {t}" if code == 4 else f"day {t}, transition {('S->E', 'E->I', 'I->R')[x]}"
            where = f"(draw {j}, location {m}, {what})"
        return ValueError(f"the stored draws cannot be replayed: {counts}; the first bad item is {names[code]} in chain {chain} at "
                          f"{where} of the {n} draw(s) loaded from slot {first}")

    def load_trace(self, theta, events, first: int = 0, chains=None) -> int:
        """Put stored draws into trace slots [first, first + n) of `chains` (default: 0 .. B'-1): `theta` [n,B',P] constrained
        draws and `events` [n,B',M,T,3], or per-chain lists of [n,P] / [n,M,T,3] (file reads need not be copied together).
        Chain state, sweep counter, thinning, the other slots and chains and every product's accumulators stay as they are.
        Raises ValueError, before anything else is enqueued, when a draw is not one the products may be run on: a count that
        is not an integer in the trace's width, a compartment below zero at a day boundary, a theta entry that is not
        finite -- naming the first such item.  Returns n."""
        rows = self._per_chain_draws(theta, events, chains)
        n = rows[0][1].shape[0] if rows else 0
        if int(first) < 0 or int(first) + n > self.cap:
            raise ValueError(f"trace range [{int(first)},{int(first) + n}) outside capacity {self.cap}")
        for c, t, e in rows:
            _lib.check(self._lib.seir_sampler_load_trace(self._s, c, int(first), n, _dptr(t), _dptr(e)))
        status = self.load_status(clear=True)
        if status.any():
            raise self._load_error(status, n)
        return n

    def replay(self, theta, events, events_out: bool = False, summarize=False, forecast=False, rt=False, check=False,
               within_between=False, groups=False) -> Trace:
        """`sample` without snapshot, reset_trace and run: the stored draws `theta` [n,B,P] / `events` [n,B,M,T,3] (or
        per-chain lists) are loaded into slots [0, n) of all chains, the products that are asked for or switched on are
        enqueued behind them in table order, and the trace and the products are read.  `hmc` and `moves` of the result are
        zeros; `events` is present only with `events_out`.  There is no persistent launch in it and nothing to recover from.
        The chain does not notice: its state, sweep counter and thinning are what they were."""
        on = self._burst_products(locals())                 # first statement: the locals are this call's keywords
        rows = self._per_chain_draws(theta, events, None)
        if len(rows) != self.B:
            raise ValueError(f"replay takes the draws of all {self.B} chain(s), have {len(rows)}")
        n = self.load_trace([t for _, t, _ in rows], [e for _, _, e in rows])
        self._enqueue_products(on, 0, n)
        tr = self.read_trace(n, events=events_out)
        for p, size, _ in on.values():
            setattr(tr, p.field, getattr(self, p.read)(*(() if p.enqueue else (size,)), n))
        return tr

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

        `forecast` (True, or a callable giving random-walk steps, see the forecast's row of `BURST_PRODUCTS`; needs
        `reset_forecast`): every burst's draws are forecast on the device right behind its summary and the forecast
        marginals cross with the trace (`trace.forecast`).

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
        on = self._burst_products(locals())                 # first statement: the locals are this call's keywords
        from concurrent.futures import ThreadPoolExecutor
        burst, num_bursts = int(burst), int(num_bursts)
        if 2 * burst > self.cap:
            raise ValueError(f"sample_bursts needs trace_capacity >= 2 * burst = {2 * burst}, have {self.cap}")
        # page-locking GBs of host memory takes tenths of a second: the two buffers are kept for the next call, until the
        # burst, `events` or the size of a product changes
        sizes = {field: size for field, (_, size, _) in on.items()}
        key = (burst, bool(events)) + tuple(sizes.items())
        if getattr(self, "_pinned_key", None) != key:
            for bf in getattr(self, "_pinned", []):
                bf.close()
            self._pinned = [PinnedTrace(self, burst, events, **sizes), PinnedTrace(self, burst, events, **sizes)]
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
                            self._enqueue_products(on, h * burst, burst, marks[i] if marks and i in marks else None)
                        if prev >= 0:
                            self.trace_wait()                    # burst prev has landed (it crossed while burst i ran)
                            futs[prev & 1] = pool.submit(consume, self.trace_view(bufs[prev & 1], burst), prev)
                            prev = -1
                            self._burst_ok()
                        if i < num_bursts:
                            self.read_trace_async(burst, h * burst, bufs[h])
                            for p, size, _ in on.values():
                                getattr(self, p.read_async)(*(() if p.enqueue else (size,)), burst, h * burst, bufs[h])
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
        on = self._burst_products(locals())                 # first statement: the locals are this call's keywords
        if num_sweeps > self.cap:
            raise ValueError(f"num_sweeps={num_sweeps} exceeds trace_capacity={self.cap}")
        while True:
            if self.auto_recover:
                self.snapshot(0)
            self.reset_trace()
            self.run(num_sweeps * self._thin)
            try:
                self._enqueue_products(on, 0, num_sweeps)
                tr = self.read_trace(num_sweeps, events=events)
                for p, size, _ in on.values():
                    setattr(tr, p.field, getattr(self, p.read)(*(() if p.enqueue else (size,)), num_sweeps))
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

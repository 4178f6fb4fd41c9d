"""Scenario forecasts: the specification of what-if rollouts, the NumPy restatement of the paired differences and their
fold (csrc/scenario_kernels.h and csrc/scenario_update.h hold THE definition), and the statistics the host forms from the
integers.

A scenario is the forecast's rollout of a draw with `log_shift[s]` added to the log baseline of forecast day s and the
commuting volume of that day multiplied by `commute[s]`; state, parameters and random numbers stay the forecast's, so the
difference of a draw's two rollouts is free of the noise that two independent rollouts would carry.  In terms of the
simulator, per chain:

    SeirModel.simulate(par, a_path + log_shift[k], spatial, W * commute[k], wd, st0, seed, first_draw_id)

gives scenario k's counts where the same call with `a_path` and `W` gives the baseline's.

A TARGETED scenario (csrc/scenario_local_kernels.h) has the two operands per location: `log_shift[k][m][s]` is added to the log
baseline of location m's hazard and `commute[k][m][s]` multiplies the commuting-borne pressure ON location m (the psi W F
term of its hazard; what m exports is not scaled).  A scenario body may carry `locations:` (a non-empty list of members in
`posterior.groups`' forms: code, prefix pattern "E0*", integer index) or `parts:`, a list of bodies {locations,
transmission, commute, from_day}; a part without `locations` applies everywhere.  The multipliers start at 1.0 [M, H]; each
part multiplies its locations from its `from_day` on, in list order, in float64; log_shift = np.log of the product.
`local_inputs` is the simulator's view.  A spec in which no scenario has `locations` or `parts` resolves exactly as before."""
from __future__ import annotations

import dataclasses
import math
from collections.abc import Mapping

import numpy as np

MAX_SCENARIOS = 4                   # SEIR_SCENARIO_MAX
Q = 4                               # SEIR_SCENARIO_Q
QUANTITIES = ("cases", "cum_cases", "prevalence", "cum_infections")
_KEYS = ("transmission", "commute", "from_day")
_PART_KEYS = _KEYS + ("locations",)


# ---- the specification ------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Scenarios:
    """A resolved specification: K names, and per scenario and forecast day the shift of the log baseline and the multiplier
    of the commuting volume, both float64 [K, H] (read-only).  K = 0: off."""
    names: tuple = ()
    horizon: int = 0
    log_shift: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros((0, 0)))
    commute: np.ndarray = dataclasses.field(default_factory=lambda: np.ones((0, 0)))

    @property
    def K(self):
        return len(self.names)

    def __bool__(self):
        return bool(self.names)


@dataclasses.dataclass(frozen=True)
class LocalScenarios(Scenarios):
    """A resolved specification with a targeted scenario in it: `log_shift` and `commute` float64 [K, M, H] (read-only), and
    `locations` uint8 [K, M], 1 where any multiplier of the row differs from the identity."""
    locations: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros((0, 0), np.uint8))


@dataclasses.dataclass(frozen=True)
class PendingScenarios:
    """Stage one of a specification with `locations` or `parts`: every key, value, from_day and list length is checked, the
    members are not yet rows.  `parts[k]` is a list of (members or None, transmission [H], commute [H]) with the days before
    the part's from_day already at 1.  `resolve_locations` makes a `LocalScenarios` of it once M and the codes are known."""
    names: tuple
    horizon: int
    parts: tuple

    @property
    def K(self):
        return len(self.names)

    def __bool__(self):
        return bool(self.names)


def is_local(sc):
    """`sc` carries per-location operands (or will, once its members are resolved)."""
    return isinstance(sc, (LocalScenarios, PendingScenarios))


def is_off(spec):
    return spec is None or spec is False or (isinstance(spec, str) and spec.lower() == "off") or (isinstance(spec, Mapping) and not spec)


def _multipliers(name, key, v, H, positive):
    """A scalar or a list of H numbers as float64 [H]: finite, > 0 (`positive`) or >= 0."""
    bound = "> 0" if positive else ">= 0"
    if isinstance(v, (list, tuple, np.ndarray)):
        if len(v) != H:
            raise ValueError(f"scenarios: {name}.{key} has {len(v)} values, the forecast has {H} days")
        seq = list(v)
    else:
        seq = [v] * H
    out = np.empty(H, dtype=np.float64)
    for s, x in enumerate(seq):
        if isinstance(x, (bool, str)) or not isinstance(x, (int, float, np.integer, np.floating)):
            raise ValueError(f"scenarios: {name}.{key}={x!r}: a number {bound}, or {H} of them")
        x = float(x)
        if not math.isfinite(x) or x < 0.0 or (positive and x == 0.0):
            raise ValueError(f"scenarios: {name}.{key}={x!r} on day {s}: the multiplier is finite and {bound}")
        out[s] = x
    return out


def parse_scenarios(spec, horizon):
    """`Mcmc.scenarios` -- {name: {transmission: f | [H floats], commute: f | [H floats], from_day: d}} -- against the
    forecast's horizon H, as a `Scenarios`.  The multipliers are > 0 (transmission; log_shift = log of it) and >= 0 (commute);
    days before `from_day` keep 1.  Refused: scenarios without a forecast, more than MAX_SCENARIOS, an empty or repeated
    name, an unknown key, a list whose length is not H, a non-finite or out-of-range value, from_day outside [0, H)."""
    if is_off(spec):
        return Scenarios()
    H = int(horizon or 0)
    if H < 1:
        raise ValueError("scenarios given without forecast: they ride on the forecast's rollout")
    if isinstance(spec, Mapping):
        items = list(spec.items())
    elif isinstance(spec, (list, tuple)) and all(isinstance(e, (list, tuple)) and len(e) == 2 for e in spec):
        items = [tuple(e) for e in spec]                     # pairs: the one form that can carry a repeated name
    else:
        raise ValueError(f"scenarios={spec!r}: a mapping name -> {{transmission, commute, from_day}}")
    if len(items) > MAX_SCENARIOS:
        raise ValueError(f"scenarios: {len(items)} given, at most {MAX_SCENARIOS} ride on one forecast")
    if any(isinstance(body, Mapping) and ("locations" in body or "parts" in body) for _, body in items):
        return _parse_local(items, H)
    names, shifts, commutes = [], [], []
    for name, body in items:
        name = "" if name is None else str(name).strip()
        if not name:
            raise ValueError("scenarios: a scenario's name is empty")
        if name in names:
            raise ValueError(f"scenarios: the name {name!r} is given twice")
        body = {} if body is None else body
        if not isinstance(body, Mapping) or set(body) - set(_KEYS):
            raise ValueError(f"scenarios: {name}: a mapping with the keys {', '.join(_KEYS)}")
        d = body.get("from_day", 0)
        if isinstance(d, bool) or not isinstance(d, (int, np.integer)) or not 0 <= int(d) < H:
            raise ValueError(f"scenarios: {name}.from_day={d!r}: a forecast day in [0, {H})")
        tr = _multipliers(name, "transmission", body.get("transmission", 1.0), H, True)
        cm = _multipliers(name, "commute", body.get("commute", 1.0), H, False)
        tr[:int(d)] = 1.0
        cm[:int(d)] = 1.0
        names.append(name)
        shifts.append(np.log(tr))
        commutes.append(cm)
    ls, cm = np.array(shifts, dtype=np.float64), np.array(commutes, dtype=np.float64)
    ls.setflags(write=False)
    cm.setflags(write=False)
    return Scenarios(tuple(names), H, ls, cm)


def _name(name, names):
    name = "" if name is None else str(name).strip()
    if not name:
        raise ValueError("scenarios: a scenario's name is empty")
    if name in names:
        raise ValueError(f"scenarios: the name {name!r} is given twice")
    return name


def _part(name, body, H):
    """One body {locations, transmission, commute, from_day} as (members or None, transmission [H], commute [H])."""
    body = {} if body is None else body
    if not isinstance(body, Mapping) or set(body) - set(_PART_KEYS):
        raise ValueError(f"scenarios: {name}: a mapping with the keys {', '.join(_PART_KEYS)}")
    d = body.get("from_day", 0)
    if isinstance(d, bool) or not isinstance(d, (int, np.integer)) or not 0 <= int(d) < H:
        raise ValueError(f"scenarios: {name}.from_day={d!r}: a forecast day in [0, {H})")
    tr = _multipliers(name, "transmission", body.get("transmission", 1.0), H, True)
    cm = _multipliers(name, "commute", body.get("commute", 1.0), H, False)
    tr[:int(d)] = 1.0
    cm[:int(d)] = 1.0
    members = None
    if "locations" in body:
        loc = body["locations"]
        if not isinstance(loc, (list, tuple)) or not loc or \
                any(isinstance(x, bool) or not isinstance(x, (str, int, np.integer)) for x in loc):
            raise ValueError(f"scenarios: {name}.locations={loc!r}: a non-empty list of location codes, prefix patterns or indices")
        members = tuple(loc)
    return members, tr, cm


def _parse_local(items, H):
    """Stage one of a specification in which some scenario has `locations` or `parts`."""
    names, parts = [], []
    for name, body in items:
        name = _name(name, names)
        body = {} if body is None else body
        if isinstance(body, Mapping) and "parts" in body:
            if set(body) - {"parts"}:
                raise ValueError(f"scenarios: {name}: a scenario with parts carries nothing else; every part has its own "
                                 f"{', '.join(_PART_KEYS)}")
            if not isinstance(body["parts"], (list, tuple)) or not body["parts"]:
                raise ValueError(f"scenarios: {name}.parts: a non-empty list of mappings with the keys {', '.join(_PART_KEYS)}")
            parts.append(tuple(_part(f"{name}.parts[{i}]", p, H) for i, p in enumerate(body["parts"])))
        else:
            parts.append((_part(name, body, H),))
        names.append(name)
    return PendingScenarios(tuple(names), H, tuple(parts))


def resolve_locations(sc, M, location_names=None):
    """Stage two: the members of a `PendingScenarios` to rows by `posterior.groups`' resolver, and the parts composed into
    [K, M, H] operands.  Refused (ValueError): an unknown code, a pattern that matches nothing, an index outside [0, M).
    Anything else -- a `Scenarios` as before, or one already resolved -- is returned as it is."""
    if not isinstance(sc, PendingScenarios):
        return sc
    from . import groups as G
    M, H = int(M), sc.horizon
    tr_all, cm_all = np.ones((sc.K, M, H)), np.ones((sc.K, M, H))
    for k, name in enumerate(sc.names):
        for members, tr, cm in sc.parts[k]:
            if members is None:
                rows = slice(None)
            else:
                try:
                    rows = G.parse_groups({name: list(members)}, M, location_names).members
                except ValueError as e:
                    raise ValueError(f"scenarios: {name}.locations: {e}") from None
            tr_all[k, rows] *= tr
            cm_all[k, rows] *= cm
    loc = ((tr_all != 1.0) | (cm_all != 1.0)).any(axis=2).astype(np.uint8)
    ls = np.log(tr_all)
    for a in (ls, cm_all, loc):
        a.setflags(write=False)
    return LocalScenarios(sc.names, H, ls, cm_all, loc)


def load_spec(path):
    """The mapping of a `--scenarios FILE.yaml`: the file's `scenarios` key, or the whole file when it has none."""
    import yaml
    with open(path, "r") as f:
        doc = yaml.safe_load(f)
    return doc["scenarios"] if isinstance(doc, Mapping) and "scenarios" in doc else doc


def scenario_inputs(a_path, W, sc, k):
    """The simulator's inputs of scenario k from the baseline's: (a_path [.., H] + log_shift[k], W [H] * commute[k]), one
    rounded add and one rounded multiply."""
    return np.asarray(a_path, dtype=np.float64) + sc.log_shift[k], np.asarray(W, dtype=np.float64) * sc.commute[k]


def local_inputs(a_path, W, sc, k):
    """The simulator's per-location inputs of targeted scenario k from the baseline's: (a_path [.., H] -> [.., M, H] +
    log_shift[k] [M, H], W [H] * commute[k] [M, H]), one rounded add and one rounded multiply per location and day."""
    return (np.asarray(a_path, dtype=np.float64)[..., None, :] + sc.log_shift[k],
            np.asarray(W, dtype=np.float64) * sc.commute[k])


# ---- the differences and their fold -----------------------------------------------------------------------------------
def differences(base_events, scenario_events):
    """The four paired differences of every draw and cell: `base_events` and `scenario_events` integer [..., H, 3] (k_se,
    k_ei, k_ir over the forecast days), the result int64 [..., H, 4] in the order of QUANTITIES:
        cases = d_ir, cum_cases = its inclusive scan over the days, prevalence = exclusive scan of d_ei minus that of d_ir (I
        at the start of the day; day 0 is 0), cum_infections = inclusive scan of d_se, with d = scenario - baseline."""
    d = np.asarray(scenario_events, dtype=np.int64) - np.asarray(base_events, dtype=np.int64)
    inc = np.cumsum(d, axis=-2)
    ex = inc - d
    return np.stack([d[..., 2], inc[..., 2], ex[..., 1] - ex[..., 2], inc[..., 0]], axis=-1)


def fold_differences(base_events, scenario_events, acc=None):
    """The device's fold in NumPy: events [n, B, M, H, 3], n draws per chain; `acc` what an earlier call returned or None.
    Returns `count`, `ref` int32 (the first draw's values), `sum` int64 and `sumsq` uint64 of the values minus ref, `lt` and
    `eq` uint32 (draws whose difference is < 0 / == 0), each [B, M, H, 4], and `overflow` (some sumsq reached 2^63)."""
    v = differences(base_events, scenario_events)
    if v.ndim != 5:
        raise ValueError(f"events {np.shape(base_events)}: need [n, B, M, H, 3]")
    if v.size and (v.min() < -2 ** 31 or v.max() >= 2 ** 31):
        raise ValueError("a difference does not fit int32: the counts are not those of populations below 2^31")
    n = v.shape[0]
    if acc is None:
        if n == 0:
            raise ValueError("no draw to take ref from")
        count, ref = 0, v[0].astype(np.int32)
        zero = np.zeros(v.shape[1:], dtype=np.int64)
        sm, sq, lt, eq, ovf = zero.copy(), zero.astype(np.uint64), zero.astype(np.uint32), zero.astype(np.uint32), False
    else:
        count, ref, sm, sq = int(acc["count"]), np.asarray(acc["ref"], np.int32), np.array(acc["sum"], np.int64), np.array(acc["sumsq"], np.uint64)
        lt, eq, ovf = np.array(acc["lt"], np.uint32), np.array(acc["eq"], np.uint32), bool(acc["overflow"])
    dev = v - ref.astype(np.int64)                           # |dev| < 2^32
    # draw by draw, since the flag is the device's test after every draw (summary_fold): 2^63 reached, or wrapped
    a = np.abs(dev).astype(np.uint64)
    for j in range(n):
        before = sq
        sq = before + a[j] * a[j]                            # wraps mod 2^64 as the device's does
        ovf = ovf or bool(np.any(sq >= np.uint64(1 << 63)) or np.any(sq < before))
    with np.errstate(over="ignore"):
        sm = (sm.astype(np.uint64) + dev.astype(np.uint64).sum(axis=0, dtype=np.uint64)).astype(np.int64)
    lt = lt + (v < 0).sum(axis=0).astype(np.uint32)
    eq = eq + (v == 0).sum(axis=0).astype(np.uint32)
    return dict(count=count + n, ref=ref, sum=sm, sumsq=sq, lt=lt, eq=eq, overflow=ovf)


# ---- the statistics ---------------------------------------------------------------------------------------------------
def statistics(count, ref, sum, sumsq, lt, eq):                                         # noqa: A002 - the accumulators' names
    """mean = ref + sum / n, var = (sumsq - sum^2 / n) / (n - 1) (NaN, without a warning, for one draw), p_below = lt / n,
    p_equal = eq / n, as float64 arrays of the accumulators' shape -- the summaries' formulas (`sampler.summary_var`): the
    shift by ref keeps sum and sumsq small, so the subtraction cancels little."""
    n = int(count)
    if n < 1:
        raise ValueError("no draw has been folded")
    s1, s2 = np.asarray(sum, dtype=np.float64), np.asarray(sumsq, dtype=np.float64)
    mean = np.asarray(ref, dtype=np.float64) + s1 / n
    var = (s2 - s1 * s1 / n) / (n - 1.0) if n > 1 else np.full(s1.shape, np.nan)
    return dict(mean=mean, var=var, p_below=np.asarray(lt, dtype=np.float64) / n, p_equal=np.asarray(eq, dtype=np.float64) / n)


def run_line(name, diff_by_day, probs=(0.05, 0.95)):
    """The log's line of one scenario: national cumulative cases at the last forecast day minus the baseline's, over the
    draws -- `diff_by_day` [n, H, 3], scenario minus baseline events by day -- as mean and the two quantiles."""
    cum = np.asarray(diff_by_day, dtype=np.float64)[..., 2].sum(axis=-1)
    lo, hi = np.quantile(cum, probs)
    return (f"Scenario {name}: cumulative cases at day {np.shape(diff_by_day)[-2] - 1} minus the baseline's: mean {cum.mean():.1f}, "
            f"{probs[0]:g} / {probs[1]:g} quantiles {lo:.1f} / {hi:.1f} over {cum.size} draws")


def group_run_line(name, group, diff_by_group, probs=(0.05, 0.95)):
    """The log's line of one scenario and one group of locations: the group's cumulative cases at the last forecast day minus
    the baseline's, over the draws -- `diff_by_group` [n, H, 3], the scenario's totals over the group minus the forecast's."""
    cum = np.asarray(diff_by_group, dtype=np.float64)[..., 2].sum(axis=-1)
    lo, hi = np.quantile(cum, probs)
    return (f"Scenario {name}, group {group}: cumulative cases at day {np.shape(diff_by_group)[-2] - 1} minus the baseline's: mean "
            f"{cum.mean():.1f}, {probs[0]:g} / {probs[1]:g} quantiles {lo:.1f} / {hi:.1f} over {cum.size} draws")

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
`local_inputs` is the simulator's view.  A spec in which no scenario has `locations` or `parts` resolves exactly as before.

A TRIGGERED scenario (csrc/scenario_trigger_kernels.h, csrc/trigger_update.h) is a targeted scenario with two operand pairs and
a rule on the draw's own simulated case counts that picks one of them per draw, location and day.  A scenario body may carry
    trigger: {cases_per_100k | cases, release_per_100k | release, window, min_days, review_every, from_day, locations}
    then:    {transmission, commute}
The body's ordinary keys give the off pair as before; `then` multiplies the off pair's multipliers in float64 on every day, which
gives the on pair.  Exactly one of `cases_per_100k` / `cases` (the threshold on the sum of a location's I->R counts over the last
`window` days); `release*` in the same form (default: the `on` value), window 7, min_days 0, review_every 1, from_day 0.
`trigger.locations` names the locations that may trigger, in `groups`' member forms; the others get on = INT32_MAX, as do all
locations of a scenario without a trigger, whose on pair is its off pair.  A per-100k value becomes the count
ceil(rate * N[m] / 1e5), the exact ceiling of the product of the numbers as given (`resolve_locations` with `populations`).
`trigger_states` is THE rule in NumPy, `triggered_inputs` the simulator's view of the two pairs, `fold_triggers` the fold of the
rule's record.  A spec without `trigger:` resolves exactly as before."""
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
_RULE_KEYS = ("trigger", "then")
_TRIGGER_KEYS = ("cases_per_100k", "release_per_100k", "cases", "release", "window", "min_days", "review_every", "from_day", "locations")
_THEN_KEYS = ("transmission", "commute")
TRIGGER_MAX_WINDOW = 28             # SEIR_TRIGGER_MAX_WINDOW
INT32_MAX = 2 ** 31 - 1             # on = INT32_MAX: the location never triggers


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
class TriggerRule:
    """One scenario's parsed `trigger:`: `per_100k` says which form `on` and `off` are in (a rate, or absolute counts);
    `members` who may trigger (None: every location)."""
    per_100k: bool
    on: float
    off: float
    window: int = 7
    from_day: int = 0
    min_days: int = 0
    review_every: int = 1
    members: tuple = None


@dataclasses.dataclass(frozen=True)
class TriggeredScenarios(LocalScenarios):
    """A resolved specification with a triggered scenario in it: `log_shift`, `commute` are the off pair, `log_shift_on`,
    `commute_on` the on pair, all float64 [K, M, H]; `trigger_on`, `trigger_off` int32 [K, M] (on = INT32_MAX: never);
    `window`, `from_day`, `min_days`, `review_every` int32 [K]; `triggered` uint8 [K], 1 where the scenario has a rule."""
    log_shift_on: np.ndarray = None
    commute_on: np.ndarray = None
    trigger_on: np.ndarray = None
    trigger_off: np.ndarray = None
    window: np.ndarray = None
    from_day: np.ndarray = None
    min_days: np.ndarray = None
    review_every: np.ndarray = None
    triggered: np.ndarray = None

    def trigger_args(self):
        """What `ChainSampler.set_scenarios(log_shift, commute, cap, triggers=...)` takes."""
        return dict(log_shift_on=self.log_shift_on, commute_on=self.commute_on, on=self.trigger_on, off=self.trigger_off,
                    window=self.window, from_day=self.from_day, min_days=self.min_days, review_every=self.review_every)


def is_triggered(sc):
    """`sc` carries a rule (or will, once its members and thresholds are resolved)."""
    return isinstance(sc, TriggeredScenarios) or (isinstance(sc, PendingScenarios) and any(r is not None for r in sc.rules))


@dataclasses.dataclass(frozen=True)
class PendingScenarios:
    """Stage one of a specification with `locations` or `parts`: every key, value, from_day and list length is checked, the
    members are not yet rows.  `parts[k]` is a list of (members or None, transmission [H], commute [H]) with the days before
    the part's from_day already at 1.  `resolve_locations` makes a `LocalScenarios` of it once M and the codes are known."""
    names: tuple
    horizon: int
    parts: tuple
    # with a `trigger:` on any scenario: per scenario a TriggerRule or None, and the `then:` multipliers (transmission [H],
    # commute [H]) or None; empty without one
    rules: tuple = ()
    then: tuple = ()

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
    if any(isinstance(body, Mapping) and ("locations" in body or "parts" in body or "trigger" in body or "then" in body)
           for _, body in items):
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


def _integer(name, key, v, lo, hi, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"scenarios: {name}.trigger.{key}={v!r}: {what}")
    return int(v)


def _trigger(name, body, H):
    """A scenario's `trigger:` mapping as a TriggerRule: every key, value and default, release <= on."""
    if not isinstance(body, Mapping) or set(body) - set(_TRIGGER_KEYS):
        raise ValueError(f"scenarios: {name}.trigger: a mapping with the keys {', '.join(_TRIGGER_KEYS)}")
    if ("cases_per_100k" in body) == ("cases" in body):
        raise ValueError(f"scenarios: {name}.trigger: exactly one of cases_per_100k and cases")
    per = "cases_per_100k" in body
    on_key, off_key = ("cases_per_100k", "release_per_100k") if per else ("cases", "release")
    other = "release" if per else "release_per_100k"
    if other in body:
        raise ValueError(f"scenarios: {name}.trigger.{other}: the release threshold takes the form of the trigger's, {off_key}")
    vals = {}
    for key in (on_key, off_key):
        v = body.get(key, vals.get(on_key))
        if per:
            if isinstance(v, (bool, str)) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)) \
                    or float(v) < 0.0:
                raise ValueError(f"scenarios: {name}.trigger.{key}={v!r}: a finite rate >= 0")
            vals[key] = float(v)
        else:
            vals[key] = _integer(name, key, v, 0, INT32_MAX, f"a count in [0, {INT32_MAX}]")
    if vals[off_key] > vals[on_key]:
        raise ValueError(f"scenarios: {name}.trigger.{off_key}={vals[off_key]!r} is above {on_key}={vals[on_key]!r}: a measure is "
                         "released below the level that triggers it")
    members = None
    if "locations" in body:
        loc = body["locations"]
        if not isinstance(loc, (list, tuple)) or not loc or \
                any(isinstance(x, bool) or not isinstance(x, (str, int, np.integer)) for x in loc):
            raise ValueError(f"scenarios: {name}.trigger.locations={loc!r}: a non-empty list of location codes, prefix patterns or "
                             "indices")
        members = tuple(loc)
    return TriggerRule(per, vals[on_key], vals[off_key],
                       _integer(name, "window", body.get("window", 7), 1, TRIGGER_MAX_WINDOW, f"days in [1, {TRIGGER_MAX_WINDOW}]"),
                       _integer(name, "from_day", body.get("from_day", 0), 0, H, f"a forecast day in [0, {H}]"),
                       _integer(name, "min_days", body.get("min_days", 0), 0, INT32_MAX, "days >= 0"),
                       _integer(name, "review_every", body.get("review_every", 1), 1, INT32_MAX, "days >= 1"), members)


def _then(name, body, H):
    if not isinstance(body, Mapping) or set(body) - set(_THEN_KEYS):
        raise ValueError(f"scenarios: {name}.then: a mapping with the keys {', '.join(_THEN_KEYS)}")
    return (_multipliers(f"{name}.then", "transmission", body.get("transmission", 1.0), H, True),
            _multipliers(f"{name}.then", "commute", body.get("commute", 1.0), H, False))


def _parse_local(items, H):
    """Stage one of a specification in which some scenario has `locations`, `parts` or `trigger`."""
    names, parts, rules, then = [], [], [], []
    for name, body in items:
        name = _name(name, names)
        body = {} if body is None else body
        rule = mult = None
        if isinstance(body, Mapping) and (set(body) & set(_RULE_KEYS)):
            if "trigger" not in body:
                raise ValueError(f"scenarios: {name}.then without {name}.trigger: `then` is what a triggered measure does")
            rule = _trigger(name, body["trigger"], H)
            mult = _then(name, body.get("then", {}), H)
            body = {k: v for k, v in body.items() if k not in _RULE_KEYS}
        rules.append(rule)
        then.append(mult)
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
    if all(r is None for r in rules):
        return PendingScenarios(tuple(names), H, tuple(parts))
    return PendingScenarios(tuple(names), H, tuple(parts), tuple(rules), tuple(then))


def threshold_counts(rate, populations):
    """A per-100k rate as counts per location: ceil(rate * N[m] / 1e5), the exact ceiling of the product of the numbers as they
    are given (a float is the rational it holds), as Python ints."""
    from fractions import Fraction
    r = Fraction(float(rate))
    return [math.ceil(r * Fraction(float(n)) / 100000) for n in np.asarray(populations, dtype=np.float64).reshape(-1)]


def resolve_locations(sc, M, location_names=None, populations=None):
    """Stage two: the members of a `PendingScenarios` to rows by `posterior.groups`' resolver, and the parts composed into
    [K, M, H] operands.  Refused (ValueError): an unknown code, a pattern that matches nothing, an index outside [0, M).
    Anything else -- a `Scenarios` as before, or one already resolved -- is returned as it is.
    With a rule on any scenario the result is a `TriggeredScenarios`: `populations` [M] turns per-100k thresholds into counts
    (refused above INT32_MAX, and when a rate is given without populations)."""
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
    if not sc.rules:
        return LocalScenarios(sc.names, H, ls, cm_all, loc)
    tr_on, cm_on = tr_all.copy(), cm_all.copy()
    on, off = np.full((sc.K, M), INT32_MAX, np.int64), np.zeros((sc.K, M), np.int64)
    par = np.tile(np.array([7, 0, 0, 1], np.int32), (sc.K, 1))
    for k, (name, rule) in enumerate(zip(sc.names, sc.rules)):
        if rule is None:
            continue
        tr_on[k] *= sc.then[k][0]
        cm_on[k] *= sc.then[k][1]
        par[k] = (rule.window, rule.from_day, rule.min_days, rule.review_every)
        rows = np.arange(M)
        if rule.members is not None:
            try:
                rows = np.asarray(G.parse_groups({name: list(rule.members)}, M, location_names).members)
            except ValueError as e:
                raise ValueError(f"scenarios: {name}.trigger.locations: {e}") from None
        if rule.per_100k:
            if populations is None or np.size(populations) != M:
                raise ValueError(f"scenarios: {name}.trigger: per-100k thresholds need the {M} populations")
            hi, lo = threshold_counts(rule.on, populations), threshold_counts(rule.off, populations)
        else:
            hi, lo = [int(rule.on)] * M, [int(rule.off)] * M
        for m in rows:
            if hi[m] > INT32_MAX:
                raise ValueError(f"scenarios: {name}.trigger: the threshold of location {m} is {hi[m]} cases, above {INT32_MAX}")
            on[k, m], off[k, m] = hi[m], lo[m]
    out = [np.log(tr_on), cm_on, on.astype(np.int32), off.astype(np.int32)] + [np.ascontiguousarray(par[:, i]) for i in range(4)] + \
        [np.array([r is not None for r in sc.rules], np.uint8)]
    for a in out:
        a.setflags(write=False)
    return TriggeredScenarios(sc.names, H, ls, cm_all, loc, *out)


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


def triggered_inputs(a_path, W, sc, k):
    """The simulator's per-location inputs of triggered scenario k under its two pairs: ((a_off, W_off), (a_on, W_on)), each as
    `local_inputs` gives them -- one rounded add and one rounded multiply per location and day, either way."""
    a, W = np.asarray(a_path, dtype=np.float64)[..., None, :], np.asarray(W, dtype=np.float64)
    return (a + sc.log_shift[k], W * sc.commute[k]), (a + sc.log_shift_on[k], W * sc.commute_on[k])


# ---- the rule ---------------------------------------------------------------------------------------------------------
def trigger_states(history, cases, on, off, window, from_day, min_days, review_every):
    """THE rule in NumPy (csrc/trigger_update.h), a day loop vectorised over the rest: `cases` integer [.., H], the I->R counts
    of the rollout days; `history` [.., h], the counts of the h days before day 0 of the rollout, oldest first (the last
    `window` of them count; a shorter history is preceded by zeros); `on`, `off` broadcast against the leading axes.  Returns
    `active` uint8 [.., H]: 1 where day s is rolled under the measure.
        c = the sum of the `window` days before day s;  review = s >= from_day and (s - from_day) % review_every == 0
        on a review: not active and c >= on: active <- 1, age <- 0; otherwise active and age >= min_days and c < off: active <- 0
        behind the day, if active: age <- age + 1"""
    cases = np.asarray(cases, dtype=np.int64)
    lead, H, w = cases.shape[:-1], cases.shape[-1], int(window)
    hist = np.asarray(history, dtype=np.int64)
    hist = np.broadcast_to(hist, lead + hist.shape[-1:])[..., max(hist.shape[-1] - w, 0):]
    series = np.concatenate([np.zeros(lead + (w - hist.shape[-1],), np.int64), hist, cases], axis=-1)   # day s is index w + s
    on, off = np.broadcast_to(np.asarray(on, np.int64), lead), np.broadcast_to(np.asarray(off, np.int64), lead)
    active, age = np.zeros(lead, dtype=bool), np.zeros(lead, dtype=np.int64)
    out = np.zeros(lead + (H,), dtype=np.uint8)
    c = series[..., :w].sum(axis=-1)
    for s in range(H):
        if s >= from_day and (s - from_day) % review_every == 0:
            fire = ~active & (c >= on)
            release = active & (age >= min_days) & (c < off)
            age = np.where(fire, 0, age)
            active = (active | fire) & ~release
        out[..., s] = active
        age = age + active
        c = c + series[..., w + s] - series[..., s]
    return out


def trigger_masks(active):
    """`active` [.., H] (H <= 128) as the device's record: uint64 [.., 2], bit s of the 128 set iff active on day s."""
    a = np.asarray(active).astype(bool)
    H = a.shape[-1]
    out = np.zeros(a.shape[:-1] + (2,), dtype=np.uint64)
    for s in range(H):
        out[..., s >> 6] |= a[..., s].astype(np.uint64) << np.uint64(s & 63)
    return out


def fold_triggers(masks, H, acc=None):
    """The device's fold of the record in NumPy bit operations: `masks` uint64 [n, B, M, 2]; returns `count`, `active_count`
    uint32 [B, M, H] (plus `acc`'s) and `active_by_day` int32 [n, B, H]."""
    mk = np.asarray(masks, dtype=np.uint64)
    bits = np.stack([(mk[..., s >> 6] >> np.uint64(s & 63)) & np.uint64(1) for s in range(H)], axis=-1)   # [n, B, M, H]
    cnt = bits.sum(axis=0).astype(np.uint32)
    if acc is not None:
        cnt = cnt + np.asarray(acc["active_count"], np.uint32)
    return dict(count=mk.shape[0] + (0 if acc is None else int(acc["count"])), active_count=cnt,
                active_by_day=bits.sum(axis=2).astype(np.int32))


def trigger_run_line(name, active_by_day):
    """The log's line of one triggered scenario: `active_by_day` [n, H], the locations under the measure per draw and day."""
    a = np.asarray(active_by_day, dtype=np.int64)
    any_ = a.any(axis=-1)
    first = np.argmax(a > 0, axis=-1)[any_]
    return (f"Scenario {name}: the measure triggers somewhere in {any_.mean():.3f} of {a.shape[0]} draws, mean location-days under "
            f"it {a.sum(axis=-1).mean():.1f}, mean first day " + (f"{first.mean():.1f}" if first.size else "none"))


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

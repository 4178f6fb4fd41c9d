"""The product options of a run (Mcmc.thin, summaries, diagnostics, forecast, rt, check, within_between, their quantiles,
the groups): parsed, refused and declared on the command line here and nowhere else.  `resolve_products` turns an Mcmc
section and the command line's overrides into the canonical section and a `Products`, once, before the data file is opened;
`Products.bind` then holds them against the data (the group table, the windows against T), still before any GPU call.
`inference.mcmc`, `inference.product_records` and `posterior.replay.replay_files` read the `Products` and parse nothing."""
from __future__ import annotations

import dataclasses

import numpy as np

from .. import _lib
from ..posterior import groups as G_mod
from ..posterior.quantiles import parse_probs

SUMMARIES = ("off", "on", "only")
DIAGNOSTICS = ("off", "on")


# ---- one parser per kind of option ----------------------------------------------------------------------------------
def _day_count(name, noun, v, bound=None, T=None, series=True):
    """A number of days, or off (None, False, "off": 0): an int, a numpy integer or a digit string, 1 <= days, days <=
    `bound` (the option's fixed upper bound, if any) and days <= T when the length of the series is given.  `noun` is what
    the message calls it; `series=False`: the days lie behind the series and T does not bound them."""
    if v is None or v is False or (isinstance(v, str) and v.lower() == "off"):
        return 0
    def upper(t):                                           # the upper end as the messages write it
        return str(bound) if not series else t if bound is None else f"min({t}, {bound})"
    if isinstance(v, bool) or (not isinstance(v, (int, np.integer)) and not (isinstance(v, str) and v.strip().lstrip("+-").isdigit())):
        raise ValueError(f"{name}={v!r}: the {noun} is a number of days, 1 .. {upper('T')}")
    days = int(v)
    if days < 1 or (bound is not None and days > bound) or (T is not None and days > int(T)):
        raise ValueError(f"{name}={days}: the {noun} is 1 .. {upper('T' if T is None else f'T = {int(T)}')} days")
    return days


def _choice(name, value, choices):
    """One of `choices`; YAML reads a bare `on` / `off` as a boolean."""
    if value is False or value is True:
        value = "on" if value else "off"
    if value not in choices:
        raise ValueError(f"{name}={value!r}: choose one of {', '.join(choices)}")
    return value


def _quantiles(key, product, config, override, on):
    """Mcmc.<key> (absent: off) or the command line's: 1 to 8 probabilities in [0, 1], strictly increasing (`parse_probs`);
    () for off.  With `on` given (0: `product` is off) quantiles without their product are refused."""
    probs = parse_probs(config.get(key) if override is None else override, name=key)
    if probs and on is not None and not on:
        raise ValueError(f"{key} given without {product}: it would have no effect")
    return probs


def thin_interval(config, override=None):
    """Mcmc.thin ("Thin MCMC samples every 'thin' iterations", example_config.yaml:33; absent: 1), or the command line's
    `--thin`.  Anything below 1 is refused -- here, before a sampler exists."""
    thin = int(config.get("thin", 1) if override is None else override)
    if thin < 1:
        raise ValueError(f"thin={thin}: the thinning interval is >= 1 (1 keeps every draw)")
    return thin


def summaries_mode(config, override=None):
    """Mcmc.summaries (absent: "off"), or the command line's `--summaries`: "on" adds the device-side summaries of the
    latent epidemic to the output, "only" also keeps the event tensors on the device.  Anything else is refused."""
    return _choice("summaries", config.get("summaries", "off") if override is None else override, SUMMARIES)


def diagnostics_mode(config, override=None, batch=None):
    """Mcmc.diagnostics (absent: "off") and Mcmc.diagnostics_batch, or `--diagnostics` / `--diagnostics-batch`: (mode, batch
    length).  With "on" the batch length defaults to num_burst_samples (one burst is one batch) and must divide it or be a
    multiple of it, and the run needs two bursts for its two halves; a batch length given with "off" is refused."""
    mode = _choice("diagnostics", config.get("diagnostics", "off") if override is None else override, DIAGNOSTICS)
    if batch is None:
        batch = config.get("diagnostics_batch")
    if mode == "off":
        if batch is not None:
            raise ValueError(f"diagnostics batch length {batch} given with diagnostics=off: it would have no effect")
        return mode, 0
    nb, ns = int(config["num_bursts"]), int(config["num_burst_samples"])
    if nb < 2:
        raise ValueError(f"diagnostics=on needs num_bursts >= 2 (the two halves of split R-hat are whole bursts), have {nb}")
    L = ns if batch is None else int(batch)
    if L < 1 or ns < 1 or (L % ns != 0 and ns % L != 0):
        raise ValueError(f"diagnostics batch length {L}: it must divide num_burst_samples = {ns} or be a multiple of it")
    return mode, L


def forecast_mode(config, override=None, walk=None):
    """Mcmc.forecast (absent: off) and Mcmc.forecast_walk, or `--forecast H` / `--forecast-walk`: (H, walk), H = 0 for off.
    H days are simulated forward from the end of the series for every kept draw of the sampling phase, 1 <= H <= 128
    (SEIR_FORECAST_MAX_H); `walk` lets the log baseline go on as the prior's random walk instead of holding its last value."""
    w = config.get("forecast_walk", False) if walk is None else walk
    if isinstance(w, str):
        if w.lower() not in ("on", "off", "true", "false"):
            raise ValueError(f"forecast_walk={w!r}: on or off")
        w = w.lower() in ("on", "true")
    H = _day_count("forecast", "horizon", config.get("forecast") if override is None else override, _lib.FORECAST_MAX_H, series=False)
    if not H and w:
        raise ValueError("forecast_walk given without forecast: it would have no effect")
    return H, bool(w)


def forecast_quantiles_mode(config, override=None, horizon=None):
    """Mcmc.forecast_quantiles / `--forecast-quantiles 0.05,0.5,0.95`: exact per-location quantiles of the forecast draws."""
    return _quantiles("forecast_quantiles", "forecast", config, override, horizon)


def rt_mode(config, override=None, T=None):
    """Mcmc.rt (absent: off), or `--rt D`: the number of days D of the window [T - D, T) over which the reproduction number
    of every kept draw of the sampling phase is formed on the device; 0 for off."""
    return _day_count("rt", "window", config.get("rt") if override is None else override, T=T)


def rt_quantiles_mode(config, override=None, rt_days=None):
    """Mcmc.rt_quantiles / `--rt-quantiles 0.05,0.5,0.95`: exact per-day, per-location quantiles of the R_it draws."""
    return _quantiles("rt_quantiles", "rt", config, override, rt_days)


def within_between_mode(config, override=None, T=None):
    """Mcmc.within_between (absent: off), or `--within-between D`: the number of days D of the window [T - D, T) over which the
    within/between pressure shares of every kept draw of the sampling phase are formed on the device; 0 for off."""
    return _day_count("within_between", "window", config.get("within_between") if override is None else override, T=T)


def check_mode(config, override=None, T=None):
    """Mcmc.check (absent: off), or `--check K`: the number of days K of the window [T - K, T) that is simulated again from
    every kept draw of the sampling phase and set against the observed removals, K <= 128 (SEIR_CHECK_MAX_DAYS); 0 for off."""
    return _day_count("check", "window", config.get("check") if override is None else override, _lib.CHECK_MAX_DAYS, T)


# The check's Philox key is the run's seed with this constant folded in: the check and the forecast (keyed by the run's seed
# itself) share a protocol and a draw-id space, and so must never share a key
CHECK_SEED_SALT = 0x636865636B5F6B31                        # "check_k1"


def check_seed(seed):
    return (int(seed) ^ CHECK_SEED_SALT) & (2 ** 64 - 1)


# ---- one resolution ---------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Products:
    """What one resolution of the product options gives: every field normalised, 0 / () / False / None / "off" for off."""
    thin: int = 1
    summaries: str = "off"
    diagnostics: str = "off"
    batch_len: int = 0
    horizon: int = 0
    walk: bool = False
    fq_probs: tuple = ()
    rq_probs: tuple = ()
    rt_days: int = 0
    check_days: int = 0
    wb_days: int = 0
    group_spec: object = None       # "nations" or a mapping name -> members; None for off
    grp_rt_on: bool = False
    grp_wb_on: bool = False
    grp_ngm_on: bool = False

    def require(self, table):
        """What the group options need of each other and of the other products, given the group table (or None)."""
        G_mod.require_curves(table, self.grp_rt_on, self.rt_days, self.grp_wb_on, self.wb_days)
        G_mod.require_ngm(table, self.grp_ngm_on, self.rt_days, self.grp_rt_on)
        G_mod.require_source(table, self.summaries, self.horizon, self.check_days, self.grp_rt_on, self.grp_wb_on)

    def windows(self, T):
        """The three windows against the length of the series (None: not known, nothing to hold them to)."""
        _day_count("rt", "window", self.rt_days or None, T=T)
        _day_count("check", "window", self.check_days or None, _lib.CHECK_MAX_DAYS, T)
        _day_count("within_between", "window", self.wb_days or None, T=T)

    def bind(self, M, T, location_names):
        """The options against the data, before any GPU call: the group table of M locations or None (`location_names`: a
        callable that reads the input's location coordinate, not called when the groups are off), `require`, `windows`."""
        table = None if self.group_spec is None else G_mod.parse_groups(self.group_spec, M, location_names())
        self.require(table)
        self.windows(T)
        return table


def _switch(key):
    return lambda c, o, r: (G_mod.switch(c.get(key) if o.get(key) is None else o[key], key),)


# (fields of `Products`, their keys in the section and on the command line, (section, overrides, fields so far) -> values),
# in the order in which the refusals come
_OPTIONS = (
    (("wb_days",), ("within_between",), lambda c, o, r: (within_between_mode(c, o.get("within_between")),)),
    (("check_days",), ("check",), lambda c, o, r: (check_mode(c, o.get("check")),)),
    (("rt_days",), ("rt",), lambda c, o, r: (rt_mode(c, o.get("rt")),)),
    (("rq_probs",), ("rt_quantiles",), lambda c, o, r: (rt_quantiles_mode(c, o.get("rt_quantiles"), rt_days=r["rt_days"]),)),
    (("horizon", "walk"), ("forecast", "forecast_walk"), lambda c, o, r: forecast_mode(c, o.get("forecast"), o.get("forecast_walk"))),
    (("fq_probs",), ("forecast_quantiles",),
     lambda c, o, r: (forecast_quantiles_mode(c, o.get("forecast_quantiles"), horizon=r["horizon"]),)),
    (("thin",), ("thin",), lambda c, o, r: (thin_interval(c, o.get("thin")),)),
    (("summaries",), ("summaries",), lambda c, o, r: (summaries_mode(c, o.get("summaries")),)),
    (("diagnostics", "batch_len"), ("diagnostics", "diagnostics_batch"),
     lambda c, o, r: diagnostics_mode(c, o.get("diagnostics"), o.get("diagnostics_batch"))),
    (("group_spec",), ("groups",),
     lambda c, o, r: (None if G_mod.is_off(spec := c.get("groups") if o.get("groups") is None else o["groups"]) else spec,)),
    (("grp_rt_on",), ("groups_rt",), _switch("groups_rt")),
    (("grp_wb_on",), ("groups_within_between",), _switch("groups_within_between")),
    (("grp_ngm_on",), ("groups_ngm",), _switch("groups_ngm")),
)
PRODUCT_KEYS = tuple(k for _, keys, _ in _OPTIONS for k in keys)
_ALWAYS = ("thin", "summaries")                             # in the canonical section whatever their value
_OFF = (None, False, "off", 0, (), [])


def resolve_products(config, **overrides):
    """(section, `Products`): the Mcmc section with the command line's overrides (the keywords: `PRODUCT_KEYS`; None: not
    given) applied, every product option resolved by its `*_mode` function and refused here where it cannot run -- before the
    data file is opened.  The section is canonical: `thin` and `summaries` always, every other product key exactly when its
    product is on, holding its normalised value; resolving it again gives the same pair."""
    for k in overrides:
        if k not in PRODUCT_KEYS:
            raise TypeError(f"resolve_products() got an unexpected keyword argument {k!r}")
    fields = {}
    section = {k: v for k, v in config.items() if k not in PRODUCT_KEYS}
    for names, keys, resolve in _OPTIONS:
        values = resolve(config, overrides, fields)
        fields.update(zip(names, values))
        for k, v in zip(keys, values):
            if k in _ALWAYS or v not in _OFF:
                section[k] = list(v) if isinstance(v, tuple) else v
    return section, Products(**fields)


def resolve_scenarios(config, horizon, override=None):
    """Mcmc.scenarios (absent: off), or the mapping of a `--scenarios FILE.yaml` (`posterior.scenarios.load_spec`), against
    the forecast's horizon (`Products.horizon`): a frozen `posterior.scenarios.Scenarios`, empty for off.  A resolution of
    its own, beside `resolve_products`: with the key absent nothing of the products moves.  Every refusal -- scenarios without
    a forecast, more than four, a bad name, length or value -- comes here, before any GPU call.
    A specification in which a scenario has `locations` or `parts` (targeted scenarios) resolves in two stages: this one,
    before the data file is opened, checks keys, values, from_day, list lengths and the form of `locations` and gives a
    `posterior.scenarios.PendingScenarios`; `bind_scenarios` resolves the members to rows once M and the codes are known."""
    from ..posterior.scenarios import parse_scenarios
    return parse_scenarios(config.get("scenarios") if override is None else override, horizon)


def bind_scenarios(scenarios, M, location_names=None, populations=None):
    """Stage two of `resolve_scenarios`, before any GPU call: the members of a targeted specification to rows of the M
    locations (`location_names`: a callable that reads the input's location coordinate, or the codes themselves, or None; as
    for the groups, not called unless a member is a code or a pattern) -- an unknown code, a pattern that matches nothing and
    an index out of range are refused here.  Anything else is returned as it is.
    With a `trigger:` on any scenario `populations` [M] turns its per-100k thresholds into counts, here, where the driver holds
    them: a threshold above INT32_MAX and a rate without populations are refused."""
    from ..posterior.scenarios import PendingScenarios, resolve_locations
    if not isinstance(scenarios, PendingScenarios):
        return scenarios
    named = any(isinstance(x, str) for parts in scenarios.parts for members, _, _ in parts for x in members or ()) or \
        any(isinstance(x, str) for r in scenarios.rules if r is not None for x in r.members or ())
    names = location_names() if callable(location_names) and named else None if callable(location_names) else location_names
    if not scenarios.rules:
        return resolve_locations(scenarios, M, names)
    return resolve_locations(scenarios, M, names, populations)


def resolve_scenario_groups(config, scenarios, group_spec, override=None):
    """Mcmc.groups_scenarios (absent: off), or `--groups-scenarios`: the per-draw region totals of the scenarios, formed on
    the device (include/seir_hip.h, "Targeted scenarios on the device").  It needs `scenarios` (what `resolve_scenarios`
    gave) and `groups` (`Products.group_spec`, or a bound table): refused otherwise, before any GPU call.  A resolution beside
    `resolve_scenarios`: with the key absent nothing moves."""
    on = G_mod.switch(config.get("groups_scenarios") if override is None else override, "groups_scenarios")
    if on and not scenarios:
        raise ValueError("groups_scenarios given without scenarios: there is no scenario to sum over the groups")
    if on and group_spec is None:
        raise ValueError("groups_scenarios given without groups: there is no table of groups to sum the scenarios over")
    return on


def resolve_verify(config, horizon, override=None):
    """Mcmc.verify (absent: off), or the path of a `--verify FILE`, against the forecast's horizon (`Products.horizon`): the path of
    the later input file the forecast is scored against (`posterior.verify`), or None.  A resolution of its own, beside
    `resolve_products` and `resolve_scenarios`: with the key absent nothing of the products moves.  `verify` without a forecast
    is refused here; what the file holds is refused by `posterior.verify.load_truth` -- both before any GPU call."""
    from ..posterior.verify import parse_verify
    return parse_verify(config.get("verify") if override is None else override, horizon)


def posterior_kwargs(config, opt, group_table, kept):
    """The keywords of `Posterior` for the products that are on, `kept` rows in the per-draw datasets of the sampling phase."""
    days = dict(forecast=opt.horizon, rt=opt.rt_days, check=opt.check_days, within_between=opt.wb_days)
    curves = {k: (days[k], kept) for k, on in (("rt", opt.grp_rt_on), ("within_between", opt.grp_wb_on)) if on}
    return dict(**({} if config["summaries"] == "off" else dict(summaries=config["summaries"])),
                **{k: (d, kept) for k, d in days.items() if d},
                **(dict(groups=group_table.G) if group_table is not None else {}),
                **(dict(group_curves=curves) if curves else {}))


def product_inputs(cov, dates, T, opt, seed, group_table):
    """What the products need beyond the sampler, as keywords of `run_mcmc` / `product_records`: the calendars of the
    forecast and of the check, the national weights, the seed, the group table and the population."""
    kw = {}
    if opt.horizon:
        from ..posterior.predict import forecast_calendar
        kw = dict(forecast_calendar=forecast_calendar(cov, dates, T, opt.horizon), seed=seed)
    if opt.rt_days:
        N = np.asarray(cov.N, dtype=np.float64).reshape(-1)
        kw["rt_weight"] = N / N.sum()                       # reproduction_number.py:82-83
    if opt.check_days:
        from ..posterior.predict import check_calendar
        kw["check_calendar"] = check_calendar(cov, dates, T, opt.check_days)
        kw["seed"] = seed
    if group_table is not None:
        kw["groups"] = group_table
        if opt.grp_rt_on:
            kw["population"] = np.asarray(cov.N, dtype=np.float64).reshape(-1)
    return kw


# ---- the command line: the one declaration of the product arguments -------------------------------------------------
_ARGUMENTS = (
    ("--summaries", dict(choices=list(SUMMARIES)),
     "summaries of the latent epidemic formed on the device (overrides Mcmc.summaries; default off): on = per-draw marginals "
     "samples/seir_by_day, seir_by_location, state_by_day and per-cell summaries/* mean and variance of events and state over the sampling "
     "phase, next to samples/seir; only = the same without samples/seir, whose tensors then never leave the device"),
    ("--diagnostics", dict(choices=list(DIAGNOSTICS)),
     "convergence diagnostics formed on the device and the host as the run goes (overrides Mcmc.diagnostics; default off): on = a group "
     "diagnostics/ in every chain's file with split R-hat over this process's chains, batch-means ESS and the half-chain moments that "
     "`python -m covid19uk_amd.posterior.diagnostics` pools over files; needs num_bursts >= 2 and folds the sampling phase's draws on the "
     "device whatever --summaries says"),
    ("--diagnostics-batch", dict(type=int, metavar="L"),
     "batch length of the batch-means ESS in kept draws (overrides Mcmc.diagnostics_batch; default num_burst_samples, which it must divide "
     "or be a multiple of)"),
    ("--forecast", dict(type=int, metavar="H"),
     "simulate H days (1..128) forward from the end of the series for every kept draw of the sampling phase, on the device (overrides "
     "Mcmc.forecast; default off): a group forecast/ with the mean and variance of events and state per location and forecast day, and "
     "per-draw samples/forecast_by_day, forecast_by_location, forecast_state_by_day; works with --summaries only"),
    ("--forecast-walk", dict(action="store_true"),
     "let the forecast's log baseline continue as the prior's random walk (N(0, 0.005) steps) instead of holding its last value (overrides "
     "Mcmc.forecast_walk; needs --forecast)"),
    ("--forecast-quantiles", dict(type=str, metavar="P,P,..."),
     "exact quantiles of the forecast draws per location and forecast day, selected on the device (overrides Mcmc.forecast_quantiles; "
     "needs --forecast): 1 to 8 increasing probabilities in [0, 1], e.g. 0.05,0.5,0.95; forecast/cases_quantiles, cum_cases_quantiles, "
     "prevalence_quantiles per chain and forecast/pooled_* over the chains of the process; works with --summaries only and --thin"),
    ("--rt", dict(type=int, metavar="D"),
     "form the reproduction number R_it of every kept draw of the sampling phase over the last D days (1..T) on the device (overrides "
     "Mcmc.rt; default off): a group rt/ with the mean, variance and P(R > 1) per day and location, and the national curve per draw "
     "samples/R_t; works with --summaries only, --thin and --forecast"),
    ("--rt-quantiles", dict(type=str, metavar="P,P,...", dest="rt_quantiles"),
     "exact quantiles of the R_it draws per day of the window and location, selected on the device (overrides Mcmc.rt_quantiles; needs "
     "--rt): 1 to 8 increasing probabilities in [0, 1], e.g. 0.05,0.5,0.95; rt/R_it_quantiles per chain, rt/pooled_R_it_quantiles over the "
     "chains of the process and rt/R_t_quantiles of the national curve; works with --summaries only and --thin"),
    ("--check", dict(type=int, metavar="K"),
     "simulate the last K observed days (1..min(T, 128)) again from every kept draw of the sampling phase and set them against the "
     "observed removals, on the device (overrides Mcmc.check; default off): a group check/ with the moments of the re-simulated window, "
     "the counts of draws below / at the data per cell, location, day and in total with their mid-p values, and per-draw "
     "samples/check_by_day, check_by_location, check_state_by_day; works with --summaries only, --thin, --forecast and --rt"),
    ("--within-between", dict(type=int, metavar="D", dest="within_between"),
     "form the within- and between-location shares of the infection pressure of every kept draw of the sampling phase over the last D days "
     "(1..T) on the device (overrides Mcmc.within_between; default off): a group within_between/ with the mean and variance of the within "
     "share, the mean of the between share and P(within > between) per day and location, and the national pressures per draw "
     "samples/within_pressure, between_pressure; works with --summaries only, --thin, --forecast, --rt and --check"),
    ("--groups", dict(type=str, metavar="SPEC"),
     "per-draw totals over groups of locations, formed on the device for the recorded epidemic (--summaries on/only), the forecast and the "
     "check (overrides Mcmc.groups; default off): 'nations' groups by the first letter of the location code (needs an input file with a "
     "location coordinate), or a path to a YAML mapping name: [members], a member being a location code, a prefix pattern E0* or an "
     "integer index; groups/*, samples/*_by_group and the group_* datasets of forecast/ and check/; needs one of --summaries on/only, "
     "--forecast, --check"),
    ("--groups-rt", dict(action="store_true", dest="groups_rt"),
     "R_t of every kept draw per group, population-weighted over the group's members, formed on the device (overrides Mcmc.groups_rt; "
     "needs --groups and --rt): samples/R_t_by_group, rt/group_R_t_mean, group_R_t_var, group_prob_gt1 and, with --rt-quantiles, "
     "rt/group_R_t_quantiles"),
    ("--groups-within-between", dict(action="store_true", dest="groups_within_between"),
     "within / between infection pressure of every kept draw per group, formed on the device (overrides Mcmc.groups_within_between; needs "
     "--groups and --within-between): samples/within_pressure_by_group, between_pressure_by_group and within_between/group_*; 'between' is "
     "from outside each member location, as in the national figure, not from outside the group"),
    ("--groups-ngm", dict(action="store_true", dest="groups_ngm"),
     "group next-generation matrix of every kept draw, formed on the device (overrides Mcmc.groups_ngm; needs --groups, --rt and "
     "--groups-rt): K[g][h][t], the expected infections in group g caused by one typical infective of group h -- samples/ngm_by_group, "
     "ngm/K_mean, K_var, local_share_mean (the part of a group's R_t that stays inside it), with --rt-quantiles their quantiles, and for a "
     "partition samples/ngm_spectral_radius"),
)


def add_product_arguments(parser, help=True):
    """The fourteen product arguments of `inference.main` and `posterior.replay.main`; every default is None: not given."""
    for flag, kw, text in _ARGUMENTS:
        parser.add_argument(flag, default=None, help=text if help else None, **kw)


def product_overrides(args, always=()):
    """The keywords of `resolve_products` from the parsed arguments: an option that was given, and every one of `always`
    (None when it was not)."""
    given = {k: getattr(args, k) for k in PRODUCT_KEYS if k != "thin" and getattr(args, k) is not None}
    if "groups" in given:
        given["groups"] = G_mod.load_spec(given["groups"])
    return {**{k: None for k in always}, **given}


def add_scenarios_argument(parser):
    """`--scenarios FILE.yaml` of both command lines: declared beside the product arguments, resolved by `resolve_scenarios`."""
    parser.add_argument("--scenarios", type=str, default=None, metavar="FILE.yaml",
                        help="what-if scenarios riding on the forecast (overrides Mcmc.scenarios; needs --forecast): a YAML mapping name: "
                             "{transmission: f | [H floats], commute: f | [H floats], from_day: d}, at most four; every kept draw is also "
                             "rolled forward under each scenario with the forecast's random numbers -- scenarios/* with the moments and the "
                             "paired differences to the forecast per location and day, samples/scenario_by_day, scenario_state_by_day, "
                             "scenario_diff_by_day; a scenario may carry locations: [codes, prefix patterns E0*, indices] or parts: a "
                             "list of {locations, transmission, commute, from_day} applied in order (a part without locations applies "
                             "everywhere): a targeted scenario, whose commute scales the commuting-borne pressure on its locations; "
                             "a scenario may also carry trigger: {cases_per_100k | cases, release_per_100k | release, window, min_days, "
                             "review_every, from_day, locations} and then: {transmission, commute}: a measure that switches on and off "
                             "per draw and location by the draw's own simulated case counts -- scenarios/active_count, p_active, "
                             "samples/scenario_active_by_day")
    parser.add_argument("--groups-scenarios", action="store_true", default=None, dest="groups_scenarios",
                        help="per-draw totals of every scenario over the groups of locations, formed on the device (overrides "
                             "Mcmc.groups_scenarios; needs --scenarios and --groups): samples/scenario_by_group, "
                             "scenario_diff_by_group and, with --forecast-quantiles, scenarios/group_diff_quantiles")


def add_verify_argument(parser):
    """`--verify FILE` of both command lines: declared beside the product arguments, resolved by `resolve_verify`."""
    parser.add_argument("--verify", type=str, default=None, metavar="FILE",
                        help="score the forecast against later data (overrides Mcmc.verify; needs --forecast): an input file (.nc / "
                             ".hd5 / .npz) whose first T dates are the fitted file's; its cases of the H days behind them are the truth "
                             "-- verify/* with PIT, MAE and, with --forecast-quantiles, CRPS and interval coverage per location and "
                             "forecast day")


def verify_override(args):
    """The keyword of `inference.mcmc` / `posterior.replay.replay_files` from the parsed arguments: nothing when the flag was not given."""
    if getattr(args, "verify", None) is None:
        return {}
    return dict(verify=args.verify)


def scenarios_override(args):
    """The keyword of `inference.mcmc` / `posterior.replay.replay_files` from the parsed arguments: nothing when the flag was not given."""
    out = {}
    if getattr(args, "groups_scenarios", None) is not None:
        out["groups_scenarios"] = args.groups_scenarios
    if getattr(args, "scenarios", None) is None:
        return out
    from ..posterior.scenarios import load_spec
    return dict(out, scenarios=load_spec(args.scenarios))

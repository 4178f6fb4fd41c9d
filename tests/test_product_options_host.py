"""The product options and the product records against a recording of the commit before `inference/options.py`: what
`resolve_products` gives and refuses, what `mcmc` refuses once the data is read, the calls `run_mcmc` and a replay make on the
sampler, what they write and log, and what the two command lines hand on.  No GPU and no sampler: the stand-ins are those of
the other host tests.  tests/golden/product_options.json holds the outcomes of `record()` below, run on that commit."""
import contextlib
import dataclasses
import io
import json
import os
import sys

import numpy as np
import pytest

from covid19uk_amd import synth
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.posterior import groups as G
from covid19uk_amd.posterior import replay as R
from tests.test_diagnostics_host import DiagStub
from tests.test_group_curves_host import POP, TABLE
from tests.test_groups_host import GroupStub, QuantileStub
from tests.test_ngm_host import NgmStub
from tests.test_replay_host import ReplayStub, StubSource
from tests.test_summary_host import CFG

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "product_options.json")
FIELDS = ("thin", "summaries", "diagnostics", "batch_len", "horizon", "walk", "fq_probs", "rq_probs", "rt_days", "check_days",
          "wb_days", "group_spec", "grp_rt_on", "grp_wb_on", "grp_ngm_on")
PRODUCT_KEYS = ("thin", "summaries", "diagnostics", "diagnostics_batch", "forecast", "forecast_walk", "forecast_quantiles", "rt",
                "rt_quantiles", "check", "within_between", "groups", "groups_rt", "groups_within_between", "groups_ngm")
OFF = (None, False, "off", 0, (), [])
BASE = dict(CFG, num_bursts=2, num_burst_samples=2)
GRP = {"all": [0, 1, 2], "ends": [0, 2]}
EVERYTHING = dict(BASE, summaries="on", diagnostics="on", forecast=3, forecast_walk=True, forecast_quantiles=[0.05, 0.5, 0.95], rt=3,
                  rt_quantiles=[0.1, 0.9], check=2, within_between=2, groups=GRP, groups_rt="on", groups_within_between="on",
                  groups_ngm="on")


def plain(x):
    """x as JSON holds it: tuples as lists, numpy scalars as Python's, arrays by shape and dtype, callables by a word."""
    if isinstance(x, np.ndarray):
        return {"array": list(x.shape), "dtype": str(x.dtype)}
    if isinstance(x, dict):
        return {str(k): plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, (np.integer, np.bool_)):
        return x.item()
    if isinstance(x, np.floating):
        return float(x)
    return "<callable>" if callable(x) else x


# ---- 1. resolution ---------------------------------------------------------------------------------------------------
def fields(section, opt):
    """The fields of `Products`: from `opt` where it has them, from the resolved section otherwise (the commit before had
    half of them there); a group specification that says off is None."""
    derived = dict(thin=section["thin"], summaries=section["summaries"], diagnostics=section.get("diagnostics", "off"),
                   batch_len=section.get("diagnostics_batch", 0), walk=section.get("forecast_walk", False),
                   fq_probs=tuple(section.get("forecast_quantiles", ())), rq_probs=tuple(section.get("rt_quantiles", ())))
    out = {k: getattr(opt, k) if hasattr(opt, k) else derived[k] for k in FIELDS}
    out["group_spec"] = None if G.is_off(out["group_spec"]) else out["group_spec"]
    return plain(out)


def canonical(section):
    """The section without the product keys that hold an off value, and without `groups`: the commit before handed the
    specification on in `opt.group_spec` alone, so the key is compared there (`test_resolution`)."""
    return plain({k: v for k, v in section.items() if k != "groups" and not (k in PRODUCT_KEYS and v in OFF)})


def resolution(section, over):
    sec, opt = inf.resolve_products(section, **over)
    return dict(fields=fields(sec, opt), section=canonical(sec))


def _spellings():
    out = {"empty": ({}, {})}
    days = dict(rt=5, check=4, within_between=6, forecast=7)
    for key, d in days.items():
        out[f"{key}/section"] = ({key: d}, {})
        out[f"{key}/override"] = ({}, {key: d})
        out[f"{key}/override beats section"] = ({key: d}, {key: d + 1})
        out[f"{key}/override off beats section"] = ({key: d}, {key: "off"})
        for name, v in (("none", None), ("false", False), ("off", "off"), ("OFF", "OFF"), ("numpy", np.int64(d)), ("digits", str(d)),
                        ("signed digits", f" +{d} ")):
            out[f"{key}/{name}"] = ({key: v}, {})
    for key in ("summaries", "diagnostics"):
        for name, v in (("on", "on"), ("off", "off"), ("true", True), ("false", False)):
            out[f"{key}/{name}"] = ({key: v}, {})
        out[f"{key}/override"] = ({}, {key: "on"})
        out[f"{key}/override beats section"] = ({key: "on"}, {key: "off"})
    out["summaries/only"] = (dict(summaries="only"), {})
    out["summaries/override only"] = (dict(summaries="on"), dict(summaries="only"))
    out["diagnostics/batch"] = (dict(diagnostics="on", diagnostics_batch=1), {})
    out["diagnostics/batch override"] = (dict(diagnostics="on", diagnostics_batch=1), dict(diagnostics_batch=4))
    out["diagnostics/batch of the override alone"] = ({}, dict(diagnostics="on", diagnostics_batch=2))
    for name, v in (("section", 3), ("string", "4"), ("one", 1)):
        out[f"thin/{name}"] = (dict(thin=v), {})
    out["thin/override"] = (dict(thin=3), dict(thin=2))
    for name, v in (("true", True), ("false", False), ("on", "on"), ("off", "off"), ("TRUE", "TRUE"), ("false string", "false")):
        out[f"forecast_walk/{name}"] = (dict(forecast=3, forecast_walk=v), {})
    out["forecast_walk/override"] = (dict(forecast=3), dict(forecast_walk=True))
    out["forecast_walk/off without forecast"] = (dict(forecast_walk=False), {})
    for key, product in (("forecast_quantiles", "forecast"), ("rt_quantiles", "rt")):
        out[f"{key}/list"] = ({product: 3, key: [0.05, 0.5, 0.95]}, {})
        out[f"{key}/string override"] = ({product: 3}, {key: "0.1,0.9"})
        out[f"{key}/one number"] = ({product: 3, key: 0.5}, {})
        out[f"{key}/off"] = ({product: 3, key: "off"}, {})
        out[f"{key}/off without its product"] = ({key: False}, {})
        out[f"{key}/override beats section"] = ({product: 3, key: [0.5]}, {key: "0.25,0.75"})
    for name, v in (("mapping", GRP), ("nations", "nations"), ("off", "off"), ("false", False), ("none", None)):
        out[f"groups/{name}"] = (dict(summaries="on", groups=v), {})
    out["groups/override"] = (dict(summaries="on"), dict(groups=GRP))
    out["groups/override off beats section"] = (dict(summaries="on", groups=GRP), dict(groups="off"))
    for key in ("groups_rt", "groups_within_between", "groups_ngm"):
        for name, v in (("on", "on"), ("off", "off"), ("true", True), ("false", False), ("spaced", " On ")):
            out[f"{key}/{name}"] = ({key: v}, {})
        out[f"{key}/override"] = ({}, {key: True})
        out[f"{key}/override off beats section"] = ({key: "on"}, {key: False})
    out["everything/section"] = (EVERYTHING, {})
    out["everything/overrides"] = (BASE, {k: v for k, v in EVERYTHING.items() if k in PRODUCT_KEYS})
    out["everything/overrides beat the section"] = (EVERYTHING, dict(summaries="only", forecast=9, rt="4", check=np.int32(1), thin=5,
                                                                   groups="nations", groups_ngm=False, forecast_walk="off"))
    return {k: (dict(BASE, **sec), over) for k, (sec, over) in out.items()}


RESOLUTIONS = _spellings()


# ---- 2. refusals -----------------------------------------------------------------------------------------------------
class _Reached(Exception):
    """`mcmc` got as far as its first GPU call: nothing was refused."""


def refused(call):
    try:
        call()
    except Exception as e:                                      # noqa: BLE001 -- the type is part of what is compared
        return dict(type=type(e).__name__, message=str(e))
    return dict(type=None, message=None)


def bound(data, section, over):
    """`mcmc` on a real input file with the model's constructor standing for the first GPU call: the refusals that need the data."""
    def reached(*a, **k):
        raise _Reached()
    keep, inf.SeirModel = inf.SeirModel, reached
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            return refused(lambda: inf.mcmc(data, os.path.join(os.path.dirname(data), "never.npz"), section, **over))
    finally:
        inf.SeirModel = keep


def write_data(folder):
    cov = synth.make_covariates("ni11")
    events, _, _ = synth.simulate_epidemic(cov)
    path = os.path.join(str(folder), "data.npz")
    inf.write_inference_data(path, cov, events[..., 2])
    return path, cov.M, cov.T


def refusal_cases(T):
    """{id: ("resolve" | "mode" | "bound", ...)}: `resolve_products(section, **over)`, `inf.<mode>(section, **kw)`, `mcmc` on the data."""
    out = {}
    bad_days = (("zero", 0), ("negative", -2), ("true", True), ("float", 2.5), ("word", "many"), ("signed word", "+x"), ("digits below 1", "0"))
    for key, mode, limit in (("rt", "rt_mode", None), ("within_between", "within_between_mode", None), ("check", "check_mode", 128),
                             ("forecast", "forecast_mode", 128)):
        for name, v in bad_days + ((("above the bound", limit + 1),) if limit else ()):
            out[f"{key}/{name}"] = ("resolve", {key: v}, {})
            out[f"{key}/{name} as override"] = ("resolve", {}, {key: v})
        if key != "forecast":
            out[f"{key}/above T"] = ("mode", mode, {key: 6}, dict(T=5))
            out[f"{key}/above T as numpy"] = ("mode", mode, {}, dict(override=np.int64(9), T=np.int64(8)))
            out[f"{key}/zero with T"] = ("mode", mode, {key: 0}, dict(T=5))
            out[f"{key}/above the series"] = ("bound", {key: T + 1, "summaries": "on"}, {})
    out["check/above the bound and T"] = ("mode", "check_mode", dict(check=200), dict(T=150))
    for key in ("summaries", "diagnostics"):
        for name, v in (("unknown", "sometimes"), ("number", 1), ("none", None)):
            out[f"{key}/{name}"] = ("resolve", {key: v}, {})
        out[f"{key}/unknown override"] = ("resolve", {key: "on"}, {key: "maybe"})
    out["diagnostics/only"] = ("resolve", dict(diagnostics="only"), {})
    out["forecast_walk/without forecast"] = ("resolve", dict(forecast_walk=True), {})
    out["forecast_walk/override without forecast"] = ("resolve", {}, dict(forecast_walk=True))
    out["forecast_walk/with forecast off"] = ("resolve", dict(forecast="off", forecast_walk="on"), {})
    out["forecast_walk/unknown"] = ("resolve", dict(forecast=3, forecast_walk="perhaps"), {})
    out["forecast_walk/unknown and a bad horizon"] = ("resolve", dict(forecast=0, forecast_walk="perhaps"), {})
    for key in ("forecast_quantiles", "rt_quantiles"):
        out[f"{key}/without its product"] = ("resolve", {key: [0.5]}, {})
        out[f"{key}/override without its product"] = ("resolve", {}, {key: "0.5"})
        for name, v in (("decreasing", [0.9, 0.1]), ("outside", [1.5]), ("word", "half"), ("true", True), ("empty", []), ("nine", list(np.arange(9) / 10))):
            out[f"{key}/{name}"] = ("resolve", {key.split("_")[0]: 3, key: v}, {})
    out["diagnostics/batch with off"] = ("resolve", dict(diagnostics_batch=2), {})
    out["diagnostics/batch override with off"] = ("resolve", dict(diagnostics="off"), dict(diagnostics_batch=2))
    out["diagnostics/one burst"] = ("resolve", dict(diagnostics="on", num_bursts=1), {})
    out["diagnostics/batch fits neither way"] = ("resolve", dict(diagnostics="on", num_burst_samples=4, diagnostics_batch=3), {})
    out["diagnostics/batch zero"] = ("resolve", dict(diagnostics="on", diagnostics_batch=0), {})
    out["thin/zero"], out["thin/negative"] = ("resolve", dict(thin=0), {}), ("resolve", dict(thin=-1), {})
    out["thin/zero override"] = ("resolve", dict(thin=2), dict(thin=0))
    for key in ("groups_rt", "groups_within_between", "groups_ngm"):
        out[f"{key}/unknown"] = ("resolve", {key: "sometimes"}, {})
        out[f"{key}/number override"] = ("resolve", {}, {key: 1})
    # two refusals in one input: the first in the order of the resolution wins
    out["two/within_between before check"] = ("resolve", dict(within_between=0, check=0), {})
    out["two/check before rt"] = ("resolve", dict(check=-1, rt=-1), {})
    out["two/rt before rt_quantiles"] = ("resolve", dict(rt=0, rt_quantiles=[2.0]), {})
    out["two/rt_quantiles before forecast"] = ("resolve", dict(rt_quantiles=[0.5], forecast=999), {})
    out["two/forecast before forecast_quantiles"] = ("resolve", dict(forecast=999, forecast_quantiles="x"), {})
    out["two/forecast_quantiles before thin"] = ("resolve", dict(forecast_quantiles=[0.5], thin=0), {})
    out["two/thin before summaries"] = ("resolve", dict(thin=0, summaries="x"), {})
    out["two/summaries before diagnostics"] = ("resolve", dict(summaries="x", diagnostics="x"), {})
    out["two/diagnostics before groups_rt"] = ("resolve", dict(diagnostics="x", groups_rt="x"), {})
    out["two/groups_rt before groups_within_between"] = ("resolve", dict(groups_rt="x", groups_within_between="y"), {})
    out["two/groups_within_between before groups_ngm"] = ("resolve", dict(groups_within_between="y", groups_ngm="z"), {})
    out["two/an option before the data"] = ("bound", dict(rt=T + 1, summaries="x"), {})
    # what `mcmc` refuses once the data is read: the table, what the groups require, the windows
    grp = {"a": [0, 1]}
    on = dict(summaries="on", groups=grp)
    out["bound/nothing refused"] = ("bound", dict(on, rt=3, within_between=3, check=3, groups_rt=True, groups_within_between=True,
                                                  groups_ngm=True), {})
    out["bound/no groups, nothing refused"] = ("bound", dict(rt=T, check=min(T, 128), within_between=T), {})
    out["bound/unknown group spec"] = ("bound", dict(summaries="on", groups="counties"), {})
    out["bound/nations without names"] = ("bound", dict(summaries="on"), dict(groups="nations"))
    out["bound/index outside"] = ("bound", dict(summaries="on", groups={"a": [0, 99]}), {})
    out["bound/groups_rt without groups"] = ("bound", dict(rt=3, groups_rt="on"), {})
    out["bound/groups_rt without rt"] = ("bound", dict(on, groups_rt=True), {})
    out["bound/groups_within_between without groups"] = ("bound", dict(within_between=3), dict(groups_within_between=True))
    out["bound/groups_within_between without within_between"] = ("bound", dict(on, rt=3, groups_within_between=True), {})
    out["bound/groups_ngm without groups"] = ("bound", dict(rt=3, groups_ngm="on"), {})
    out["bound/groups_ngm without rt"] = ("bound", dict(on, groups_ngm=True), {})
    out["bound/groups_ngm without groups_rt"] = ("bound", dict(on, rt=3), dict(groups_ngm=True))
    out["bound/groups without a source"] = ("bound", dict(rt=3, within_between=3, groups=grp), {})
    out["bound/curves before the matrix"] = ("bound", dict(on, groups_rt=True, groups_ngm=True), {})
    out["bound/the matrix before the source"] = ("bound", dict(groups=grp, rt=3, groups_ngm=True), {})
    out["bound/the groups before the windows"] = ("bound", dict(rt=T + 1, groups_rt=True), {})
    out["bound/rt before check before within_between"] = ("bound", dict(rt=T + 1, check=T + 1, within_between=T + 1), {})
    out["bound/check before within_between"] = ("bound", dict(check=T + 1, within_between=T + 1, summaries="on"), {})
    return {k: v if v[0] == "mode" else (v[0], dict(BASE, **v[1]), v[2]) for k, v in out.items()}


def refusal(case, data):
    if case[0] == "resolve":
        return refused(lambda: inf.resolve_products(case[1], **case[2]))
    if case[0] == "mode":
        return refused(lambda: getattr(inf, case[1])(case[2], **case[3]))
    return bound(data, case[1], case[2])


# ---- 3. the driver's calls -------------------------------------------------------------------------------------------
class Everything:
    """The stand-ins of the other host tests in one sampler: in front of `NgmStub` or `ReplayStub` (R_t and its draw store,
    check, within / between, the table, the group curves, the matrix) the forecast's draw store and the group sums of the
    forecast and the check (tests/test_groups_host.py) and the diagnostics (tests/test_diagnostics_host.py)."""
    keep_forecast_draws, forecast_quantiles, _rows = QuantileStub.keep_forecast_draws, QuantileStub.forecast_quantiles, GroupStub._rows
    reset_diagnostics, diagnostics, mark, sample_bursts = DiagStub.reset_diagnostics, DiagStub.diagnostics, DiagStub.mark, DiagStub.sample_bursts

    def _trace(self, n, groups=False, **kw):
        tr = super()._trace(n, groups=("trace",) if groups and "trace" in groups else False, **kw)
        idx = self.sweeps - n + np.arange(n)
        tr.theta = np.sin(idx)[:, None, None] * (1.0 + np.arange(self.B))[None, :, None] + np.arange(self.P)[None, None, :]
        for src, L in (("forecast", getattr(self, "H", 0)), ("check", getattr(self, "K", 0))):
            if groups and src in groups:
                assert kw.get(src)
                tr.groups = dict(tr.groups or {}, **{f"{src}_by_group": self._rows(idx, L), f"{src}_group_state0": 1000 + self._rows(idx, 1)[:, :, :, 0]})
        return tr

    def read_group_ngm(self, count, first=0):                   # CheckStub keeps its days in self.K, over NgmStub's method K
        self.calls.append(("read_group_ngm", count, first))
        return NgmStub.K(self, first + np.arange(count))


class LiveStub(Everything, NgmStub):
    pass


class StoredStub(Everything, ReplayStub):                      # what a replay must never call is recorded as forbidden
    pass


class RecordingPosterior(inf.Posterior):
    """`inference.Posterior` (its .npz form) that notes every write: (dataset, row offset or None, shape)."""

    def __init__(self, *a, **kw):
        self.writes = []
        super().__init__(*a, **kw)

    def write(self, name, value, first_dim_offset):
        self.writes.append((name, int(first_dim_offset), list(np.shape(value))))
        super().write(name, value, first_dim_offset)

    def create_dataset(self, name, data, dtype=None):
        self.writes.append((name, None, list(np.shape(data))))
        super().create_dataset(name, data, dtype)


DRIVER = {
    "off": {}, "summaries on": dict(summaries="on"), "diagnostics": dict(diagnostics="on"),
    "summaries only with diagnostics": dict(summaries="only", diagnostics="on", diagnostics_batch=1), "forecast": dict(forecast=3),
    "rt": dict(rt=3), "rt quantiles": dict(rt=3, rt_quantiles=[0.1, 0.9]), "check": dict(check=2),
    "within_between": dict(within_between=2), "groups of the summaries": dict(summaries="on", groups=GRP),
    "everything": {k: v for k, v in EVERYTHING.items() if k in PRODUCT_KEYS},
}


def driver(folder, tag, products, replay):
    """One run of `run_mcmc` (or, `replay`, of `product_records(..., total=n, results=False)` under `replay_bursts`) over the
    stand-ins: the sampler's calls, the first chain's writes, the log without its wall-clock line."""
    s = StoredStub() if replay else LiveStub()
    s.loaded = []
    nb, ns = BASE["num_bursts"], BASE["num_burst_samples"]
    n = nb * ns
    section, opt = inf.resolve_products(dict(BASE, **products, **(dict(thin=1) if replay else {})))
    table = None if G.is_off(opt.group_spec) else TABLE
    rows = n if replay else inf.warmup_size() + n
    posts = [RecordingPosterior(os.path.join(str(folder), f"{tag}_{c}.npz"), s.M, s.T, 2, rows, burst=ns,
                                **(dict(results=False) if replay else {}), **inf.posterior_kwargs(section, opt, table, n)) for c in range(s.B)]
    kw = dict(seed=21)
    if opt.horizon:
        kw["forecast_calendar"] = (np.arange(opt.horizon) + 0.5, np.arange(opt.horizon) - 1.0)
    if opt.rt_days:
        kw["rt_weight"] = POP / POP.sum()
    if opt.check_days:
        kw["check_calendar"] = (np.arange(opt.check_days) + 0.25, np.arange(opt.check_days) - 2.0)
    if table is not None:
        kw.update(groups=table, population=POP)
    log = io.StringIO()
    if replay:
        pr = inf.product_records(s, section, posts, log=log, total=n, results=False, **kw)
        R.replay_bursts(s, [StubSource(c, 40, s.P, s.M, s.T) for c in range(s.B)], np.arange(7, 7 + 3 * n, 3), ns, pr, log=log)
    else:
        inf.run_mcmc(s, dict(BASE, **products), posts, log=log, **kw)
    for p in posts:
        p.close()
    assert posts[0].writes == posts[1].writes
    return dict(calls=plain(s.calls), writes=plain(posts[0].writes),
                log=[ln for ln in log.getvalue().splitlines() if not ln.startswith("Sampling: ")])


# ---- 4. the command lines --------------------------------------------------------------------------------------------
FLAGS = {"--summaries": "only", "--diagnostics": "on", "--diagnostics-batch": "2", "--forecast": "14", "--forecast-walk": None,
         "--forecast-quantiles": "0.1,0.9", "--rt": "7", "--rt-quantiles": "0.5", "--check": "3", "--within-between": "2",
         "--groups": "nations", "--groups-rt": None, "--groups-within-between": None, "--groups-ngm": None}
COMMANDS = {"no flag": [], "every flag": [x for k, v in FLAGS.items() for x in ([k] if v is None else [k, v])],
            **{k: [k] if v is None else [k, v] for k, v in FLAGS.items()}}


def command(folder, which, flags):
    """What `inference.main` hands to `mcmc`, or `replay.main` to `replay_files`: (positional, keywords)."""
    cfg = os.path.join(str(folder), "c.yaml")
    with open(cfg, "w") as f:
        f.write("Mcmc:\n  num_burst_samples: 4\n  num_bursts: 2\n")
    seen = {}
    module, name = (inf, "mcmc") if which == "inference" else (R, "replay_files")
    keep = getattr(module, name)
    setattr(module, name, lambda *a, **k: seen.update(args=a, kw=k))
    try:
        module.main(["-c", cfg, "-o", "out.hd5", "data.nc"] + (["p0.hd5"] if which == "replay" else []) + flags)
    finally:
        setattr(module, name, keep)
    return plain(dict(args=seen["args"], kw=seen["kw"]))


# ---- the recording, and the tests against it -------------------------------------------------------------------------
def record(folder):
    data, _, T = write_data(folder)
    return dict(
        resolution={k: resolution(*v) for k, v in RESOLUTIONS.items()},
        refusals={k: refusal(v, data) for k, v in refusal_cases(T).items()},
        driver={f"{k}/{'replay' if replay else 'run_mcmc'}": driver(folder, f"d{i}{int(replay)}", v, replay)
                for i, (k, v) in enumerate(DRIVER.items()) for replay in (False, True)},
        commands={f"{which}/{k}": command(folder, which, v) for which in ("inference", "replay") for k, v in COMMANDS.items()})


# ---- the recording as the fixture holds it: nothing twice ------------------------------------------------------------
DEFAULTS = dict(thin=1, summaries="off", diagnostics="off", batch_len=0, horizon=0, walk=False, fq_probs=[], rq_probs=[], rt_days=0,
                check_days=0, wb_days=0, group_spec=None, grp_rt_on=False, grp_wb_on=False, grp_ngm_on=False)


def squeeze(writes):
    """[(dataset, offset, shape)] as runs at one offset with one number of rows, [offset, rows, [[dataset, shape of a row]]];
    datasets written whole (offset None) as [None, None, [[dataset, shape]]]."""
    out = []
    for name, off, shape in writes:
        head, item = ([None, None], [name, shape]) if off is None else ([off, shape[0]], [name, shape[1:]])
        if out and out[-1][:2] == head:
            out[-1][2].append(item)
        else:
            out.append(head + [[item]])
    return out


def spread(runs):
    return [[name, off, shape if off is None else [rows] + shape] for off, rows, items in runs for name, shape in items]


def _rest(case):
    """The keys of a resolution's input that are no product's: a resolved section holds them unchanged."""
    return plain({k: v for k, v in RESOLUTIONS[case][0].items() if k not in PRODUCT_KEYS})


def pack(doc):
    """`record()`'s outcomes with every distinct call, log line, refusal and run of datasets once, in `table`; of a resolution
    the fields that are not the default and the product keys of the section; of a command the keywords that differ from
    those of the command without flags."""
    table, index = [], {}

    def ref(x):
        key = json.dumps(x, sort_keys=True)
        if key not in index:
            index[key] = len(table)
            table.append(x)
        return index[key]
    out = dict(table=table, resolution={}, commands={})
    for case, r in doc["resolution"].items():
        assert {k: v for k, v in r["section"].items() if k not in PRODUCT_KEYS} == _rest(case), case
        out["resolution"][case] = [{k: v for k, v in r["fields"].items() if v != DEFAULTS[k]},
                                   {k: v for k, v in r["section"].items() if k in PRODUCT_KEYS}]
    out["refusals"] = {case: ref(r) for case, r in doc["refusals"].items()}
    out["driver"] = {case: [[ref(c) for c in r["calls"]], [[off, rows, ref(items)] for off, rows, items in squeeze(r["writes"])],
                            [ref(ln) for ln in r["log"]]] for case, r in doc["driver"].items()}
    for case, r in doc["commands"].items():
        base = doc["commands"][case.split("/")[0] + "/no flag"]
        assert r["args"] == base["args"] and set(base["kw"]) <= set(r["kw"]), case
        out["commands"][case] = r if r is base else {k: v for k, v in r["kw"].items() if k not in base["kw"] or base["kw"][k] != v}
    return out


def unpack(doc):
    t = doc["table"]
    out = dict(refusals={case: t[i] for case, i in doc["refusals"].items()}, commands={})
    out["resolution"] = {case: dict(fields=dict(DEFAULTS, **f), section=dict(_rest(case), **sec)) for case, (f, sec) in doc["resolution"].items()}
    out["driver"] = {case: dict(calls=[t[i] for i in c], writes=spread([off, rows, t[i]] for off, rows, i in w), log=[t[i] for i in lg])
                     for case, (c, w, lg) in doc["driver"].items()}
    for case, r in doc["commands"].items():
        base = doc["commands"][case.split("/")[0] + "/no flag"]
        out["commands"][case] = r if r is base else dict(args=base["args"], kw=dict(base["kw"], **r))
    return out


WANT = unpack(json.load(open(GOLDEN))) if os.path.exists(GOLDEN) else None     # absent where the recording is being taken


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return write_data(tmp_path_factory.mktemp("data"))


def test_the_case_lists_are_the_recordings(data):
    assert set(WANT["resolution"]) == set(RESOLUTIONS) and set(WANT["refusals"]) == set(refusal_cases(data[2]))
    assert set(WANT["driver"]) == {f"{k}/{p}" for k in DRIVER for p in ("run_mcmc", "replay")}
    assert set(WANT["commands"]) == {f"{w}/{k}" for w in ("inference", "replay") for k in COMMANDS}
    assert all(r["type"] == "ValueError" for k, r in WANT["refusals"].items() if "nothing refused" not in k), \
        [k for k, r in WANT["refusals"].items() if r["type"] != "ValueError"]


@pytest.mark.parametrize("case", sorted(RESOLUTIONS))
def test_resolution(case):
    section, over = RESOLUTIONS[case]
    want = WANT["resolution"][case]
    sec, opt = inf.resolve_products(section, **over)
    assert dataclasses.is_dataclass(opt) and [f.name for f in dataclasses.fields(opt)] == list(FIELDS)
    with pytest.raises(dataclasses.FrozenInstanceError):
        opt.thin = 2
    assert plain(dataclasses.asdict(opt)) == want["fields"] == fields(sec, opt)
    assert canonical(sec) == want["section"]
    # the canonical section: thin and summaries always, every other product key exactly when it is on; `groups` is the
    # specification the commit before handed on in opt.group_spec
    assert "thin" in sec and "summaries" in sec
    assert all(sec[k] not in OFF for k in PRODUCT_KEYS if k in sec and k not in ("thin", "summaries"))
    assert plain(sec.get("groups")) == want["fields"]["group_spec"]
    assert inf.resolve_products(sec) == (sec, opt)              # a resolved section resolves to itself


def test_refusals(data):
    path, M, T = data
    for case, spec in refusal_cases(T).items():
        want = WANT["refusals"][case]
        assert refusal(spec, path) == want, case
        if spec[0] == "bound" and case != "two/an option before the data":
            # the same refusal from `bind` itself; without groups the location names are not read
            _, opt = inf.resolve_products(spec[1], **spec[2])
            names = (lambda: None) if opt.group_spec is not None else (lambda: pytest.fail("the location names were read"))
            got = refused(lambda: opt.bind(M, T, names))
            assert got == (dict(type=None, message=None) if want["type"] == "_Reached" else want), case


@pytest.mark.parametrize("replay", [False, True], ids=["run_mcmc", "replay"])
@pytest.mark.parametrize("case", sorted(DRIVER))
def test_the_drivers_calls_writes_and_log(tmp_path, case, replay):
    want = WANT["driver"][f"{case}/{'replay' if replay else 'run_mcmc'}"]
    got = driver(tmp_path, "run", DRIVER[case], replay)
    assert got["calls"] == want["calls"]
    assert got["writes"] == want["writes"]
    assert got["log"] == want["log"]


@pytest.mark.parametrize("which", ["inference", "replay"])
def test_the_command_lines(tmp_path, which):
    for case, flags in COMMANDS.items():
        assert command(tmp_path, which, flags) == WANT["commands"][f"{which}/{case}"], case


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        full = json.loads(json.dumps(record(tmp)))
    out = pack(full)
    assert unpack(json.loads(json.dumps(out))) == full          # nothing is lost in the packing

    def dumps(v):
        return json.dumps(v, sort_keys=True, separators=(",", ":"))
    with open(sys.argv[1], "w") as f:                           # one line per case and per entry of the table
        parts = ['"table": [\n' + ",\n".join(dumps(v) for v in out["table"]) + "\n]"]
        parts += [f'"{part}": {{\n' + ",\n".join(f"{json.dumps(k)}: {dumps(v)}" for k, v in sorted(out[part].items())) + "\n}"
                  for part in ("commands", "driver", "refusals", "resolution")]
        f.write("{\n" + ",\n".join(parts) + "\n}\n")

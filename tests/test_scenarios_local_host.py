"""Targeted scenarios, the parts that need no GPU: the three entry points declared, exported and bound with the header's
types; the specification with `locations` and `parts` against plain Python loops, its two stages and every refusal; the NumPy
definition `local_inputs`; run_mcmc and the replay driver with a stub sampler and the datasets they write; the compiler's
account of the new kernels."""
import os

import numpy as np
import pytest

from covid19uk_amd import _lib, hdf5io, kernel_resources, synth
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.inference import options
from covid19uk_amd.posterior import groups as G
from covid19uk_amd.posterior import replay as R
from covid19uk_amd.posterior import scenarios as SC
from tests import abi_lib
from tests import helpers as H
from tests.test_groups_host import TABLE, GroupStub
from tests.test_scenarios_host import READS, SCEN_SETS, SPEC, ScenarioStub
from tests.test_summary_host import CFG, _read

NEW = {
    "seir_sampler_scenarios_set_local": "seir_sampler *s, int32_t K, const double *log_shift, const double *commute, int64_t cap",
    "seir_sampler_scenario_groups_set": "seir_sampler *s, int32_t on",
    "seir_sampler_read_scenario_group_draws": "seir_sampler *s, int64_t first, int64_t count, int64_t *by_group",
}
CODES = [str(x) for x in np.load(synth._DATA)["lad19cd"]]


# ---- 1. the entry points ----------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound_with_the_headers_types():
    lib = abi_lib.check_symbols(NEW)
    text = open(abi_lib.HEADER).read()
    assert "Targeted scenarios on the device" in text
    for call in (lambda: lib.seir_sampler_scenarios_set_local(None, 0, None, None, 0),
                 lambda: lib.seir_sampler_scenario_groups_set(None, 1),
                 lambda: lib.seir_sampler_read_scenario_group_draws(None, 0, 0, None)):
        assert call() == _lib.ERR_INVALID and b"null sampler" in lib.seir_last_error()


# ---- 2. the specification ---------------------------------------------------------------------------------------------
def test_locations_resolve_by_code_prefix_and_index_against_the_bundled_codes():
    M, Hn = len(CODES), 4
    wales = [m for m, c in enumerate(CODES) if c.startswith("W")]
    assert M == 380 and len(wales) == 22
    pend = SC.parse_scenarios({"w": {"locations": ["W*", CODES[0], 7], "transmission": 0.5, "from_day": 1}}, Hn)
    assert isinstance(pend, SC.PendingScenarios) and pend.K == 1 and bool(pend) and SC.is_local(pend)
    sc = SC.resolve_locations(pend, M, CODES)
    assert isinstance(sc, SC.LocalScenarios) and sc.names == ("w",) and sc.horizon == Hn
    assert sc.log_shift.shape == sc.commute.shape == (1, M, Hn) and sc.locations.shape == (1, M) and sc.locations.dtype == np.uint8
    rows = sorted(set(wales) | {0, 7})
    assert np.flatnonzero(sc.locations[0]).tolist() == rows
    want = np.zeros((M, Hn))
    want[rows, 1:] = np.log(0.5)
    assert np.array_equal(sc.log_shift[0], want) and np.array_equal(sc.commute[0], np.ones((M, Hn)))
    with pytest.raises(ValueError):
        sc.log_shift[0, 0, 0] = 1.0                        # read-only, as the global arrays are
    assert SC.resolve_locations(sc, M, CODES) is sc


def test_parts_compose_in_list_order_and_from_day_is_per_part():
    M, Hn = 6, 5
    parts = [{"locations": [0, 1, 2], "transmission": 0.5, "commute": 0.25, "from_day": 1},
             {"transmission": [1.0, 2.0, 0.5, 0.5, 3.0], "from_day": 2},
             {"locations": [2, 5], "commute": [0.0, 1.0, 2.0, 0.5, 0.1], "transmission": 0.7, "from_day": 4}]
    spec = {"p": {"parts": parts}, "plain": {"transmission": 0.8, "from_day": 3}, "one": {"locations": [4], "commute": 0.0}}
    sc = SC.resolve_locations(SC.parse_scenarios(spec, Hn), M)
    assert sc.names == ("p", "plain", "one") and sc.log_shift.shape == (3, M, Hn)
    # the definition, as a loop: multipliers start at 1.0; each part multiplies its rows from its from_day on, in float64
    tr, cm = [[1.0] * Hn for _ in range(M)], [[1.0] * Hn for _ in range(M)]
    for p in parts:
        for m in p.get("locations", range(M)):
            for s in range(p["from_day"], Hn):
                t, c = p.get("transmission", 1.0), p.get("commute", 1.0)
                tr[m][s] = tr[m][s] * float(t[s] if isinstance(t, list) else t)
                cm[m][s] = cm[m][s] * float(c[s] if isinstance(c, list) else c)
    assert np.array_equal(sc.log_shift[0], np.log(np.array(tr))) and np.array_equal(sc.commute[0], np.array(cm))
    assert sc.locations[0].tolist() == [1] * M
    # a scenario without the new keys inside a local spec: the global multipliers on every row, bit for bit
    glob = SC.parse_scenarios({"plain": spec["plain"]}, Hn)
    for m in range(M):
        assert np.array_equal(sc.log_shift[1, m], glob.log_shift[0]) and np.array_equal(sc.commute[1, m], glob.commute[0])
    assert sc.locations[1].tolist() == [1] * M and sc.locations[2].tolist() == [0, 0, 0, 0, 1, 0]
    assert np.array_equal(sc.commute[2, 4], np.zeros(Hn)) and not sc.log_shift[2].any()


def test_a_spec_without_the_new_keys_resolves_to_todays_object_field_for_field():
    import dataclasses
    Hn = 5
    spec = {"half": {"transmission": 0.5}, "stay": {"commute": [1, 0.5, 0, 0, 2], "from_day": 1}, "same": None}
    sc = options.bind_scenarios(options.resolve_scenarios({"scenarios": spec}, Hn), 7, lambda: 1 / 0)   # the codes are not read
    assert type(sc) is SC.Scenarios and not SC.is_local(sc)
    assert [f.name for f in dataclasses.fields(sc)] == ["names", "horizon", "log_shift", "commute"]
    # the parent's result, as a literal
    assert sc.names == ("half", "stay", "same") and sc.horizon == Hn
    assert np.array_equal(sc.log_shift, [np.log(np.full(Hn, 0.5)), np.zeros(Hn), np.zeros(Hn)])
    assert np.array_equal(sc.commute, [np.ones(Hn), [1, 0.5, 0, 0, 2], np.ones(Hn)])
    assert sc.log_shift.shape == (3, Hn) and not sc.log_shift.flags.writeable


@pytest.mark.parametrize("spec,word", [
    ({"a": {"locations": []}}, "non-empty list"),
    ({"a": {"locations": "E0*"}}, "non-empty list"),
    ({"a": {"locations": [1.5]}}, "non-empty list"),
    ({"a": {"locations": [True]}}, "non-empty list"),
    ({"a": {"locations": [0], "where": 1}}, "keys transmission, commute, from_day, locations"),
    ({"a": {"parts": []}}, "non-empty list of mappings"),
    ({"a": {"parts": {"locations": [0]}}}, "non-empty list of mappings"),
    ({"a": {"parts": [{"locations": [0]}], "transmission": 0.5}}, "carries nothing else"),
    ({"a": {"parts": [{"locations": [0], "transmission": 0.0}]}}, r"a.parts\[0\].transmission.*> 0"),
    ({"a": {"parts": [{}, {"commute": [1, 1]}]}}, r"a.parts\[1\].commute has 2 values, the forecast has 3 days"),
    ({"a": {"parts": [{"from_day": 3}]}}, "from_day=3"),
    ({"a": {"locations": [0], "commute": -1.0}}, ">= 0"),
    ({"a": {"locations": [0]}, "": {}}, "name is empty"),
    ([("a", {"locations": [0]}), ("a", {})], "given twice"),
])
def test_every_stage_one_refusal_happens_with_no_file_opened(spec, word, tmp_path):
    with pytest.raises(ValueError, match=word):
        SC.parse_scenarios(spec, 3)
    if isinstance(spec, dict):
        nofile, out = str(tmp_path / "no_such_file.nc"), str(tmp_path / "out.npz")
        with pytest.raises(ValueError, match=word):             # inference.mcmc: before the data file is opened
            inf.mcmc(nofile, out, dict(CFG, forecast=3, scenarios=spec))
        assert not os.path.exists(out)


class NoCalls:
    """A sampler that refuses every call: what comes before the first GPU call may only read its shape."""
    B, M, T, P = 2, 3, 10, 18

    def __getattr__(self, name):
        raise AssertionError(f"the sampler was called: {name}")


@pytest.mark.parametrize("spec,names,word", [
    ({"a": {"locations": ["E99"]}}, ["E01", "E02", "W01"], "unknown location code 'E99'"),
    ({"a": {"locations": ["S*"]}}, ["E01", "E02", "W01"], "matches no location code"),
    ({"a": {"locations": [3]}}, ["E01", "E02", "W01"], r"index 3 outside \[0, M=3\)"),
    ({"a": {"locations": [-1]}}, None, "index -1 outside"),
    ({"a": {"parts": [{"locations": [0]}, {"locations": ["E01"]}]}}, None, "unknown location code"),
    ({"a": {"locations": [1, 1]}}, None, "more than once"),
])
def test_every_stage_two_refusal_happens_with_no_gpu_call(spec, names, word):
    pend = SC.parse_scenarios(spec, 3)                          # stage one has nothing to object to
    with pytest.raises(ValueError, match=word):
        SC.resolve_locations(pend, 3, names)
    with pytest.raises(ValueError, match="scenarios: a.locations: .*" + word):
        inf.run_mcmc(NoCalls(), dict(CFG, forecast=3, scenarios=spec), [], log=open(os.devnull, "w"),
                     forecast_calendar=(np.ones(3), np.ones(3)), location_names=names)


def test_groups_scenarios_needs_scenarios_and_groups_and_is_refused_before_any_call(tmp_path):
    for cfg, kw, word in ((dict(CFG, forecast=3, groups_scenarios="on"), {}, "groups_scenarios given without scenarios"),
                          (dict(CFG, forecast=3, scenarios=SPEC, groups_scenarios=True), {}, "groups_scenarios given without groups"),
                          (dict(CFG, forecast=3, scenarios=SPEC, groups_scenarios="maybe"), dict(groups=TABLE), "on or off")):
        with pytest.raises(ValueError, match=word):
            inf.run_mcmc(NoCalls(), cfg, [], log=open(os.devnull, "w"), forecast_calendar=(np.ones(3), np.ones(3)), **kw)
        nofile, out = str(tmp_path / "no_such_file.nc"), str(tmp_path / "out.npz")
        with pytest.raises(ValueError, match=word):
            inf.mcmc(nofile, out, cfg)
    assert options.resolve_scenario_groups(dict(groups_scenarios="off"), None, None) is False
    assert options.resolve_scenario_groups({}, None, None) is False
    assert options.resolve_scenario_groups({}, SC.parse_scenarios(SPEC, 3), "nations", override=True) is True
    assert "groups_scenarios" not in options.PRODUCT_KEYS


# ---- 3. the NumPy definition ------------------------------------------------------------------------------------------
def test_local_inputs_against_a_loop_and_constant_tensors_against_scenario_inputs():
    rng = np.random.default_rng(3)
    n, M, Hn = 4, 5, 6
    sc = SC.LocalScenarios(("a", "b"), Hn, rng.normal(size=(2, M, Hn)), rng.uniform(0, 2, size=(2, M, Hn)))
    a_path, W = rng.normal(size=(n, Hn)), rng.uniform(1, 3, size=Hn)
    for k in range(2):
        a, w = SC.local_inputs(a_path, W, sc, k)
        assert a.shape == (n, M, Hn) and w.shape == (M, Hn)
        for d in range(n):
            for m in range(M):
                for s in range(Hn):
                    assert a[d, m, s] == float(a_path[d, s]) + float(sc.log_shift[k, m, s])
                    assert w[m, s] == float(W[s]) * float(sc.commute[k, m, s])
    # constant over m: every row is the global scenario's input, bit for bit
    glob = SC.parse_scenarios({"a": {"transmission": [0.3, 1.7, 0.9, 1.0, 2.5, 0.1], "commute": [0, 0.3, 1.1, 2, 1, 0.7]}}, Hn)
    const = SC.LocalScenarios(("a",), Hn, np.repeat(glob.log_shift[:, None], M, axis=1), np.repeat(glob.commute[:, None], M, axis=1))
    a, w = SC.local_inputs(a_path, W, const, 0)
    ag, wg = SC.scenario_inputs(a_path, W, glob, 0)
    for m in range(M):
        assert np.array_equal(a[:, m], ag) and np.array_equal(w[m], wg)


# ---- 4. run_mcmc and the replay driver with a stub sampler; the datasets ----------------------------------------------
NEW_CALLS = ("set_scenario_groups", "read_scenario_group_draws")
LOCAL_SPEC = {"half": {"transmission": 0.5, "from_day": 1}, "lock": {"parts": [{"locations": [0, 2], "commute": 0.0}]}}
LOCAL_SETS = (SCEN_SETS - {"scenarios/log_shift", "scenarios/commute"}) | {"scenarios/log_shift_by_location",
                                                                           "scenarios/commute_by_location", "scenarios/locations"}
GROUP_SETS = {"samples/scenario_by_group", "samples/scenario_diff_by_group"}
# every call, by name and in order, of `_run(..., dict(CFG, forecast=4, forecast_quantiles=[0.25, 0.75], scenarios=SPEC),
# groups=TABLE)`, recorded from the parent commit: the table, the warm-up's eight windows, the resets and sets behind it, the
# two bursts with their forecasts, the write-up's reads
PARENT_CALLS = ["set_groups", "set_thin", "sample", "sample", "sample", "sample", "sample", "sample", "sample", "sample", "set_thin",
                "reset_forecast", "keep_forecast_draws", "set_scenarios", "burst", "forecast", "burst", "forecast",
                "forecast_summary", "forecast_quantiles", "forecast_quantiles", "scenario_summary", "scenario_diffs",
                "read_scenario_draws"]


class LocalStub(ScenarioStub, GroupStub):
    """The scenarios' stub on the groups' stub, with the two new calls: scenario k's totals of a draw are the forecast's group
    sums plus k + 1."""

    def _rows(self, idx=None, L=None):
        return ScenarioStub._rows(self) if idx is None else GroupStub._rows(self, idx, L)

    def set_scenario_groups(self, on=True):
        self.calls.append(("set_scenario_groups", on))

    def read_scenario_group_draws(self, count=None, first=0):
        self.calls.append(("read_scenario_group_draws", count, first))
        f = GroupStub._rows(self, ScenarioStub._rows(self), self.H)
        return f[None] + (np.arange(self.K_sc) + 1)[:, None, None, None, None, None]

    def set_scenarios(self, log_shift, commute, cap):
        super().set_scenarios(log_shift, commute, cap)
        self.K_sc = len(log_shift)


def _run(tmp_path, tag, config, ext=".npz", groups=TABLE, **kw):
    s = LocalStub()
    s.cap = 800
    nb, ns = config["num_bursts"], config["num_burst_samples"]
    Hn, _ = inf.forecast_mode(config)
    names = [str(tmp_path / f"{tag}_{c}{ext}") for c in range(s.B)]
    posts = [inf.Posterior(name, s.M, s.T, 2, inf.warmup_size() + nb * ns, forecast=(Hn, nb * ns),
                           **({} if groups is None else dict(groups=groups.G))) for name in names]
    logname = str(tmp_path / f"{tag}.log")
    with open(logname, "w") as log:
        inf.run_mcmc(s, config, posts, log=log, forecast_calendar=(np.arange(Hn) + 0.5, np.arange(Hn) - 1.0), seed=21,
                     **({} if groups is None else dict(groups=groups)), **kw)
    for p in posts:
        p.close()
    return s, [_read(n) for n in names], open(logname).read()


def _names(s):
    return [c[0] for c in s.calls]


@pytest.mark.parametrize("ext", [".npz", ".hd5"])
def test_run_mcmc_global_local_and_with_the_region_totals(tmp_path, ext):
    assert hdf5io.available()
    Hn, nb, ns = 4, CFG["num_bursts"], CFG["num_burst_samples"]
    n = nb * ns
    base_cfg = dict(CFG, forecast=Hn, forecast_quantiles=[0.25, 0.75])
    # a global spec: today's call list and today's datasets
    g, gfiles, glog = _run(tmp_path, "global", dict(base_cfg, scenarios=SPEC), ext)
    names = _names(g)
    last = len(names) - names[::-1].index("forecast")
    assert names == PARENT_CALLS
    i = names.index("set_scenarios")
    assert g.calls[i][1].shape == (2, Hn) and names[i - 2:i] == ["reset_forecast", "keep_forecast_draws"]
    for f in gfiles:
        assert {k for k in f if k.startswith("scenarios/") or k.startswith("samples/scenario_")} == SCEN_SETS | {"scenarios/national_diff_quantiles"}
    # a local spec: the same calls, the set call's arrays [K, M, H]
    l, lfiles, llog = _run(tmp_path, "local", dict(base_cfg, scenarios=LOCAL_SPEC), ext)
    assert _names(l) == names
    sc = SC.resolve_locations(SC.parse_scenarios(LOCAL_SPEC, Hn), l.M)
    call = l.calls[_names(l).index("set_scenarios")]
    assert call[1].shape == (2, l.M, Hn) and np.array_equal(call[1], sc.log_shift) and np.array_equal(call[2], sc.commute) and call[3] == n
    for x, y in zip(l.calls, g.calls):
        if x[0] != "set_scenarios":
            assert len(x) == len(y) and all(callable(u) or isinstance(u, dict) or np.array_equal(u, v) for u, v in zip(x[1:], y[1:])), x[0]
    for c, f in enumerate(lfiles):
        new = {k for k in f if k.startswith("scenarios/") or k.startswith("samples/scenario_")}
        assert new == LOCAL_SETS | {"scenarios/national_diff_quantiles"}
        assert set(f) - new == set(gfiles[c]) - SCEN_SETS - {"scenarios/national_diff_quantiles"}
        assert np.array_equal(f["scenarios/log_shift_by_location"], sc.log_shift) and f["scenarios/log_shift_by_location"].shape == (2, l.M, Hn)
        assert np.array_equal(f["scenarios/commute_by_location"], sc.commute)
        assert (ext == ".hd5" or f["scenarios/locations"].dtype == np.uint8) and f["scenarios/locations"].tolist() == [[1, 1, 1], [1, 0, 1]]
    # with groups_scenarios: one switch call right behind the set, one read at the end
    t, tfiles, tlog = _run(tmp_path, "totals", dict(base_cfg, scenarios=LOCAL_SPEC, groups_scenarios="on"), ext)
    tn = _names(t)
    i = tn.index("set_scenarios")
    assert tn[i + 1] == "set_scenario_groups" and t.calls[i + 1][1] is True
    assert [tn.count(k) for k in NEW_CALLS] == [1, 1] and tn.index("read_scenario_group_draws") > last
    assert [nm for nm in tn if nm not in NEW_CALLS] == names
    rows = np.asarray(t.forecast_rows, np.int64)
    for c, f in enumerate(tfiles):
        new = {k for k in f if k.startswith("scenarios/") or k.startswith("samples/scenario_")}
        assert new == LOCAL_SETS | GROUP_SETS | {"scenarios/national_diff_quantiles", "scenarios/group_diff_quantiles"}
        for k in lfiles[c]:
            assert np.array_equal(f[k], lfiles[c][k], equal_nan=np.asarray(f[k]).dtype.kind == "f"), k
        fg = f["samples/forecast_by_group"]
        assert np.array_equal(fg, GroupStub._rows(t, rows, Hn)[:, c])
        by, diff = f["samples/scenario_by_group"], f["samples/scenario_diff_by_group"]
        assert by.shape == diff.shape == (n, 2, TABLE.G, Hn, 3) and by.dtype == diff.dtype == np.int64
        for k in range(2):
            assert np.array_equal(by[:, k], fg + k + 1) and np.all(diff[:, k] == k + 1)
        assert np.array_equal(diff, by - fg[:, None])
        q = f["scenarios/group_diff_quantiles"]
        assert q.shape == (2, 2, TABLE.G, Hn, 3) and np.array_equal(q, inf.draw_quantiles(diff, [0.25, 0.75]))
    lines = [ln for ln in tlog.split("\n") if ln.startswith("Scenario ") and ", group " in ln]
    assert len(lines) == 2 * TABLE.G
    assert lines[0] == SC.group_run_line("half", "all", np.ones((n * t.B, Hn, 3))) and lines[-1].startswith("Scenario lock, group ends:")
    assert "mean 8.0" in lines[-1] and "0.05 / 0.95 quantiles" in lines[-1]
    # without forecast_quantiles no quantile dataset
    _, pfiles, _ = _run(tmp_path, "noq", dict(CFG, forecast=Hn, scenarios=LOCAL_SPEC, groups_scenarios=True), ext)
    assert not any("quantiles" in k for k in pfiles[0]) and GROUP_SETS <= set(pfiles[0])
    # the key absent or off: none of the new calls
    for off in ({}, dict(groups_scenarios="off"), dict(groups_scenarios=False)):
        o, ofiles, _ = _run(tmp_path, "off", dict(base_cfg, scenarios=LOCAL_SPEC, **off), ext)
        assert _names(o) == names and set(ofiles[0]) == set(lfiles[0])


def test_the_replay_driver_sets_switches_and_reads_once(tmp_path):
    Hn, n, burst = 3, 7, 3
    cfg = dict(CFG, forecast=Hn, num_burst_samples=burst, num_bursts=3, thin=1)

    class Source:
        def __init__(self, c, P, M, T):
            rng = np.random.default_rng(c)
            self.path, self.theta, self.events = f"c{c}", rng.standard_normal((n, P)), rng.integers(0, 3, size=(n, M, T, 3)).astype(np.float64)

        def draws(self, rows):
            return self.theta[rows], self.events[rows]
    runs = {}
    for tag, extra in (("global", dict(scenarios=SPEC)), ("local", dict(scenarios=LOCAL_SPEC)),
                       ("totals", dict(scenarios=LOCAL_SPEC, groups_scenarios="on"))):
        s = LocalStub()
        names = [str(tmp_path / f"rp_{tag}_{c}.npz") for c in range(s.B)]
        posts = [inf.Posterior(name, s.M, s.T, 2, n, burst=burst, results=False, forecast=(Hn, n), groups=TABLE.G) for name in names]
        with open(os.devnull, "w") as log:
            pr = inf.product_records(s, dict(cfg, **extra), posts, log=log, seed=21, forecast_calendar=(np.ones(Hn), np.zeros(Hn)), total=n,
                                     results=False, groups=TABLE)
            R.replay_bursts(s, [Source(c, s.P, s.M, s.T) for c in range(s.B)], np.arange(n), burst, pr, log=log)
        for p in posts:
            p.close()
        runs[tag] = (s, [_read(name) for name in names])
    gn, ln, tn = (_names(runs[k][0]) for k in ("global", "local", "totals"))
    assert gn == ln and not any(k in gn for k in NEW_CALLS) and gn.count("replay") == 3
    i = tn.index("set_scenarios")
    assert tn[i - 1] == "reset_forecast" and tn[i + 1] == "set_scenario_groups" and "replay" not in tn[:i + 2]
    assert [tn.count(k) for k in NEW_CALLS] == [1, 1] and tn[-1] == "read_scenario_group_draws" and [nm for nm in tn if nm not in NEW_CALLS] == gn
    assert runs["local"][0].calls[ln.index("set_scenarios")][1].shape == (2, 3, Hn)
    g, l, t = (runs[k][1][0] for k in ("global", "local", "totals"))
    sets = lambda f: {k for k in f if k.startswith("scenarios/") or k.startswith("samples/scenario_")}   # noqa: E731
    assert sets(g) == SCEN_SETS and sets(l) == LOCAL_SETS and sets(t) == LOCAL_SETS | GROUP_SETS
    assert t["samples/scenario_by_group"].shape == (n, 2, TABLE.G, Hn, 3)


def test_the_flag_is_on_both_command_lines_and_absent_it_passes_nothing(tmp_path, monkeypatch):
    import yaml
    cpath, spath = str(tmp_path / "c.yaml"), str(tmp_path / "s.yaml")
    with open(cpath, "w") as f:
        yaml.safe_dump(dict(Mcmc=CFG), f)
    with open(spath, "w") as f:
        yaml.safe_dump(LOCAL_SPEC, f)
    seen = {}
    monkeypatch.setattr(inf, "mcmc", lambda *a, **kw: seen.update(kw=kw))
    inf.main(["-c", cpath, "-o", "x", "--forecast", "14", "--groups", "nations", "--scenarios", spath, "--groups-scenarios", "data.nc"])
    assert seen["kw"]["scenarios"] == LOCAL_SPEC and seen["kw"]["groups_scenarios"] is True and seen["kw"]["groups"] == "nations"
    inf.main(["-c", cpath, "-o", "x", "--forecast", "14", "--scenarios", spath, "data.nc"])
    assert "groups_scenarios" not in seen["kw"]
    monkeypatch.setattr(R, "replay_files", lambda *a, **kw: seen.update(kw=kw))
    R.main(["-c", cpath, "-o", "x", "--forecast", "14", "--groups", "nations", "--scenarios", spath, "--groups-scenarios", "data.nc", "p0.hd5"])
    assert seen["kw"]["scenarios"] == LOCAL_SPEC and seen["kw"]["groups_scenarios"] is True
    R.main(["-c", cpath, "-o", "x", "--forecast", "14", "data.nc", "p0.hd5"])
    assert "groups_scenarios" not in seen["kw"] and "scenarios" not in seen["kw"]


# ---- 5. the compiler's account ----------------------------------------------------------------------------------------
def test_the_kernels_account_owner_scenarios_local_and_the_resources_condition():
    res = H.kernel_account("scenarios_local")
    assert sorted(res) == ["k_scenario_local_begin<256>", "k_scenario_local_day<4>"]
    assert kernel_resources.OWNERS["scenarios_local"] == ("k_scenario_local_begin", "k_scenario_local_day")
    assert sorted(H.kernel_account("scenarios")) == ["k_scenario_begin<256>", "k_scenario_day<4>", "k_scenario_diff<4>"]
    day, ref = res["k_scenario_local_day<4>"], H.kernel_account()["k_scenario_day<4>"]
    assert day["vgpr"] <= ref["vgpr"] and day["occupancy_waves_per_simd"] >= ref["occupancy_waves_per_simd"]
    assert day["lds_bytes_per_block"] == 0
    assert day["scratch_bytes_per_lane"] <= 32 == ref["scratch_bytes_per_lane"] == H.kernel_account()["k_forecast_day"]["scratch_bytes_per_lane"]
    for k, v in res.items():
        assert v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
    begin = res["k_scenario_local_begin<256>"]
    assert begin["scratch_bytes_per_lane"] == 0 and begin["lds_bytes_per_block"] == 0


def test_the_scenario_kernels_keep_their_order_in_the_code_object(tmp_path):
    """A kernel template is emitted where the host code first names it: every begin instance lies in front of its day
    instance, the global pair in front of the local pair, and the local pair behind every other kernel of the library --
    what the host's launches (`scenarios_batch`, `scenarios_local_rollout` in seir_hip.hip) have to keep, so that no other
    kernel moves."""
    fn = H.device_functions(tmp_path)

    def at(part):
        hits = [v[0] for k, v in fn.items() if part in k]
        assert len(hits) == 1, (part, hits)
        return hits[0]

    begin, day = at("16k_scenario_beginILi256E"), at("14k_scenario_dayILi4E")
    lbegin, lday = at("22k_scenario_local_beginILi256E"), at("20k_scenario_local_dayILi4E")
    assert begin < day < lbegin < lday
    assert sorted(a for a, _ in fn.values())[-2:] == [lbegin, lday]

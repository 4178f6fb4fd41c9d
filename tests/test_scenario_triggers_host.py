"""Triggered scenarios, the parts that need no GPU: the entry points declared, exported and bound with the header's types; the
step of the rule (covid19uk_amd/csrc/trigger_update.h) compiled as plain C++ against a Python restatement on an exhaustive grid;
`trigger_states` against a plain Python loop and hand cases; the specification with `trigger:` and `then:`, every key, default
and refusal; run_mcmc and the replay driver with a stub sampler and the datasets they write; the compiler's account of the new
kernels."""
import itertools
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import __graft_entry__ as entry
from covid19uk_amd import _lib, hdf5io, kernel_resources
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.inference import options
from covid19uk_amd.posterior import replay as R
from covid19uk_amd.posterior import scenarios as SC
from tests import abi_lib
from tests import helpers as H
from tests.test_groups_host import TABLE
from tests.test_scenarios_host import SPEC
from tests.test_scenarios_local_host import LOCAL_SETS, LOCAL_SPEC, PARENT_CALLS, LocalStub, NoCalls, _names
from tests.test_summary_host import CFG, _read

INT32_MAX = 2 ** 31 - 1
NEW = {
    "seir_sampler_scenarios_set_triggered": "seir_sampler *s, int32_t K, const double *log_shift, const double *commute, "
                                            "const double *log_shift_on, const double *commute_on, const int32_t *on, "
                                            "const int32_t *off, const int32_t *params, int64_t cap",
    "seir_sampler_read_scenario_triggers": "seir_sampler *s, uint32_t *active_count",
    "seir_sampler_read_scenario_trigger_draws": "seir_sampler *s, int64_t first, int64_t count, int32_t *active_by_day",
    "seir_trigger_counts": "seir_ctx *ctx, const uint64_t *masks, int64_t n, int32_t B, int32_t M, int32_t H, uint64_t folded, "
                           "uint32_t *active_count, int32_t *active_by_day",
}


# ---- 1. the entry points ----------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound_with_the_headers_types():
    lib = abi_lib.check_symbols(NEW)
    text = open(abi_lib.HEADER).read()
    assert "Triggered scenarios on the device" in text and "#define SEIR_TRIGGER_MAX_WINDOW 28" in text
    assert "#define SEIR_ABI_VERSION 4" in text               # entry points are added, none changed
    for call in (lambda: lib.seir_sampler_scenarios_set_triggered(None, 0, None, None, None, None, None, None, None, 0),
                 lambda: lib.seir_sampler_read_scenario_triggers(None, None),
                 lambda: lib.seir_sampler_read_scenario_trigger_draws(None, 0, 0, None)):
        assert call() == _lib.ERR_INVALID and b"null sampler" in lib.seir_last_error()
    assert lib.seir_trigger_counts(None, None, 1, 1, 1, 1, 0, None, None) == _lib.ERR_INVALID


# ---- 2. trigger_update.h as plain C++ ---------------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include "trigger_update.h"
// per line "active age c on off min_days review": the step, then the day behind it; prints "active age_behind_the_step age_behind_the_day"
int main() {
    int active, age, c, on, off, min_days, review;
    while (scanf("%d %d %d %d %d %d %d", &active, &age, &c, &on, &off, &min_days, &review) == 7) {
        int32_t a = active, g = age;
        seir::trigger_step(a, g, c, on, off, min_days, review != 0);
        int32_t g2 = g;
        seir::trigger_after_day(a, g2);
        printf("%d %d %d\n", (int)a, (int)g, (int)g2);
    }
    return 0;
}
"""
REVIEW_DRIVER = r"""
#include <cstdio>
#include "trigger_update.h"
int main() {
    int s, from_day, every;
    while (scanf("%d %d %d", &s, &from_day, &every) == 3) printf("%d\n", seir::trigger_review(s, from_day, every) ? 1 : 0);
    return 0;
}
"""


def _compile(tmp, name, text):
    cxx = None
    for cand in ("g++", "c++", "clang++"):
        if shutil.which(cand):
            cxx = [cand]
            break
    if cxx is None:
        cxx = [entry._hipcc(), "-x", "c++"]
    src, exe = tmp / f"{name}.cpp", tmp / name
    src.write_text(text)
    subprocess.run(cxx + ["-std=c++17", "-O1", "-Wall", "-Werror", "-I", entry.CSRC, "-o", str(exe), str(src)],
                   check=True, capture_output=True, text=True)

    def run(rows):
        out = subprocess.run([str(exe)], input="\n".join(" ".join(str(v) for v in r) for r in rows) + "\n", check=True,
                             capture_output=True, text=True).stdout.split("\n")
        return [tuple(int(v) for v in row.split()) for row in out if row]
    return run


def _python_step(active, age, c, on, off, min_days, review):
    """The issue's words, one branch per sentence."""
    if review:
        if not active and c >= on:
            active, age = 1, 0
        elif active and age >= min_days and c < off:
            active = 0
    return active, age, age + 1 if active else age


def test_the_step_as_plain_cpp_equals_the_python_restatement_on_an_exhaustive_grid(tmp_path):
    run = _compile(tmp_path, "step", DRIVER)
    rows = []
    for on, off in ((7, 3), (7, 7), (INT32_MAX, 5), (INT32_MAX, INT32_MAX), (0, 0), (5, 0), (1, 1)):
        for c in sorted({max(off - 1, 0), off, max(on - 1, 0), on, 0}):
            for active, age, min_days, review in itertools.product((0, 1), range(4), range(4), (0, 1)):
                rows.append((active, age, c, on, off, min_days, review))
    got = run(rows)
    assert len(got) == len(rows) > 1000
    for r, g in zip(rows, got):
        assert g == _python_step(*r), (r, g)
    fired = sum(1 for r, g in zip(rows, got) if not r[0] and g[0])
    released = sum(1 for r, g in zip(rows, got) if r[0] and not g[0])
    assert fired and released
    # on = INT32_MAX: never, whatever a count below it is; on = 0: at every review; off = 0: never released
    assert not any(g[0] for r, g in zip(rows, got) if r[3] == INT32_MAX and not r[0] and r[2] < INT32_MAX)
    assert all(g[0] for r, g in zip(rows, got) if r[3] == 0 and not r[0] and r[6])
    assert all(g[0] for r, g in zip(rows, got) if r[4] == 0 and r[0])
    review = _compile(tmp_path, "review", REVIEW_DRIVER)
    grid = [(s, f, e) for s in range(12) for f in range(6) for e in (1, 2, 3, 7, 200)]
    assert [v[0] for v in review(grid)] == [int(s >= f and (s - f) % e == 0) for s, f, e in grid]


# ---- 3. trigger_states ------------------------------------------------------------------------------------------------
def _loop_states(history, cases, on, off, w, from_day, min_days, review_every):
    """One series, in plain Python: the state of the issue, the window a list."""
    past = [0] * max(w - len(history), 0) + [int(v) for v in history][-w:]
    active, age, out = 0, 0, []
    for s, y in enumerate(cases):
        c = sum(past[-w:])
        active, _, age = _python_step(active, age, c, on, off, min_days, s >= from_day and (s - from_day) % review_every == 0)
        out.append(active)
        past.append(int(y))
    return out


def test_trigger_states_equals_a_plain_loop_over_random_series():
    rng = np.random.default_rng(5)
    for w, min_days, review_every, from_day in itertools.product((1, 3, 7, 28), (0, 3), (1, 7), (0, 2)):
        n, M, Hn, h = 3, 4, 40, int(rng.integers(0, 35))
        hist, cases = rng.integers(0, 6, size=(n, M, h)), rng.integers(0, 6, size=(n, M, Hn))
        on = rng.integers(1, 3 * w + 2, size=M)
        off = on // 2
        got = SC.trigger_states(hist, cases, on, off, w, from_day, min_days, review_every)
        assert got.dtype == np.uint8 and got.shape == (n, M, Hn)
        for d in range(n):
            for m in range(M):
                assert got[d, m].tolist() == _loop_states(hist[d, m], cases[d, m], int(on[m]), int(off[m]), w, from_day, min_days,
                                                          review_every), (w, min_days, review_every, from_day, d, m)
    assert got.any() and not got.all()


def test_trigger_states_by_hand():
    st = lambda hist, cases, **kw: SC.trigger_states(hist, cases, kw.pop("on", 6), kw.pop("off", 3), kw.pop("w", 3),   # noqa: E731
                                                     kw.pop("from_day", 0), kw.pop("min_days", 0), kw.pop("review_every", 1)).tolist()
    # the window reaches 6 at the start of day 2 (1 + 2 + 3), not the day before (0 + 1 + 2)
    assert st([0, 0, 1], [2, 3, 0, 0, 0, 0, 0]) == [0, 0, 1, 1, 1, 0, 0]              # day 4: 3 + 0 + 0 is not below 3; day 5: 0 is
    # min_days = 4 keeps it on with the window below off: fired on day 2, ages 0, 1, 2, 3 behind days 2..5, released on day 6
    assert st([0, 0, 1], [2, 3, 0, 0, 0, 0, 0, 0], min_days=4) == [0, 0, 1, 1, 1, 1, 0, 0]
    # ... at the next review: reviews on days 0, 3, 6 -- fires on day 3 (2 + 3 + 1), releases on day 6, fires again on day 9
    assert st([0, 0, 1], [2, 3, 1, 0, 0, 0, 2, 2, 2, 0, 0, 0], review_every=3) == [0, 0, 0, 1, 1, 1, 0, 0, 0, 1, 1, 1]
    # only on review days: the window is at 6 on days 2 and 3 and back below it on day 4 -- a review on days 0 and 4 misses it
    assert st([0, 0, 0], [3, 3, 0, 0, 0, 0], review_every=4) == [0] * 6
    assert st([0, 0, 0], [3, 3, 0, 0, 0, 0]) == [0, 0, 1, 1, 1, 0]
    # nothing before from_day, though the window is above on from day 0
    assert st([9, 9, 9], [9] * 6, from_day=4) == [0, 0, 0, 0, 1, 1]
    assert st([9, 9, 9], [9] * 3, from_day=3) == [0, 0, 0]                             # from_day = H: no review
    # w = 1: yesterday alone; w = 28: four weeks, of which the history is the last 28
    assert st([5, 6], [0, 6, 0], w=1, off=6) == [1, 0, 1]
    assert st([1] * 40, [0] * 30, w=28, on=28, off=28) == [1] + [0] * 29
    assert st([1] * 40, [0] * 30, w=28, on=29, off=0) == [0] * 30
    # a history shorter than the window is preceded by zeros; no history at all
    assert st([4], [1, 1, 0, 0], w=3) == [0, 0, 1, 0]
    assert st(np.zeros((0,), int), [6, 0, 0, 0], w=3) == [0, 1, 1, 1]
    # on = INT32_MAX never fires; on = 0 with off = 0 fires at day 0 and stays
    assert st([9, 9, 9], [9] * 4, on=INT32_MAX) == [0] * 4
    assert st([0, 0, 0], [0] * 4, on=0, off=0) == [1] * 4


def test_the_record_and_its_fold_in_numpy():
    rng = np.random.default_rng(2)
    act = rng.integers(0, 2, size=(5, 2, 3, 100)).astype(np.uint8)
    mk = SC.trigger_masks(act)
    assert mk.dtype == np.uint64 and mk.shape == (5, 2, 3, 2)
    assert int(mk[1, 1, 2, 1]) == sum(int(v) << s for s, v in enumerate(act[1, 1, 2, 64:]))
    f = SC.fold_triggers(mk, 100)
    assert np.array_equal(f["active_count"], act.sum(axis=0)) and np.array_equal(f["active_by_day"], act.sum(axis=2))
    g = SC.fold_triggers(mk[3:], 100, acc=SC.fold_triggers(mk[:3], 100))
    assert g["count"] == 5 and np.array_equal(g["active_count"], f["active_count"])


# ---- 4. the specification ---------------------------------------------------------------------------------------------
TIER = {"trigger": {"cases_per_100k": 200, "release_per_100k": 100, "window": 7, "min_days": 14, "review_every": 7, "from_day": 0,
                    "locations": ["E0*"]},
        "then": {"transmission": 0.7, "commute": 0.5}}
TRIG_SPEC = {"half": {"transmission": 0.5, "from_day": 1},
             "tier": dict(TIER, trigger=dict(TIER["trigger"], locations=[0, 2]), locations=[0, 1], commute=0.8, from_day=1)}
POP = np.array([150000.0, 1234.0, 99999.0])


def test_every_key_and_default_of_a_trigger_and_the_two_pairs():
    Hn, M = 6, 3
    pend = SC.parse_scenarios(TRIG_SPEC, Hn)
    assert isinstance(pend, SC.PendingScenarios) and SC.is_triggered(pend) and SC.is_local(pend)
    assert pend.rules[0] is None and pend.rules[1] == SC.TriggerRule(True, 200.0, 100.0, 7, 0, 14, 7, (0, 2))
    sc = SC.resolve_locations(pend, M, None, POP)
    assert isinstance(sc, SC.TriggeredScenarios) and SC.is_triggered(sc) and sc.names == ("half", "tier")
    # the off pair is today's targeted tensors
    plain = SC.resolve_locations(SC.parse_scenarios({"half": TRIG_SPEC["half"], "tier": {"locations": [0, 1], "commute": 0.8, "from_day": 1}},
                                                    Hn), M)
    assert np.array_equal(sc.log_shift, plain.log_shift) and np.array_equal(sc.commute, plain.commute)
    assert np.array_equal(sc.locations, plain.locations)
    # the on pair: `then` multiplies the off pair's multipliers on every day, in float64
    tr_off, cm_off = np.ones((M, Hn)), np.ones((M, Hn))
    cm_off[[0, 1], 1:] = 0.8
    assert np.array_equal(sc.log_shift_on[1], np.log(tr_off * 0.7)) and np.array_equal(sc.commute_on[1], cm_off * 0.5)
    # a scenario without a trigger: on = INT32_MAX everywhere, its on pair its off pair, the default parameters
    assert np.array_equal(sc.log_shift_on[0], sc.log_shift[0]) and np.array_equal(sc.commute_on[0], sc.commute[0])
    assert sc.trigger_on[0].tolist() == [INT32_MAX] * M and sc.trigger_off[0].tolist() == [0] * M
    assert sc.triggered.tolist() == [0, 1]
    # locations that may not trigger: INT32_MAX; the others by the per-100k rule
    assert sc.trigger_on[1].tolist() == [300, INT32_MAX, 200] and sc.trigger_off[1].tolist() == [150, 0, 100]
    assert sc.trigger_on.dtype == sc.trigger_off.dtype == sc.window.dtype == np.int32
    assert (sc.window.tolist(), sc.from_day.tolist(), sc.min_days.tolist(), sc.review_every.tolist()) == ([7, 7], [0, 0], [0, 14], [1, 7])
    assert set(sc.trigger_args()) == {"log_shift_on", "commute_on", "on", "off", "window", "from_day", "min_days", "review_every"}
    with pytest.raises(ValueError):
        sc.trigger_on[0, 0] = 1                               # read-only, as every resolved array
    # the defaults: release = the on value, window 7, min_days 0, review_every 1, from_day 0, every location, then = identity
    d = SC.resolve_locations(SC.parse_scenarios({"t": {"trigger": {"cases": 40}}}, Hn), M)
    assert d.trigger_on.tolist() == [[40] * M] and d.trigger_off.tolist() == [[40] * M]
    assert (d.window[0], d.from_day[0], d.min_days[0], d.review_every[0]) == (7, 0, 0, 1)
    assert np.array_equal(d.log_shift_on, d.log_shift) and not d.log_shift.any() and np.array_equal(d.commute_on, np.ones((1, M, Hn)))
    # absolute counts need no populations; a trigger with parts; from_day = H is a rule that is never reviewed
    p = SC.resolve_locations(SC.parse_scenarios({"t": {"parts": [{"locations": [1], "transmission": 0.5}],
                                                       "trigger": {"cases": 9, "release": 2, "from_day": Hn, "window": 28},
                                                       "then": {"commute": [0, 1, 2, 3, 4, 5]}}}, Hn), M)
    assert p.trigger_off.tolist() == [[2] * M] and p.from_day[0] == Hn and p.window[0] == 28
    assert np.array_equal(p.commute_on[0], np.tile(np.arange(6.0), (M, 1))) and np.array_equal(p.log_shift_on, p.log_shift)
    # the simulator's view: one rounded add and one rounded multiply, either pair
    a_path, W = np.linspace(-1, 1, 2 * Hn).reshape(2, Hn), np.linspace(1, 2, Hn)
    (a0, w0), (a1, w1) = SC.triggered_inputs(a_path, W, sc, 1)
    assert np.array_equal(a0, SC.local_inputs(a_path, W, sc, 1)[0]) and np.array_equal(w0, SC.local_inputs(a_path, W, sc, 1)[1])
    assert a1[1, 2, 3] == float(a_path[1, 3]) + float(sc.log_shift_on[1, 2, 3]) and w1[0, 4] == float(W[4]) * float(sc.commute_on[1, 0, 4])


def test_the_per_100k_rule_against_fractions():
    rng = np.random.default_rng(1)
    pops = np.concatenate([rng.integers(1, 10 ** 7, size=200).astype(np.float64), [1.0, 1e5, 2e5, 123456.5, 9.9e6]])
    for rate in (200, 100, 0, 0.1, 1e-9, 37.5, 1e5, 99999.99999):
        got = SC.threshold_counts(rate, pops)
        for g, n in zip(got, pops):
            exact = Fraction(rate) * Fraction(n) / 100000
            assert isinstance(g, int) and g - 1 < exact <= g, (rate, n, g)
    assert SC.threshold_counts(200, [1e5, 150000, 1]) == [200, 300, 1]
    # above INT32_MAX: refused, by location
    pend = SC.parse_scenarios({"t": {"trigger": {"cases_per_100k": 1e5}}}, 3)
    with pytest.raises(ValueError, match="location 1 is 3000000000 cases, above 2147483647"):
        SC.resolve_locations(pend, 2, None, [5.0, 3e9])
    with pytest.raises(ValueError, match="need the 2 populations"):
        SC.resolve_locations(pend, 2)


def test_a_spec_without_the_new_keys_resolves_to_the_objects_it_resolves_to_today():
    import dataclasses
    Hn = 5
    g = options.bind_scenarios(options.resolve_scenarios({"scenarios": SPEC}, Hn), 3, lambda: 1 / 0, lambda: 1 / 0)
    assert type(g) is SC.Scenarios and [f.name for f in dataclasses.fields(g)] == ["names", "horizon", "log_shift", "commute"]
    pend = options.resolve_scenarios({"scenarios": LOCAL_SPEC}, Hn)
    assert type(pend) is SC.PendingScenarios and pend.rules == () and pend.then == () and not SC.is_triggered(pend)
    l = options.bind_scenarios(pend, 3, None, None)             # no populations asked for
    assert type(l) is SC.LocalScenarios and not SC.is_triggered(l)
    assert [f.name for f in dataclasses.fields(l)] == ["names", "horizon", "log_shift", "commute", "locations"]
    assert "triggers" not in " ".join(options.PRODUCT_KEYS)


@pytest.mark.parametrize("spec,word", [
    ({"a": {"trigger": {}}}, "exactly one of cases_per_100k and cases"),
    ({"a": {"trigger": {"cases": 5, "cases_per_100k": 5}}}, "exactly one of cases_per_100k and cases"),
    ({"a": {"trigger": {"cases": 5, "release_per_100k": 1}}}, "takes the form of the trigger's, release"),
    ({"a": {"trigger": {"cases_per_100k": 5, "release": 1}}}, "takes the form of the trigger's, release_per_100k"),
    ({"a": {"trigger": {"cases": 5, "release": 6}}}, "release=6 is above cases=5"),
    ({"a": {"trigger": {"cases_per_100k": 5, "release_per_100k": 5.5}}}, "release_per_100k=5.5 is above cases_per_100k=5.0"),
    ({"a": {"trigger": {"cases": 5, "when": 1}}}, "a mapping with the keys cases_per_100k"),
    ({"a": {"trigger": [5]}}, "a mapping with the keys cases_per_100k"),
    ({"a": {"trigger": {"cases": -1}}}, "a.trigger.cases=-1"),
    ({"a": {"trigger": {"cases": 2.5}}}, "a.trigger.cases=2.5"),
    ({"a": {"trigger": {"cases": 2 ** 31}}}, "a.trigger.cases=2147483648"),
    ({"a": {"trigger": {"cases": True}}}, "a.trigger.cases=True"),
    ({"a": {"trigger": {"cases_per_100k": -0.5}}}, "a finite rate >= 0"),
    ({"a": {"trigger": {"cases_per_100k": float("nan")}}}, "a finite rate >= 0"),
    ({"a": {"trigger": {"cases_per_100k": "200"}}}, "a finite rate >= 0"),
    ({"a": {"trigger": {"cases": 5, "window": 0}}}, r"window=0: days in \[1, 28\]"),
    ({"a": {"trigger": {"cases": 5, "window": 29}}}, r"window=29: days in \[1, 28\]"),
    ({"a": {"trigger": {"cases": 5, "from_day": -1}}}, r"from_day=-1: a forecast day in \[0, 3\]"),
    ({"a": {"trigger": {"cases": 5, "from_day": 4}}}, r"from_day=4: a forecast day in \[0, 3\]"),
    ({"a": {"trigger": {"cases": 5, "min_days": -1}}}, "min_days=-1: days >= 0"),
    ({"a": {"trigger": {"cases": 5, "review_every": 0}}}, "review_every=0: days >= 1"),
    ({"a": {"trigger": {"cases": 5, "review_every": 1.5}}}, "review_every=1.5"),
    ({"a": {"trigger": {"cases": 5, "locations": []}}}, "a.trigger.locations=.*non-empty list"),
    ({"a": {"trigger": {"cases": 5, "locations": "E0*"}}}, "a.trigger.locations=.*non-empty list"),
    ({"a": {"then": {"transmission": 0.5}}}, "a.then without a.trigger"),
    ({"a": {"trigger": {"cases": 5}, "then": {"transmission": 0.0}}}, "a.then.transmission.*> 0"),
    ({"a": {"trigger": {"cases": 5}, "then": {"commute": -1}}}, "a.then.commute.*>= 0"),
    ({"a": {"trigger": {"cases": 5}, "then": {"commute": [1, 1]}}}, "a.then.commute has 2 values, the forecast has 3 days"),
    ({"a": {"trigger": {"cases": 5}, "then": {"from_day": 1}}}, "a.then: a mapping with the keys transmission, commute"),
    ({"a": {"trigger": {"cases": 5}, "where": 1}}, "keys transmission, commute, from_day, locations"),
    ({"a": {"trigger": {"cases": 5}, "parts": [{}], "transmission": 0.5}}, "carries nothing else"),
])
def test_every_stage_one_refusal_happens_with_no_file_opened(spec, word, tmp_path):
    with pytest.raises(ValueError, match=word):
        SC.parse_scenarios(spec, 3)
    nofile, out = str(tmp_path / "no_such_file.nc"), str(tmp_path / "out.npz")
    with pytest.raises(ValueError, match=word):             # inference.mcmc: before the data file is opened
        inf.mcmc(nofile, out, dict(CFG, forecast=3, scenarios=spec))
    assert not os.path.exists(out)
    with pytest.raises(ValueError, match="scenarios given without forecast"):
        inf.mcmc(nofile, out, dict(CFG, scenarios={"a": {"trigger": {"cases": 5}}}))


@pytest.mark.parametrize("spec,names,pop,word", [
    ({"a": {"trigger": {"cases": 5, "locations": ["E99"]}}}, ["E01", "E02", "W01"], None, "a.trigger.locations: .*unknown location code 'E99'"),
    ({"a": {"trigger": {"cases": 5, "locations": [3]}}}, None, None, r"a.trigger.locations: .*index 3 outside \[0, M=3\)"),
    ({"a": {"trigger": {"cases_per_100k": 5}}}, None, None, "per-100k thresholds need the 3 populations"),
    ({"a": {"trigger": {"cases_per_100k": 1e5}}}, None, [1.0, 2.0, 4e9], "location 2 is 4000000000 cases"),
])
def test_every_stage_two_refusal_happens_with_no_gpu_call(spec, names, pop, word):
    pend = SC.parse_scenarios(spec, 3)                          # stage one has nothing to object to
    with pytest.raises(ValueError, match=word):
        inf.run_mcmc(NoCalls(), dict(CFG, forecast=3, scenarios=spec), [], log=open(os.devnull, "w"),
                     forecast_calendar=(np.ones(3), np.ones(3)), location_names=names,
                     **({} if pop is None else dict(population=np.asarray(pop))))
    assert SC.is_triggered(pend)


# ---- 5. run_mcmc and the replay driver with a stub sampler; the datasets ----------------------------------------------
NEW_CALLS = ("scenario_triggers", "read_scenario_trigger_draws")
TRIG_SETS = {f"scenarios/{k}" for k in ("trigger_on", "trigger_off", "trigger_window", "trigger_from_day", "trigger_min_days",
                                        "trigger_review_every", "log_shift_on_by_location", "commute_on_by_location", "active_count",
                                        "p_active")} | {"samples/scenario_active_by_day"}


class TriggerStub(LocalStub):
    """The targeted scenarios' stub with the keyword and the two reads: location m is under scenario k's measure on day s in
    (row + m + s + k) % 3 == 0 of the draws."""
    triggers = None

    def set_scenarios(self, log_shift, commute, cap, **kw):
        super().set_scenarios(log_shift, commute, cap)
        if kw:
            assert set(kw) == {"triggers"}
            self.triggers = kw["triggers"]
            self.calls[-1] = self.calls[-1] + (kw["triggers"],)

    def _active(self):
        rows = np.asarray(self.forecast_rows, np.int64)
        k, m, h = np.arange(self.K_sc), np.arange(self.M), np.arange(self.H)
        return ((rows[None, :, None, None, None] + m[None, None, None, :, None] + h[None, None, None, None, :]
                 + k[:, None, None, None, None]) % 3 == 0) & np.ones((1, 1, self.B, 1, 1), bool)     # [K, n, B, M, H]

    def scenario_triggers(self):
        self.calls.append(("scenario_triggers",))
        a = self._active()
        return dict(count=a.shape[1], active_count=a.sum(axis=1).astype(np.uint32))

    def read_scenario_trigger_draws(self, count=None, first=0):
        self.calls.append(("read_scenario_trigger_draws", count, first))
        return self._active().sum(axis=3).astype(np.int32)


def _run(tmp_path, tag, config, ext=".npz", **kw):
    s = TriggerStub()
    s.cap = 800
    nb, ns = config["num_bursts"], config["num_burst_samples"]
    Hn, _ = inf.forecast_mode(config)
    names = [str(tmp_path / f"{tag}_{c}{ext}") for c in range(s.B)]
    posts = [inf.Posterior(name, s.M, s.T, 2, inf.warmup_size() + nb * ns, forecast=(Hn, nb * ns), groups=TABLE.G) for name in names]
    logname = str(tmp_path / f"{tag}.log")
    with open(logname, "w") as log:
        inf.run_mcmc(s, config, posts, log=log, forecast_calendar=(np.arange(Hn) + 0.5, np.arange(Hn) - 1.0), seed=21, groups=TABLE, **kw)
    for p in posts:
        p.close()
    return s, [_read(n) for n in names], open(logname).read()


@pytest.mark.parametrize("ext", [".npz", ".hd5"])
def test_run_mcmc_sets_one_triggered_set_and_reads_twice_at_the_end(tmp_path, ext):
    assert hdf5io.available()
    Hn, nb, ns = 4, CFG["num_bursts"], CFG["num_burst_samples"]
    n = nb * ns
    base_cfg = dict(CFG, forecast=Hn, forecast_quantiles=[0.25, 0.75])
    spec = dict(LOCAL_SPEC, tier=dict(TIER, trigger=dict(TIER["trigger"], locations=[0, 2])))
    # without the key: the parent's calls and datasets, nothing new called
    l, lfiles, _ = _run(tmp_path, "local", dict(base_cfg, scenarios=LOCAL_SPEC), ext, population=POP)
    assert _names(l) == PARENT_CALLS and l.triggers is None and len(l.calls[_names(l).index("set_scenarios")]) == 4
    t, tfiles, tlog = _run(tmp_path, "trig", dict(base_cfg, scenarios=spec), ext, population=POP)
    tn = _names(t)
    assert [nm for nm in tn if nm not in NEW_CALLS] == PARENT_CALLS and [tn.count(k) for k in NEW_CALLS] == [1, 1]
    last = len(tn) - tn[::-1].index("forecast")
    assert tn.count("set_scenarios") == 1 and min(tn.index(k) for k in NEW_CALLS) > last
    sc = SC.resolve_locations(SC.parse_scenarios(spec, Hn), t.M, None, POP)
    call = t.calls[tn.index("set_scenarios")]
    assert np.array_equal(call[1], sc.log_shift) and np.array_equal(call[2], sc.commute) and call[3] == n
    assert set(call[4]) == set(sc.trigger_args()) and all(np.array_equal(call[4][k], v) for k, v in sc.trigger_args().items())
    assert call[4]["on"].tolist() == [[INT32_MAX] * 3, [INT32_MAX] * 3, [300, INT32_MAX, 200]]
    # every other call and keyword as in the run without the key (the scenarios' own arrays aside: one scenario more)
    others = lambda s: [c for c in s.calls if c[0] not in NEW_CALLS + ("set_scenarios",)]   # noqa: E731
    for x, y in zip(others(t), others(l)):
        assert x[0] == y[0] and len(x) == len(y)
        assert all(callable(u) or isinstance(u, dict) or np.array_equal(u, v) for u, v in zip(x[1:], y[1:])), x[0]
    act = t._active()
    for c, f in enumerate(tfiles):
        new = {k for k in f if k.startswith("scenarios/") or k.startswith("samples/scenario_")}
        assert new == LOCAL_SETS | TRIG_SETS | {"scenarios/national_diff_quantiles", "scenarios/active_by_day_quantiles"}
        assert set(f) - new == set(lfiles[c]) - LOCAL_SETS - {"scenarios/national_diff_quantiles"}
        assert np.array_equal(f["scenarios/trigger_on"], sc.trigger_on) and np.array_equal(f["scenarios/trigger_off"], sc.trigger_off)
        for key, v in (("window", sc.window), ("from_day", sc.from_day), ("min_days", sc.min_days), ("review_every", sc.review_every)):
            assert np.array_equal(f[f"scenarios/trigger_{key}"], v) and f[f"scenarios/trigger_{key}"].shape == (3,)
        assert np.array_equal(f["scenarios/log_shift_on_by_location"], sc.log_shift_on) and np.array_equal(f["scenarios/commute_on_by_location"], sc.commute_on)
        cnt = f["scenarios/active_count"]
        assert cnt.shape == (3, t.M, Hn) and (ext == ".hd5" or cnt.dtype == np.uint32) and np.array_equal(cnt, act[:, :, c].sum(axis=1))
        assert np.array_equal(f["scenarios/p_active"], cnt / f["scenarios/count"][0]) and f["scenarios/count"][0] == n
        by = f["samples/scenario_active_by_day"]
        assert by.shape == (n, 3, Hn) and (ext == ".hd5" or by.dtype == np.int32)
        assert np.array_equal(by, np.moveaxis(act[:, :, c].sum(axis=2), 0, 1))
        q = f["scenarios/active_by_day_quantiles"]
        assert q.shape == (2, 3, Hn) and np.array_equal(q, inf.draw_quantiles(by, [0.25, 0.75]))
    lines = [ln for ln in tlog.split("\n") if "the measure triggers somewhere" in ln]
    assert len(lines) == 1 and lines[0] == SC.trigger_run_line("tier", np.moveaxis(act[2].sum(axis=2), 0, 1).reshape(-1, Hn))
    assert lines[0].startswith("Scenario tier: the measure triggers somewhere in 1.000 of") and "mean first day 0.0" in lines[0]
    # without forecast_quantiles no quantile dataset
    _, pfiles, _ = _run(tmp_path, "noq", dict(CFG, forecast=Hn, scenarios=spec), ext, population=POP)
    assert not any("quantiles" in k for k in pfiles[0]) and TRIG_SETS <= set(pfiles[0])


def test_the_replay_driver_sets_one_triggered_set_and_reads_twice_at_the_end(tmp_path):
    Hn, n, burst = 3, 7, 3
    cfg = dict(CFG, forecast=Hn, num_burst_samples=burst, num_bursts=3, thin=1)
    spec = dict(LOCAL_SPEC, tier={"trigger": {"cases": 4, "release": 2, "window": 3}, "then": {"transmission": 0.5}})

    class Source:
        def __init__(self, c, P, M, T):
            rng = np.random.default_rng(c)
            self.path, self.theta, self.events = f"c{c}", rng.standard_normal((n, P)), rng.integers(0, 3, size=(n, M, T, 3)).astype(np.float64)

        def draws(self, rows):
            return self.theta[rows], self.events[rows]
    runs = {}
    for tag, extra in (("local", dict(scenarios=LOCAL_SPEC)), ("trig", dict(scenarios=spec))):
        s = TriggerStub()
        names = [str(tmp_path / f"rp_{tag}_{c}.npz") for c in range(s.B)]
        posts = [inf.Posterior(name, s.M, s.T, 2, n, burst=burst, results=False, forecast=(Hn, n), groups=TABLE.G) for name in names]
        with open(os.devnull, "w") as log:
            pr = inf.product_records(s, dict(cfg, **extra), posts, log=log, seed=21, forecast_calendar=(np.ones(Hn), np.zeros(Hn)), total=n,
                                     results=False, groups=TABLE)
            R.replay_bursts(s, [Source(c, s.P, s.M, s.T) for c in range(s.B)], np.arange(n), burst, pr, log=log)
        for p in posts:
            p.close()
        runs[tag] = (s, [_read(name) for name in names])
    ln, tn = (_names(runs[k][0]) for k in ("local", "trig"))
    assert not any(k in ln for k in NEW_CALLS) and runs["local"][0].triggers is None
    assert [nm for nm in tn if nm not in NEW_CALLS] == ln and tn[-2:] == list(NEW_CALLS) and tn.count("set_scenarios") == 1
    i = tn.index("set_scenarios")
    assert tn[i - 1] == "reset_forecast" and "replay" not in tn[:i + 1]
    assert runs["trig"][0].triggers["on"].tolist() == [[INT32_MAX] * 3, [INT32_MAX] * 3, [4, 4, 4]]
    sets = lambda f: {k for k in f if k.startswith("scenarios/") or k.startswith("samples/scenario_")}   # noqa: E731
    assert sets(runs["local"][1][0]) == LOCAL_SETS and sets(runs["trig"][1][0]) == LOCAL_SETS | TRIG_SETS
    assert runs["trig"][1][0]["samples/scenario_active_by_day"].shape == (n, 3, Hn)


def test_a_scenarios_file_with_a_trigger_reaches_both_drivers(tmp_path, monkeypatch):
    import yaml
    cpath, spath = str(tmp_path / "c.yaml"), str(tmp_path / "s.yaml")
    with open(cpath, "w") as f:
        yaml.safe_dump(dict(Mcmc=CFG), f)
    with open(spath, "w") as f:
        yaml.safe_dump({"tier": TIER}, f)
    seen = {}
    monkeypatch.setattr(inf, "mcmc", lambda *a, **kw: seen.update(kw=kw))
    inf.main(["-c", cpath, "-o", "x", "--forecast", "14", "--scenarios", spath, "data.nc"])
    assert seen["kw"]["scenarios"] == {"tier": TIER}
    monkeypatch.setattr(R, "replay_files", lambda *a, **kw: seen.update(kw=kw))
    R.main(["-c", cpath, "-o", "x", "--forecast", "14", "--scenarios", spath, "data.nc", "p0.hd5"])
    assert seen["kw"]["scenarios"] == {"tier": TIER}


# ---- 6. the compiler's account ----------------------------------------------------------------------------------------
def test_the_kernels_account_owner_scenario_triggers_and_the_day_kernels_keep_theirs():
    res = H.kernel_account("scenario_triggers")
    assert sorted(res) == ["k_scenario_trigger_day<4>", "k_trigger_begin<0>", "k_trigger_begin<1>", "k_trigger_fold<4>"]
    assert kernel_resources.OWNERS["scenario_triggers"] == ("k_trigger_begin", "k_scenario_trigger_day", "k_trigger_fold")
    for k, v in res.items():
        assert v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["lds_bytes_per_block"] == 0, (k, v)
    every = H.kernel_account()
    day, ref = res["k_scenario_trigger_day<4>"], every["k_scenario_local_day<4>"]
    print("k_scenario_trigger_day<4>:", day, "k_scenario_local_day<4>:", ref)
    assert ref["vgpr"] == 118 and ref["occupancy_waves_per_simd"] == 4 and ref["scratch_bytes_per_lane"] == 32
    assert day["scratch_bytes_per_lane"] <= 32          # sim_binomial's, as in every day kernel: nothing of the rule is in scratch
    for k in ("k_trigger_begin<0>", "k_trigger_begin<1>", "k_trigger_fold<4>"):
        assert res[k]["scratch_bytes_per_lane"] == 0
    # the three existing day kernels: the figures the account held for them before the rule came, as literals
    was = {
        'k_forecast_day': {"agpr": 0, "lds_bytes_per_block": 0, "occupancy_waves_per_simd": 4, "scratch_bytes_per_lane": 32, "sgpr": 62, "sgpr_spill": 0, "vgpr": 118, "vgpr_spill": 0},
        'k_scenario_day<4>': {"agpr": 0, "lds_bytes_per_block": 0, "occupancy_waves_per_simd": 4, "scratch_bytes_per_lane": 32, "sgpr": 54, "sgpr_spill": 0, "vgpr": 118, "vgpr_spill": 0},
        'k_scenario_local_day<4>': {"agpr": 0, "lds_bytes_per_block": 0, "occupancy_waves_per_simd": 4, "scratch_bytes_per_lane": 32, "sgpr": 57, "sgpr_spill": 0, "vgpr": 118, "vgpr_spill": 0}
    }
    for k, v in was.items():
        assert every[k] == v, (k, every[k])


def test_the_new_kernels_lie_in_front_of_the_local_pair_and_behind_every_other_kernel(tmp_path):
    """A kernel template is emitted where the host code first names it (all four are templates for that reason): begin, day and
    fold lie behind every kernel the library had but `k_scenario_local_begin / _day`, which keep the last two places of the code
    object (tests/test_scenarios_local_host.py) -- so no other kernel moves."""
    fn = H.device_functions(tmp_path)

    def at(part):
        hits = [v[0] for k, v in fn.items() if part in k]
        assert len(hits) == 1, (part, hits)
        return hits[0]

    new = [at("15k_trigger_beginILi1E"), at("15k_trigger_beginILi0E"), at("22k_scenario_trigger_dayILi4E"), at("14k_trigger_foldILi4E")]
    assert new == sorted(new)                                   # a begin in front of the day kernel, the fold behind it
    assert sorted(a for a, _ in fn.values())[-6:-2] == new
    assert new[-1] < at("22k_scenario_local_beginILi256E") < at("20k_scenario_local_dayILi4E")

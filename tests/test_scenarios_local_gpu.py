"""Targeted scenarios on the device (include/seir_hip.h, "Targeted scenarios on the device"; covid19uk_amd/csrc/
scenario_local_kernels.h): scenarios whose two operands differ by location, and the scenarios' per-draw region totals.

The references are exact without a new simulator:
  1. tensors constant over m are the global set, bit for bit;
  2. with commute = 0 the rows decouple, so a local scenario is a row-wise mix of global `SeirModel.simulate` calls;
  3. on day 0 every scenario sees the common state, so with H = 1 a row is the global scenario's row with that row's operands;
  4. before its from_day a local scenario is the baseline;
  5. at micro sizes a day loop built from `oracle.sim_oracle.day_rates` and `binomial` (which broadcast per-location operands);
  6. the region totals are sums over members of the above.
Every comparison is `np.array_equal` on integers; seeds are fixed.  As in tests/test_forecast_gpu.py a differing cell against the
CPU simulator would be a finding to explain against the near-tie mark of tests/binomial_lib.py, not a reason for a tolerance."""
import os

import numpy as np
import pytest

from covid19uk_amd import _lib, synth
from covid19uk_amd.posterior import groups as G
from covid19uk_amd.posterior import scenarios as SC
from covid19uk_amd.sampler import forecast_draw_id
from oracle import mcmc_oracle, sim_oracle
from tests import helpers as H
from tests import test_forecast_gpu as FG
from tests.test_recovery_gpu import _case
from tests.test_sampler_gpu import CFG_REF, CFG_SMALL, api  # noqa: F401  (fixture)
from tests.test_scenarios_gpu import KEYS, _sims
from tests.test_summary_gpu import _sampler

pytestmark = pytest.mark.gpu

# name, cfg, eps, B, record, n, H, K: the shapes of tests/test_scenarios_gpu.py's SCEN_CASES -- M = 1 / H = 1; one row past the day
# kernel's 4-row block and the fold's 8-row block with H one chunk and one day past it; one row past a 64-row tile; several
# row tiles with two day chunks; K = 1, 2, 4; 1, 3, 8 chains; both trace widths; and NI-11 with 13 draws of 5 chains -- M no
# multiple of the day kernel's 4 rows, ND = 65 (two column blocks per scenario, the second with one live draw), K = 2, B not
# dividing 64 -- all at once
SHAPES = {
    "M=11,H=3,K=2,B=5,ND=65,u16": ("ni11", CFG_REF, 0.002, 5, "u16", 13, 3, 2),
    "M=1,H=1,K=1,B=3,u16": ("micro_1x70", CFG_SMALL, 0.002, 3, "u16", 6, 1, 1),
    "M=9,H=64,K=4,B=3,u16": ("micro_9x64", CFG_SMALL, 0.0004, 3, "u16", 5, 64, 4),
    "M=9,H=65,K=2,B=8": ("micro_9x64", CFG_SMALL, 0.0004, 8, True, 4, 65, 2),
    "M=65,H=7,K=1,B=1,u16": ("micro_65x70", CFG_SMALL, 0.0001, 1, "u16", 9, 7, 1),
    "M=520,H=128,K=2,B=2": ("slow_520x70", CFG_SMALL, 3e-5, 2, True, 3, 128, 2),
}


def _build(api, case_id, cap=None):  # noqa: F811
    name, cfg, eps, B, record, n, Hn, K = SHAPES[case_id]
    case = H.build_case(name, 43, alpha_t_sd=0.005)
    u = synth.jitter_params(case["u"], B, scale=0.01, seed=3, T=case["k"].T)
    ev = np.stack([case["events"]] * B)
    model, s = _sampler(api, case, cfg, u, ev, eps, n if cap is None else cap, record_events=record)
    return case, model, s, n, Hn, K, B


def _everything(s):
    """Every moment, difference accumulator and per-draw curve of the scenarios in force, by name."""
    out = {}
    for k, m in enumerate(s.scenario_summary()):
        for key in ("count", "ref", "sum", "sumsq"):
            out[f"moments{k}.{key}"] = np.array(getattr(m, key))
    d = s.scenario_diffs()
    out.update({f"diffs.{key}": np.array(d[key]) for key in KEYS + ("count",)})
    out.update({f"draws.{key}": v for key, v in s.read_scenario_draws().items()})
    return out


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


def _over_rows(x, M):
    """[K, H] -> [K, M, H], constant over m."""
    return np.ascontiguousarray(np.repeat(np.asarray(x)[:, None, :], M, axis=1))


def _global(Hn, ls, cm):
    """A one-scenario `Scenarios` of the arrays [H]: what `SC.scenario_inputs` takes."""
    return SC.Scenarios(("x",), Hn, np.asarray(ls, np.float64)[None], np.asarray(cm, np.float64)[None])


def _against(s, base, st0, sims):
    """The scenarios in force against the expected simulated counts `sims[k]` [n,B,M,H,3] and the baseline's `base`: moments,
    per-draw curves and difference accumulators (tests/test_scenarios_gpu.py's `_holds`, the counts given)."""
    n, B = base.shape[:2]
    sums, diffs, draws = s.scenario_summary(), s.scenario_diffs(), s.read_scenario_draws()
    assert diffs["count"] == n and len(sums) == len(sims)
    for k, sim in enumerate(sims):
        want = dict(count=np.full(B, n, np.uint64), ref=[], sum=[], sumsq=[])
        for b in range(B):
            FG._fold(FG._quantities(sim[:, b], st0[:, b]), want)
        FG._same_moments(sums[k], {key: (np.stack(v) if isinstance(v, list) else v) for key, v in want.items()})
        x = np.stack([FG._quantities(sim[:, b], st0[:, b]) for b in range(B)], axis=1)
        assert np.array_equal(draws["by_day"][k], x[..., :3].sum(axis=2)), k
        assert np.array_equal(draws["state_by_day"][k], x[..., 3:].sum(axis=2)), k
        fold = SC.fold_differences(base, sim)
        for key in KEYS:
            assert diffs[key].dtype == fold[key].dtype and np.array_equal(diffs[key][k], fold[key]), (k, key)


def _region(case_id, M):
    """The rows of the targeted region: the last row alone, or rows 3..5, which straddle a 4-row block of the day kernel."""
    if M == 1:
        return [0]
    return [M - 1] if case_id in ("M=9,H=65,K=2,B=8", "M=520,H=128,K=2,B=2") else [3, 4, 5]


def _decoupled(case, model, theta, events, Hn, rows, **kw):
    """Test 2's local scenario -- commute = 0 everywhere, transmission x 0.5 from day min(2, H - 1) on in `rows`, the identity
    elsewhere -- as tensors [1, M, H], and its counts: the row-wise mix of two global `simulate` calls with commute = 0."""
    M, d = case["k"].M, min(2, Hn - 1)
    prof = np.zeros(Hn)
    prof[d:] = np.log(0.5)
    ls = np.zeros((1, M, Hn))
    ls[0, rows] = prof
    cm = np.zeros((1, M, Hn))
    inside, _ = _sims(model, case, theta, events, Hn, _global(Hn, prof, np.zeros(Hn)), 0, **kw)
    outside, _ = _sims(model, case, theta, events, Hn, _global(Hn, np.zeros(Hn), np.zeros(Hn)), 0, **kw)
    mix = outside.copy()
    mix[:, :, rows] = inside[:, :, rows]
    return ls, cm, mix


# ---------------------------------------------------------------------------------------------------------------------
# 1. constant over m is the global set
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", list(SHAPES))
def test_tensors_constant_over_locations_are_the_global_set_bit_for_bit(api, case_id):  # noqa: F811
    case, model, s, n, Hn, K, B = _build(api, case_id)
    M = case["k"].M
    rng = np.random.default_rng([Hn, K])
    ls, cm = rng.normal(0.0, 0.3, size=(K, Hn)), rng.uniform(0.0, 2.0, size=(K, Hn))
    with model, s:
        FG._reset(s, case, Hn)
        s.set_scenarios(ls, cm, n)
        s.sample(n, forecast=True)
        want = _everything(s)
        FG._reset(s, case, Hn)                              # the same draws again, the same numbers through the local entry point
        s.set_scenarios(_over_rows(ls, M), _over_rows(cm, M), n)
        assert s.scenario_state() == dict(K=K, H=Hn, cap=n, j=0)
        s.forecast(0, n)
        _same(_everything(s), want)
        assert want["diffs.sumsq"].any() or M == 1
        assert not s.pair_timeouts().any()


# ---------------------------------------------------------------------------------------------------------------------
# 2. no commuting decouples the rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", list(SHAPES))
def test_without_commuting_a_local_scenario_is_the_row_wise_mix_of_two_global_ones(api, case_id):  # noqa: F811
    case, model, s, n, Hn, _, B = _build(api, case_id)
    M = case["k"].M
    rows = _region(case_id, M)
    with model, s:
        FG._reset(s, case, Hn)
        tr = s.sample(n, forecast=True)
        base, st0 = _sims(model, case, tr.theta, tr.events, Hn)
        ls, cm, mix = _decoupled(case, model, tr.theta, tr.events, Hn, rows)
        FG._reset(s, case, Hn)
        s.set_scenarios(ls, cm, n)
        s.forecast(0, n)
        _against(s, base, st0, [mix])
        FG._same_moments(s.forecast_summary(), FG._oracle(model, case, tr.theta, tr.events, Hn))   # the forecast keeps its bits


# ---------------------------------------------------------------------------------------------------------------------
# 3. day 0 under coupling
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,eps,B", [("slow_520x70", 3e-5, 2), ("micro_9x64", 0.0004, 3)])
def test_on_day_zero_a_row_is_the_global_scenarios_row_with_its_own_operands(api, name, eps, B):  # noqa: F811
    """H = 1, commuting on: the hazard of day 0 uses the common state, so a region row equals the row of the global scenario
    with that row's (log_shift, commute) -- which differ by row -- and every other row the baseline's."""
    case = H.build_case(name, 43, alpha_t_sd=0.005)
    u = synth.jitter_params(case["u"], B, scale=0.01, seed=3, T=case["k"].T)
    model, s = _sampler(api, case, CFG_SMALL, u, np.stack([case["events"]] * B), eps, 4)
    M, n, Hn, rows = case["k"].M, 4, 1, [3, 4, 5]
    ops = {3: (np.log(0.5), 0.25), 4: (np.log(1.5), 3.0), 5: (np.log(0.25), 0.0)}
    ls, cm = np.zeros((1, M, 1)), np.ones((1, M, 1))
    for m, (a, c) in ops.items():
        ls[0, m, 0], cm[0, m, 0] = a, c
    with model, s:
        FG._reset(s, case, Hn)
        s.set_scenarios(ls, cm, n)
        tr = s.sample(n, forecast=True)
        base, st0 = _sims(model, case, tr.theta, tr.events, Hn)
        mix = base.copy()
        for m, (a, c) in ops.items():
            sim, _ = _sims(model, case, tr.theta, tr.events, Hn, _global(Hn, [a], [c]), 0)
            mix[:, :, m] = sim[:, :, m]
        _against(s, base, st0, [mix])
        assert not np.array_equal(mix[:, :, rows], base[:, :, rows])


# ---------------------------------------------------------------------------------------------------------------------
# 4. the prefix before from_day is the baseline
# ---------------------------------------------------------------------------------------------------------------------
def test_before_its_from_day_a_local_scenario_is_the_baseline_and_from_it_on_it_is_not(api):  # noqa: F811
    """H = 128, commuting on, rows 3..5 with transmission x 0.5 and commute x 0.5 from day d: every difference of the days < d is 0
    in every cell (eq == count); from day d on some cell differs.  d = 1, 63, 64, 65: around the fold's 64-day chunk.  A `slow`
    epidemic, which is still running 190 days in."""
    case = H.build_case("slow_9x64", 43, alpha_t_sd=0.005)
    B, n, Hn = 2, 4, 128
    u = synth.jitter_params(case["u"], B, scale=0.01, seed=3, T=case["k"].T)
    model, s = _sampler(api, case, CFG_SMALL, u, np.stack([case["events"]] * B), 1e-4, n)
    sc0 = SC.parse_scenarios({"a": {"locations": [3, 4, 5], "transmission": 0.5, "commute": 0.5, "from_day": 1}}, Hn)
    with model, s:
        FG._reset(s, case, Hn)
        one = SC.resolve_locations(sc0, 9)
        s.set_scenarios(one.log_shift, one.commute, n)
        s.sample(n, forecast=True)
        for d in (1, 63, 64, 65):
            sc = SC.resolve_locations(SC.parse_scenarios(
                {"a": {"locations": [3, 4, 5], "transmission": 0.5, "commute": 0.5, "from_day": d}}, Hn), 9)
            FG._reset(s, case, Hn)
            s.set_scenarios(sc.log_shift, sc.commute, n)
            s.forecast(0, n)
            df = s.scenario_diffs()
            print(f"from_day {d}: cells differing from day {d} on:", int((df["eq"][0][:, :, d:] < n).sum()))
            assert np.all(df["eq"][0][:, :, :d] == n) and not df["lt"][0][:, :, :d].any()
            for key in ("ref", "sum", "sumsq"):
                assert not df[key][0][:, :, :d].any(), (d, key)
            assert (df["eq"][0][:, :, d:] < n).any(), d


# ---------------------------------------------------------------------------------------------------------------------
# 5. against the independent CPU simulator
# ---------------------------------------------------------------------------------------------------------------------
def _cpu_local(k, par, a_loc, spatial, W_loc, wd, st0, seed, first):
    """`oracle.sim_oracle.simulate`'s day loop with per-location operands: a_loc [n, M, H], W_loc [M, H] (`SC.local_inputs`)."""
    n, M, Hn = a_loc.shape
    out = np.zeros((n, M, Hn, 3))
    for d in range(n):
        state = np.array(st0[d], dtype=np.float64)
        th = np.concatenate([np.asarray(par[d], np.float64), np.asarray(spatial[d], np.float64)])
        for s in range(Hn):
            lam, nu, rir = sim_oracle.day_rates(state, th, a_loc[d, :, s], W_loc[:, s], float(wd[s]), k)
            p_ei, p_ir = sim_oracle._prob(nu * 1.0), sim_oracle._prob(rir * 1.0)
            for m in range(M):
                cell = s * M + m
                for x, (src, p) in enumerate(((0, sim_oracle._prob(float(lam[m]) * 1.0)), (1, p_ei), (2, p_ir))):
                    out[d, m, s, x] = sim_oracle.binomial(
                        state[m, src], p, lambda att, x=x, cell=cell: tuple(
                            float(v[0]) for v in mcmc_oracle.rng_uniform2(seed, first + d, cell, sim_oracle.RS_SIM_BASE + x, att)))
            state = state + out[d, :, s, :] @ sim_oracle.so.STOICHIOMETRY
    return out


@pytest.mark.parametrize("name,Hn", [("micro_9x64", 3), ("micro_3x1", 4)])
def test_local_scenarios_equal_the_independent_cpu_simulator(api, name, Hn):  # noqa: F811
    """The two micro cases of tests/test_scenarios_gpu.py with multipliers that vary over both m and s, both tensors at once."""
    assert sim_oracle.so.TIME_DELTA == 1.0
    case, u, ev, cfg, eps = _case(name, 2)
    M, n = case["k"].M, 3
    rng = np.random.default_rng([M, Hn])
    sc = SC.LocalScenarios(("a", "b"), Hn, rng.normal(0.0, 0.4, size=(2, M, Hn)), rng.uniform(0.0, 2.0, size=(2, M, Hn)))
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        FG._reset(s, case, Hn)
        s.set_scenarios(sc.log_shift, sc.commute, n)
        tr = s.sample(n, forecast=True)
        k = H.oracle_constants(case["cov"], case["init"])
        base, st0 = _sims(model, case, tr.theta, tr.events, Hn, simulate=lambda *a, **kw: sim_oracle.simulate(k, *a, **kw))
        W, wd = FG._calendar(case, Hn)
        sims = []
        for kk in range(2):
            per_chain = []
            for b in range(tr.theta.shape[1]):
                par, a_path, spatial, s0 = FG._inputs(tr.theta[:, b], tr.events[:, b], case["init"], case["k"].T, Hn)
                a_loc, W_loc = SC.local_inputs(a_path, W, sc, kk)
                sim = _cpu_local(k, par, a_loc, spatial, W_loc, wd, s0.astype(np.float64), FG.SEED, forecast_draw_id(b, 0))
                per_chain.append(sim.astype(np.int64))
            sims.append(np.stack(per_chain, axis=1))
        _against(s, base, st0, sims)


# ---------------------------------------------------------------------------------------------------------------------
# 6. region totals
# ---------------------------------------------------------------------------------------------------------------------
def _csr(groups):
    off = np.cumsum([0] + [len(g) for g in groups]).astype(np.int32)
    return off, np.concatenate([np.asarray(g, np.int32) for g in groups])


def _by_group(x, groups):
    """[n,B,M,L,3] -> [n,B,G,L,3]."""
    return np.stack([x[:, :, np.asarray(g)].astype(np.int64).sum(axis=2) for g in groups], axis=2)


def _totals(api, name, cfg, eps, B, record, n, Hn, groups, identity=True):  # noqa: F811
    """Through the local entry point: a global scenario (constant over m) and test 2's local one, K = 2, and in front of them,
    with `identity`, the identity: K = 3.  The all-locations group (groups[0]) is the by_day store; a global scenario's totals
    are `simulate`'s counts summed over the members, the local one's the mix's; the identity's are forecast_by_group."""
    case = H.build_case(name, 43, alpha_t_sd=0.005)
    u = synth.jitter_params(case["u"], B, scale=0.002 if name == "uk380" else 0.01, seed=3, T=case["k"].T)
    M = case["k"].M
    assert groups[0] == list(range(M))
    model, s = _sampler(api, case, cfg, u, np.stack([case["events"]] * B), eps, n, record_events=record)
    rng = np.random.default_rng([M, Hn])
    gl, gc = rng.normal(0.0, 0.3, size=Hn), rng.uniform(0.0, 2.0, size=Hn)
    with model, s:
        s.set_groups(*_csr(groups))
        FG._reset(s, case, Hn)
        tr = s.sample(n, forecast=True, groups=True)
        fbg = np.array(tr.groups["forecast_by_group"])
        rows = [M - 1] if M < 6 else [3, 4, 5]
        ls2, cm2, mix = _decoupled(case, model, tr.theta, tr.events, Hn, rows)
        glob, _ = _sims(model, case, tr.theta, tr.events, Hn, _global(Hn, gl, gc), 0)
        i0 = 1 if identity else 0
        ls = np.concatenate([np.zeros((i0, M, Hn)), _over_rows(gl[None], M), ls2])
        cm = np.concatenate([np.ones((i0, M, Hn)), _over_rows(gc[None], M), cm2])
        FG._reset(s, case, Hn)
        s.set_scenarios(ls, cm, n)
        s.set_scenario_groups(True)
        s.forecast(0, n)
        got = s.read_scenario_group_draws()
        assert got.dtype == np.int64 and got.shape == (i0 + 2, n, B, len(groups), Hn, 3)
        assert np.array_equal(got[:, :, :, 0], s.read_scenario_draws()["by_day"])
        if identity:
            assert np.array_equal(got[0], fbg)
        assert np.array_equal(got[i0], _by_group(glob, groups))
        assert np.array_equal(got[i0 + 1], _by_group(mix, groups))
        assert np.array_equal(s.read_scenario_group_draws(1, first=n - 1), got[:, n - 1:])
        assert got[i0].any() or Hn == 1


@pytest.mark.parametrize("name,eps,B,record,n,Hn,kind", [
    ("micro_9x64", 0.0004, 3, "u16", 4, 1, "G=1"),
    ("micro_9x64", 0.0004, 3, True, 4, 64, "mixed"),
    ("micro_65x70", 0.0001, 1, "u16", 5, 65, "mixed"),
    ("slow_256x70", 3e-5, 2, True, 3, 128, "G=256"),
    ("slow_256x70", 3e-5, 2, True, 3, 7, "65,129"),
])
def test_the_scenarios_region_totals(api, name, eps, B, record, n, Hn, kind):  # noqa: F811
    """G = 1; singletons, the all-locations group and an overlapping pair; G = 256 at M = 256 (all, then 255 singletons); groups
    of 65 and 129 members (a second and a third segment); H = 1, 64, 65, 128 (one lane, a chunk, one past it, two chunks)."""
    M = int(name.split("_")[1].split("x")[0])
    every = list(range(M))
    groups = {"G=1": [every], "mixed": [every] + [[m] for m in range(min(M, 12))] + [every[:(2 * M) // 3], every[M // 3:]],
              "G=256": [every] + [[m] for m in range(255)],
              "65,129": [every, list(range(0, 130, 2)), list(range(M - 129, M))]}[kind]
    if kind == "65,129":
        assert [len(g) for g in groups[1:]] == [65, 129]
    _totals(api, name, CFG_SMALL, eps, B, record, n, Hn, groups)


def test_the_scenarios_region_totals_at_uk380_with_the_nations(api):  # noqa: F811
    """UK-380 x 8 chains x 12 draws x H = 14 with `nations` (behind the all-locations group), K = 2: a global scenario and the
    local one; the identity against forecast_by_group is the other shapes'."""
    codes = [str(x) for x in np.load(synth._DATA)["lad19cd"]]
    tab = G.parse_groups("nations", len(codes), codes)
    groups = [list(range(len(codes)))] + [list(tab.rows(g)) for g in range(tab.G)]
    _totals(api, "uk380", CFG_REF, 1.2e-5, 8, "u16", 12, 14, groups, identity=False)


# ---------------------------------------------------------------------------------------------------------------------
# 7. robustness: the forecast's list
# ---------------------------------------------------------------------------------------------------------------------
def _local_pair(M, Hn):
    """Two targeted scenarios whose operands vary over m and s (commuting on)."""
    rng = np.random.default_rng([M, Hn, 7])
    return rng.normal(0.0, 0.3, size=(2, M, Hn)), rng.uniform(0.0, 2.0, size=(2, M, Hn))


def _with_totals(s):
    return dict(_everything(s), totals=s.read_scenario_group_draws())


def test_cuts_halves_resets_horizons_and_a_global_set_after_a_local_one(api):  # noqa: F811
    """Two bursts in the buffer's halves, one call, uneven calls: the same integers, the stores by draw position and not by
    slot.  A second reset keeps a local set and empties the stores; another horizon frees them; a global set replaces a local
    one and back; K = 0 frees."""
    case, u, ev, cfg, eps = _case("micro_20x60", 3)
    n, Hn, M = 11, 9, 20
    ls, cm = _local_pair(M, Hn)
    groups = [list(range(M)), [0, 5, 19], list(range(7, 15))]
    model, s = _sampler(api, case, cfg, u, ev, eps, 2 * n)
    with model, s:
        s.set_groups(*_csr(groups))
        FG._reset(s, case, Hn)
        s.set_scenarios(ls, cm, 2 * n)
        s.set_scenario_groups(True)
        for first in (0, n):
            s.reset_trace(at=first)
            s.run(n)
            s.forecast(first, n)
        halves = _with_totals(s)
        assert halves["diffs.sumsq"].any() and halves["totals"].shape == (2, 2 * n, 3, 3, Hn, 3)
        assert np.array_equal(halves["totals"][:, :, :, 0], halves["draws.by_day"])
        for cuts in (((0, 2 * n),), ((0, 3), (3, 1), (4, 9), (13, 2 * n - 13))):
            FG._reset(s, case, Hn)                             # empties, keeps the local set
            assert s.scenario_state() == dict(K=2, H=Hn, cap=2 * n, j=0)
            assert s.read_scenario_group_draws().shape[1] == 0
            for first, count in cuts:
                s.forecast(first, count)
            _same(_with_totals(s), halves)
        # the second half alone lands at positions 0..n-1, whatever its slots: slots n..2n-1 under test 2's decoupled scenario,
        # held to `simulate` on those draws with the draw ids of positions 0..n-1
        tr = s.read_trace(2 * n)
        th2, ev2 = tr.theta[n:], tr.events[n:]
        base2, st02 = _sims(model, case, th2, ev2, Hn)
        ls_d, cm_d, mix = _decoupled(case, model, th2, ev2, Hn, [3, 4, 5])
        FG._reset(s, case, Hn)
        s.set_scenarios(ls_d, cm_d, 2 * n)
        s.forecast(n, n)
        assert s.scenario_state()["j"] == n
        _against(s, base2, st02, [mix])
        second_half = s.read_scenario_group_draws()
        assert second_half.shape == (1, n, 3, 3, Hn, 3) and np.array_equal(second_half[0], _by_group(mix, groups))
        FG._reset(s, case, Hn)
        s.set_scenarios(ls, cm, 2 * n)
        s.forecast(0, n)
        first_half = s.read_scenario_group_draws()
        assert np.array_equal(first_half, halves["totals"][:, :n])
        # a global set after a local one, and back
        FG._reset(s, case, Hn)
        s.set_scenarios(ls[:, 0], cm[:, 0], 2 * n)
        s.forecast(0, 2 * n)
        glob = _with_totals(s)
        FG._reset(s, case, Hn)
        s.set_scenarios(_over_rows(ls[:, 0], M), _over_rows(cm[:, 0], M), 2 * n)
        s.forecast(0, 2 * n)
        _same(_with_totals(s), glob)
        FG._reset(s, case, Hn)
        s.set_scenarios(ls, cm, 2 * n)
        s.forecast(0, 2 * n)
        _same(_with_totals(s), halves)
        # another horizon frees the set and its stores; K = 0 frees
        FG._reset(s, case, Hn + 1)
        assert s.scenario_state()["K"] == 0
        with pytest.raises(_lib.SeirError, match="no scenarios are set") as e:
            s.read_scenario_group_draws(0)
        assert e.value.code == _lib.ERR_STATE
        ls2, cm2 = _local_pair(M, Hn + 1)
        s.set_scenarios(ls2, cm2, n)
        s.forecast(0, n)
        assert np.array_equal(s.read_scenario_group_draws()[:, :, :, 0], s.read_scenario_draws()["by_day"])
        FG._reset(s, case, Hn + 1)
        s.set_scenarios(np.zeros((0, M, Hn + 1)), np.ones((0, M, Hn + 1)), 0)
        assert s.scenario_state() == dict(K=0, H=0, cap=0, j=0)
        assert not s.pair_timeouts().any()


def test_two_host_batches_workgroup_skew_and_the_same_run_twice(api):  # noqa: F811
    """130 slots: two batches of the host's cut.  The same integers under every debug skew, and twice without one."""
    case, u, ev, cfg, eps = _case("micro_5x24", 2)
    n, Hn, M = 130, 3, 5
    ls, cm = _local_pair(M, Hn)
    res = {}
    for tag, skew in (("a", 0), ("b", 0), (1, 1), (2, 2), (3, 3)):
        model, s = _sampler(api, case, cfg, u, ev, 0.002, n, skew=skew)
        with model, s:
            s.set_groups(*_csr([list(range(M)), [1, 3]]))
            FG._reset(s, case, Hn)
            s.set_scenarios(ls, cm, n)
            s.set_scenario_groups(True)
            tr = s.sample(n, forecast=True)
            res[tag] = dict(_with_totals(s), events=np.array(tr.events))
    assert res["a"]["diffs.sumsq"].any()
    for tag in ("b", 1, 2, 3):
        _same(res[tag], res["a"])


def test_chain_sharding_and_thinning(api):  # noqa: F811
    """Chains 2 and 3 of a 4-chain sampler against a 2-chain sampler created with first_chain_id = 2; with thin = 3 the scenarios
    are those of the kept draws."""
    case, u, ev, cfg, eps = _case("micro_20x60", 4)
    n, Hn, M = 5, 8, 20
    ls, cm = _local_pair(M, Hn)

    def run(uu, evv, cap, **kw):
        model, s = _sampler(api, case, cfg, uu, evv, eps, cap, **kw)
        with model, s:
            s.set_groups(*_csr([list(range(M)), [2, 4, 6]]))
            FG._reset(s, case, Hn)
            s.set_scenarios(ls, cm, n)
            s.set_scenario_groups(True)
            tr = s.sample(n, forecast=True)
            return _with_totals(s), np.array(tr.events)
    four, ev4 = run(u, ev, n)
    two, ev2 = run(u[2:], ev[2:], n, first_chain_id=2)
    assert np.array_equal(ev4[:, 2:], ev2) and four["diffs.sumsq"].any()
    for key, v in four.items():
        if key.startswith("moments"):
            assert np.array_equal(v[2:], two[key]), key
        elif key.startswith("diffs.") and key != "diffs.count":
            assert np.array_equal(v[:, 2:], two[key]), key
        elif key != "diffs.count":
            assert np.array_equal(v[:, :, 2:], two[key]), key
    k = 3
    kept, evk = run(u, ev, n, thin=k)
    model, s = _sampler(api, case, cfg, u, ev, eps, n * k)
    with model, s:
        every = s.sample(n * k)
        assert np.array_equal(every.events[k - 1::k], evk)
        # the kept draws loaded back into slots 0..n-1 would be a replay; here: the same chain, forecast from the kept slots
        s.set_groups(*_csr([list(range(M)), [2, 4, 6]]))
        FG._reset(s, case, Hn)
        s.set_scenarios(ls, cm, n)
        s.set_scenario_groups(True)
        for i in range(n):
            s.forecast(k - 1 + i * k, 1)
        _same(_with_totals(s), kept)


def test_a_burst_run_again_after_a_time_out_is_counted_once_in_both_stores(api):  # noqa: F811
    """tests/test_forecast_gpu.py's disturbance (the existing hook, once) with test 2's local set and the region totals on: the
    re-run burst's moments, differences, curves and totals are those of its own draws, counted once."""
    case, u, ev, cfg, eps = _case("micro_20x60", 8)
    B, nb, burst, Hn, M = 8, 6, 4, 5, 20
    groups = [list(range(M)), [0, 1, 2], [4, 19]]
    rows = [3, 4, 5]
    prof = np.zeros(Hn)
    prof[2:] = np.log(0.5)
    ls, cm = np.zeros((1, M, Hn)), np.zeros((1, M, Hn))
    ls[0, rows] = prof
    model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
    with model, s:
        s.set_groups(*_csr(groups))
        FG._reset(s, case, Hn)
        s.set_scenarios(ls, cm, nb * burst)
        s.set_scenario_groups(True)
        got = {}

        def consume(tr, i):
            got[i] = (tr.events.copy(), tr.theta.copy())
            if i == 1 and not s.recoveries:
                _lib.check(s._lib.seir_sampler_debug_fail_handoff(s._s, B - 1))
        s.sample_bursts(nb, burst, consume, forecast=True)
        assert len(s.recoveries) == 1 and sorted(got) == list(range(nb))
        theta, events = np.concatenate([got[i][1] for i in range(nb)]), np.concatenate([got[i][0] for i in range(nb)])
        base, st0 = _sims(model, case, theta, events, Hn)
        ls_w, cm_w, mix = _decoupled(case, model, theta, events, Hn, rows)
        assert np.array_equal(ls_w, ls) and np.array_equal(cm_w, cm)
        _against(s, base, st0, [mix])
        assert np.array_equal(s.read_scenario_group_draws()[0], _by_group(mix, groups))


# ---------------------------------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(api, monkeypatch):  # noqa: F811
    case, u, ev, cfg, eps = _case("micro_20x60", 2)
    n, Hn, M = 4, 6, 20
    ls, cm = _local_pair(M, Hn)
    model, s = _sampler(api, case, cfg, u, ev, eps, n)

    def refused(code, word, f, *a, **kw):
        with pytest.raises(_lib.SeirError) as e:
            f(*a, **kw)
        assert e.value.code == code and word in str(e.value), str(e.value)
        return str(e.value)

    with model, s:
        refused(_lib.ERR_STATE, "seir_sampler_forecast_reset", s.set_scenarios, ls, cm, n)
        FG._reset(s, case, Hn)
        with pytest.raises(ValueError, match="need two of"):
            s.set_scenarios(ls[:, :5], cm[:, :5], n)
        for bad, word in ((np.nan, "log_shift[1][7][2] is not finite"), (np.inf, "log_shift[1][7][2] is not finite")):
            x = ls.copy()
            x[1, 7, 2] = bad
            refused(_lib.ERR_INVALID, word, s.set_scenarios, x, cm, n)
        for bad in (-0.5, np.nan, np.inf):
            x = cm.copy()
            x[0, 19, 5] = bad
            refused(_lib.ERR_INVALID, "commute[0][19][5]=", s.set_scenarios, ls, x, n)
        refused(_lib.ERR_INVALID, "K=5", s.set_scenarios, np.zeros((5, M, Hn)), np.ones((5, M, Hn)), n)
        assert s.scenario_state()["K"] == 0
        # the switch without a table; a read with the store off
        refused(_lib.ERR_STATE, "no group table is set", s.set_scenario_groups, True)
        s.set_scenarios(ls, cm, n)
        refused(_lib.ERR_STATE, "group sums are off", s.read_scenario_group_draws, 0)
        s.set_groups(*_csr([list(range(M)), [1, 2]]))
        s.set_scenario_groups(True)
        s.sample(n, forecast=True)
        refused(_lib.ERR_STATE, "first seir_sampler_forecast", s.set_scenarios, ls, cm, n)       # a set behind the first forecast
        assert s.read_scenario_group_draws().shape == (2, n, 2, 2, Hn, 3)
        refused(_lib.ERR_INVALID, "outside the 4 draws", s.read_scenario_group_draws, 2, first=3)
        # a new table at j > 0: the store is off until the next reset
        s.set_groups(*_csr([list(range(M)), [1, 2], [3]]))
        refused(_lib.ERR_STATE, "group sums are off", s.read_scenario_group_draws, 0)
        FG._reset(s, case, Hn)
        s.forecast(0, n)
        got = s.read_scenario_group_draws()
        assert got.shape == (2, n, 2, 3, Hn, 3) and np.array_equal(got[:, :, :, 0], s.read_scenario_draws()["by_day"])
        # above half of the free memory.  At the set: the scenarios alone fit, with the region totals' store they do not -- the
        # forecast is then without scenarios.  The figures come from the library's own message with the switch off.
        FG._reset(s, case, Hn)
        s.set_scenario_groups(False)
        monkeypatch.setenv("SEIR_DEBUG_FREE_BYTES", "1")
        msg = refused(_lib.ERR_INVALID, "the scenarios need", s.set_scenarios, ls, cm, n)
        alone = int(msg.split("the scenarios need ")[1].split(" bytes")[0])
        store = 2 * n * 2 * 3 * Hn * 3 * 8                      # K x cap x B x G x H x 24
        assert s.scenario_state()["K"] == 0
        monkeypatch.setenv("SEIR_DEBUG_FREE_BYTES", str(2 * (alone + store) - 2))
        s.set_scenarios(ls, cm, n)                              # fits without the store
        s.set_scenario_groups(False)
        monkeypatch.delenv("SEIR_DEBUG_FREE_BYTES")
        s.set_scenario_groups(True)
        monkeypatch.setenv("SEIR_DEBUG_FREE_BYTES", str(2 * (alone + store) - 2))
        msg = refused(_lib.ERR_INVALID, "the scenarios need", s.set_scenarios, ls, cm, n)
        assert int(msg.split("the scenarios need ")[1].split(" bytes")[0]) == alone + store
        assert s.scenario_state()["K"] == 0
        # at groups_set: the new table's forecast outputs alone fit, with the scenarios' store they do not; the refused table
        # leaves the table in force, and the store that is sized for it
        monkeypatch.delenv("SEIR_DEBUG_FREE_BYTES")
        s.set_scenarios(ls, cm, n)
        outputs = n * 2 * 1 * (Hn + 1) * 24                     # trace slots x B x G x (H days and the state) x 24, G = 1
        store1 = 2 * n * 2 * 1 * Hn * 24                        # K x cap x B x G x H x 24
        monkeypatch.setenv("SEIR_DEBUG_FREE_BYTES", str(2 * (outputs + store1) - 2))
        msg = refused(_lib.ERR_INVALID, "the group sums need", s.set_groups, *_csr([list(range(M))]))
        assert int(msg.split("the group sums need ")[1].split(" bytes")[0]) == outputs + store1
        monkeypatch.delenv("SEIR_DEBUG_FREE_BYTES")
        s.forecast(0, n)
        assert np.array_equal(s.read_scenario_group_draws(), got)
        assert not s.pair_timeouts().any()


# ---------------------------------------------------------------------------------------------------------------------
# 9. nothing else notices
# ---------------------------------------------------------------------------------------------------------------------
def test_no_other_product_notices_the_local_set_or_the_switch(api):  # noqa: F811
    """Every product on at once -- summaries, the forecast with its draw store, quantiles, group sums and the truth it is scored
    against, R_t, the check, within / between, both group curves: the run with a local set and the region totals on against the
    run with the same numbers set globally and the switch off -- every field of every burst's trace and every product's
    accumulators bit for bit.  The verification's fold runs in the same hook right behind the scenarios' batch."""
    from covid19uk_amd.posterior import predict
    from covid19uk_amd.sampler import Trace
    from tests.test_scenarios_gpu import _flat, inf_steps
    case, u, ev, cfg, eps = _case("micro_20x60", 3)
    B, nb, burst, Hn, K, D = 3, 3, 4, 6, 5, 4
    cov, T, M = case["cov"], case["k"].T, case["k"].M
    N = np.asarray(cov.N, np.float64).reshape(-1)
    tab = G.parse_groups({"all": list(range(M)), "low": list(range(0, M, 2)), "one": [M - 1]}, M)
    rng = np.random.default_rng(9)
    ls, cm = rng.normal(0.0, 0.3, size=(2, Hn)), rng.uniform(0.0, 2.0, size=(2, Hn))
    truth = rng.integers(0, 6, size=(M, Hn)).astype(np.int32)
    truth[3, 2:] = -1                                       # a row whose cum_cases lose their truth from day 2 on
    truth[7, 4] = -1
    kw = dict(summarize=True, forecast=inf_steps(7, list(range(B)), Hn), rt=True, check=True, within_between=True, groups=True)
    fields = tuple(f for f in Trace.__dataclass_fields__ if f not in ("hmc", "moves"))
    runs = {}
    for local in (False, True):
        model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
        with model, s:
            s.set_groups(tab.offsets, tab.members)
            s.set_group_rt(G.rt_weights(tab, N))
            s.set_group_within_between(True)
            s.reset_forecast(Hn, *predict.forecast_calendar(cov, None, T, Hn), 5)
            s.keep_forecast_draws(nb * burst)
            if local:
                s.set_scenarios(_over_rows(ls, M), _over_rows(cm, M), nb * burst)
                s.set_scenario_groups(True)
            else:
                s.set_scenarios(ls, cm, nb * burst)
            s.set_verify(truth)                             # behind the scenarios, as the drivers set it
            s.reset_check(K, *predict.check_calendar(cov, None, T, K), 6)
            s.reset_rt(D, N / N.sum())
            s.reset_within_between(D)
            got = {}

            def consume(tr, i, got=got):
                got[i] = {f: ({k: np.array(a) for k, a in getattr(tr, f).items()} if isinstance(getattr(tr, f), dict)
                              else np.array(getattr(tr, f))) for f in fields if getattr(tr, f) is not None}
            s.sample_bursts(nb, burst, consume, **kw)
            runs[local] = (got, _flat(dict(summary=s.summary(), forecast=s.forecast_summary(), rt=s.rt_summary(),
                                           check=s.check_summary(), wb=s.within_between_summary(), scen=_everything(s),
                                           q=dict(q=s.forecast_quantiles([0.05, 0.5, 0.95], pooled=True)),
                                           verify=s.verify_summary(), vstate={k: np.array(v) for k, v in s.verify_state().items()},
                                           pairs=dict(own=s.forecast_pair_sums(), pooled=s.forecast_pair_sums(pooled=True)))),
                           s.get_state())
            assert s.verify_state() == dict(on=True, H=Hn, j=nb * burst, store=True)
            if local:
                tot = s.read_scenario_group_draws()
                assert np.array_equal(tot[:, :, :, 0], s.read_scenario_draws()["by_day"]) and tot.any()
    a, b = runs[False], runs[True]
    for i in range(nb):
        assert set(a[0][i]) == set(b[0][i]) >= {"theta", "events", "marginals", "forecast", "rt", "check", "wb", "groups", "group_curves"}
        for f in a[0][i]:
            for k, v in _flat({f: a[0][i][f]}).items():
                assert np.array_equal(v, _flat({f: b[0][i][f]})[k], equal_nan=True), (i, k)
    assert set(a[1]) == set(b[1]) and any(k.startswith("scen.") for k in a[1])
    assert {"verify.lt", "verify.eq", "verify.abs_sum", "pairs.own", "pairs.pooled"} <= set(a[1])
    assert a[1]["verify.abs_sum"].any() and a[1]["pairs.own"].any()
    for k in a[1]:
        assert np.array_equal(a[1][k], b[1][k], equal_nan=True), k
    for x, y in zip(a[2], b[2]):
        assert np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------------------------------
# 10. both command lines
# ---------------------------------------------------------------------------------------------------------------------
def test_the_command_lines_with_a_targeted_scenario_and_the_region_totals(api, tmp_path):  # noqa: F811
    """The inference command line on NI-11 (its locations carrying codes of three nations), two chains, with --forecast 14
    --groups nations --scenarios FILE --groups-scenarios, FILE holding one global and one `parts` scenario, and the replay command
    line on its two files with the same flags: every scenarios/* and samples/scenario_* dataset equal.  Both runs without the
    two new keys -- FILE with the global scenario alone, no --groups-scenarios -- write the datasets they always wrote."""
    import yaml
    from covid19uk_amd.inference import inference as inf
    from tests.test_replay_gpu import _run
    from tests.test_summary_gpu import _datasets
    tmp = str(tmp_path)
    cov = synth.make_covariates("ni11")
    events, _, _ = synth.simulate_epidemic(cov)
    codes = ["E0%d" % m for m in range(5)] + ["S1%d" % m for m in range(4)] + ["W06", "W07"]
    data = os.path.join(tmp, "data.h5")
    inf.write_inference_data(data, cov, events[..., 2], locations=codes)
    cfg = os.path.join(tmp, "config.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump(dict(Mcmc=dict(dmax=84, nmax=25, m=2, occult_nmax=15, num_event_time_updates=5, num_bursts=2,
                                      num_burst_samples=6, thin=1)), f)
    glob = {"fifth_down": {"transmission": 0.8, "from_day": 7}}
    both = dict(glob, lockdown={"parts": [{"locations": ["E0*", 8], "transmission": 0.5, "commute": 0.25, "from_day": 3},
                                          {"commute": 0.5, "from_day": 10}]})
    paths = {}
    for tag, spec in (("global", glob), ("local", both)):
        paths[tag] = os.path.join(tmp, f"{tag}.yaml")
        with open(paths[tag], "w") as f:
            yaml.safe_dump(spec, f, sort_keys=False)
    flags = ["--forecast", "14", "--forecast-quantiles", "0.05,0.95", "--groups", "nations"]
    outs = {}
    for tag, extra in (("local", flags + ["--scenarios", paths["local"], "--groups-scenarios"]),
                       ("global", flags + ["--scenarios", paths["global"]])):
        out = os.path.join(tmp, f"{tag}.h5")
        log = _run("covid19uk_amd.inference.inference", ["-c", cfg, "-o", out, "--seed", "4", "--chains", "2", data] + extra, tmp)
        assert ("Scenario lockdown, group E:" in log) == (tag == "local") and "Scenario fifth_down:" in log
        files = [inf.chain_file_name(out, c, 2) for c in range(2)]
        rout = os.path.join(tmp, f"{tag}_replay.h5")
        rlog = _run("covid19uk.posterior.replay", ["-c", cfg, "-o", rout, "--seed", "4", data] + files + extra, tmp)
        assert ("Scenario lockdown, group E:" in rlog) == (tag == "local")
        outs[tag] = ([_datasets(f) for f in files], [_datasets(inf.chain_file_name(rout, c, 2)) for c in range(2)])
    n, M, Hn = 12, 11, 14
    for c in range(2):
        live, rep = outs["local"][0][c], outs["local"][1][c]
        new = {k for k in live if k.startswith("scenarios/") or k.startswith("samples/scenario_")}
        assert {"scenarios/log_shift_by_location", "scenarios/commute_by_location", "scenarios/locations", "scenarios/group_diff_quantiles",
                "samples/scenario_by_group", "samples/scenario_diff_by_group"} <= new
        assert "scenarios/log_shift" not in new and "scenarios/commute" not in new
        for k in sorted(new):
            assert live[k].dtype == rep[k].dtype and live[k].shape == rep[k].shape and live[k].tobytes() == rep[k].tobytes(), k
        assert live["scenarios/log_shift_by_location"].shape == (2, M, Hn)
        assert live["scenarios/locations"].tolist() == [[1] * M, [1] * M]        # fifth_down and the second part apply everywhere
        assert live["samples/scenario_by_group"].shape == (n, 2, 3, Hn, 3)
        assert np.array_equal(live["samples/scenario_diff_by_group"],
                              live["samples/scenario_by_group"] - live["samples/forecast_by_group"][:, None])
        assert np.array_equal(live["samples/scenario_by_group"].sum(axis=2), live["samples/scenario_by_day"])     # a partition
        assert live["scenarios/group_diff_quantiles"].shape == (2, 2, 3, Hn, 3)
        # the global scenario is the same scenario in both runs: the same draws, the same curves
        plain, prep = outs["global"][0][c], outs["global"][1][c]
        assert np.array_equal(plain["samples/scenario_by_day"][:, 0], live["samples/scenario_by_day"][:, 0])
        # without the two new keys: today's datasets and nothing else
        old = {k for k in plain if k.startswith("scenarios/") or k.startswith("samples/scenario_")}
        assert len(old) == 20 and {"scenarios/log_shift", "scenarios/commute"} <= old and not any("group" in k or "location" in k for k in old)
        assert {k for k in prep if k.startswith("scenarios/") or k.startswith("samples/scenario_")} == old
        assert plain["scenarios/log_shift"].shape == (1, Hn)
        assert set(plain) - old == set(live) - new

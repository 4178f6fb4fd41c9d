"""Scenario forecasts on the device (include/seir_hip.h, "Scenario forecasts on the device"; covid19uk_amd/csrc/
scenario_kernels.h): the fold of a scenario's paired differences against the baseline, `SeirModel.scenario_diffs`, held to
the NumPy definition `posterior.scenarios.fold_differences` at the shapes that turn the kernel's branches.  Every
comparison is `np.array_equal` on integers.

The inputs are random int32 counts whose row totals over the days stay below 2^29 per transition, so that every one of the
four differences (a difference of two prefixes, and for the prevalence of two such differences) fits int32 as the
definition requires; 2^29 is below the 2^31 that bounds a population."""
import numpy as np
import pytest

from covid19uk_amd import _lib
from covid19uk_amd.posterior import scenarios as SC
from tests import helpers as H
from tests.test_sampler_gpu import api  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ROWS, JMAX, U = 8, 128, 4            # SC_ROWS, SC_JMAX, SC_U of scenario_kernels.h
KEYS = ("ref", "sum", "sumsq", "lt", "eq")


@pytest.fixture(scope="module")
def model(api):
    case = H.build_case("micro_3x1", 43)
    with api[0](case["cov"], case["init"], max_chains=1) as m:
        yield m


def _pair(rng, n, B, M, Hd, hi=None):
    """Two count tensors [n, B, M, H, 3]; `hi`: the bound of one count, by default the largest with row totals below 2^29."""
    hi = (2 ** 29 - 1) // Hd if hi is None else hi
    a = rng.integers(0, hi + 1, size=(n, B, M, Hd, 3), dtype=np.int64).astype(np.int32)
    b = rng.integers(0, hi + 1, size=(n, B, M, Hd, 3), dtype=np.int64).astype(np.int32)
    return a, b


def _same(got, want):
    assert got["count"] == want["count"] and got["overflow"] == want["overflow"]
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("Hd", [1, 63, 64, 65, 128])
@pytest.mark.parametrize("M", [1, 8, 9])
def test_the_fold_equals_numpy_at_the_chunk_and_workgroup_edges(model, M, Hd):
    """Days: one lane, one short of / exactly / one past a 64-day chunk, two chunks.  Rows: one, a whole workgroup's waves,
    one past them.  Two chains, five draws (one past a group of loads), small and large counts."""
    rng = np.random.default_rng([M, Hd])
    for hi in (3, None):
        fev, sev = _pair(rng, 5, 2, M, Hd, hi)
        got = model.scenario_diffs(fev, sev)
        _same(got, SC.fold_differences(fev, sev))
        assert not got["overflow"] or hi is None


@pytest.mark.parametrize("n", [1, 15, 16, 17, 128])
def test_the_draws_cut_into_two_calls_and_into_launches(model, n):
    """1, 15, 16, 17 and 128 draws (the forecast fold's flush edges; 128 fills a launch), whole and cut into two calls at
    every kind of place; 129 and 257 draws take two and three launches of one call."""
    rng = np.random.default_rng(n)
    fev, sev = _pair(rng, n, 3, 9, 65, 50)
    want = SC.fold_differences(fev, sev)
    _same(model.scenario_diffs(fev, sev), want)
    for cut in sorted(c for c in {1, U, n // 2, n - 1} if 0 < c < n):
        first = model.scenario_diffs(fev[:cut], sev[:cut])
        _same(first, SC.fold_differences(fev[:cut], sev[:cut]))
        _same(model.scenario_diffs(fev[cut:], sev[cut:], acc=first), want)
    if n == 128:
        for more in (JMAX + 1, 2 * JMAX + 1):
            f2, s2 = _pair(rng, more, 1, 3, 10, 50)
            _same(model.scenario_diffs(f2, s2), SC.fold_differences(f2, s2))


def test_all_equal_inputs_give_zeros_and_eq_is_the_count(model):
    rng = np.random.default_rng(5)
    fev, _ = _pair(rng, 17, 2, 9, 65)
    got = model.scenario_diffs(fev, fev.copy())
    for k in ("ref", "sum", "sumsq", "lt"):
        assert not got[k].any(), k
    assert np.all(got["eq"] == 17) and not got["overflow"]


def test_one_cell_differing_moves_its_own_days_and_nothing_else(model):
    """One more I->R event at (draw 3, chain 1, row 4, day 70): cases there, cum_cases from that day on, prevalence one day
    later; no other row, chain or earlier day moves."""
    rng = np.random.default_rng(6)
    fev, _ = _pair(rng, 6, 2, 9, 128, 100)
    sev = fev.copy()
    sev[3, 1, 4, 70, 2] += 1
    got = model.scenario_diffs(fev, sev)
    _same(got, SC.fold_differences(fev, sev))
    lt, eq = got["lt"], got["eq"]
    moved = np.zeros(eq.shape, bool)
    moved[1, 4, 70, 0] = True
    moved[1, 4, 70:, 1] = True
    moved[1, 4, 71:, 2] = True
    assert np.all(eq[~moved] == 6) and np.all(eq[moved] == 5)
    assert np.all(lt[1, 4, 71:, 2] == 1) and lt.sum() == 128 - 71     # prevalence falls by one; nothing else is below


def test_the_overflow_flag_is_raised_and_sticky(model):
    """Differences of +-2^30 against ref = 0: each adds 2^60 to sumsq, the eighth reaches 2^63."""
    n, big = 10, 2 ** 30
    fev = np.zeros((n, 1, 1, 1, 3), np.int32)
    sev = fev.copy()
    sev[1:, ..., 2] = big
    assert not model.scenario_diffs(fev[:8], sev[:8])["overflow"]
    got = model.scenario_diffs(fev, sev)
    _same(got, SC.fold_differences(fev, sev))
    assert got["overflow"]
    again = model.scenario_diffs(fev[:1], sev[:1], acc=got)
    assert again["overflow"] and again["count"] == n + 1


def test_the_fold_does_not_depend_on_workgroup_timing(api):
    case = H.build_case("micro_3x1", 43)
    fev, sev = _pair(np.random.default_rng(3), 17, 2, 17, 70, 1000)
    want = SC.fold_differences(fev, sev)
    for skew in (1, 2, 3):
        with api[0](case["cov"], case["init"], max_chains=1) as m:
            m.set_option(debug_skew=skew)
            _same(m.scenario_diffs(fev, sev), want)


def test_refusals(model):
    fev = np.zeros((2, 1, 3, 4, 3), np.int32)
    with pytest.raises(ValueError, match="need two of"):
        model.scenario_diffs(fev, fev[:1])
    with pytest.raises(ValueError, match="need two of"):
        model.scenario_diffs(fev[..., :2], fev[..., :2])

    def refused(f, word, **kw):
        with pytest.raises(_lib.SeirError) as e:
            model.scenario_diffs(f, f, **kw)
        assert e.value.code == _lib.ERR_INVALID and word in str(e.value), str(e.value)

    refused(np.zeros((0, 1, 3, 4, 3), np.int32), "at least one")
    refused(np.zeros((1, 1, 0, 4, 3), np.int32), "at least one")
    refused(np.zeros((1, 1, 1, 129, 3), np.int32), "H=129 outside [1, 128]")
    acc = model.scenario_diffs(fev, fev)
    refused(fev, "2^32 - 1", acc=dict(acc, count=2 ** 32 - 2))
    with pytest.raises(ValueError, match="these events need"):
        model.scenario_diffs(fev[:, :, :2], fev[:, :, :2], acc=acc)


# ---------------------------------------------------------------------------------------------------------------------
# scenarios riding on the sampler's forecast
# ---------------------------------------------------------------------------------------------------------------------
# The oracle is tests/test_forecast_gpu.py's: the same run's recorded draws, `SeirModel.simulate` per chain with
# first_draw_id = chain << 20, and for scenario k the stated equivalence -- a_path + log_shift[k] and W * commute[k].  Its
# docstring's rule holds here too: seeds are fixed, no tolerance; on a trip show the variate and take another seed.
from covid19uk_amd import synth  # noqa: E402
from covid19uk_amd.sampler import forecast_draw_id  # noqa: E402
from oracle import sim_oracle  # noqa: E402
from tests import test_forecast_gpu as FG  # noqa: E402
from tests.test_recovery_gpu import _case  # noqa: E402
from tests.test_sampler_gpu import CFG_REF, CFG_SMALL  # noqa: E402
from tests.test_summary_gpu import _sampler  # noqa: E402


def _spec(Hn, **scen):
    return SC.parse_scenarios(scen, Hn)


def _sims(model, case, theta, events, Hn, sc=None, k=None, seed=FG.SEED, chain0=0, j0=0, steps=None, simulate=None):
    """The simulated counts [n,B,M,H,3] of the baseline (k None) or of scenario k, and the state at T [n,B,M,4]."""
    n, B = theta.shape[:2]
    W, wd = FG._calendar(case, Hn)
    sims, st0s = [], []
    for b in range(B):
        par, a_path, spatial, st0 = FG._inputs(theta[:, b], events[:, b], case["init"], case["k"].T, Hn,
                                               None if steps is None else steps[:, b])
        a_k, W_k = (a_path, W) if k is None else SC.scenario_inputs(a_path, W, sc, k)
        sim = (simulate or model.simulate)(par, a_k, spatial, W_k, wd, st0.astype(np.float64), seed=seed,
                                           first_draw_id=forecast_draw_id(chain0 + b, j0))
        assert np.array_equal(sim, np.rint(sim))
        sims.append(sim.astype(np.int64))
        st0s.append(st0)
    return np.stack(sims, axis=1), np.stack(st0s, axis=1)


def _holds(model, s, case, theta, events, Hn, sc, **kw):
    """Every scenario's moments, curves and difference accumulators against the oracle; returns (baseline sims, diffs)."""
    base, st0 = _sims(model, case, theta, events, Hn, **kw)
    n, B = theta.shape[:2]
    assert s.scenario_state() == dict(K=sc.K, H=Hn, cap=s.scenario_state()["cap"], j=n)
    sums, diffs, draws = s.scenario_summary(), s.scenario_diffs(), s.read_scenario_draws()
    assert diffs["count"] == n and draws["by_day"].shape == (sc.K, n, B, Hn, 3)
    for k in range(sc.K):
        sim, _ = _sims(model, case, theta, events, Hn, sc, k, **kw)
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
    return base, diffs


def test_the_identity_scenario_is_the_forecast_and_every_difference_is_zero(api):
    case, u, ev, cfg, eps = _case("micro_9x64", 3)
    n, Hn = 5, 65
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        FG._reset(s, case, Hn)
        s.set_scenarios(np.zeros((1, Hn)), np.ones((1, Hn)), n)
        tr = s.sample(n, forecast=True)
        sm, sc = s.forecast_summary(), s.scenario_summary()[0]
        assert sm.sumsq.any()
        FG._same_moments(sc, dict(count=sm.count, ref=sm.ref, sum=sm.sum, sumsq=sm.sumsq))
        draws = s.read_scenario_draws()
        assert np.array_equal(draws["by_day"][0], tr.forecast["forecast_by_day"])
        assert np.array_equal(draws["state_by_day"][0], tr.forecast["forecast_state_by_day"])
        d = s.scenario_diffs()
        for key in ("ref", "sum", "sumsq", "lt"):
            assert not d[key].any(), key
        assert np.all(d["eq"] == n) and d["count"] == n


# name, cfg, eps, B, record, n, H, scenarios, steps
SCEN_CASES = {
    "M=1,H=1,K=1": ("micro_1x70", CFG_SMALL, 0.002, 3, "u16", 6, 1, dict(half=dict(transmission=0.5)), False),
    "T=1,K=2": ("micro_3x1", CFG_SMALL, 0.002, 1, True, 4, 7, dict(a=dict(transmission=0.5), b=dict(commute=0.0)), False),
    "9x64,H=64,K=4,from_day": ("micro_9x64", CFG_SMALL, 0.0004, 3, "u16", 5, 64,
                               dict(a=dict(transmission=0.5), b=dict(commute=0.0), c=dict(transmission=1.5, commute=0.5, from_day=7),
                                    d=dict(transmission=[1.0 - 0.5 * i / 64 for i in range(64)])), False),
    "9x64,H=65,K=2,steps": ("micro_9x64", CFG_SMALL, 0.0004, 8, True, 4, 65,
                            dict(a=dict(transmission=0.8, from_day=64), b=dict(commute=2.0)), True),
    "M=65,H=7,K=1": ("micro_65x70", CFG_SMALL, 0.0001, 1, "u16", 9, 7, dict(a=dict(transmission=0.5, commute=0.5)), False),
    "M=520,H=128,K=2": ("slow_520x70", CFG_SMALL, 3e-5, 2, True, 3, 128, dict(a=dict(transmission=0.5), b=dict(commute=0.0)), False),
    "uk380x8,12,H=14,K=2": ("uk380", CFG_REF, 1.2e-5, 8, "u16", 12, 14, dict(a=dict(transmission=0.8, from_day=7), b=dict(commute=0.5)),
                            False),
    # the day cell's indexing all at once: M no multiple of the day kernel's 4 rows, ND = 65 (two column blocks per scenario, the
    # second with one live draw), K = 2, and B = 5, which does not divide 64: a wave's draws begin in the middle of a slot
    "ni11,B=5,ND=65,H=3,K=2": ("ni11", CFG_REF, 0.002, 5, "u16", 13, 3,
                               dict(a=dict(transmission=0.5), b=dict(transmission=1.2, commute=0.5, from_day=1)), False),
}


@pytest.mark.parametrize("case_id", list(SCEN_CASES))
def test_scenarios_equal_simulate_on_the_recorded_draws(api, case_id):
    name, cfg, eps, B, record, n, Hn, scen, walk = SCEN_CASES[case_id]
    case = H.build_case(name, 43, alpha_t_sd=0.005)
    u = synth.jitter_params(case["u"], B, scale=0.002 if name == "uk380" else 0.01, seed=3, T=case["k"].T)
    ev = np.stack([case["events"]] * B)
    sc = _spec(Hn, **scen)
    steps = np.random.default_rng(5).normal(0.0, 0.05, size=(n, B, Hn)) if walk else None
    model, s = _sampler(api, case, cfg, u, ev, eps, n, record_events=record)
    with model, s:
        FG._reset(s, case, Hn)
        s.set_scenarios(sc.log_shift, sc.commute, n)
        tr = s.sample(n, forecast=(lambda j0, count: steps[j0:j0 + count]) if walk else True)
        # the forecast keeps its bits with scenarios on
        want = FG._oracle(model, case, tr.theta, tr.events, Hn, steps=steps)
        FG._same_marginals(tr.forecast, want)
        FG._same_moments(s.forecast_summary(), want)
        base, _ = _holds(model, s, case, tr.theta, tr.events, Hn, sc, steps=steps)
        assert np.array_equal(base, want["sim"])
        assert not s.pair_timeouts().any()


@pytest.mark.parametrize("name,Hn", [("micro_9x64", 3), ("micro_3x1", 4)])
def test_scenarios_equal_the_independent_cpu_simulator(api, name, Hn):
    case, u, ev, cfg, eps = _case(name, 2)
    n = 3
    sc = _spec(Hn, a=dict(transmission=0.5), b=dict(commute=0.0, from_day=1))
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        FG._reset(s, case, Hn)
        s.set_scenarios(sc.log_shift, sc.commute, n)
        tr = s.sample(n, forecast=True)
        k = H.oracle_constants(case["cov"], case["init"])
        _holds(model, s, case, tr.theta, tr.events, Hn, sc, simulate=lambda *a, **kw: sim_oracle.simulate(k, *a, **kw))


def test_halving_transmission_lowers_raises_and_leaves_cells_and_day_zero_prevalence_is_equal(api):
    """transmission x 0.5 on micro_9x64: over 24 draws the daily `cases` difference has cells with draws below, equal and above
    the baseline -- the sign structure a paired difference shows; the prevalence of day 0 is the common state's: equal."""
    case, u, ev, cfg, eps = _case("micro_9x64", 3)
    n, Hn = 8, 14
    sc = _spec(Hn, half=dict(transmission=0.5))
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        FG._reset(s, case, Hn, seed=43)
        s.set_scenarios(sc.log_shift, sc.commute, n)
        s.sample(n, forecast=True)
        d = s.scenario_diffs()
    lt, eq = d["lt"][0].astype(np.int64), d["eq"][0].astype(np.int64)
    gt = n - lt - eq
    print("cases: cells with draws below / equal / above:", (lt[..., 0] > 0).sum(), (eq[..., 0] > 0).sum(), (gt[..., 0] > 0).sum())
    assert (lt[..., 0] > 0).any() and (eq[..., 0] > 0).any() and (gt[..., 0] > 0).any()
    assert np.all(eq[:, :, 0, 2] == n)
    assert lt[..., 3].sum() > gt[..., 3].sum()            # cumulative infections: mostly below


def test_cuts_batches_resets_and_refusals(api):
    """Two calls in the buffer's halves, one call, uneven calls: the same integers.  A second reset empties and keeps the
    scenarios; another horizon frees them; K = 0 frees; a call past cap and a set behind the first forecast are refused; a
    store above half of the free memory is refused and the forecast runs on."""
    case, u, ev, cfg, eps = _case("micro_20x60", 3)
    n, Hn = 11, 9
    sc = _spec(Hn, a=dict(transmission=0.5), b=dict(commute=0.0, from_day=2))
    model, s = _sampler(api, case, cfg, u, ev, eps, 2 * n)
    with model, s:
        assert s.scenario_state() == dict(K=0, H=0, cap=0, j=0)
        with pytest.raises(_lib.SeirError, match="seir_sampler_forecast_reset") as e:
            s.set_scenarios(sc.log_shift, sc.commute, 2 * n)
        assert e.value.code == _lib.ERR_STATE
        FG._reset(s, case, Hn)
        s.set_scenarios(sc.log_shift, sc.commute, 2 * n)
        for first in (0, n):
            s.reset_trace(at=first)
            s.run(n)
            s.forecast(first, n)
        tr = s.read_trace(2 * n)
        _, halves = _holds(model, s, case, tr.theta, tr.events, Hn, sc)
        draws = s.read_scenario_draws()
        assert halves["sumsq"].any() and (halves["lt"] > 0).any()
        with pytest.raises(_lib.SeirError, match="the draw store holds 22") as e:      # past cap: before any launch
            s.forecast(0, 1)
        assert e.value.code == _lib.ERR_INVALID and s.scenario_state()["j"] == 2 * n
        with pytest.raises(_lib.SeirError, match="first seir_sampler_forecast") as e:
            s.set_scenarios(sc.log_shift, sc.commute, 4 * n)
        assert e.value.code == _lib.ERR_STATE
        for cuts in (((0, 2 * n),), ((0, 3), (3, 1), (4, 9), (13, 2 * n - 13))):
            FG._reset(s, case, Hn)                             # empties, keeps the scenarios
            assert s.scenario_state() == dict(K=2, H=Hn, cap=2 * n, j=0)
            for first, count in cuts:
                s.forecast(first, count)
            again = s.scenario_diffs()
            for key in KEYS:
                assert np.array_equal(again[key], halves[key]), key
            got = s.read_scenario_draws()
            assert np.array_equal(got["by_day"], draws["by_day"]) and np.array_equal(got["state_by_day"], draws["state_by_day"])
            assert np.array_equal(s.read_scenario_draws(3, first=5)["by_day"], draws["by_day"][:, 5:8])
        with pytest.raises(_lib.SeirError, match="outside the 22 draws"):
            s.read_scenario_draws(2, first=21)
        # refusals of the values, and of a store that cannot be held: the forecast runs on without scenarios
        FG._reset(s, case, Hn)
        for ls, cm, word in ((np.full((1, Hn), np.nan), np.ones((1, Hn)), "not finite"), (np.zeros((1, Hn)), -np.ones((1, Hn)), ">= 0"),
                             (np.zeros((5, Hn)), np.ones((5, Hn)), "K=5")):
            with pytest.raises(_lib.SeirError, match=word) as e:
                s.set_scenarios(ls, cm, 4)
            assert e.value.code == _lib.ERR_INVALID
        assert s.scenario_state()["K"] == 2                    # a refused set leaves the scenarios in force alone
        # another horizon frees them; K = 0 frees
        FG._reset(s, case, Hn)
        s.set_scenarios(sc.log_shift, sc.commute, n)
        FG._reset(s, case, Hn + 1)
        assert s.scenario_state()["K"] == 0
        sc2 = _spec(Hn + 1, a=dict(commute=0.0))
        s.set_scenarios(sc2.log_shift, sc2.commute, n)
        s.forecast(0, n)
        _holds(model, s, case, tr.theta[:n], tr.events[:n], Hn + 1, sc2)
        FG._reset(s, case, Hn + 1)
        s.set_scenarios(None, None, 0)
        assert s.scenario_state() == dict(K=0, H=0, cap=0, j=0)
        with pytest.raises(_lib.SeirError, match="no scenarios are set") as e:
            s.scenario_diffs()
        assert e.value.code == _lib.ERR_STATE
        assert not s.pair_timeouts().any()


def test_stores_above_half_of_the_free_memory_are_refused_and_the_forecast_runs_on(api):
    """4 scenarios x 2^20 draws x 8 chains x 128 days x 3 x 16 bytes of stores are 206 GB, above half of any free memory of
    the device: refused, the scenarios that were set go, and the forecast is what it is without them."""
    case, u, ev, cfg, eps = _case("micro_20x60", 8)
    n, Hn = 3, 128
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        FG._reset(s, case, Hn)
        s.set_scenarios(np.zeros((1, Hn)), np.ones((1, Hn)), n)
        with pytest.raises(_lib.SeirError, match=r"the scenarios need \d+ bytes .* more than half of the \d+ bytes free") as e:
            s.set_scenarios(np.zeros((4, Hn)), np.ones((4, Hn)), 2 ** 20)
        assert e.value.code == _lib.ERR_INVALID and s.scenario_state() == dict(K=0, H=0, cap=0, j=0)
        tr = s.sample(n, forecast=True)
        want = FG._oracle(model, case, tr.theta, tr.events, Hn)
        FG._same_moments(s.forecast_summary(), want)
        FG._same_marginals(tr.forecast, want)


def test_a_call_of_two_host_batches_and_workgroup_skew(api):
    """130 slots: two batches of the host's cut.  The same integers under every debug skew."""
    case, u, ev, cfg, eps = _case("micro_5x24", 2)
    n, Hn = 130, 3
    sc = _spec(Hn, a=dict(transmission=0.5), b=dict(commute=0.0))
    res = {}
    for skew in (0, 1, 2, 3):
        model, s = _sampler(api, case, cfg, u, ev, 0.002, n, skew=skew)
        with model, s:
            FG._reset(s, case, Hn)
            s.set_scenarios(sc.log_shift, sc.commute, n)
            tr = s.sample(n, forecast=True)
            if skew == 0:
                _holds(model, s, case, tr.theta, tr.events, Hn, sc)
            res[skew] = (s.scenario_diffs(), s.read_scenario_draws(), [(m.ref, m.sum, m.sumsq) for m in s.scenario_summary()], tr.events)
    for skew in (1, 2, 3):
        assert np.array_equal(res[skew][3], res[0][3])
        for key in KEYS:
            assert np.array_equal(res[skew][0][key], res[0][0][key]), (skew, key)
        for key in ("by_day", "state_by_day"):
            assert np.array_equal(res[skew][1][key], res[0][1][key]), (skew, key)
        for a, b in zip(res[skew][2], res[0][2]):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_a_burst_run_again_after_a_time_out_is_counted_once(api):
    """tests/test_forecast_gpu.py's disturbance (the existing hook, once) with scenarios on: the re-run burst's scenario
    moments, differences and curves are those of its own draws, counted once."""
    case, u, ev, cfg, eps = _case("micro_20x60", 8)
    B, nb, burst, Hn = 8, 6, 4, 5
    sc = _spec(Hn, a=dict(transmission=0.5))
    model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
    with model, s:
        got = {}
        FG._reset(s, case, Hn)
        s.set_scenarios(sc.log_shift, sc.commute, nb * burst)

        def consume(tr, i):
            got[i] = (tr.events.copy(), tr.theta.copy())
            if i == 1 and not s.recoveries:
                _lib.check(s._lib.seir_sampler_debug_fail_handoff(s._s, B - 1))
        s.sample_bursts(nb, burst, consume, forecast=True)
        assert len(s.recoveries) == 1 and sorted(got) == list(range(nb))
        theta, events = np.concatenate([got[i][1] for i in range(nb)]), np.concatenate([got[i][0] for i in range(nb)])
        _holds(model, s, case, theta, events, Hn, sc)


def test_nothing_else_notices_the_scenarios(api):
    """The chain, the summaries, the forecast's moments, marginals, draw store and quantiles: bit for bit those of the same
    run without scenarios."""
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    nb, burst, Hn = 3, 5, 6
    sc = _spec(Hn, a=dict(transmission=0.5), b=dict(commute=0.0))
    runs = {}
    for on in (False, True):
        model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
        with model, s:
            got = {}
            FG._reset(s, case, Hn)
            s.keep_forecast_draws(nb * burst)
            if on:
                s.set_scenarios(sc.log_shift, sc.commute, nb * burst)

            def consume(tr, i, got=got):
                got[i] = (tr.theta.copy(), tr.events.copy(), {k: v.copy() for k, v in tr.marginals.items()},
                          {k: v.copy() for k, v in tr.forecast.items()})
            s.sample_bursts(nb, burst, consume, summarize=True, forecast=True)
            runs[on] = (got, s.get_state() + s.get_kernel(), s.summary(), s.forecast_summary(),
                        s.forecast_order_stats([0, nb * burst - 1]), s.forecast_quantiles([0.05, 0.5, 0.95], pooled=True))
    a, b = runs[False], runs[True]
    for i in range(nb):
        assert np.array_equal(a[0][i][0], b[0][i][0]) and np.array_equal(a[0][i][1], b[0][i][1])
        for part in (2, 3):
            for k in a[0][i][part]:
                assert np.array_equal(a[0][i][part][k], b[0][i][part][k]), k
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x, y)
    for part in (2, 3):
        for k in ("count", "ref", "sum", "sumsq"):
            assert np.array_equal(getattr(a[part], k), getattr(b[part], k)), k
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])


def _flat(x):
    """Every array of a summary record (a dataclass, possibly nested) or of a dict, by name."""
    import dataclasses
    if dataclasses.is_dataclass(x):
        x = {f.name: getattr(x, f.name) for f in dataclasses.fields(x)}
    out = {}
    for k, v in x.items():
        if dataclasses.is_dataclass(v) or isinstance(v, dict):
            out.update({f"{k}.{kk}": vv for kk, vv in _flat(v).items()})
        else:
            out[k] = np.asarray(v)
    return out


def test_no_other_product_notices_the_scenarios(api):
    """Every product on at once -- summaries, the forecast with its group sums, R_t, the check, within / between, the group
    sums of all three sources and both group curves -- with and without scenarios: every field of every burst's trace and
    every product's accumulators bit for bit.  The forecast's group sums run in the same hook just in front of the scenarios."""
    from covid19uk_amd.posterior import groups as G
    from covid19uk_amd.posterior import predict
    from covid19uk_amd.sampler import Trace
    case, u, ev, cfg, eps = _case("micro_20x60", 3)
    B, nb, burst, Hn, K, D = 3, 3, 4, 6, 5, 4
    cov, T, M = case["cov"], case["k"].T, case["k"].M
    N = np.asarray(cov.N, np.float64).reshape(-1)
    tab = G.parse_groups({"all": list(range(M)), "low": list(range(0, M, 2)), "one": [M - 1]}, M)
    sc = _spec(Hn, a=dict(transmission=0.5), b=dict(commute=0.0, from_day=2))
    kw = dict(summarize=True, forecast=inf_steps(7, list(range(B)), Hn), rt=True, check=True, within_between=True, groups=True)
    fields = tuple(f for f in Trace.__dataclass_fields__ if f not in ("hmc", "moves"))
    runs = {}
    for on in (False, True):
        model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
        with model, s:
            s.set_groups(tab.offsets, tab.members)
            s.set_group_rt(G.rt_weights(tab, N))
            s.set_group_within_between(True)
            s.reset_forecast(Hn, *predict.forecast_calendar(cov, None, T, Hn), 5)
            if on:
                s.set_scenarios(sc.log_shift, sc.commute, nb * burst)
            s.reset_check(K, *predict.check_calendar(cov, None, T, K), 6)
            s.reset_rt(D, N / N.sum())
            s.reset_within_between(D)
            got = {}

            def consume(tr, i, got=got):
                got[i] = {f: ({k: np.array(a) for k, a in getattr(tr, f).items()} if isinstance(getattr(tr, f), dict)
                              else np.array(getattr(tr, f))) for f in fields if getattr(tr, f) is not None}
            s.sample_bursts(nb, burst, consume, **kw)
            runs[on] = (got, _flat(dict(summary=s.summary(), forecast=s.forecast_summary(), rt=s.rt_summary(), check=s.check_summary(),
                                        wb=s.within_between_summary())), s.get_state())
            if on:
                assert s.scenario_state()["j"] == nb * burst and (s.scenario_diffs()["lt"] > 0).any()
    a, b = runs[False], runs[True]
    for i in range(nb):
        assert set(a[0][i]) == set(b[0][i]) >= {"theta", "events", "marginals", "forecast", "rt", "check", "wb", "groups", "group_curves"}
        for f in a[0][i]:
            for k, v in _flat({f: a[0][i][f]}).items():
                assert np.array_equal(v, _flat({f: b[0][i][f]})[k], equal_nan=True), (i, k)
    assert set(a[1]) == set(b[1]) and any(k.startswith("check.") for k in a[1]) and any(k.startswith("wb.") for k in a[1])
    for k in a[1]:
        assert np.array_equal(a[1][k], b[1][k], equal_nan=True), k
    for x, y in zip(a[2], b[2]):
        assert np.array_equal(x, y)


def inf_steps(seed, chain_ids, Hn):
    from covid19uk_amd.inference import inference as inf
    return inf.forecast_steps_fn(seed, chain_ids, Hn)


def test_repeated_runs_chain_sharding_and_thinning(api):
    """The same run twice gives the same integers.  Chains 2 and 3 of a 4-chain sampler against a 2-chain sampler created with
    first_chain_id = 2 (the global chain id enters the day kernel's RNG key), held to the oracle with chain0 = 2.  With
    thin = 3 the scenarios are those of the kept draws."""
    case, u, ev, cfg, eps = _case("micro_20x60", 4)
    n, Hn = 5, 8
    sc = _spec(Hn, a=dict(transmission=0.5), b=dict(commute=0.0))
    res = []
    for rep in range(2):
        model, s = _sampler(api, case, cfg, u, ev, eps, n)
        with model, s:
            FG._reset(s, case, Hn)
            s.set_scenarios(sc.log_shift, sc.commute, n)
            tr4 = s.sample(n, forecast=True)
            res.append((s.scenario_diffs(), s.read_scenario_draws(), [(m.count, m.ref, m.sum, m.sumsq) for m in s.scenario_summary()],
                        tr4.events))
    d4, dr4, sm4, ev4 = res[0]
    assert np.array_equal(res[1][3], ev4)
    for key in KEYS:
        assert np.array_equal(res[1][0][key], d4[key]), key
    assert np.array_equal(res[1][1]["by_day"], dr4["by_day"]) and np.array_equal(res[1][1]["state_by_day"], dr4["state_by_day"])
    assert all(np.array_equal(x, y) for a, b in zip(res[1][2], sm4) for x, y in zip(a, b))
    model, s = _sampler(api, case, cfg, u[2:], ev[2:], eps, n, first_chain_id=2)
    with model, s:
        FG._reset(s, case, Hn)
        s.set_scenarios(sc.log_shift, sc.commute, n)
        tr2 = s.sample(n, forecast=True)
        assert np.array_equal(tr4.events[:, 2:], tr2.events)
        _, d2 = _holds(model, s, case, tr2.theta, tr2.events, Hn, sc, chain0=2)
        dr2 = s.read_scenario_draws()
    assert d2["sumsq"].any()
    for key in KEYS:
        assert np.array_equal(d4[key][:, 2:], d2[key]), key
    assert np.array_equal(dr4["by_day"][:, :, 2:], dr2["by_day"]) and np.array_equal(dr4["state_by_day"][:, :, 2:], dr2["state_by_day"])
    # thinning
    k = 3
    model, s = _sampler(api, case, cfg, u, ev, eps, n, thin=k)
    with model, s:
        FG._reset(s, case, Hn)
        s.set_scenarios(sc.log_shift, sc.commute, n)
        kept = s.sample(n, forecast=True)
        got = (s.scenario_diffs(), s.read_scenario_draws())
    model, s = _sampler(api, case, cfg, u, ev, eps, n * k)
    with model, s:
        every = s.sample(n * k)
        assert np.array_equal(every.events[k - 1::k], kept.events)
        FG._reset(s, case, Hn)
        s.set_scenarios(sc.log_shift, sc.commute, n)
        base, _ = _sims(model, case, every.theta[k - 1::k], every.events[k - 1::k], Hn)
        for kk in range(sc.K):
            sim, _ = _sims(model, case, every.theta[k - 1::k], every.events[k - 1::k], Hn, sc, kk)
            fold = SC.fold_differences(base, sim)
            for key in KEYS:
                assert np.array_equal(got[0][key][kk], fold[key]), (kk, key)
            assert np.array_equal(got[1]["by_day"][kk], sim.sum(axis=2))


def test_the_command_lines_with_scenarios(api, tmp_path):
    """The inference command line on NI-11, two chains, with --forecast 14 --scenarios FILE, and the replay command line on its two
    files with the same flags: every scenarios/* and samples/scenario_* dataset equal.  The same live run without the flag
    writes every other dataset as the run with it, and nothing of the scenarios; so does the replay.  With --summaries only
    --thin 2 the datasets are written too, and the draws' differences are the scenario's curve minus the forecast's."""
    import os

    import yaml
    from covid19uk_amd.inference import inference as inf
    from tests.test_replay_gpu import _run
    from tests.test_summary_gpu import _datasets
    tmp = str(tmp_path)
    cov = synth.make_covariates("ni11")
    events, _, _ = synth.simulate_epidemic(cov)
    data = os.path.join(tmp, "data.h5")
    inf.write_inference_data(data, cov, events[..., 2])
    cfg, spath = os.path.join(tmp, "config.yaml"), os.path.join(tmp, "scenarios.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump(dict(Mcmc=dict(dmax=84, nmax=25, m=2, occult_nmax=15, num_event_time_updates=5, num_bursts=2,
                                      num_burst_samples=6, thin=1)), f)
    with open(spath, "w") as f:
        yaml.safe_dump({"fifth_down": {"transmission": 0.8, "from_day": 7}, "commuting_halved": {"commute": 0.5}}, f, sort_keys=False)      # the file's order is the scenarios'
    flags = ["--forecast", "14", "--forecast-quantiles", "0.05,0.95"]
    outs = {}
    for tag, extra in (("with", flags + ["--scenarios", spath]), ("without", flags)):
        out = os.path.join(tmp, f"{tag}.h5")
        log = _run("covid19uk_amd.inference.inference", ["-c", cfg, "-o", out, "--seed", "4", "--chains", "2", data] + extra, tmp)
        assert ("Scenario fifth_down:" in log and "Scenario commuting_halved:" in log) == (tag == "with")
        files = [inf.chain_file_name(out, c, 2) for c in range(2)]
        rout = os.path.join(tmp, f"{tag}_replay.h5")
        rlog = _run("covid19uk.posterior.replay", ["-c", cfg, "-o", rout, "--seed", "4", data] + files + extra, tmp)
        assert ("Scenario fifth_down:" in rlog) == (tag == "with")
        outs[tag] = ([_datasets(f) for f in files], [_datasets(inf.chain_file_name(rout, c, 2)) for c in range(2)])
    n = 12
    for c in range(2):
        live, rep = outs["with"][0][c], outs["with"][1][c]
        plain, prep = outs["without"][0][c], outs["without"][1][c]
        new = {k for k in live if k.startswith("scenarios/") or k.startswith("samples/scenario_")}
        assert {"scenarios/names", "scenarios/diff_mean", "scenarios/p_below", "scenarios/diff_lt", "scenarios/national_diff_quantiles",
                "samples/scenario_by_day", "samples/scenario_state_by_day", "samples/scenario_diff_by_day"} <= new and len(new) == 20
        # without the flag both command lines write what they write with it, less the scenarios' datasets
        assert set(plain) == set(live) - new and set(prep) == set(rep) - new
        for k in plain:
            assert plain[k].tobytes() == live[k].tobytes(), k
        for k in prep:
            if k != "replay/source":
                assert prep[k].tobytes() == rep[k].tobytes(), k
        # the replay gives the live run's scenario datasets
        for k in sorted(new):
            assert live[k].dtype == rep[k].dtype and live[k].shape == rep[k].shape and live[k].tobytes() == rep[k].tobytes(), k
        assert [x.decode() for x in live["scenarios/names"]] == ["fifth_down", "commuting_halved"] and live["scenarios/count"][0] == n
        assert live["samples/scenario_by_day"].shape == (n, 2, 14, 3)
        assert np.array_equal(live["samples/scenario_diff_by_day"], live["samples/scenario_by_day"] - live["samples/forecast_by_day"][:, None])
        assert not live["samples/scenario_diff_by_day"][:, 0, :7].any() and live["samples/scenario_diff_by_day"].any()
    out = os.path.join(tmp, "only.h5")
    _run("covid19uk_amd.inference.inference", ["-c", cfg, "-o", out, "--seed", "4", data, "--summaries", "only", "--thin", "2",
                                               "--forecast", "14", "--scenarios", spath], tmp)
    only = _datasets(inf.chain_file_name(out, 0, 1))
    assert "samples/seir" not in only and only["scenarios/diff_mean"].shape == (2, 11, 14, 4) and only["scenarios/count"][0] == n
    assert np.array_equal(only["samples/scenario_diff_by_day"], only["samples/scenario_by_day"] - only["samples/forecast_by_day"][:, None])
    assert np.array_equal(only["scenarios/diff_lt"] + only["scenarios/diff_eq"] <= n, np.ones((2, 11, 14, 4), bool))

"""Triggered scenarios on the device (include/seir_hip.h, "Triggered scenarios on the device"; covid19uk_amd/csrc/
scenario_trigger_kernels.h, trigger_update.h): measures that switch on and off by the draw's own simulated case counts.

The references need no new simulator:
  1. a rule that never fires is the targeted set with the off tensors, bit for bit;
  2. a rule that fires everywhere at day 0 and never releases is the targeted set with the on tensors;
  3. a rule that fires everywhere on day d is the targeted set whose tensors are off before d and on from d;
  4. with the on pair equal to the off pair the rollout does not notice the rule, so the record of the rule is
     `posterior.scenarios.trigger_states` applied to `SeirModel.simulate`'s counts and the recorded events;
  5. with commute = 0 and one review the active set is fixed by the recorded events and the rows decouple: a mix of two global
     `simulate` calls selected by a NumPy mask;
  6. with feedback, at micro sizes, the independent CPU simulator's day loop with the rule inside it;
  7. before the first day under the measure a triggered scenario is its off scenario;
  8. the fold alone against NumPy bit operations.
Every comparison is `np.array_equal` on integers; seeds are fixed.  A cell differing from the CPU simulator would be a finding to
explain against the near-tie mark of tests/binomial_lib.py, not a reason for a tolerance."""
import itertools

import numpy as np
import pytest

from covid19uk_amd import _lib, synth
from covid19uk_amd.posterior import scenarios as SC
from covid19uk_amd.sampler import forecast_draw_id
from oracle import mcmc_oracle, sim_oracle
from tests import helpers as H
from tests import test_forecast_gpu as FG
from tests.test_recovery_gpu import _case
from tests.test_sampler_gpu import CFG_REF, CFG_SMALL, api  # noqa: F401  (fixture)
from tests.test_scenarios_gpu import _sims
from tests.test_scenarios_local_gpu import SHAPES, _against, _build, _by_group, _csr, _everything, _global, _over_rows, _same
from tests.test_summary_gpu import _sampler

pytestmark = pytest.mark.gpu

NEVER = SC.INT32_MAX
# the shapes of tests/test_scenarios_local_gpu.py and one series shorter than the window: T = 3 < w = 7
TRIG_SHAPES = dict(SHAPES, **{"M=5,T=3,H=9,K=2,B=3": ("micro_5x3", CFG_SMALL, 0.002, 3, True, 4, 9, 2)})


def _build_any(api, case_id, cap=None):  # noqa: F811
    if case_id in SHAPES:
        return _build(api, case_id, cap)
    name, cfg, eps, B, record, n, Hn, K = TRIG_SHAPES[case_id]
    case = H.build_case(name, 43, alpha_t_sd=0.005)
    u = synth.jitter_params(case["u"], B, scale=0.01, seed=3, T=case["k"].T)
    model, s = _sampler(api, case, cfg, u, np.stack([case["events"]] * B), eps, n if cap is None else cap, record_events=record)
    return case, model, s, n, Hn, K, B


def _trig(K, M, on, off, ls_on, cm_on, window=7, from_day=0, min_days=0, review_every=1):
    """What `set_scenarios(triggers=...)` takes: thresholds a scalar or [K, M], parameters a scalar or [K]."""
    full = lambda v, shape: np.broadcast_to(np.asarray(v, np.int64), shape).astype(np.int32)   # noqa: E731
    return dict(log_shift_on=ls_on, commute_on=cm_on, on=full(on, (K, M)), off=full(off, (K, M)), window=full(window, (K,)),
                from_day=full(from_day, (K,)), min_days=full(min_days, (K,)), review_every=full(review_every, (K,)))


def _pairs(K, M, Hn, seed=5):
    """Two operand pairs that vary over k, m and s (commuting on)."""
    rng = np.random.default_rng([K, M, Hn, seed])
    return (rng.normal(0.0, 0.3, size=(K, M, Hn)), rng.uniform(0.0, 2.0, size=(K, M, Hn)),
            rng.normal(-0.5, 0.3, size=(K, M, Hn)), rng.uniform(0.0, 2.0, size=(K, M, Hn)))


def _record(s):
    return s.scenario_triggers(), s.read_scenario_trigger_draws()


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2. never fires: the off tensors; always fires: the on tensors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", list(TRIG_SHAPES))
def test_a_rule_that_never_fires_is_the_off_set_and_one_that_always_fires_the_on_set(api, case_id):  # noqa: F811
    case, model, s, n, Hn, K, B = _build_any(api, case_id)
    M = case["k"].M
    ls, cm, ls_on, cm_on = _pairs(K, M, Hn)
    with model, s:
        FG._reset(s, case, Hn)
        s.set_scenarios(ls, cm, n)
        s.sample(n, forecast=True)
        off_set = _everything(s)
        with pytest.raises(_lib.SeirError, match="no triggers") as e:
            s.scenario_triggers()
        assert e.value.code == _lib.ERR_STATE
        FG._reset(s, case, Hn)
        s.set_scenarios(ls_on, cm_on, n)
        s.forecast(0, n)
        on_set = _everything(s)
        assert M == 1 or any(not np.array_equal(off_set[k], on_set[k]) for k in off_set)
        # never: a window of every length, a review every day
        FG._reset(s, case, Hn)
        s.set_scenarios(ls, cm, n, triggers=_trig(K, M, NEVER, 0, ls_on, cm_on, window=[1, 7, 28, 3][:K]))
        assert s.scenario_state() == dict(K=K, H=Hn, cap=n, j=0)
        s.forecast(0, n)
        _same(_everything(s), off_set)
        cnt, by_day = _record(s)
        assert cnt["count"] == n and cnt["active_count"].dtype == np.uint32 and cnt["active_count"].shape == (K, B, M, Hn)
        assert by_day.dtype == np.int32 and by_day.shape == (K, n, B, Hn)
        assert not cnt["active_count"].any() and not by_day.any()
        # always: on = 0 from day 0, off = 0 never releases (no count is below 0)
        FG._reset(s, case, Hn)
        s.set_scenarios(ls, cm, n, triggers=_trig(K, M, 0, 0, ls_on, cm_on, window=[28, 1, 7, 3][:K], min_days=[0, 3, 0, 1][:K]))
        s.forecast(0, n)
        _same(_everything(s), on_set)
        cnt, by_day = _record(s)
        assert np.all(cnt["active_count"] == n) and np.all(by_day == M)
        assert not s.pair_timeouts().any()


# ---------------------------------------------------------------------------------------------------------------------
# 3. fires from day d
# ---------------------------------------------------------------------------------------------------------------------
def test_a_rule_that_fires_on_day_d_is_the_set_that_is_off_before_d_and_on_from_d(api):  # noqa: F811
    """H = 128, d = 1, 63, 64, 65: around the two words of the record and the fold's 64-day chunk."""
    case = H.build_case("slow_9x64", 43, alpha_t_sd=0.005)
    B, n, Hn, M, K = 2, 4, 128, 9, 1
    u = synth.jitter_params(case["u"], B, scale=0.01, seed=3, T=case["k"].T)
    model, s = _sampler(api, case, CFG_SMALL, u, np.stack([case["events"]] * B), 1e-4, n)
    ls, cm, ls_on, cm_on = _pairs(K, M, Hn)
    with model, s:
        FG._reset(s, case, Hn)
        s.sample(n, forecast=True)
        for d in (1, 63, 64, 65):
            FG._reset(s, case, Hn)
            s.set_scenarios(np.concatenate([ls[..., :d], ls_on[..., d:]], axis=-1),
                            np.concatenate([cm[..., :d], cm_on[..., d:]], axis=-1), n)
            s.forecast(0, n)
            want = _everything(s)
            FG._reset(s, case, Hn)
            s.set_scenarios(ls, cm, n, triggers=_trig(K, M, 0, 0, ls_on, cm_on, from_day=d, review_every=1 if d != 64 else 200))
            s.forecast(0, n)
            _same(_everything(s), want)
            cnt, by_day = _record(s)
            assert not cnt["active_count"][..., :d].any() and np.all(cnt["active_count"][..., d:] == n), d
            assert not by_day[..., :d].any() and np.all(by_day[..., d:] == M), d
        # from_day = H: no review at all
        FG._reset(s, case, Hn)
        s.set_scenarios(ls, cm, n, triggers=_trig(K, M, 0, 0, ls_on, cm_on, from_day=Hn))
        s.forecast(0, n)
        assert not _record(s)[1].any()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the rule alone
# ---------------------------------------------------------------------------------------------------------------------
def _window_sums(hist, cases, w):
    """c at the start of every rollout day: hist [.., h], cases [.., H] -> [.., H]."""
    h = hist[..., max(hist.shape[-1] - w, 0):]
    series = np.concatenate([np.zeros(cases.shape[:-1] + (w - h.shape[-1],), np.int64), h, cases], axis=-1)
    cs = np.concatenate([np.zeros(cases.shape[:-1] + (1,), np.int64), np.cumsum(series, axis=-1)], axis=-1)
    return (cs[..., w:] - cs[..., :-w])[..., :cases.shape[-1]]


PARAMS = list(itertools.product((1, 7, 28), (0, 3), (1, 7), (0, 2)))     # window, min_days, review_every, from_day


@pytest.mark.parametrize("case_id", list(TRIG_SHAPES))
def test_the_rule_alone_equals_trigger_states_on_simulates_counts(api, case_id):  # noqa: F811
    """The on pair is the off pair, constant over m: the rollout is `SeirModel.simulate` per chain whatever the rule does, and
    the record is `trigger_states` of those counts with the history taken from the recorded events.  on[m] is the median over
    the draws of the row's largest window sum and off half of it, so that firing and not firing occur by construction."""
    case, model, s, n, Hn, K, B = _build_any(api, case_id)
    M, T = case["k"].M, case["k"].T
    rng = np.random.default_rng([Hn, K, 4])
    gl, gc = rng.normal(0.0, 0.2, size=(K, Hn)), rng.uniform(0.5, 1.5, size=(K, Hn))
    sc = SC.Scenarios(tuple("abcd"[:K]), Hn, gl, gc)
    ls, cm = _over_rows(gl, M), _over_rows(gc, M)
    seen = dict(fired=0, never=0, released=0, again=0)
    with model, s:
        FG._reset(s, case, Hn)
        tr = s.sample(n, forecast=True)
        base, st0 = _sims(model, case, tr.theta, tr.events, Hn)
        sims = [_sims(model, case, tr.theta, tr.events, Hn, sc, k)[0] for k in range(K)]
        hist = np.asarray(tr.events)[..., 2].astype(np.int64)                       # [n, B, M, T]
        assert hist.shape == (n, B, M, T)
        for i, (w, min_days, review_every, from_day) in enumerate(PARAMS):
            if from_day > Hn:
                continue
            on = np.stack([np.median(_window_sums(hist, sims[k][..., 2], w).max(axis=-1).reshape(n * B, M), axis=0)
                           for k in range(K)]).astype(np.int64)
            off = on // 2
            FG._reset(s, case, Hn)
            s.set_scenarios(ls, cm, n, triggers=_trig(K, M, on, off, ls, cm, window=w, from_day=from_day, min_days=min_days,
                                                      review_every=review_every))
            s.forecast(0, n)
            if i == 0:
                _against(s, base, st0, sims)
            cnt, by_day = _record(s)
            for k in range(K):
                act = SC.trigger_states(hist, sims[k][..., 2], on[k], off[k], w, from_day, min_days, review_every)   # [n, B, M, H]
                assert np.array_equal(cnt["active_count"][k], act.sum(axis=0)), (w, min_days, review_every, from_day, k)
                assert np.array_equal(by_day[k], act.sum(axis=2)), (w, min_days, review_every, from_day, k)
                a = act.astype(np.int8)
                steps = np.diff(a, axis=-1)
                seen["fired"] += int(a.any(axis=-1).sum())
                seen["never"] += int((~a.any(axis=-1)).sum())
                seen["released"] += int((steps < 0).any(axis=-1).sum())
                seen["again"] += int(((steps > 0).sum(axis=-1) + a[..., 0] > 1).sum())
        print(case_id, seen)
        assert seen["fired"] and (seen["never"] or n * B * M == 1 or Hn == 1)
        if case_id in ("M=9,H=64,K=4,B=3,u16", "M=9,H=65,K=2,B=8"):                # a micro epidemic, which burns out within H
            assert seen["released"]
        assert not s.pair_timeouts().any()


# ---------------------------------------------------------------------------------------------------------------------
# 5. decoupled, one review
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ["M=9,H=65,K=2,B=8", "M=520,H=128,K=2,B=2"])
def test_without_commuting_and_with_one_review_the_counts_are_a_mix_selected_by_the_recorded_events(api, case_id):  # noqa: F811
    """commute = 0 in both pairs, review_every >= H: the one review is day 0, its window the recorded events alone.  The on
    pair halves transmission.  on[m] is the median over the draws of the row's recorded window sum, plus one in the odd rows."""
    case, model, s, n, Hn, _, B = _build_any(api, case_id)
    M, w = case["k"].M, 7
    zero = np.zeros(Hn)
    with model, s:
        FG._reset(s, case, Hn)
        tr = s.sample(n, forecast=True)
        base, st0 = _sims(model, case, tr.theta, tr.events, Hn)
        inside, _ = _sims(model, case, tr.theta, tr.events, Hn, _global(Hn, np.full(Hn, np.log(0.5)), zero), 0)
        outside, _ = _sims(model, case, tr.theta, tr.events, Hn, _global(Hn, zero, zero), 0)
        c0 = np.asarray(tr.events)[..., -w:, 2].astype(np.int64).sum(axis=-1)           # [n, B, M]
        on = np.median(c0.reshape(n * B, M), axis=0).astype(np.int64) + np.arange(M) % 2
        mask = c0 >= on
        print(case_id, "active cells:", int(mask.sum()), "of", mask.size)
        assert mask.any() and not mask.all() and len({tuple(mask[:, :, m].reshape(-1)) for m in range(M)}) > 1
        mix = np.where(mask[..., None, None], inside, outside)
        FG._reset(s, case, Hn)
        s.set_scenarios(np.zeros((1, M, Hn)), np.zeros((1, M, Hn)), n,
                        triggers=_trig(1, M, on[None], 0, np.full((1, M, Hn), np.log(0.5)), np.zeros((1, M, Hn)), window=w,
                                       review_every=Hn))
        s.forecast(0, n)
        _against(s, base, st0, [mix])
        cnt, by_day = _record(s)
        assert np.array_equal(cnt["active_count"][0], np.repeat(mask.sum(axis=0)[..., None], Hn, axis=-1))
        assert np.array_equal(by_day[0], np.repeat(mask.sum(axis=2)[..., None], Hn, axis=-1))
        assert not np.array_equal(inside, outside)


# ---------------------------------------------------------------------------------------------------------------------
# 6. feedback, against the independent CPU simulator
# ---------------------------------------------------------------------------------------------------------------------
def _cpu_triggered(k, par, ops, spatial, wd, st0, seed, first, hist, rule):
    """`oracle.sim_oracle.simulate`'s day loop with per-location operands and the rule inside it.  ops = ((a_off [n, M, H],
    W_off [M, H]), (a_on, W_on)) (`SC.triggered_inputs`); hist [n, M, h] the recorded I->R counts; rule = (on [M], off [M],
    window, from_day, min_days, review_every).  Returns the counts [n, M, H, 3] and active [n, M, H]."""
    (a_off, W_off), (a_on, W_on) = ops
    on, off, w, from_day, min_days, review_every = rule
    n, M, Hn = a_off.shape
    out, act = np.zeros((n, M, Hn, 3)), np.zeros((n, M, Hn), np.uint8)
    for d in range(n):
        state = np.array(st0[d], dtype=np.float64)
        th = np.concatenate([np.asarray(par[d], np.float64), np.asarray(spatial[d], np.float64)])
        h = hist[d][:, max(hist.shape[-1] - w, 0):]
        past = [np.zeros(M, np.int64)] * (w - h.shape[-1]) + [h[:, i].astype(np.int64) for i in range(h.shape[-1])]
        active, age = np.zeros(M, bool), np.zeros(M, np.int64)
        for s in range(Hn):
            c = np.sum(past[-w:], axis=0)
            if s >= from_day and (s - from_day) % review_every == 0:
                for m in range(M):                                       # the rule as the issue states it, cell by cell
                    if not active[m] and c[m] >= on[m]:
                        active[m], age[m] = True, 0
                    elif active[m] and age[m] >= min_days and c[m] < off[m]:
                        active[m] = False
            act[d, :, s] = active
            a_s = np.where(active, a_on[d, :, s], a_off[d, :, s])
            W_s = np.where(active, W_on[:, s], W_off[:, s])
            lam, nu, rir = sim_oracle.day_rates(state, th, a_s, W_s, float(wd[s]), k)
            p_ei, p_ir = sim_oracle._prob(nu * 1.0), sim_oracle._prob(rir * 1.0)
            for m in range(M):
                cell = s * M + m
                for x, (src, p) in enumerate(((0, sim_oracle._prob(float(lam[m]) * 1.0)), (1, p_ei), (2, p_ir))):
                    out[d, m, s, x] = sim_oracle.binomial(
                        state[m, src], p, lambda att, x=x, cell=cell: tuple(
                            float(v[0]) for v in mcmc_oracle.rng_uniform2(seed, first + d, cell, sim_oracle.RS_SIM_BASE + x, att)))
            state = state + out[d, :, s, :] @ sim_oracle.so.STOICHIOMETRY
            age = age + active
            past.append(out[d, :, s, 2].astype(np.int64))
    return out, act


@pytest.mark.parametrize("name", ["micro_9x64", "micro_3x1"])
def test_triggered_scenarios_with_feedback_equal_the_independent_cpu_simulator(api, name):  # noqa: F811
    """H = 16, w = 3, then: transmission x 0.3, min_days = 2.  The off scenario is transmission x 0.2, under which the recoveries
    decline within the horizon whatever the rule does -- with the baseline's transmission these epidemics grow or hold their level
    over 16 days even under the measure (the I -> R counts lag the infections by the two sojourn times), and no window comes back
    below the level that triggered.  Thresholds from an oracle pass of the off scenario: on[m] the median of the row's window sums
    over draws and days (at least 1), off the same level; every third row has on one above the largest window sum of any draw of
    that pass, and never fires."""
    assert sim_oracle.so.TIME_DELTA == 1.0
    case, u, ev, cfg, eps = _case(name, 2)
    M, T, n, Hn, w = case["k"].M, case["k"].T, 4, 16, 3
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    ls, cm = np.full((1, M, Hn), np.log(0.2)), np.ones((1, M, Hn))
    ls_on = ls + np.log(0.3)
    pending = SC.TriggeredScenarios(("tier",), Hn, ls, cm, np.ones((1, M), np.uint8), ls_on, cm)
    with model, s:
        FG._reset(s, case, Hn)
        tr = s.sample(n, forecast=True)
        k = H.oracle_constants(case["cov"], case["init"])
        B = tr.theta.shape[1]
        cpu = lambda *a, **kw: sim_oracle.simulate(k, *a, **kw)   # noqa: E731
        base, st0 = _sims(model, case, tr.theta, tr.events, Hn, simulate=cpu)
        hist = np.asarray(tr.events)[..., 2].astype(np.int64)                       # [n, B, M, T]
        off_pass, _ = _sims(model, case, tr.theta, tr.events, Hn, _global(Hn, ls[0, 0], cm[0, 0]), 0, simulate=cpu)
        sums = _window_sums(hist, off_pass[..., 2], w)                              # [n, B, M, H]
        on = np.maximum(np.quantile(np.moveaxis(sums, 2, 0).reshape(M, -1), 0.5, axis=1).astype(np.int64), 1)
        off = on.copy()                             # released as soon as the window is back below the level that triggers
        on[2::3] = sums.max(axis=(0, 1, 3))[2::3] + 1    # every third row: above every window of the off pass, so it never fires
        W, wd = FG._calendar(case, Hn)
        sims, acts = [], []
        for b in range(B):
            par, a_path, spatial, s0 = FG._inputs(tr.theta[:, b], tr.events[:, b], case["init"], T, Hn)
            sim, act = _cpu_triggered(k, par, SC.triggered_inputs(a_path, W, pending, 0), spatial, wd, s0.astype(np.float64), FG.SEED,
                                      forecast_draw_id(b, 0), hist[:, b], (on, off, w, 0, 2, 1))
            sims.append(sim.astype(np.int64))
            acts.append(act)
        sim, act = np.stack(sims, axis=1), np.stack(acts, axis=1)                  # [n, B, M, H(, 3)]
        FG._reset(s, case, Hn)
        s.set_scenarios(ls, cm, n, triggers=_trig(1, M, on[None], off[None], ls_on, cm, window=w, min_days=2))
        s.forecast(0, n)
        cnt, by_day = _record(s)
        steps = np.diff(act.astype(np.int8), axis=-1)
        print(name, "fired", int(act.any(axis=-1).sum()), "released", int((steps < 0).any(axis=-1).sum()), "never",
              int((~act.any(axis=-1)).sum()), "of", act[..., 0].size, "differing from the off pass:", int((sim != off_pass).sum()))
        assert np.array_equal(cnt["active_count"][0], act.sum(axis=0)) and np.array_equal(by_day[0], act.sum(axis=2))
        _against(s, base, st0, [sim])
        assert act.any(axis=-1).any() and (steps < 0).any() and (~act.any(axis=-1)).any()
        assert not np.array_equal(sim, off_pass)              # the measure fed back into the epidemic


# ---------------------------------------------------------------------------------------------------------------------
# 7. the prefix
# ---------------------------------------------------------------------------------------------------------------------
def test_before_the_first_day_under_the_measure_a_triggered_scenario_is_its_off_scenario(api):  # noqa: F811
    case, u, ev, cfg, eps = _case("micro_20x60", 3)
    n, Hn, M, w = 6, 24, 20, 7
    ls, cm, ls_on, cm_on = _pairs(1, M, Hn)
    ls_on = ls + np.log(0.3)
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        FG._reset(s, case, Hn)
        tr = s.sample(n, forecast=True)
        c0 = np.asarray(tr.events)[..., -w:, 2].astype(np.int64).sum(axis=-1)
        on = np.full((2, M), NEVER, np.int64)
        on[1] = np.quantile(c0.reshape(-1, M), 0.75, axis=0).astype(np.int64) + 2  # above most windows at day 0: it fires later
        FG._reset(s, case, Hn)
        s.set_scenarios(np.concatenate([ls, ls]), np.concatenate([cm, cm]), n,
                        triggers=_trig(2, M, on, 0, np.concatenate([ls_on, ls_on]), np.concatenate([cm_on, cm_on]), window=w))
        s.forecast(0, n)
        by_day, (cnt, act) = s.read_scenario_draws()["by_day"], _record(s)
        assert not act[0].any() and act[1].any()
        differs = later = 0
        for j in range(n):
            for b in range(3):
                first = int(np.argmax(act[1, j, b] > 0)) if act[1, j, b].any() else Hn
                assert np.array_equal(by_day[0, j, b, :first], by_day[1, j, b, :first]), (j, b, first)
                differs += int(not np.array_equal(by_day[0, j, b, first:], by_day[1, j, b, first:]))
                later += int(0 < first < Hn)
        print("draws differing from the first day under the measure on:", differs, "first day behind day 0:", later)
        assert differs and later


# ---------------------------------------------------------------------------------------------------------------------
# 8. the fold alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(api):  # noqa: F811
    case = H.build_case("micro_3x1", 43)
    with api[0](case["cov"], case["init"], max_chains=1) as m:
        yield m


def _masks(rng, n, B, M):
    return rng.integers(0, 2 ** 63, size=(n, B, M, 2), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, B, M, 2), dtype=np.uint64)


def _same_fold(got, want):
    assert got["count"] == want["count"]
    for key, ty in (("active_count", np.uint32), ("active_by_day", np.int32)):
        assert got[key].dtype == ty and got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), key


@pytest.mark.parametrize("M,Hd", [(1, 1), (8, 63), (9, 64), (9, 65), (8, 128), (1, 128)])
def test_the_fold_of_the_record_equals_numpy_bit_operations(model, M, Hd):
    rng = np.random.default_rng([M, Hd])
    for n, B in ((1, 1), (5, 3), (3, 65)):
        mk = _masks(rng, n, B, M)
        _same_fold(model.trigger_counts(mk, Hd), SC.fold_triggers(mk, Hd))
    one = np.zeros((2, 2, M, 2), np.uint64)
    one[1, 0, M - 1, (Hd - 1) >> 6] = np.uint64(1) << np.uint64((Hd - 1) & 63)     # the last day of the last row of one draw
    got = model.trigger_counts(one, Hd)
    assert got["active_count"].sum() == 1 and got["active_count"][0, M - 1, Hd - 1] == 1 and got["active_by_day"][1, 0, Hd - 1] == 1


@pytest.mark.parametrize("n", [1, 127, 128, 129])
def test_the_records_draws_cut_into_two_calls_and_into_launches(model, n):
    rng = np.random.default_rng(n)
    B, M, Hd = 2, 9, 65
    mk = _masks(rng, n, B, M)
    want = SC.fold_triggers(mk, Hd)
    _same_fold(model.trigger_counts(mk, Hd), want)
    if n > 1:
        cut = n // 3 + 1
        first = model.trigger_counts(mk[:cut], Hd)
        second = model.trigger_counts(mk[cut:], Hd, acc=first)
        assert second["count"] == n and np.array_equal(second["active_count"], want["active_count"])
        assert np.array_equal(np.concatenate([first["active_by_day"], second["active_by_day"]]), want["active_by_day"])


def test_the_fold_of_the_record_does_not_depend_on_workgroup_timing_and_its_refusals(api):  # noqa: F811
    case = H.build_case("micro_3x1", 43)
    rng = np.random.default_rng(8)
    mk = _masks(rng, 130, 3, 9)
    want = SC.fold_triggers(mk, 128)
    for skew in (1, 2, 3):
        with api[0](case["cov"], case["init"], max_chains=1) as m:
            m.set_option(debug_skew=skew)
            _same_fold(m.trigger_counts(mk, 128), want)
    with api[0](case["cov"], case["init"], max_chains=1) as m:
        with pytest.raises(ValueError, match="need"):
            m.trigger_counts(mk[..., :1], 8)
        for bad in (0, 129):
            with pytest.raises(_lib.SeirError, match="H=") as e:
                m.trigger_counts(mk, bad)
            assert e.value.code == _lib.ERR_INVALID
        with pytest.raises(_lib.SeirError, match="at least one of each"):
            m.trigger_counts(mk[:0], 8)
        with pytest.raises(_lib.SeirError, match="2\\^32 - 1"):
            m.trigger_counts(mk[:2], 8, acc=dict(count=2 ** 32 - 2, active_count=np.zeros((3, 9, 8), np.uint32)))
        with pytest.raises(ValueError, match="these masks need"):
            m.trigger_counts(mk[:2], 8, acc=dict(count=1, active_count=np.zeros((3, 9, 7), np.uint32)))


# ---------------------------------------------------------------------------------------------------------------------
# 9. plumbing
# ---------------------------------------------------------------------------------------------------------------------
def _near(case, w):
    """Per row a threshold next to the window sum the chains start from (the case's own events: the draws stay near them): one
    below, at and one above it in turn, so that some cells are under the measure on day 0 and some are not."""
    c = np.asarray(case["events"])[:, -w:, 2].astype(np.int64).sum(axis=-1)
    return np.maximum(c + np.arange(len(c)) % 3 - 1, 0)


def _rule(case, Hn, K=2):
    """A set whose rule fires in some cells and not in others: thresholds next to the recorded 7- and 3-day window sums, released at
    half of them, a minimum stay of 2 and 0 days, a review every day and every second day."""
    M = case["k"].M
    ls, cm, ls_on, cm_on = _pairs(K, M, Hn, seed=11)
    on = np.stack([_near(case, 7), _near(case, 3)])[:K]
    return ls, cm, _trig(K, M, on, on // 2, ls_on, cm_on, window=[7, 3][:K], min_days=[2, 0][:K], review_every=[1, 2][:K])


def _all(s, totals=False):
    cnt, by_day = _record(s)
    out = dict(_everything(s), active_count=cnt["active_count"], active_by_day=by_day)
    if totals:
        out["totals"] = s.read_scenario_group_draws()
    return out


def test_cuts_halves_resets_horizons_region_totals_and_another_set_after_a_triggered_one(api):  # noqa: F811
    case, u, ev, cfg, eps = _case("micro_20x60", 3)
    n, Hn, M = 11, 9, 20
    ls, cm, trig = _rule(case, Hn)
    groups = [list(range(M)), [0, 5, 19], list(range(7, 15))]
    model, s = _sampler(api, case, cfg, u, ev, eps, 2 * n)
    with model, s:
        s.set_groups(*_csr(groups))
        FG._reset(s, case, Hn)
        s.set_scenarios(ls, cm, 2 * n, triggers=trig)
        s.set_scenario_groups(True)
        for first in (0, n):
            s.reset_trace(at=first)
            s.run(n)
            s.forecast(first, n)
        halves = _all(s, True)
        frac = halves["active_count"].mean() / (2 * n)
        print("share of cell-days under the measure:", frac)
        assert 0.02 < frac < 0.98 and halves["diffs.sumsq"].any()
        assert np.array_equal(halves["totals"][:, :, :, 0], halves["draws.by_day"])          # the region totals read sev
        assert np.array_equal(halves["active_by_day"].sum(axis=(1, 3)), halves["active_count"].sum(axis=(2, 3)))
        for cuts in (((0, 2 * n),), ((0, 3), (3, 1), (4, 9), (13, 2 * n - 13))):
            FG._reset(s, case, Hn)                             # empties, keeps the triggered set
            assert s.scenario_state() == dict(K=2, H=Hn, cap=2 * n, j=0)
            assert not s.scenario_triggers()["active_count"].any() and s.read_scenario_trigger_draws().shape[1] == 0
            for first, count in cuts:
                s.forecast(first, count)
            _same(_all(s, True), halves)
        assert np.array_equal(s.read_scenario_trigger_draws(2, first=5), halves["active_by_day"][:, 5:7])
        with pytest.raises(_lib.SeirError, match="outside the 22 draws"):
            s.read_scenario_trigger_draws(2, first=21)
        # a targeted set after a triggered one, and a global one: the record is refused; and back
        FG._reset(s, case, Hn)
        s.set_scenarios(ls, cm, 2 * n)
        s.forecast(0, 2 * n)
        local = _everything(s)
        with pytest.raises(_lib.SeirError, match="no triggers"):
            s.read_scenario_trigger_draws()
        FG._reset(s, case, Hn)
        s.set_scenarios(ls, cm, 2 * n, triggers=dict(trig, on=np.full((2, M), NEVER, np.int32)))
        s.forecast(0, 2 * n)
        _same(_everything(s), local)
        FG._reset(s, case, Hn)
        s.set_scenarios(ls[:, 0], cm[:, 0], 2 * n)
        s.forecast(0, 2 * n)
        with pytest.raises(_lib.SeirError, match="no triggers"):
            s.scenario_triggers()
        FG._reset(s, case, Hn)
        s.set_scenarios(ls, cm, 2 * n, triggers=trig)
        s.forecast(0, 2 * n)
        _same(_all(s, True), halves)
        # another horizon frees the set
        FG._reset(s, case, Hn + 1)
        assert s.scenario_state()["K"] == 0
        with pytest.raises(_lib.SeirError, match="no scenarios are set"):
            s.scenario_triggers()
        assert not s.pair_timeouts().any()


def test_two_host_batches_workgroup_skew_and_the_same_run_twice(api):  # noqa: F811
    case, u, ev, cfg, eps = _case("micro_5x24", 2)
    n, Hn, M = 130, 5, 5
    ls, cm, trig = _rule(case, Hn)
    res = {}
    for tag, skew in (("a", 0), ("b", 0), (1, 1), (2, 2), (3, 3)):
        model, s = _sampler(api, case, cfg, u, ev, 0.002, n, skew=skew)
        with model, s:
            FG._reset(s, case, Hn)
            s.set_scenarios(ls, cm, n, triggers=trig)
            tr = s.sample(n, forecast=True)
            res[tag] = dict(_all(s), events=np.array(tr.events))
    frac = res["a"]["active_count"].mean() / n
    print("share of cell-days under the measure:", frac)
    assert 0.0 < frac < 1.0
    for tag in ("b", 1, 2, 3):
        _same(res[tag], res["a"])


def test_chain_sharding_and_thinning(api):  # noqa: F811
    case, u, ev, cfg, eps = _case("micro_20x60", 4)
    n, Hn, M = 5, 8, 20
    ls, cm, trig = _rule(case, Hn)

    def run(uu, evv, cap, **kw):
        model, s = _sampler(api, case, cfg, uu, evv, eps, cap, **kw)
        with model, s:
            FG._reset(s, case, Hn)
            s.set_scenarios(ls, cm, n, triggers=trig)
            tr = s.sample(n, forecast=True)
            return _all(s), np.array(tr.events)
    four, ev4 = run(u, ev, n)
    two, ev2 = run(u[2:], ev[2:], n, first_chain_id=2)
    assert np.array_equal(ev4[:, 2:], ev2) and four["active_count"].any()
    assert np.array_equal(four["active_count"][:, 2:], two["active_count"])
    assert np.array_equal(four["active_by_day"][:, :, 2:], two["active_by_day"])
    assert np.array_equal(four["draws.by_day"][:, :, 2:], two["draws.by_day"])
    k = 3
    kept, evk = run(u, ev, n, thin=k)
    model, s = _sampler(api, case, cfg, u, ev, eps, n * k)
    with model, s:
        every = s.sample(n * k)
        assert np.array_equal(every.events[k - 1::k], evk)
        FG._reset(s, case, Hn)
        s.set_scenarios(ls, cm, n, triggers=trig)
        for i in range(n):
            s.forecast(k - 1 + i * k, 1)
        _same(_all(s), kept)


def test_a_burst_run_again_after_a_time_out_is_counted_once_in_both_outputs(api):  # noqa: F811
    """tests/test_forecast_gpu.py's disturbance (the existing hook, once) with test 5's decoupled set: the re-run burst's counts
    and curves are those of its own draws, counted once."""
    case, u, ev, cfg, eps = _case("micro_20x60", 8)
    B, nb, burst, Hn, M, w = 8, 6, 4, 5, 20, 7
    on = _near(case, w)
    zero = np.zeros((1, M, Hn))
    model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
    with model, s:
        FG._reset(s, case, Hn)
        s.set_scenarios(zero, zero, nb * burst, triggers=_trig(1, M, on[None], 0, zero + np.log(0.5), zero, window=w, review_every=Hn))
        got = {}

        def consume(tr, i):
            got[i] = (tr.events.copy(), tr.theta.copy())
            if i == 1 and not s.recoveries:
                _lib.check(s._lib.seir_sampler_debug_fail_handoff(s._s, B - 1))
        s.sample_bursts(nb, burst, consume, forecast=True)
        assert len(s.recoveries) == 1 and sorted(got) == list(range(nb))
        theta, events = np.concatenate([got[i][1] for i in range(nb)]), np.concatenate([got[i][0] for i in range(nb)])
        base, st0 = _sims(model, case, theta, events, Hn)
        inside, _ = _sims(model, case, theta, events, Hn, _global(Hn, np.full(Hn, np.log(0.5)), np.zeros(Hn)), 0)
        outside, _ = _sims(model, case, theta, events, Hn, _global(Hn, np.zeros(Hn), np.zeros(Hn)), 0)
        mask = events[..., -w:, 2].astype(np.int64).sum(axis=-1) >= on
        assert mask.any() and not mask.all()
        _against(s, base, st0, [np.where(mask[..., None, None], inside, outside)])
        cnt, by_day = _record(s)
        assert cnt["count"] == nb * burst
        assert np.array_equal(cnt["active_count"][0], np.repeat(mask.sum(axis=0)[..., None], Hn, axis=-1))
        assert np.array_equal(by_day[0], np.repeat(mask.sum(axis=2)[..., None], Hn, axis=-1))


def test_refusals(api, monkeypatch):  # noqa: F811
    case, u, ev, cfg, eps = _case("micro_20x60", 2)
    n, Hn, M = 4, 6, 20
    ls, cm, trig = _rule(case, Hn)
    model, s = _sampler(api, case, cfg, u, ev, eps, n)

    def refused(code, word, *a, **kw):
        with pytest.raises(_lib.SeirError) as e:
            s.set_scenarios(*a, **kw)
        assert e.value.code == code and word in str(e.value), str(e.value)
        return str(e.value)

    def but(key, idx, v):
        x = np.array(trig[key])
        x[idx] = v
        return dict(trig, **{key: x})

    with model, s:
        refused(_lib.ERR_STATE, "seir_sampler_forecast_reset", ls, cm, n, triggers=trig)
        FG._reset(s, case, Hn)
        with pytest.raises(ValueError, match="as \\[K"):
            s.set_scenarios(ls[:, 0], cm[:, 0], n, triggers=trig)
        with pytest.raises(ValueError, match="need two of"):
            s.set_scenarios(ls, cm, n, triggers=dict(trig, commute_on=trig["commute_on"][:, :5]))
        with pytest.raises(ValueError, match="triggers\\['on'\\]"):
            s.set_scenarios(ls, cm, n, triggers=dict(trig, on=trig["on"][:, :5]))
        refused(_lib.ERR_INVALID, "log_shift_on[1][7][2] is not finite", ls, cm, n, triggers=but("log_shift_on", (1, 7, 2), np.nan))
        refused(_lib.ERR_INVALID, "commute_on[0][19][5]=", ls, cm, n, triggers=but("commute_on", (0, 19, 5), -0.5))
        x = ls.copy()
        x[1, 7, 2] = np.inf
        refused(_lib.ERR_INVALID, "log_shift[1][7][2] is not finite", x, cm, n, triggers=trig)
        refused(_lib.ERR_INVALID, "on[1][3]=", ls, cm, n, triggers=but("off", (1, 3), int(trig["on"][1, 3]) + 1))   # off > on
        refused(_lib.ERR_INVALID, "on[0][2]=", ls, cm, n, triggers=but("off", (0, 2), -1))
        for key, i, bad in (("window", 0, 0), ("window", 0, 29), ("from_day", 1, -1), ("from_day", 1, Hn + 1), ("min_days", 2, -1),
                            ("review_every", 3, 0)):
            refused(_lib.ERR_INVALID, f"params[1][{i}]={bad}", ls, cm, n, triggers=but(key, 1, bad))
        refused(_lib.ERR_INVALID, "K=5", np.zeros((5, M, Hn)), np.ones((5, M, Hn)), n,
                triggers=_trig(5, M, 1, 0, np.zeros((5, M, Hn)), np.ones((5, M, Hn))))
        assert s.scenario_state()["K"] == 0
        # above half of the free memory: the forecast runs on without scenarios
        monkeypatch.setenv("SEIR_DEBUG_FREE_BYTES", "1")
        msg = refused(_lib.ERR_INVALID, "the scenarios need", ls, cm, n, triggers=trig)
        need = int(msg.split("the scenarios need ")[1].split(" bytes")[0])
        msg = refused(_lib.ERR_INVALID, "the scenarios need", ls, cm, n)
        plain = int(msg.split("the scenarios need ")[1].split(" bytes")[0])
        print("bytes of the triggered set", need, "of the targeted set", plain)
        assert need > plain
        monkeypatch.setenv("SEIR_DEBUG_FREE_BYTES", str(2 * need - 2))
        refused(_lib.ERR_INVALID, "the scenarios need", ls, cm, n, triggers=trig)
        s.set_scenarios(ls, cm, n)                              # the targeted set fits where the triggered one does not
        monkeypatch.setenv("SEIR_DEBUG_FREE_BYTES", "1")
        refused(_lib.ERR_INVALID, "the scenarios need", ls, cm, n, triggers=trig)
        assert s.scenario_state()["K"] == 0
        monkeypatch.delenv("SEIR_DEBUG_FREE_BYTES")
        tr = s.sample(n, forecast=True)
        assert tr.forecast is not None and s.scenario_state()["K"] == 0
        refused(_lib.ERR_STATE, "first seir_sampler_forecast", ls, cm, n, triggers=trig)
        FG._reset(s, case, Hn)
        s.set_scenarios(ls, cm, n, triggers=trig)
        s.forecast(0, n)
        assert s.scenario_triggers()["count"] == n
        with pytest.raises(_lib.SeirError, match="outside the 4 draws"):
            s.read_scenario_trigger_draws(2, first=3)
        s.set_scenarios(np.zeros((0, M, Hn)), np.ones((0, M, Hn)), 0)
        assert s.scenario_state() == dict(K=0, H=0, cap=0, j=0)


def test_no_other_product_notices_the_triggered_set(api):  # noqa: F811
    """Every product on at once -- summaries, the forecast with its draw store, quantiles, group sums, the scenarios' region totals
    and the truth it is scored against, R_t, the check, within / between, both group curves: the run with a triggered set whose
    rule fires in some cells against the run with a targeted set -- every field of every burst's trace and every accumulator that
    is not the scenarios' own bit for bit; and with a rule that never fires the scenarios' own too."""
    from covid19uk_amd.posterior import groups as G
    from covid19uk_amd.posterior import predict
    from covid19uk_amd.sampler import Trace
    from tests.test_scenarios_gpu import _flat, inf_steps
    case, u, ev, cfg, eps = _case("micro_20x60", 3)
    B, nb, burst, Hn, K, D = 3, 3, 4, 6, 5, 4
    cov, T, M = case["cov"], case["k"].T, case["k"].M
    N = np.asarray(cov.N, np.float64).reshape(-1)
    tab = G.parse_groups({"all": list(range(M)), "low": list(range(0, M, 2)), "one": [M - 1]}, M)
    ls, cm, trig = _rule(case, Hn)
    truth = np.random.default_rng(9).integers(0, 6, size=(M, Hn)).astype(np.int32)
    truth[3, 2:] = -1
    kw = dict(summarize=True, forecast=inf_steps(7, list(range(B)), Hn), rt=True, check=True, within_between=True, groups=True)
    fields = tuple(f for f in Trace.__dataclass_fields__ if f not in ("hmc", "moves"))
    runs = {}
    for tag, triggers in (("targeted", None), ("never", dict(trig, on=np.full((2, M), NEVER, np.int32))), ("fires", trig)):
        model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
        with model, s:
            s.set_groups(tab.offsets, tab.members)
            s.set_group_rt(G.rt_weights(tab, N))
            s.set_group_within_between(True)
            s.reset_forecast(Hn, *predict.forecast_calendar(cov, None, T, Hn), 5)
            s.keep_forecast_draws(nb * burst)
            s.set_scenarios(ls, cm, nb * burst, **({} if triggers is None else dict(triggers=triggers)))
            s.set_scenario_groups(True)
            s.set_verify(truth)
            s.reset_check(K, *predict.check_calendar(cov, None, T, K), 6)
            s.reset_rt(D, N / N.sum())
            s.reset_within_between(D)
            got = {}

            def consume(tr, i, got=got):
                got[i] = {f: ({k: np.array(a) for k, a in getattr(tr, f).items()} if isinstance(getattr(tr, f), dict)
                              else np.array(getattr(tr, f))) for f in fields if getattr(tr, f) is not None}
            s.sample_bursts(nb, burst, consume, **kw)
            runs[tag] = (got, _flat(dict(summary=s.summary(), forecast=s.forecast_summary(), rt=s.rt_summary(),
                                         check=s.check_summary(), wb=s.within_between_summary(),
                                         q=dict(q=s.forecast_quantiles([0.05, 0.5, 0.95], pooled=True)), verify=s.verify_summary(),
                                         pairs=dict(own=s.forecast_pair_sums(), pooled=s.forecast_pair_sums(pooled=True)))),
                         s.get_state(), dict(_everything(s), totals=s.read_scenario_group_draws()),
                         None if triggers is None else _record(s))
    a = runs["targeted"]
    for tag in ("never", "fires"):
        b = runs[tag]
        for i in range(nb):
            assert set(a[0][i]) == set(b[0][i]) >= {"theta", "events", "marginals", "forecast", "rt", "check", "wb", "groups", "group_curves"}
            for f in a[0][i]:
                for k, v in _flat({f: a[0][i][f]}).items():
                    assert np.array_equal(v, _flat({f: b[0][i][f]})[k], equal_nan=True), (tag, i, k)
        assert set(a[1]) == set(b[1]) and a[1]["verify.abs_sum"].any() and a[1]["pairs.own"].any()
        for k in a[1]:
            assert np.array_equal(a[1][k], b[1][k], equal_nan=True), (tag, k)
        for x, y in zip(a[2], b[2]):
            assert np.array_equal(x, y)
    _same(runs["never"][3], a[3])
    assert not runs["never"][4][1].any() and runs["fires"][4][1].any()
    assert any(not np.array_equal(runs["fires"][3][k], a[3][k]) for k in a[3])
    assert np.array_equal(runs["fires"][3]["totals"][:, :, :, 0], runs["fires"][3]["draws.by_day"])


# ---------------------------------------------------------------------------------------------------------------------
# 10. the size users run
# ---------------------------------------------------------------------------------------------------------------------
def test_uk380_with_a_seven_day_rule_per_100k(api):  # noqa: F811
    """UK-380 x 8 chains x 12 draws x H = 14, K = 2: scenario 0 never fires (identity 1), scenario 1 has a 7-day per-100k rule
    whose on pair is its off pair (identity 4)."""
    case, u, ev, cfg, eps = _case("uk380", 8)
    n, Hn, M, B, w = 12, 14, case["k"].M, 8, 7
    N = np.asarray(case["cov"].N, np.float64).reshape(-1)
    rng = np.random.default_rng(380)
    gl, gc = rng.normal(0.0, 0.2, size=(2, Hn)), rng.uniform(0.5, 1.5, size=(2, Hn))
    ls, cm = _over_rows(gl, M), _over_rows(gc, M)
    model, s = _sampler(api, case, cfg, u, ev, eps, n, record_events="u16")
    with model, s:
        FG._reset(s, case, Hn)
        s.set_scenarios(ls, cm, n)
        tr = s.sample(n, forecast=True)
        local = _everything(s)
        hist = np.asarray(tr.events)[..., 2].astype(np.int64)
        sim = _sims(model, case, tr.theta, tr.events, Hn, SC.Scenarios(("a", "b"), Hn, gl, gc), 1)[0]
        rate = float(np.median(_window_sums(hist, sim[..., 2], w).max(axis=-1) / N * 1e5))
        on = np.array([[NEVER] * M, SC.threshold_counts(rate, N)], np.int64)
        off = np.array([[0] * M, SC.threshold_counts(rate / 2, N)], np.int64)
        FG._reset(s, case, Hn)
        s.set_scenarios(ls, cm, n, triggers=_trig(2, M, on, off, ls, cm, window=w, min_days=3, review_every=[1, 7]))
        s.forecast(0, n)
        _same(_everything(s), local)
        cnt, by_day = _record(s)
        act = SC.trigger_states(hist, sim[..., 2], on[1], off[1], w, 0, 3, 7)
        print("rate per 100k:", rate, "cell-days under the measure:", int(act.sum()), "of", act.size)
        assert not cnt["active_count"][0].any() and not by_day[0].any()
        assert np.array_equal(cnt["active_count"][1], act.sum(axis=0)) and np.array_equal(by_day[1], act.sum(axis=2))
        assert act.any() and not act.all()


# ---------------------------------------------------------------------------------------------------------------------
# 11. both command lines
# ---------------------------------------------------------------------------------------------------------------------
def test_the_command_lines_with_a_triggered_scenario(api, tmp_path):  # noqa: F811
    """The inference command line on NI-11 (its locations carrying codes of three nations), two chains, with --forecast 14
    --forecast-quantiles --scenarios FILE, FILE holding one global scenario and one with a per-100k trigger on the E0* locations, and
    the replay command line on its two files with the same flags: every scenarios/* and samples/scenario_* dataset equal, the
    record consistent with itself and with the rule's thresholds."""
    import os

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
    N = np.asarray(cov.N, np.float64).reshape(-1)
    rate = float(np.median(events[:, -7:, 2].sum(axis=1) / N * 1e5))               # about half of the locations start above it
    spec = {"fifth_down": {"transmission": 0.8, "from_day": 7},
            "tier": {"trigger": {"cases_per_100k": rate, "release_per_100k": rate / 2, "window": 7, "min_days": 3, "review_every": 2,
                                 "locations": ["E0*", 8]},
                     "then": {"transmission": 0.5, "commute": 0.5}}}
    path = os.path.join(tmp, "tier.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(spec, f, sort_keys=False)
    flags = ["--forecast", "14", "--forecast-quantiles", "0.05,0.95", "--scenarios", path]
    out = os.path.join(tmp, "live.h5")
    log = _run("covid19uk_amd.inference.inference", ["-c", cfg, "-o", out, "--seed", "4", "--chains", "2", data] + flags, tmp)
    assert "Scenario tier: the measure triggers somewhere in" in log and "Scenario fifth_down: the measure" not in log
    files = [inf.chain_file_name(out, c, 2) for c in range(2)]
    rout = os.path.join(tmp, "replay.h5")
    rlog = _run("covid19uk.posterior.replay", ["-c", cfg, "-o", rout, "--seed", "4", data] + files + flags, tmp)
    assert "Scenario tier: the measure triggers somewhere in" in rlog
    n, M, Hn = 12, 11, 14
    may = [0, 1, 2, 3, 4, 8]
    for c in range(2):
        live, rep = _datasets(files[c]), _datasets(inf.chain_file_name(rout, c, 2))
        new = {k for k in live if k.startswith("scenarios/") or k.startswith("samples/scenario_")}
        assert {"scenarios/trigger_on", "scenarios/trigger_off", "scenarios/trigger_window", "scenarios/trigger_from_day",
                "scenarios/trigger_min_days", "scenarios/trigger_review_every", "scenarios/log_shift_on_by_location",
                "scenarios/commute_on_by_location", "scenarios/active_count", "scenarios/p_active", "samples/scenario_active_by_day",
                "scenarios/active_by_day_quantiles"} <= new
        for k in sorted(new):
            assert live[k].dtype == rep[k].dtype and live[k].shape == rep[k].shape and live[k].tobytes() == rep[k].tobytes(), k
        on = live["scenarios/trigger_on"]
        assert on.shape == (2, M) and np.all(on[0] == NEVER) and np.all(on[1, [5, 6, 7, 9, 10]] == NEVER)
        assert on[1, may].tolist() == [SC.threshold_counts(rate, N)[m] for m in may]
        assert live["scenarios/trigger_off"][1, may].tolist() == [SC.threshold_counts(rate / 2, N)[m] for m in may]
        assert live["scenarios/trigger_review_every"].tolist() == [1, 2] and live["scenarios/trigger_min_days"].tolist() == [0, 3]
        cnt, by = live["scenarios/active_count"], live["samples/scenario_active_by_day"]
        assert cnt.shape == (2, M, Hn) and by.shape == (n, 2, Hn)
        assert not cnt[0].any() and not cnt[1][[5, 6, 7, 9, 10]].any() and cnt[1].any() and cnt.max() <= n
        assert np.array_equal(cnt.sum(axis=1), by.sum(axis=0)) and by.max() <= len(may)
        assert np.array_equal(live["scenarios/p_active"], cnt / n)
        assert live["scenarios/active_by_day_quantiles"].shape == (2, 2, Hn)
        # the scenario without a trigger is the scenario it is in a file without one: the first day under the measure bounds nothing of it
        assert live["samples/scenario_by_day"].shape == (n, 2, Hn, 3)

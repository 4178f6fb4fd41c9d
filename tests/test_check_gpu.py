"""In-sample predictive check on the device (include/seir_hip.h, "In-sample predictive check on the device";
covid19uk_amd/csrc/check_kernels.h): for every kept draw the last K observed days are simulated again from the state the
draw's recorded events leave at day T - K, folded into moments and per-draw marginals, and counted against the observed
removals, which are the I->R plane of the draw itself.

The oracle uses the same run's recorded draws: `tr.theta` and `tr.events` are read back, the state at day T - K is formed
by NumPy integer sums, the log baseline by `predict.log_baseline_path(..., T - K, K)`, the calendar by
`predict.prediction_calendar`, and `SeirModel.simulate` is called per chain with `first_draw_id = chain << 20` -- the stated
equivalence.  The six quantities, moments and marginals are formed as tests/test_forecast_gpu.py forms them; lt / eq and the
totals are NumPy comparisons with `tr.events[..., T - K:, 2]`.  Two micro cases also go through `oracle/sim_oracle.simulate`,
which does not share the device's binomial code.  Every comparison of device results is `np.array_equal` on integers."""
import os

import numpy as np
import pytest

from covid19uk_amd import _lib, synth
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.posterior import predict
from covid19uk_amd.sampler import forecast_draw_id, mid_p, summary_mean, summary_var
from oracle import sim_oracle
from tests import helpers as H
from tests import test_forecast_gpu as FG
from tests.test_forecast_gpu import _fold, _quantities, _same_moments
from tests.test_recovery_gpu import _case, _same_bits
from tests.test_sampler_gpu import CFG_REF, CFG_SMALL, api  # noqa: F401  (fixture)
from tests.test_summary_gpu import _cli, _datasets, _sampler

pytestmark = pytest.mark.gpu

CK = ("check_by_day", "check_by_location", "check_state_by_day")
COUNTS = ("observed", "lt", "eq", "location_lt", "location_eq", "day_lt", "day_eq", "total_lt", "total_eq")
SEED = 91


def _calendar(case, K):
    return predict.check_calendar(case["cov"], None, case["k"].T, K)


def _reset(s, case, K, seed=SEED):
    W, wd = _calendar(case, K)
    s.reset_check(K, W, wd, seed)


def _state_at(init, events, t0):
    """init [M,4], events [n,M,T,3] integer -> [n,M,4] int64: S0 + stoichiometry . sum_{t < t0} events."""
    tot = events[:, :, :t0].astype(np.int64).sum(axis=2)
    i0 = np.asarray(init).astype(np.int64)
    assert np.array_equal(i0, init)
    return np.stack([i0[:, 0] - tot[..., 0], i0[:, 1] + tot[..., 0] - tot[..., 1], i0[:, 2] + tot[..., 1] - tot[..., 2],
                     i0[:, 3] + tot[..., 2]], axis=-1)


def _oracle(model, case, theta, events, K, seed=SEED, chain0=0, j0=0, folds=None, simulate=None):
    """theta [n,B,P], events [n,B,M,T,3] of one run -> the check's moments and counts (over the draws `folds`) and
    marginals (of all draws)."""
    n, B = theta.shape[:2]
    T = case["k"].T
    t0 = T - K
    cov = case["cov"]
    W, wd = predict.prediction_calendar(cov.W, cov.weekday, t0, K)
    out = dict(count=np.zeros(B, np.uint64), ref=[], sum=[], sumsq=[], sim=[], **{k: [] for k in CK + COUNTS})
    for b in range(B):
        th = theta[:, b]
        a_path = predict.log_baseline_path(th[:, 5], th[:, 6:6 + T - 1], t0, K)
        st0 = _state_at(case["init"], events[:, b], t0)
        kw = dict(seed=seed, first_draw_id=forecast_draw_id(chain0 + b, j0))
        sim = (model.simulate if simulate is None else simulate)(th[:, :5], a_path, th[:, 6 + T - 1:], W, wd,
                                                                 st0.astype(np.float64), **kw)
        assert np.array_equal(sim, np.rint(sim))
        sim = sim.astype(np.int64)
        x = _quantities(sim, st0)
        out["sim"].append(sim)
        out["check_by_day"].append(x[..., :3].sum(axis=1))
        out["check_by_location"].append(x[..., :3].sum(axis=2))
        out["check_state_by_day"].append(x[..., 3:].sum(axis=1))
        sel = slice(None) if folds is None else folds
        f = x[sel]
        out["count"][b] = len(f)
        _fold(f, out)
        obs = events[:, b, :, t0:, 2].astype(np.int64)[sel]      # [n,M,K]: every draw's own recorded removals
        assert np.array_equal(obs, np.broadcast_to(obs[:1], obs.shape)), "the data moved between draws"
        y = sim[sel][..., 2]
        out["observed"].append(obs[0].astype(np.int32))
        for name, a, o in (("", y, obs), ("location_", y.sum(axis=2), obs.sum(axis=2)), ("day_", y.sum(axis=1), obs.sum(axis=1)),
                           ("total_", y.sum(axis=(1, 2)), obs.sum(axis=(1, 2)))):
            out[name + "lt"].append((a < o).sum(axis=0).astype(np.uint32))
            out[name + "eq"].append((a == o).sum(axis=0).astype(np.uint32))
    for k in ("ref", "sum", "sumsq") + COUNTS:
        out[k] = np.stack(out[k])
    for k in CK + ("sim",):
        out[k] = np.stack(out[k], axis=1)
    return out


def _same_counts(cs, want):
    assert cs.observed.dtype == np.int32
    for k in COUNTS:
        got = getattr(cs, k)
        assert k == "observed" or got.dtype == np.uint32, k
        assert got.shape == want[k].shape and np.array_equal(got, want[k]), k


def _same_marginals(m, want, rows=slice(None)):
    for k in CK:
        assert m[k].dtype == np.int64
        assert np.array_equal(m[k], want[k][rows]), k


def _same_summary(cs, want):
    _same_moments(cs.moments, want)
    _same_counts(cs, want)


def _same_check(a, b):
    """(CheckSummary, marginals) twice."""
    for k in ("count", "ref", "sum", "sumsq"):
        assert np.array_equal(getattr(a[0].moments, k), getattr(b[0].moments, k)), k
    for k in COUNTS:
        assert np.array_equal(getattr(a[0], k), getattr(b[0], k)), k
    for k in CK:
        assert np.array_equal(a[1][k], b[1][k]), k


def _all_three_occur(cs):
    """Non-vacuity: per cell, draws below, at and above the data each occur somewhere."""
    n = cs.count[:, None, None].astype(np.int64)
    lt, eq = cs.lt.astype(np.int64), cs.eq.astype(np.int64)
    gt = n - lt - eq
    assert gt.min() >= 0
    assert lt.any() and eq.any() and gt.any(), (int(lt.sum()), int(eq.sum()), int(gt.sum()))


# the case ids name the branch they turn: where the window starts (the prepare's lane-strided row sums over t' < T - K),
# the window's length (the compare's two 64-day chunks, the fold's carry) and ND = draws x B against the 64-draw tile
CASES = {
    # name, cfg, eps, B, record, n, K
    "M=1,K=7": ("micro_1x70", CFG_SMALL, 0.002, 3, "u16", 6, 7),
    "T=1,K=1,no_alpha_t,start=0": ("micro_3x1", CFG_SMALL, 0.002, 2, True, 4, 1),
    "T=64,K=1,ND=15": ("micro_9x64", CFG_SMALL, 0.0004, 3, "u16", 5, 1),
    "T=64,K=64=T,start=0": ("micro_9x64", CFG_SMALL, 0.0004, 3, True, 5, 64),
    "T=65,K=64,start=1,ND=64": ("micro_7x65", CFG_SMALL, 0.0004, 8, True, 8, 64),
    # K = 1 leaves 7 cells a chain: removals of some hundreds a day have a standard deviation near 17, a simulated count hits
    # the observed one about once in 40 draws, so 8 chains x 16 draws (896 cell comparisons) for "equal" to occur (2 chains x
    # 4 draws, 56 comparisons, gave 36 below, none equal, 20 above)
    "T=65,K=1,start=64,ND=128": ("micro_7x65", CFG_SMALL, 0.0004, 8, "u16", 16, 1),
    "T=65,K=2,start=63": ("micro_7x65", CFG_SMALL, 0.0004, 2, True, 4, 2),
    "M=65,K=65,ND=65": ("micro_65x70", CFG_SMALL, 0.0001, 1, "u16", 65, 65),
    "T=70,K=5,start=65": ("micro_65x70", CFG_SMALL, 0.0001, 2, True, 3, 5),
    "M=520,K=7": ("slow_520x70", CFG_SMALL, 3e-5, 2, True, 6, 7),
    "T=800,K=128,ND=72": ("slower_4x800", CFG_REF, 3e-5, 8, True, 9, 128),
    "T=800,u16,K=7": ("slower_4x800", CFG_REF, 3e-5, 1, "u16", 8, 7),
    "uk380x8,12,K=14": ("uk380", CFG_REF, 1.2e-5, 8, "u16", 12, 14),
}


@pytest.mark.parametrize("case_id", list(CASES))
def test_check_equals_simulate_and_numpy_on_the_recorded_draws(api, case_id):
    name, cfg, eps, B, record, n, K = CASES[case_id]
    case = H.build_case(name, 43, alpha_t_sd=0.005)
    M, T = case["k"].M, case["k"].T
    u = synth.jitter_params(case["u"], B, scale=0.002 if name == "uk380" else 0.01, seed=3, T=T)
    ev = np.stack([case["events"]] * B)
    model, s = _sampler(api, case, cfg, u, ev, eps, n, record_events=record)
    with model, s:
        _reset(s, case, K)
        tr = s.sample(n, check=True)
        cs = s.check_summary()
        assert tr.events.dtype == (np.uint16 if record == "u16" else np.int32)
        assert cs.moments.ref.shape == (B, M, K, 6) and tr.check["check_by_day"].shape == (n, B, K, 3)
        assert tr.check["check_by_location"].shape == (n, B, M, 3)
        want = _oracle(model, case, tr.theta, tr.events, K)
        # the data: the case's own removals, whatever the chain did to the other two planes
        assert np.array_equal(cs.observed, np.broadcast_to(case["events"][:, T - K:, 2].astype(np.int32), (B, M, K)))
        _same_marginals(tr.check, want)
        _same_summary(cs, want)
        if M > 1 and T > 1:
            _all_three_occur(cs)
        # the mid-p values are what the counts give
        assert np.array_equal(cs.pit, mid_p(cs.count, cs.lt, cs.eq)) and np.all((cs.total_pit >= 0) & (cs.total_pit <= 1))
        # a second reset starts j at 0 again: the last slot alone becomes obs / ref and is draw 0 of every chain
        _reset(s, case, K)
        s.check(n - 1, 1)
        one = _oracle(model, case, tr.theta[n - 1:], tr.events[n - 1:], K)
        _same_summary(s.check_summary(), one)
        _same_marginals(s.read_check_marginals(1, first=n - 1), one)
        assert not s.pair_timeouts().any()


@pytest.mark.parametrize("name,K", [("micro_9x64", 3), ("micro_3x1", 1)])
def test_check_equals_the_independent_cpu_simulator(api, name, K):
    """oracle/sim_oracle.simulate shares the Philox protocol and nothing of the device's binomial code."""
    case, u, ev, cfg, eps = _case(name, 2)
    n = 3
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        _reset(s, case, K)
        tr = s.sample(n, check=True)
        want = _oracle(model, case, tr.theta, tr.events, K,
                       simulate=lambda *a, **kw: sim_oracle.simulate(H.oracle_constants(case["cov"], case["init"]), *a, **kw))
        assert want["sim"].any()
        _same_marginals(tr.check, want)
        _same_summary(s.check_summary(), want)


def test_cutting_a_burst_into_calls_halves_or_batches_does_not_matter(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    n, K = 11, 9
    model, s = _sampler(api, case, cfg, u, ev, eps, 2 * n)
    with model, s:
        _reset(s, case, K)
        for first in (0, n):                                   # two bursts in the two halves of the buffer
            s.reset_trace(at=first)
            s.run(n)
            s.check(first, n)
        tr = s.read_trace(2 * n)
        halves = (s.check_summary(), s.read_check_marginals(2 * n))
        want = _oracle(model, case, tr.theta, tr.events, K)
        _all_three_occur(halves[0])
        _same_summary(halves[0], want)
        _same_marginals(halves[1], want)
        _reset(s, case, K)
        s.check(0, 2 * n)                                      # one call over everything
        _same_check((s.check_summary(), s.read_check_marginals(2 * n)), halves)
        _reset(s, case, K)
        for first, count in ((0, 3), (3, 1), (4, 9), (13, 2 * n - 13)):
            s.check(first, count)
        _same_check((s.check_summary(), s.read_check_marginals(2 * n)), halves)


def test_a_call_longer_than_one_host_batch_holds(api):
    """More slots than one batch of the host's cut (128): the same integers as in calls of 50, and as the oracle's."""
    case, u, ev, cfg, eps = _case("micro_5x24", 2)
    n, K = 150, 3
    model, s = _sampler(api, case, cfg, u, ev, 0.002, n)
    with model, s:
        _reset(s, case, K)
        tr = s.sample(n, check=True)
        whole = (s.check_summary(), tr.check)
        want = _oracle(model, case, tr.theta, tr.events, K)
        assert want["sim"].any() and whole[0].moments.sumsq.any()
        _same_summary(whole[0], want)
        _same_marginals(whole[1], want)
        _reset(s, case, K)
        for first in range(0, n, 50):
            s.check(first, 50)
        _same_check((s.check_summary(), s.read_check_marginals(n)), whole)


@pytest.mark.parametrize("skew", [1, 2, 3])
def test_checks_do_not_depend_on_workgroup_timing_and_repeat(api, skew):
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    n, K = 6, 10
    res = {}
    for tag, sk in (("a", 0), ("b", 0), ("skew", skew)):
        if tag == "b" and skew != 1:
            continue                                           # the repeat of the plain run is checked once
        model, s = _sampler(api, case, cfg, u, ev, eps, n, skew=sk, record_events="u16")
        with model, s:
            _reset(s, case, K)
            tr = s.sample(n, check=True)
            res[tag] = (s.check_summary(), tr.check, tr)
    assert res["a"][0].moments.sumsq.any()
    for tag in res:
        assert np.array_equal(res["a"][2].events, res[tag][2].events)
        _same_check(res[tag], res["a"])


def test_chains_keep_their_checks_however_they_are_sharded(api):
    """Chains 2 and 3 of a 4-chain sampler against a 2-chain sampler created with first_chain_id = 2."""
    case, u, ev, cfg, eps = _case("micro_20x60", 4)
    n, K = 5, 8
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        _reset(s, case, K)
        tr4 = s.sample(n, check=True)
        cs4 = s.check_summary()
    model, s = _sampler(api, case, cfg, u[2:], ev[2:], eps, n, first_chain_id=2)
    with model, s:
        _reset(s, case, K)
        tr2 = s.sample(n, check=True)
        cs2 = s.check_summary()
        _same_summary(cs2, _oracle(model, case, tr2.theta, tr2.events, K, chain0=2))
    assert np.array_equal(tr4.events[:, 2:], tr2.events) and cs2.moments.sumsq.any()
    for k in CK:
        assert np.array_equal(tr4.check[k][:, 2:], tr2.check[k]), k
    for k in ("count", "ref", "sum", "sumsq"):
        assert np.array_equal(getattr(cs4.moments, k)[2:], getattr(cs2.moments, k)), k
    for k in COUNTS:
        assert np.array_equal(getattr(cs4, k)[2:], getattr(cs2, k)), k


def test_with_thinning_the_checks_are_those_of_the_kept_draws(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 4)
    n, K, k = 6, 5, 3
    model, s = _sampler(api, case, cfg, u, ev, eps, n, thin=k)
    with model, s:
        _reset(s, case, K)
        kept = s.sample(n, check=True)
        cs = s.check_summary()
    model, s = _sampler(api, case, cfg, u, ev, eps, n * k)
    with model, s:
        every = s.sample(n * k)
        assert np.array_equal(every.events[k - 1::k], kept.events)
        want = _oracle(model, case, every.theta[k - 1::k], every.events[k - 1::k], K)
    _same_summary(cs, want)
    _same_marginals(kept.check, want)


def _copy_burst(tr):
    return (tr.theta.copy(), tr.events.copy(), {k: v.copy() for k, v in tr.hmc.items()},
            {mk: {kk: v.copy() for kk, v in mv.items()} for mk, mv in tr.moves.items()},
            {k: v.copy() for k, v in tr.marginals.items()}, {k: v.copy() for k, v in tr.forecast.items()}, tr.rt.copy(),
            None if tr.check is None else {k: v.copy() for k, v in tr.check.items()})


def test_chain_summaries_forecast_and_rt_do_not_notice_the_check_and_share_nothing_with_it(api):
    """Overlapped bursts with summaries, forecast and R_t, once with the check behind them and once without: traces, final
    state and kernel, and the three other products bit for bit.  The forecast has the check's window length here, so
    that a shared staging tensor or a shared draw counter would show; a check alone gives the same check."""
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    nb, burst, K = 4, 5, 6
    N = np.asarray(case["cov"].N, np.float64).reshape(-1)
    runs = {}
    for ck in (False, True):
        model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
        with model, s:
            got = {}
            FG._reset(s, case, K)
            s.reset_rt(K, N / N.sum())
            if ck:
                _reset(s, case, K)
            s.sample_bursts(nb, burst, lambda tr, i, got=got: got.__setitem__(i, _copy_burst(tr)), summarize=True, forecast=True,
                            rt=True, **(dict(check=True) if ck else {}))
            fs, rs = s.forecast_summary(), s.rt_summary()
            runs[ck] = (got, s.get_state() + s.get_kernel(), s.summary(), fs, rs, s.check_summary() if ck else None)
            if ck:
                theta = np.concatenate([got[i][0] for i in range(nb)])
                events = np.concatenate([got[i][1] for i in range(nb)])
                want = _oracle(model, case, theta, events, K)
                _all_three_occur(runs[ck][5])
                _same_summary(runs[ck][5], want)
                marg = {k: np.concatenate([got[i][7][k] for i in range(nb)]) for k in CK}
                _same_marginals(marg, want)
                # the forecast of the same run is the forecast's own oracle: neither took the other's staging or counter
                fwant = FG._oracle(model, case, theta, events, K)
                _same_moments(fs, fwant)
                # ... and they are two different products
                assert any((marg[k] != np.concatenate([got[i][5]["forecast" + k[5:]] for i in range(nb)])).any() for k in CK)
    from types import SimpleNamespace
    for i in range(nb):
        a, b = (SimpleNamespace(theta=x[0], events=x[1], hmc=x[2], moves=x[3]) for x in (runs[False][0][i], runs[True][0][i]))
        _same_bits(a, b)
        assert runs[False][0][i][7] is None
        for j in (4, 5):
            for k in runs[False][0][i][j]:
                assert np.array_equal(runs[False][0][i][j][k], runs[True][0][i][j][k]), k
        assert np.array_equal(runs[False][0][i][6], runs[True][0][i][6])
    for x, y in zip(runs[False][1], runs[True][1]):
        assert np.array_equal(x, y)
    for j in (2, 3):
        for k in ("count", "ref", "sum", "sumsq"):
            assert np.array_equal(getattr(runs[False][j], k), getattr(runs[True][j], k)), k
    for k in ("count", "ref", "sum", "sumsq", "gt1"):
        assert np.array_equal(getattr(runs[False][4], k), getattr(runs[True][4], k)), k


def test_forecast_and_check_together_each_equal_their_solo_result(api):
    """Both on one sampler, with the same key on purpose and the same length (they differ in start day, baseline and
    calendar): each gives what it gives alone.  The check is moved on by two draws in between, so that a counter shared
    with the forecast, or a staging tensor used by both at once, would show."""
    case, u, ev, cfg, eps = _case("micro_20x60", 3)
    n, K = 7, 12
    res = {}
    for tag, kw in (("both", dict(forecast=True, check=True)), ("fc", dict(forecast=True)), ("ck", dict(check=True))):
        model, s = _sampler(api, case, cfg, u, ev, eps, n)
        with model, s:
            if "forecast" in kw:
                FG._reset(s, case, K, seed=SEED)
            if "check" in kw:
                _reset(s, case, K, seed=SEED)
            s.sample(3, **kw)
            if "check" in kw:
                s.check(0, 2)                                  # the check's counter alone runs ahead: j = 5, the forecast's 3
            tr = s.sample(n, **kw)
            res[tag] = (tr, (s.forecast_summary(), tr.forecast) if "forecast" in kw else None,
                        (s.check_summary(), tr.check) if "check" in kw else None)
            if tag == "both":
                _same_marginals(tr.check, _oracle(model, case, tr.theta, tr.events, K, j0=5))
                FG._same_marginals(tr.forecast, FG._oracle(model, case, tr.theta, tr.events, K, seed=SEED, j0=3))
    assert np.array_equal(res["both"][0].events, res["ck"][0].events) and np.array_equal(res["both"][0].events, res["fc"][0].events)
    _same_check(res["both"][2], res["ck"][2])
    FG._same_forecast(res["both"][1], res["fc"][1])
    assert res["both"][2][0].moments.sumsq.any() and res["both"][1][0].sumsq.any()
    assert np.array_equal(res["both"][2][0].count, [3 + 2 + n] * 3) and np.array_equal(res["both"][1][0].count, [3 + n] * 3)


def test_a_burst_run_again_after_a_time_out_is_checked_and_counted_once(api):
    """seir_sampler_debug_fail_handoff (the existing test hook, once) in the middle of overlapped bursts that are checked:
    the burst is restored -- accumulators, counts, obs and the draw counter included -- and run again one launch form down."""
    case, u, ev, cfg, eps = _case("micro_20x60", 8)
    B, nb, burst, K = 8, 6, 4, 5
    runs = {}
    for disturb in (False, True):
        model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
        with model, s:
            got = {}
            _reset(s, case, K)

            def consume(tr, i, got=got, s=s, disturb=disturb):
                got[i] = (tr.events.copy(), {k: v.copy() for k, v in tr.check.items()}, tr.theta.copy())
                if disturb and i == 1 and not s.recoveries:    # while burst 2 or 3 is in flight
                    _lib.check(s._lib.seir_sampler_debug_fail_handoff(s._s, B - 1))
            s.sample_bursts(nb, burst, consume, check=True)
            runs[disturb] = (got, s.check_summary(), list(s.recoveries))
            if not disturb:
                want = _oracle(model, case, np.concatenate([got[i][2] for i in range(nb)]),
                               np.concatenate([got[i][0] for i in range(nb)]), K)
    ref, got = runs[False], runs[True]
    assert not ref[2] and len(got[2]) == 1, got[2]
    assert sorted(got[0]) == list(range(nb))
    for i in range(nb):
        assert np.array_equal(ref[0][i][0], got[0][i][0]), i
    _same_summary(ref[1], want)
    assert np.array_equal(got[1].count, np.full(B, nb * burst))
    # theta of the re-run bursts agrees to the order of summation only (another launch form), so the disturbed run is
    # held to its own draws: counted once, and checked with the draw numbers it would have had undisturbed
    with api[0](case["cov"], case["init"], max_chains=B) as model:
        want2 = _oracle(model, case, np.concatenate([got[0][i][2] for i in range(nb)]),
                        np.concatenate([got[0][i][0] for i in range(nb)]), K)
    _same_summary(got[1], want2)
    _same_marginals({k: np.concatenate([got[0][i][1][k] for i in range(nb)]) for k in CK}, want2)


def test_data_that_move_between_draws_raise_the_flag_and_the_read_fails_with_its_message(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 2)
    n, K = 3, 6
    T = case["k"].T
    ir = case["events"][:, T - K:T - 1, 2]
    m, t = np.argwhere(ir > 0)[0]
    moved = ev.copy()                                          # one removal a day later: the state stays valid
    moved[:, m, T - K + t, 2] -= 1
    moved[:, m, T - K + t + 1, 2] += 1
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        _reset(s, case, K)
        s.sample(n, check=True)
        assert np.array_equal(s.check_summary().count, [n, n])
        s.set_state(u, moved)
        s.sample(n, check=True)                                # no reset in between: obs is still the first data's
        with pytest.raises(_lib.SeirError, match="observed removals moved") as e:
            s.check_summary()
        assert e.value.code == _lib.ERR_STATE
        with pytest.raises(_lib.SeirError, match="observed removals moved"):   # sticky
            s.check_summary()
        _reset(s, case, K)                                     # a reset takes the flag down: the moved data are the data now
        tr = s.sample(n, check=True)
        cs = s.check_summary()
        assert np.array_equal(cs.observed[0], moved[0, :, T - K:, 2])
        _same_summary(cs, _oracle(model, case, tr.theta, tr.events, K))


def test_a_reset_with_another_window_on_a_checking_sampler_starts_everything_again(api):
    """A reset with another K while the check is on: every buffer is sized again (K = 1, then K = T: window start 0), and a
    snapshot from before the reset no longer holds anything of the check -- restoring it leaves moments, comparison counts
    and the library's j alone."""
    case, u, ev, cfg, eps = _case("micro_20x60", 3)
    n, T = 5, case["k"].T
    assert T == 60
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        _reset(s, case, 12)
        tr = s.sample(n, check=True)
        cs = s.check_summary()
        want = _oracle(model, case, tr.theta, tr.events, 12)
        assert want["sim"].any() and cs.moments.sumsq.any()
        _same_summary(cs, want)
        _same_marginals(tr.check, want)
        s.snapshot(0)
        _reset(s, case, 1)
        s.check(0, n)
        want = _oracle(model, case, tr.theta, tr.events, 1)
        _same_summary(s.check_summary(), want)
        _same_marginals(s.read_check_marginals(n), want)
        s.restore(0)                                           # the snapshot predates the reset: the check is left alone
        cs = s.check_summary()
        assert np.array_equal(cs.count, [n] * 3)
        assert np.all(cs.lt.astype(np.int64) + cs.eq <= cs.count[:, None, None].astype(np.int64))
        _same_summary(cs, want)
        s.check(0, 1)                                          # the library's j is still n (the call passes none)
        one = _oracle(model, case, tr.theta[:1], tr.events[:1], 1, j0=n)
        _same_marginals(s.read_check_marginals(1), one)
        cs = s.check_summary()
        assert np.array_equal(cs.count, [n + 1] * 3)
        assert np.array_equal(cs.observed, want["observed"])
        for k in COUNTS[1:]:
            assert np.array_equal(getattr(cs, k), want[k] + one[k]), k
        _reset(s, case, T)                                     # larger: the whole series, window start 0
        s.check(0, n)
        want = _oracle(model, case, tr.theta, tr.events, T)
        _same_summary(s.check_summary(), want)
        _same_marginals(s.read_check_marginals(n), want)
        assert not s.pair_timeouts().any()


def test_refusals(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 2)
    T = case["k"].T
    assert T == 60
    W, wd = _calendar(case, 5)
    model, s = _sampler(api, case, cfg, u, ev, eps, 4, record_events=False)
    with model, s:
        for call in (lambda: s.reset_check(5, W, wd), lambda: s.check(0, 1), lambda: s.read_check_marginals(1),
                     lambda: s.check_summary()):
            with pytest.raises(_lib.SeirError) as e:
                call()
            assert e.value.code == _lib.ERR_STATE
    model, s = _sampler(api, case, cfg, u, ev, eps, 4)
    with model, s:
        for call in (lambda: s.check(0, 1), lambda: s.read_check_marginals(1), lambda: s.check_summary()):
            with pytest.raises(_lib.SeirError, match="seir_sampler_check_reset") as e:    # before a reset
                call()
            assert e.value.code == _lib.ERR_STATE
        one = np.zeros(130)
        for K in (0, T + 1, 129):                              # past the Python check too: the library refuses
            with pytest.raises(ValueError):
                s.reset_check(K, one[:K], one[:K])
            rc = s._lib.seir_sampler_check_reset(s._s, K, one.ctypes.data_as(_lib.c_double_p), one.ctypes.data_as(_lib.c_double_p), 0)
            assert rc == _lib.ERR_INVALID
        s.reset_check(5, W, wd)
        for first, count in ((-1, 1), (0, 5), (4, 1), (3, 2), (0, -1)):
            calls = [lambda: s.check(first, count)]
            if count >= 0:
                calls.append(lambda: s.read_check_marginals(count, first=first))
            for call in calls:
                with pytest.raises(_lib.SeirError) as e:
                    call()
                assert e.value.code == _lib.ERR_INVALID, (first, count)
        s.sample(4, check=True)                                # and the sampler is as usable as before
        assert np.array_equal(s.check_summary().count, [4, 4])
    model, s = _sampler(api, case, cfg, u, ev, eps, 4, first_chain_id=2047)     # chain ids 2047 and 2048
    with model, s:
        with pytest.raises(_lib.SeirError, match="chain id 2048") as e:
            s.reset_check(5, W, wd)
        assert e.value.code == _lib.ERR_INVALID


def test_m_above_the_simulators_limit_is_refused_with_its_message(api):
    case = H.build_case("micro_1281x2", 43)
    u = case["u"][None]
    model, s = _sampler(api, case, CFG_SMALL, u, case["events"][None], 1e-4, 2)
    with model, s:
        with pytest.raises(_lib.SeirError, match="M=1281 needs .* B of LDS for the simulator") as e:
            s.reset_check(2, np.ones(2), np.zeros(2))
        assert e.value.code == _lib.ERR_INVALID


# ---- CLI end to end -------------------------------------------------------------------------------------------------------
def test_cli_check(api, tmp_path):
    """`--check 7` on an NI-11 data set: the group and datasets with the right shapes, equal to the oracle from the file's
    own samples/seir and parameters; `--summaries only --thin 2 --forecast 7 --rt 7 --check 7` works without samples/seir;
    without the flag the file has exactly today's datasets."""
    tmp_path = str(tmp_path)
    cov = synth.make_covariates("ni11")
    events, init, _ = synth.simulate_epidemic(cov)
    data = os.path.join(tmp_path, "data.npz")
    inf.write_inference_data(data, cov, events[..., 2])
    ck_path, ck_log = _cli(tmp_path, "ck", data, ["--check", "7"])
    ck = _datasets(ck_path)
    allf = _datasets(_cli(tmp_path, "all", data, ["--summaries", "only", "--thin", "2", "--forecast", "7", "--rt", "7", "--check", "7"])[0])
    plain = _datasets(_cli(tmp_path, "plain", data, [])[0])
    new = {f"check/{k}" for k in ("days", "first_day", "count", "seir_mean", "seir_var", "state_mean", "state_var", "observed", "lt",
                                  "eq", "location_lt", "location_eq", "day_lt", "day_eq", "total_lt", "total_eq", "pit",
                                  "location_pit", "day_pit", "total_pit")} | {f"samples/{k}" for k in CK}
    assert set(ck) - set(plain) == new and set(plain) <= set(ck)
    for k in plain:
        if plain[k].dtype.kind in "fiub":
            assert np.array_equal(plain[k], ck[k], equal_nan=plain[k].dtype.kind == "f"), k
    assert "samples/seir" not in allf and new <= set(allf) and "rt/R_it_mean" in allf and "forecast/seir_mean" in allf
    assert "Check: last 7 day(s)" in ck_log
    M, T, K, ns = cov.M, cov.T, 7, 2 * 6
    cases = events[..., 2]
    for f in (ck, allf):                                       # whatever else is on: the data are the file's cases
        assert np.array_equal(f["check/observed"], cases[:, T - K:]) and f["check/count"].reshape(-1)[0] == ns
        assert f["check/days"].reshape(-1)[0] == K and f["check/first_day"].reshape(-1)[0] == T - K
        assert f["samples/check_by_day"].shape == (ns, K, 3) and f["samples/check_by_day"].dtype == np.int64
        assert f["samples/check_by_location"].shape == (ns, M, 3) and f["samples/check_state_by_day"].shape == (ns, K, 3)
        assert f["check/seir_mean"].shape == (M, K, 3) and f["check/pit"].shape == (M, K) and f["check/day_pit"].shape == (K,)
        assert np.all(f["check/lt"] + f["check/eq"] <= ns)
    # the oracle from the file's own draws: the sampling phase is the last ns rows
    cov2, _, dates = inf.read_inference_data(data)
    W, wd = predict.check_calendar(cov2, dates, T, K)
    seir = ck["samples/seir"][-ns:]
    assert np.array_equal(seir, np.rint(seir))
    seir = seir.astype(np.int64)
    theta = np.concatenate([ck[f"samples/{k}"][-ns:].reshape(ns, -1) for k in
                            ("psi", "sigma_space", "beta_area", "gamma0", "gamma1", "alpha_0", "alpha_t", "spatial_effect")], axis=1)
    init_f = ck["initial_state"]
    st0 = _state_at(init_f, seir, T - K)
    a_path = predict.log_baseline_path(theta[:, 5], theta[:, 6:6 + T - 1], T - K, K)
    with api[0](cov2, init_f, max_chains=1) as model:
        sim = model.simulate(theta[:, :5], a_path, theta[:, 6 + T - 1:], W, wd, st0.astype(np.float64), seed=inf.check_seed(0),
                             first_draw_id=0).astype(np.int64)
    assert sim.any()
    x = _quantities(sim, st0)
    assert np.array_equal(ck["samples/check_by_day"], x[..., :3].sum(axis=1))
    assert np.array_equal(ck["samples/check_by_location"], x[..., :3].sum(axis=2))
    assert np.array_equal(ck["samples/check_state_by_day"], x[..., 3:].sum(axis=1))
    d = x - x[:1]
    cnt = np.array(ns, np.uint64)
    mean = summary_mean(cnt, x[0], d.sum(axis=0))
    var = summary_var(cnt, d.sum(axis=0), (d * d).sum(axis=0))
    assert np.array_equal(ck["check/seir_mean"], mean[..., :3]) and np.array_equal(ck["check/state_mean"], mean[..., 3:])
    assert np.array_equal(ck["check/seir_var"], var[..., :3]) and np.array_equal(ck["check/state_var"], var[..., 3:])
    y, obs = sim[..., 2], seir[:, :, T - K:, 2]
    for name, a, o in (("", y, obs), ("location_", y.sum(axis=2), obs.sum(axis=2)), ("day_", y.sum(axis=1), obs.sum(axis=1)),
                       ("total_", y.sum(axis=(1, 2)), obs.sum(axis=(1, 2)))):
        lt, eq = (a < o).sum(axis=0), (a == o).sum(axis=0)
        assert np.array_equal(ck[f"check/{name}lt"].reshape(lt.shape), lt), name
        assert np.array_equal(ck[f"check/{name}eq"].reshape(eq.shape), eq), name
        pit = "pit" if name == "" else name + "pit"
        assert np.array_equal(ck[f"check/{pit}"].reshape(lt.shape), mid_p(cnt, lt, eq)), name

"""Reproduction number on the device (include/seir_hip.h, "Reproduction number on the device";
covid19uk_amd/csrc/rt_trace_kernels.h): for every kept draw R_it over the window [T - D, T) is formed from the burst buffer
where it lies, folded into per-chain moments and summed into the national curve of the draw.

The reference for every equality is the same run's recorded draws: `tr.theta` and `tr.events` are read back and put
through the stateless `SeirModel.reproduction_number` (k_rt) of a context of their own, then folded by a NumPy loop in draw
order -- separately rounded operations, as the device's.  ref, sum, sumsq, gt1 and count are held to `np.array_equal`.
R_t per draw is held to rtol = 1e-12 against (R_it * weight).sum(-1): all terms are non-negative and M <= 2048, so any
summation order is within about 2 M 2^-53 < 5e-13 of any other.  Two micro cases also go through
`oracle/rt_oracle.posterior_rit(stable=True)`, which shares nothing with the device's arithmetic."""
import os

import numpy as np
import pytest

from covid19uk_amd import _lib, synth
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.posterior import predict
from oracle import rt_oracle as ro
from tests import helpers as H
from tests.test_recovery_gpu import _case, _same_bits
from tests.test_sampler_gpu import CFG_REF, CFG_SMALL, api  # noqa: F401  (fixture)
from tests.test_summary_gpu import _cli, _datasets, _sampler

pytestmark = pytest.mark.gpu

RT_DT = 4                     # k_rt_trace's day tile (rt_trace_kernels.h)


def _weight(case):
    N = np.asarray(case["cov"].N, dtype=np.float64).reshape(-1)
    return N / N.sum()                                         # reproduction_number.py:82-83


def _reference(api, case, theta, events, D):
    """theta [n,B,P], events [n,B,M,T,3] of one run -> R_it [n,B,D,M] over the window, by the stateless kernel."""
    n, B = theta.shape[:2]
    T = case["k"].T
    with api[0](case["cov"], case["init"], max_chains=min(n * B, 16)) as model:
        R = model.reproduction_number(theta.reshape(n * B, -1), events.reshape((n * B,) + events.shape[2:]).astype(np.float64))
    return R.reshape(n, B, T, -1)[:, :, T - D:]


def _fold(R):
    """R [n,B,D,M] -> the accumulators, by the loop the header states: d = r - ref; sum = sum + d; sumsq = sumsq + d * d."""
    ref = R[0].copy()
    sm, sq = np.zeros_like(ref), np.zeros_like(ref)
    for r in R:
        d = r - ref
        sm = sm + d
        sq = sq + d * d
    return dict(count=np.full(R.shape[1], len(R), np.uint64), ref=ref, sum=sm, sumsq=sq,
                gt1=(R > 1.0).sum(axis=0).astype(np.uint32))


def _same_acc(rs, want):
    assert rs.count.dtype == np.uint64 and rs.gt1.dtype == np.uint32
    assert rs.ref.dtype == rs.sum.dtype == rs.sumsq.dtype == np.float64
    for k in ("count", "ref", "sum", "sumsq", "gt1"):
        assert np.array_equal(getattr(rs, k), want[k]), k


def _same_rt(got, R, w):
    np.testing.assert_allclose(got, (R * w).sum(-1), rtol=1e-12, atol=0.0)


def _same_run(a, b):
    """(RtSummary, R_t) of two runs: every bit."""
    for k in ("count", "ref", "sum", "sumsq", "gt1"):
        assert np.array_equal(getattr(a[0], k), getattr(b[0], k)), k
    assert np.array_equal(a[1], b[1])


# the case ids name the branch they turn: column blocks of 64 (M), the day tile of 4 and the prefix over [0, T - D) (D),
# the a_t quirks (T), chains, trace width, one draw and a full burst (n = the buffer's capacity)
CASES = {
    # name, cfg, eps, B, record, n, D
    "M=1,D=tile+1": ("micro_1x70", CFG_SMALL, 0.002, 3, "u16", 6, RT_DT + 1),
    "M=9,T=64,D=tile": ("micro_9x64", CFG_SMALL, 0.0004, 3, "u16", 5, RT_DT),
    "M=65,second_partial_column_block,D=tile-1": ("micro_65x70", CFG_SMALL, 0.0001, 1, "u16", 3, RT_DT - 1),
    "M=520,Mp>512,T=20,D=5": ("slow_520x20", CFG_SMALL, 3e-5, 1, True, 3, 5),
    "T=1,D=1,alpha_0_day": ("micro_3x1", CFG_SMALL, 0.002, 2, True, 4, 1),
    "T=2,D=T,clip_at_T-1": ("micro_2x2", CFG_SMALL, 0.002, 1, True, 4, 2),
    "T=65,D=T,8_chains,full_burst": ("micro_7x65", CFG_SMALL, 0.0004, 8, True, 8, 65),
    "T=70,D=1,one_draw": ("micro_20x70", CFG_SMALL, 0.0004, 3, "u16", 1, 1),
    "T=70,D=66,prefix_of_4": ("micro_20x70", CFG_SMALL, 0.0004, 3, True, 4, 66),
    "uk380x8,12,D=14": ("uk380", CFG_REF, 1.2e-5, 8, "u16", 12, 14),
}


@pytest.mark.parametrize("case_id", list(CASES))
def test_rt_equals_the_stateless_kernel_on_the_recorded_draws(api, case_id):
    name, cfg, eps, B, record, n, D = CASES[case_id]
    case = H.build_case(name, 43, alpha_t_sd=0.005)
    u = synth.jitter_params(case["u"], B, scale=0.002 if name == "uk380" else 0.01, seed=3, T=case["k"].T)
    ev = np.stack([case["events"]] * B)
    w = _weight(case)
    model, s = _sampler(api, case, cfg, u, ev, eps, n, record_events=record)
    with model, s:
        s.reset_rt(D, w)
        tr = s.sample(n, rt=True)
        rs = s.rt_summary()
        assert tr.events.dtype == (np.uint16 if record == "u16" else np.int32)
        assert rs.ref.shape == (B, D, case["k"].M) and tr.rt.shape == (n, B, D)
        R = _reference(api, case, tr.theta, tr.events, D)
        assert np.all(np.isfinite(R)) and R.min() >= 0.0
        _same_acc(rs, _fold(R))
        _same_rt(tr.rt, R, w)
        if n > 1:
            assert rs.sumsq.any(), "every draw has the same R_it"
        # a second reset: the last slot alone becomes ref, with nothing left of the first fold
        s.reset_rt(D, w)
        s.rt(n - 1, 1)
        _same_acc(s.rt_summary(), _fold(R[n - 1:]))
        _same_rt(s.read_rt_draws(1, first=n - 1), R[n - 1:], w)
        # ... and another window allocates again
        D2 = 1 if D > 1 else case["k"].T
        s.reset_rt(D2, w)
        s.rt(0, n)
        R2 = R[:, :, D - D2:] if D2 <= D else _reference(api, case, tr.theta, tr.events, D2)
        _same_acc(s.rt_summary(), _fold(R2))
        _same_rt(s.read_rt_draws(n), R2, w)
        assert not s.pair_timeouts().any()


@pytest.mark.parametrize("name,D", [("micro_3x5", 5), ("ni11", 7)])
def test_the_mean_equals_the_independent_cpu_oracle(api, name, D):
    """oracle/rt_oracle.posterior_rit(stable=True) on the recorded draws, with tests/test_rt.py's normalised error.  The
    project's pinned per-draw bound is 1e-11; a mean of values that each meet it meets it too, and the fold's rounding at
    n <= 1000 is far below that: 2e-11."""
    case, u, ev, cfg, eps = _case(name, 2)
    n = 4
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        s.reset_rt(D, _weight(case))
        tr = s.sample(n, rt=True)
        rs = s.rt_summary()
    T = case["k"].T
    for b in range(2):
        want, want_t = ro.posterior_rit(tr.theta[:, b], tr.events[:, b].astype(np.float64), case["k"], stable=True)
        want, want_t = want[:, T - D:], want_t[:, T - D:]
        mean = want.mean(axis=0)
        err = np.max(np.abs(rs.mean[b] - mean) / np.maximum(np.abs(mean), 1e-12 * np.abs(mean).max()))
        print(f"{name} chain {b}: normalised error of the mean {err:.3e}")
        assert err < 2e-11, err
        np.testing.assert_allclose(tr.rt[:, b], want_t, rtol=1e-10)


def test_gt1_equals_the_count_from_the_cpu_oracle(api):
    """micro_20x60, seed 43, every day: chosen on the CPU with the oracle alone -- at the starting point about four fifths of
    the cells lie above one and none within 1e-4 of it.  The conditions are checked again on the recorded draws, and then no
    cell is exempted."""
    case, u, ev, cfg, eps = _case("micro_20x60", 3)
    n, D = 5, 60
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        s.reset_rt(D, _weight(case))
        tr = s.sample(n, rt=True)
        rs = s.rt_summary()
    for b in range(3):
        want, _ = ro.posterior_rit(tr.theta[:, b], tr.events[:, b].astype(np.float64), case["k"], stable=True)
        above = want > 1.0
        assert np.abs(want - 1.0).min() > 1e-9
        assert above.mean() >= 0.1 and (~above).mean() >= 0.1
        assert np.array_equal(rs.gt1[b], above.sum(axis=0))
        assert np.array_equal(rs.prob_gt1[b], above.sum(axis=0) / float(n))


def test_cutting_a_burst_into_calls_halves_or_batches_does_not_matter(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    n, D = 11, 9
    w = _weight(case)
    model, s = _sampler(api, case, cfg, u, ev, eps, 2 * n)
    with model, s:
        s.reset_rt(D, w)
        for first in (0, n):                                   # two bursts in the two halves of the buffer
            s.reset_trace(at=first)
            s.run(n)
            s.rt(first, n)
        tr = s.read_trace(2 * n)
        halves = (s.rt_summary(), s.read_rt_draws(2 * n))
        R = _reference(api, case, tr.theta, tr.events, D)
        _same_acc(halves[0], _fold(R))
        _same_rt(halves[1], R, w)
        s.reset_rt(D, w)
        s.rt(0, 2 * n)                                         # one call over everything
        _same_run((s.rt_summary(), s.read_rt_draws(2 * n)), halves)
        s.reset_rt(D, w)
        for first, count in ((0, 3), (3, 1), (4, 9), (13, 2 * n - 13)):
            s.rt(first, count)
        _same_run((s.rt_summary(), s.read_rt_draws(2 * n)), halves)
        # the host's own cut: a staging bound of 64 KiB holds 64 KiB / (5 chains x 64 rows x 9 days x 4 B) = 5 slots,
        # so the 22 slots go as batches of 5, 5, 5, 5 and 2 (the bound is read when the window changes)
        model.set_option(rt_staging_kib=64)
        s.reset_rt(D + 1, w)
        s.reset_rt(D, w)
        s.rt(0, 2 * n)
        _same_run((s.rt_summary(), s.read_rt_draws(2 * n)), halves)
        model.set_option(rt_staging_kib=1)                     # less than one slot: one slot per batch
        s.reset_rt(D + 1, w)
        s.reset_rt(D, w)
        s.rt(0, 2 * n)
        _same_run((s.rt_summary(), s.read_rt_draws(2 * n)), halves)


@pytest.mark.parametrize("skew", [1, 2, 3])
def test_results_do_not_depend_on_workgroup_timing_and_repeat(api, skew):
    case, u, ev, cfg, eps = _case("micro_65x70", 2)
    n, D = 4, 6
    res = {}
    for tag, sk in (("a", 0), ("b", 0), ("skew", skew)):
        if tag == "b" and skew != 1:
            continue                                           # the repeat of the plain run is checked once
        model, s = _sampler(api, case, cfg, u, ev, 0.0001, n, skew=sk, record_events="u16")
        with model, s:
            s.reset_rt(D, _weight(case))
            tr = s.sample(n, rt=True)
            res[tag] = (s.rt_summary(), tr.rt, tr)
    assert res["a"][0].sumsq.any()
    for tag in res:
        assert np.array_equal(res["a"][2].events, res[tag][2].events)
        _same_run(res[tag], res["a"])


def test_chains_keep_their_numbers_however_they_are_sharded(api):
    """Chains 2 and 3 of a 4-chain sampler against a 2-chain sampler created with first_chain_id = 2."""
    case, u, ev, cfg, eps = _case("micro_20x60", 4)
    n, D = 5, 8
    w = _weight(case)
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        s.reset_rt(D, w)
        tr4 = s.sample(n, rt=True)
        rs4 = s.rt_summary()
    model, s = _sampler(api, case, cfg, u[2:], ev[2:], eps, n, first_chain_id=2)
    with model, s:
        s.reset_rt(D, w)
        tr2 = s.sample(n, rt=True)
        rs2 = s.rt_summary()
    assert np.array_equal(tr4.events[:, 2:], tr2.events) and np.array_equal(tr4.theta[:, 2:], tr2.theta)
    assert rs2.sumsq.any()
    assert np.array_equal(tr4.rt[:, 2:], tr2.rt)
    for k in ("count", "ref", "sum", "sumsq", "gt1"):
        assert np.array_equal(getattr(rs4, k)[2:], getattr(rs2, k)), k


def test_with_thinning_the_numbers_are_those_of_the_kept_draws(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 4)
    n, D, k = 6, 5, 3
    w = _weight(case)
    model, s = _sampler(api, case, cfg, u, ev, eps, n, thin=k)
    with model, s:
        s.reset_rt(D, w)
        kept = s.sample(n, rt=True)
        rs = s.rt_summary()
    model, s = _sampler(api, case, cfg, u, ev, eps, n * k)
    with model, s:
        every = s.sample(n * k)
    assert np.array_equal(every.events[k - 1::k], kept.events)
    R = _reference(api, case, every.theta[k - 1::k], every.events[k - 1::k], D)
    _same_acc(rs, _fold(R))
    _same_rt(kept.rt, R, w)


def test_the_chain_its_summaries_and_its_forecast_do_not_notice(api):
    """A sampler that forms R_it behind every burst's summary and forecast against one that never does: traces, marginals,
    forecast, moments, final state and kernel bit for bit."""
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    nb, burst, Hn, D = 4, 5, 6, 7
    w = _weight(case)
    W, wd = predict.forecast_calendar(case["cov"], None, case["k"].T, Hn)
    runs = {}
    for rt in (False, True):
        model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
        with model, s:
            got = {}
            s.reset_forecast(Hn, W, wd, 77)
            if rt:
                s.reset_rt(D, w)

            def consume(tr, i, got=got):
                got[i] = (tr.theta.copy(), tr.events.copy(), {k: v.copy() for k, v in tr.hmc.items()},
                          {mk: {kk: v.copy() for kk, v in mv.items()} for mk, mv in tr.moves.items()},
                          {k: v.copy() for k, v in tr.marginals.items()}, {k: v.copy() for k, v in tr.forecast.items()},
                          None if tr.rt is None else tr.rt.copy())
            s.sample_bursts(nb, burst, consume, summarize=True, forecast=True, **(dict(rt=True) if rt else {}))
            runs[rt] = (got, s.get_state() + s.get_kernel(), s.summary(), s.forecast_summary(), s.rt_summary() if rt else None)
    from types import SimpleNamespace
    for i in range(nb):
        a, b = (SimpleNamespace(theta=x[0], events=x[1], hmc=x[2], moves=x[3]) for x in (runs[False][0][i], runs[True][0][i]))
        _same_bits(a, b)
        assert runs[False][0][i][6] is None
        for part in (4, 5):
            for k in runs[False][0][i][part]:
                assert np.array_equal(runs[False][0][i][part][k], runs[True][0][i][part][k]), k
    for x, y in zip(runs[False][1], runs[True][1]):
        assert np.array_equal(x, y)
    for which in (2, 3):
        for k in ("count", "ref", "sum", "sumsq"):
            assert np.array_equal(getattr(runs[False][which], k), getattr(runs[True][which], k)), k
    got = runs[True][0]
    R = _reference(api, case, np.concatenate([got[i][0] for i in range(nb)]), np.concatenate([got[i][1] for i in range(nb)]), D)
    _same_acc(runs[True][4], _fold(R))
    _same_rt(np.concatenate([got[i][6] for i in range(nb)]), R, w)      # through the asynchronous reader


def test_a_burst_run_again_after_a_time_out_is_counted_once(api):
    """seir_sampler_debug_fail_handoff (the existing test hook, once) in the middle of overlapped bursts: the burst is
    restored -- the accumulators and count included -- and run again one launch form down."""
    case, u, ev, cfg, eps = _case("micro_20x60", 8)
    B, nb, burst, D = 8, 6, 4, 5
    w = _weight(case)
    model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
    with model, s:
        got = {}
        s.reset_rt(D, w)

        def consume(tr, i):
            got[i] = (tr.events.copy(), tr.rt.copy(), tr.theta.copy())
            if i == 1 and not s.recoveries:                    # while burst 2 or 3 is in flight
                _lib.check(s._lib.seir_sampler_debug_fail_handoff(s._s, B - 1))
        s.sample_bursts(nb, burst, consume, rt=True)
        rs, recoveries = s.rt_summary(), list(s.recoveries)
    assert len(recoveries) == 1, recoveries
    assert sorted(got) == list(range(nb))
    # the run is held to its own draws: every delivered draw folded once, in order
    R = _reference(api, case, np.concatenate([got[i][2] for i in range(nb)]), np.concatenate([got[i][0] for i in range(nb)]), D)
    _same_acc(rs, _fold(R))
    _same_rt(np.concatenate([got[i][1] for i in range(nb)]), R, w)


def test_refusals(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 2)
    w = _weight(case)
    T = case["k"].T
    wp = w.ctypes.data_as(_lib.c_double_p)
    model, s = _sampler(api, case, cfg, u, ev, eps, 4, record_events=False)
    with model, s:
        for call in (lambda: s.reset_rt(3, w), lambda: s.rt(0, 1), lambda: s.read_rt_draws(1), lambda: s.rt_summary()):
            with pytest.raises(_lib.SeirError, match="record_events=0") as e:
                call()
            assert e.value.code == _lib.ERR_INVALID
    model, s = _sampler(api, case, cfg, u, ev, eps, 4)
    with model, s:
        for call in (lambda: s.rt(0, 1), lambda: s.read_rt_draws(1), lambda: s.rt_summary()):
            with pytest.raises(_lib.SeirError, match="seir_sampler_rt_reset") as e:         # before a reset
                call()
            assert e.value.code == _lib.ERR_STATE
        for D in (0, T + 1, -1):
            with pytest.raises(ValueError):
                s.reset_rt(D, w)
            assert s._lib.seir_sampler_rt_reset(s._s, D, wp) == _lib.ERR_INVALID
        assert s._lib.seir_sampler_rt_reset(s._s, 3, None) == _lib.ERR_INVALID             # null weight
        with pytest.raises(ValueError):
            s.reset_rt(3, w[:-1])
        s.reset_rt(3, w)
        for first, count in ((-1, 1), (0, 5), (4, 1), (3, 2), (0, -1)):
            calls = [lambda: s.rt(first, count)]
            if count >= 0:
                calls.append(lambda: s.read_rt_draws(count, first=first))
            for call in calls:
                with pytest.raises(_lib.SeirError) as e:
                    call()
                assert e.value.code == _lib.ERR_INVALID, (first, count)
        tr = s.sample(4, rt=True)                              # and the sampler is as usable as before
        assert np.array_equal(s.rt_summary().count, [4, 4]) and tr.rt.shape == (4, 2, 3)


# ---- CLI end to end -------------------------------------------------------------------------------------------------------
PLAIN = {"initial_state", "time"} | {f"samples/{k}" for k in ("psi", "sigma_space", "beta_area", "gamma0", "gamma1", "alpha_0",
                                                                  "alpha_t", "spatial_effect", "seir")} | \
    {f"results/hmc/{k}" for k in ("is_accepted", "target_log_prob", "step_size")} | \
    {f"results/{m}/{k}" for m in inf.MOVE_KEYS for k in ("is_accepted", "target_log_prob", "proposed_delta")}


def test_cli_rt(api, tmp_path):
    """`--rt 7` on an NI-11 data set: the group and samples/R_t, equal to the stateless kernel on the file's own draws;
    `--summaries only --thin 2 --forecast 7 --rt 7` works without samples/seir; without the flag the file has exactly the
    datasets of a run before the option existed."""
    from covid19uk_amd.sampler import rt_prob_gt1, summary_mean, summary_var
    tmp_path = str(tmp_path)
    cov = synth.make_covariates("ni11")
    events, init, _ = synth.simulate_epidemic(cov)
    data = os.path.join(tmp_path, "data.npz")
    inf.write_inference_data(data, cov, events[..., 2])
    rt_path, rt_log = _cli(tmp_path, "rt", data, ["--rt", "7"])
    rt = _datasets(rt_path)
    both = _datasets(_cli(tmp_path, "both", data, ["--summaries", "only", "--thin", "2", "--forecast", "7", "--rt", "7"])[0])
    plain_path, plain_log = _cli(tmp_path, "plain", data, [])
    plain = _datasets(plain_path)
    new = {"rt/days", "rt/first_day", "rt/count", "rt/R_it_mean", "rt/R_it_var", "rt/R_it_prob_gt1", "samples/R_t"}
    assert set(plain) == PLAIN and "R_t" not in plain_log
    assert set(rt) == PLAIN | new
    for k in plain:
        if plain[k].dtype.kind in "fiub":
            assert np.array_equal(plain[k], rt[k], equal_nan=plain[k].dtype.kind == "f"), k
    M, T, D, ns = cov.M, cov.T, 7, 2 * 6
    assert "samples/seir" not in both and new <= set(both) and "forecast/count" in both and "summaries/count" in both
    for f in (rt, both):
        assert f["samples/R_t"].shape == (ns, D) and f["samples/R_t"].dtype == np.float64
        assert f["rt/days"].reshape(-1)[0] == D and f["rt/first_day"].reshape(-1)[0] == T - D
        assert f["rt/count"].reshape(-1)[0] == ns
        for k in ("R_it_mean", "R_it_var", "R_it_prob_gt1"):
            assert f[f"rt/{k}"].shape == (D, M) and np.all(np.isfinite(f[f"rt/{k}"]))
        assert np.all(f["samples/R_t"] > 0.0)
    assert rt_log.count("R_t:") == 1 and f"window of {D} day(s) from day {T - D}" in rt_log
    # the reference from the file's own draws: the sampling phase is the last ns rows
    cov2, _, _ = inf.read_inference_data(data)
    seir = rt["samples/seir"][-ns:]
    theta = np.concatenate([rt[f"samples/{k}"][-ns:].reshape(ns, -1) for k in
                            ("psi", "sigma_space", "beta_area", "gamma0", "gamma1", "alpha_0", "alpha_t", "spatial_effect")], axis=1)
    with api[0](cov2, rt["initial_state"], max_chains=ns) as model:
        R = model.reproduction_number(theta, seir)[:, T - D:]
    N = np.asarray(cov2.N, dtype=np.float64).reshape(-1)
    np.testing.assert_allclose(rt["samples/R_t"], (R * (N / N.sum())).sum(-1), rtol=1e-12, atol=0.0)
    want = _fold(R[:, None])
    cnt = np.array(ns, np.uint64)
    assert np.array_equal(rt["rt/R_it_mean"], summary_mean(cnt, want["ref"][0], want["sum"][0]))
    assert np.array_equal(rt["rt/R_it_var"], summary_var(cnt, want["sum"][0], want["sumsq"][0]))
    assert np.array_equal(rt["rt/R_it_prob_gt1"], rt_prob_gt1(cnt, want["gt1"][0]))

"""R_t intervals on the device (include/seir_hip.h, "R_t intervals on the device"): k_rt_trace_keep
(covid19uk_amd/csrc/rt_keep_kernels.h) runs in place of k_rt_trace and leaves every draw's R_it in the store
keepR[B][D][M][cap]; k_order_stats_f64 (order_stats_kernels.h) selects exact order statistics from it.

The selection alone is held, bit for bit (`.view(np.uint64)`), to Python's sorted() under the total-order key of
tests/test_rt_quantiles_host.py through `SeirModel.order_stats_f64`, on values no model produces.  The store plus the
selection is held, bit for bit, to np.sort over the draws of the stateless `SeirModel.reproduction_number` (k_rt) on the same
run's recorded draws, as tests/test_rt_device_gpu.py holds the fold.  The quantiles are held to np.quantile of those draws at
rtol 1e-12, the tolerance of `posterior.quantiles.interpolate`: the order statistics themselves are exact."""
import os

import numpy as np
import pytest

from covid19uk_amd import _lib, synth
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.posterior import predict
from tests import helpers as H
from tests.test_forecast_quantiles_gpu import _ranks
from tests.test_recovery_gpu import _case, _same_bits
from tests.test_rt_device_gpu import CASES, PLAIN, _fold, _reference, _same_acc, _same_rt, _same_run, _weight
from tests.test_rt_quantiles_host import total_order_sorted, value_families
from tests.test_sampler_gpu import api  # noqa: F401  (fixture)
from tests.test_summary_gpu import _cli, _datasets, _sampler

pytestmark = pytest.mark.gpu

RUN = 4                       # RT_KEEP_RUN: the draws k_rt_trace_keep stages per cell (rt_keep_kernels.h)
GAP = np.array([0x7FF8DEADBEEF0001], np.uint64).view(np.float64)[0]      # a NaN that would show if a gap were read


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


# ---- 1. the selection alone ------------------------------------------------------------------------------------------------
def _lay_out(cells_values, segs, seg_len, pad):
    """cells_values [cells][segs * seg_len] -> the flat array with seg_stride = seg_len + pad, the gaps filled with GAP."""
    cells = len(cells_values)
    seg_stride = seg_len + pad
    cell_stride = segs * seg_stride + 3
    flat = np.full(cells * cell_stride, GAP, np.float64)
    for c, vals in enumerate(cells_values):
        v = np.asarray(vals, np.float64).reshape(segs, seg_len)
        for g in range(segs):
            flat[c * cell_stride + g * seg_stride:c * cell_stride + g * seg_stride + seg_len] = v[g]
    return flat, seg_stride, cell_stride


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 5000])
def test_order_stats_f64_equal_the_total_order_on_every_array_family(api, n):
    """n values per segment, 1 / 3 / 8 segments: totals on both sides of the one-wave / four-wave launch forms."""
    case = H.build_case("micro_3x1", 43)
    with api[0](case["cov"], case["init"], max_chains=1) as model:
        for segs in (1, 3, 8):
            total = segs * n
            for name, (xs, as_numpy) in value_families(total, seed=segs).items():
                flat, ss, cs = _lay_out([xs], segs, n, pad=5)
                want = total_order_sorted(xs)
                if as_numpy:
                    assert np.array_equal(_bits(want), _bits(np.sort(xs))), name
                r16 = _ranks(total)
                got = model.order_stats_f64(flat, r16, cells=1, segs=segs, seg_len=n, seg_stride=ss, cell_stride=cs)
                assert got.dtype == np.float64 and got.shape == (len(r16), 1)
                assert 0 in r16 and total - 1 in r16
                assert np.array_equal(_bits(got[:, 0]), _bits(want[r16])), (name, segs)
                for r1 in {0, total - 1}:                      # R = 1
                    one = model.order_stats_f64(flat, [r1], cells=1, segs=segs, seg_len=n, seg_stride=ss, cell_stride=cs)
                    assert one.shape == (1, 1) and _bits(one)[0, 0] == _bits(want[r1:r1 + 1])[0], (name, segs, r1)


@pytest.mark.parametrize("cells,n,segs", [(2, 5000, 3), (700, 65, 3), (700, 257, 1), (1, 256, 1), (2, 1, 8)])
def test_order_stats_f64_of_many_cells_in_one_launch_each_with_its_own_values(api, cells, n, segs):
    case = H.build_case("micro_3x1", 43)
    total = segs * n
    vals = []
    for c in range(cells):
        fam = value_families(total, seed=100 + c)
        vals.append(fam[sorted(fam)[c % len(fam)]][0])
    flat, ss, cs = _lay_out(vals, segs, n, pad=2)
    want = np.stack([total_order_sorted(v) for v in vals])       # [cells, total]
    with api[0](case["cov"], case["init"], max_chains=1) as model:
        for r in (_ranks(total), np.array([total - 1]), np.array([0])):
            got = model.order_stats_f64(flat, r, cells=cells, segs=segs, seg_len=n, seg_stride=ss, cell_stride=cs)
            assert got.shape == (len(r), cells) and np.array_equal(_bits(got), _bits(want[:, r].T))
        # refusals of the stateless entry point: seir_order_stats's
        for ranks in ([total], [-1], [0, 0], [1, 0][:total], list(range(17)), []):
            if len(ranks) == 2 and total == 1:
                continue
            with pytest.raises(_lib.SeirError) as e:
                model.order_stats_f64(flat, ranks, cells=cells, segs=segs, seg_len=n, seg_stride=ss, cell_stride=cs)
            assert e.value.code == _lib.ERR_INVALID, ranks
        dp, ip = flat.ctypes.data_as(_lib.c_double_p), np.zeros(1, np.int64).ctypes.data_as(_lib.c_int64_p)
        for c_, sg, sl, sst, cst in ((0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1, -1, 1), (1, 1, 1, 1, -1),
                                     (1, 2, 4, 3, 8), (1, 2, 2 ** 30, 2 ** 30, 1)):
            assert model._lib.seir_order_stats_f64(model._ctx, dp, c_, sg, sl, sst, cst, ip, 1, dp) == _lib.ERR_INVALID
        assert model._lib.seir_order_stats_f64(model._ctx, None, 1, 1, 1, 1, 1, ip, 1, dp) == _lib.ERR_INVALID


# ---- 2. the store plus the selection against the stateless kernel ------------------------------------------------------------
def _same_store(s, R):
    """Per-chain and pooled order statistics of sampler `s` against R [n,B,D,M], the R_it of its draws: every bit."""
    n, B = R.shape[:2]
    r = _ranks(n)
    got = s.rt_order_stats(r)
    assert got.dtype == np.float64 and got.shape == (len(r), B) + R.shape[2:]
    assert np.array_equal(_bits(got), _bits(np.sort(R, axis=0)[r]))
    rp = _ranks(n * B)
    gp = s.rt_order_stats(rp, pooled=True)
    assert gp.shape == (len(rp),) + R.shape[2:]
    assert np.array_equal(_bits(gp), _bits(np.sort(R.reshape((n * B,) + R.shape[2:]), axis=0)[rp]))
    return got, gp


PROBS = (0.05, 0.5, 0.95)


@pytest.mark.parametrize("case_id", list(CASES))
def test_the_kept_draws_equal_the_stateless_kernel_and_the_fold_is_what_it_was(api, case_id):
    name, cfg, eps, B, record, n, D = CASES[case_id]
    case = H.build_case(name, 43, alpha_t_sd=0.005)
    u = synth.jitter_params(case["u"], B, scale=0.002 if name == "uk380" else 0.01, seed=3, T=case["k"].T)
    ev = np.stack([case["events"]] * B)
    w = _weight(case)
    model, s = _sampler(api, case, cfg, u, ev, eps, n, record_events=record)
    with model, s:
        s.reset_rt(D, w)
        s.keep_rt_draws(n + 1)                                 # a cap that is no multiple of the run for most n
        tr = s.sample(n, rt=True)
        on = (s.rt_summary(), tr.rt.copy())
        R = _reference(api, case, tr.theta, tr.events, D)
        assert np.all(np.isfinite(R)) and R.min() >= 0.0 and not np.signbit(R).any()
        _same_store(s, R)
        # the quantiles: np.quantile of the same draws
        q, qp = s.rt_quantiles(PROBS), s.rt_quantiles(PROBS, pooled=True)
        assert q.shape == (3, B, D, case["k"].M) and qp.shape == (3, D, case["k"].M)
        np.testing.assert_allclose(q, np.quantile(R, PROBS, axis=0), rtol=1e-12, atol=0.0)
        np.testing.assert_allclose(qp, np.quantile(R.reshape((n * B,) + R.shape[2:]), PROBS, axis=0), rtol=1e-12, atol=0.0)
        # the fold and the national curve with the store on: the stateless kernel's, and the same call's without the store
        _same_acc(on[0], _fold(R))
        _same_rt(on[1], R, w)
        s.keep_rt_draws(0)
        s.reset_rt(D, w)
        s.rt(0, n)
        _same_run((s.rt_summary(), s.read_rt_draws(n)), on)
        with pytest.raises(_lib.SeirError, match="seir_sampler_rt_keep") as e:
            s.rt_order_stats([0])
        assert e.value.code == _lib.ERR_STATE
        # a second reset with the same window empties the store: the last slot alone, at position 0
        s.reset_rt(D, w)
        s.keep_rt_draws(n + 1)
        s.rt(0, n)
        s.reset_rt(D, w)
        with pytest.raises(_lib.SeirError, match="no draws kept") as e:
            s.rt_order_stats([0])
        assert e.value.code == _lib.ERR_STATE
        s.rt(n - 1, 1)
        _same_store(s, R[n - 1:])
        _same_acc(s.rt_summary(), _fold(R[n - 1:]))
        # ... and another window frees it (T = 1 has no other window)
        D2 = 1 if D > 1 else case["k"].T
        if D2 != D:
            s.reset_rt(D2, w)
            with pytest.raises(_lib.SeirError, match="seir_sampler_rt_keep"):
                s.rt_order_stats([0])
        assert not s.pair_timeouts().any()


def test_cutting_a_burst_into_calls_halves_or_batches_does_not_matter(api):
    """The staged write: calls of 1, RUN - 1, RUN and RUN + 1 draws, calls that start off a run boundary, the two halves
    of the buffer, and the host's own batches -- the same store and the same fold, bit for bit."""
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    n, D = 11, 9
    w = _weight(case)
    model, s = _sampler(api, case, cfg, u, ev, eps, 2 * n)
    with model, s:
        s.reset_rt(D, w)
        s.keep_rt_draws(2 * n)
        for first in (0, n):                                   # two bursts in the two halves of the buffer: 11 + 11
            s.reset_trace(at=first)
            s.run(n)
            s.rt(first, n)
        tr = s.read_trace(2 * n)
        halves = (s.rt_summary(), s.read_rt_draws(2 * n))
        R = _reference(api, case, tr.theta, tr.events, D)
        _same_acc(halves[0], _fold(R))
        stats = _same_store(s, R)
        cuts = {
            "one call": ((0, 2 * n),),
            "one draw at a time": tuple((i, 1) for i in range(2 * n)),
            "run - 1, run, run + 1": ((0, RUN - 1), (RUN - 1, RUN), (2 * RUN - 1, RUN + 1), (3 * RUN, 2 * n - 3 * RUN)),
            "runs": tuple((i, min(RUN, 2 * n - i)) for i in range(0, 2 * n, RUN)),
            "off the boundary": ((0, 1), (1, 2 * RUN), (2 * RUN + 1, 1), (2 * RUN + 2, 2 * n - 2 * RUN - 2)),
        }
        for tag, calls in cuts.items():
            assert sum(c for _, c in calls) == 2 * n
            s.reset_rt(D, w)
            for first, count in calls:
                s.rt(first, count)
            _same_run((s.rt_summary(), s.read_rt_draws(2 * n)), halves)
            got = _same_store(s, R)
            assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, stats)), tag
        # the host's own cut: a staging bound of 64 KiB holds 5 slots (batches of 5, 5, 5, 5, 2), one of 1 KiB one slot; the
        # bound is read when the window changes, which frees the store as well
        for kib in (64, 1):
            model.set_option(rt_staging_kib=kib)
            s.reset_rt(D + 1, w)
            s.reset_rt(D, w)
            s.keep_rt_draws(2 * n)
            s.rt(0, 2 * n)
            _same_run((s.rt_summary(), s.read_rt_draws(2 * n)), halves)
            _same_store(s, R)


@pytest.mark.parametrize("skew", [1, 2, 3])
def test_results_do_not_depend_on_workgroup_timing_and_repeat(api, skew):
    case, u, ev, cfg, eps = _case("micro_65x70", 2)
    n, D = 5, 6
    res = {}
    for tag, sk in (("a", 0), ("b", 0), ("skew", skew)):
        if tag == "b" and skew != 1:
            continue                                           # the repeat of the plain run is checked once
        model, s = _sampler(api, case, cfg, u, ev, 0.0001, n, skew=sk, record_events="u16")
        with model, s:
            s.reset_rt(D, _weight(case))
            s.keep_rt_draws(n)
            tr = s.sample(n, rt=True)
            res[tag] = (s.rt_summary(), tr.rt, tr, s.rt_order_stats(_ranks(n)), s.rt_order_stats(_ranks(2 * n), pooled=True))
    assert res["a"][0].sumsq.any()
    for tag in res:
        assert np.array_equal(res["a"][2].events, res[tag][2].events)
        _same_run(res[tag], res["a"])
        for i in (3, 4):
            assert np.array_equal(_bits(res[tag][i]), _bits(res["a"][i]))


def test_chains_keep_their_numbers_however_they_are_sharded(api):
    """Chains 2 and 3 of a 4-chain sampler against a 2-chain sampler created with first_chain_id = 2."""
    case, u, ev, cfg, eps = _case("micro_20x60", 4)
    n, D = 5, 8
    w = _weight(case)
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        s.reset_rt(D, w)
        s.keep_rt_draws(n)
        tr4 = s.sample(n, rt=True)
        st4 = s.rt_order_stats(_ranks(n))
    model, s = _sampler(api, case, cfg, u[2:], ev[2:], eps, n, first_chain_id=2)
    with model, s:
        s.reset_rt(D, w)
        s.keep_rt_draws(n)
        tr2 = s.sample(n, rt=True)
        st2 = s.rt_order_stats(_ranks(n))
    assert np.array_equal(tr4.events[:, 2:], tr2.events) and np.array_equal(tr4.theta[:, 2:], tr2.theta)
    assert np.array_equal(_bits(st4[:, 2:]), _bits(st2)) and len(np.unique(st2[:, 0, 0, 0])) > 1


def test_with_thinning_the_store_holds_the_kept_draws(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 4)
    n, D, k = 6, 5, 3
    w = _weight(case)
    model, s = _sampler(api, case, cfg, u, ev, eps, n, thin=k)
    with model, s:
        s.reset_rt(D, w)
        s.keep_rt_draws(n)
        kept = s.sample(n, rt=True)
        R = _reference(api, case, kept.theta, kept.events, D)
        _same_store(s, R)
        _same_acc(s.rt_summary(), _fold(R))
    model, s = _sampler(api, case, cfg, u, ev, eps, n * k)
    with model, s:
        every = s.sample(n * k)
    assert np.array_equal(every.events[k - 1::k], kept.events) and np.array_equal(every.theta[k - 1::k], kept.theta)


def test_the_chain_and_the_other_products_do_not_notice(api):
    """A sampler that keeps R_it behind every burst's summary, forecast, R_t, check and shares against one that never does:
    traces, marginals, forecast, R_t, check, shares, moments, final state and kernel bit for bit."""
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    nb, burst, Hn, D, K, Dw = 4, 5, 6, 7, 5, 6
    w = _weight(case)
    W, wd = predict.forecast_calendar(case["cov"], None, case["k"].T, Hn)
    cW, cwd = predict.check_calendar(case["cov"], None, case["k"].T, K)
    runs = {}
    for on in (False, True):
        model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
        with model, s:
            got = {}
            s.reset_forecast(Hn, W, wd, 77)
            s.reset_rt(D, w)
            if on:
                s.keep_rt_draws(nb * burst)
            s.reset_check(K, cW, cwd, 78)
            s.reset_within_between(Dw)

            def consume(tr, i, got=got):
                got[i] = (tr.theta.copy(), tr.events.copy(), {k: v.copy() for k, v in tr.hmc.items()},
                          {mk: {kk: v.copy() for kk, v in mv.items()} for mk, mv in tr.moves.items()},
                          {k: v.copy() for k, v in tr.marginals.items()}, {k: v.copy() for k, v in tr.forecast.items()},
                          {k: v.copy() for k, v in tr.check.items()}, {"rt": tr.rt.copy()},
                          {k: v.copy() for k, v in tr.wb.items()})
            s.sample_bursts(nb, burst, consume, summarize=True, forecast=True, rt=True, check=True, within_between=True)
            cs, ws = s.check_summary(), s.within_between_summary()
            runs[on] = (got, s.get_state() + s.get_kernel(), s.summary(), s.forecast_summary(), cs.moments, s.rt_summary(), cs, ws,
                        (s.rt_order_stats(_ranks(nb * burst)), s.rt_order_stats(_ranks(5 * nb * burst), pooled=True)) if on else None)
    from types import SimpleNamespace
    for i in range(nb):
        a, b = (SimpleNamespace(theta=x[0], events=x[1], hmc=x[2], moves=x[3]) for x in (runs[False][0][i], runs[True][0][i]))
        _same_bits(a, b)
        for part in (4, 5, 6, 7, 8):
            for k in runs[False][0][i][part]:
                assert np.array_equal(runs[False][0][i][part][k], runs[True][0][i][part][k]), k
    for x, y in zip(runs[False][1], runs[True][1]):
        assert np.array_equal(x, y)
    for which in (2, 3, 4):
        for k in ("count", "ref", "sum", "sumsq"):
            assert np.array_equal(getattr(runs[False][which], k), getattr(runs[True][which], k)), k
    for k in ("count", "ref", "sum", "sumsq", "gt1"):
        assert np.array_equal(getattr(runs[False][5], k), getattr(runs[True][5], k)), k
    for k in ("observed", "lt", "eq", "location_lt", "location_eq", "day_lt", "day_eq", "total_lt", "total_eq"):
        assert np.array_equal(getattr(runs[False][6], k), getattr(runs[True][6], k)), k
    for k in ("count", "ref_w", "sum_w", "sumsq_w"):
        assert np.array_equal(getattr(runs[False][7], k), getattr(runs[True][7], k), equal_nan=True), k
    got = runs[True][0]
    R = _reference(api, case, np.concatenate([got[i][0] for i in range(nb)]), np.concatenate([got[i][1] for i in range(nb)]), D)
    r, rp = _ranks(nb * burst), _ranks(5 * nb * burst)
    assert np.array_equal(_bits(runs[True][8][0]), _bits(np.sort(R, axis=0)[r]))     # filled through the overlapped bursts
    assert np.array_equal(_bits(runs[True][8][1]), _bits(np.sort(R.reshape((-1,) + R.shape[2:]), axis=0)[rp]))


def test_a_burst_run_again_after_a_time_out_overwrites_its_own_positions(api):
    """seir_sampler_debug_fail_handoff (the existing test hook, once) in the middle of overlapped bursts: the burst is
    restored -- count included, and the host's copy of it -- and run again one launch form down into the same positions."""
    case, u, ev, cfg, eps = _case("micro_20x60", 8)
    B, nb, burst, D = 8, 6, 5, 5
    w = _weight(case)
    model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
    with model, s:
        got = {}
        s.reset_rt(D, w)
        s.keep_rt_draws(nb * burst)                            # exactly: a burst counted twice would be refused

        def consume(tr, i):
            got[i] = (tr.events.copy(), tr.rt.copy(), tr.theta.copy())
            if i == 1 and not s.recoveries:                    # while burst 2 or 3 is in flight
                _lib.check(s._lib.seir_sampler_debug_fail_handoff(s._s, B - 1))
        s.sample_bursts(nb, burst, consume, rt=True)
        rs, recoveries = s.rt_summary(), list(s.recoveries)
        assert len(recoveries) == 1, recoveries
        assert sorted(got) == list(range(nb))
        R = _reference(api, case, np.concatenate([got[i][2] for i in range(nb)]), np.concatenate([got[i][0] for i in range(nb)]), D)
        _same_acc(rs, _fold(R))
        _same_store(s, R)


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 2)
    w = _weight(case)
    n, D = 4, 3
    model, s = _sampler(api, case, cfg, u, ev, eps, n, record_events=False)
    with model, s:
        for call in (lambda: s.keep_rt_draws(4), lambda: s.rt_order_stats([0])):
            with pytest.raises(_lib.SeirError, match="record_events=0") as e:
                call()
            assert e.value.code == _lib.ERR_INVALID
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        for call in (lambda: s.keep_rt_draws(4), lambda: s.rt_order_stats([0])):
            with pytest.raises(_lib.SeirError, match="seir_sampler_rt_reset") as e:         # before a reset
                call()
            assert e.value.code == _lib.ERR_STATE
        s.reset_rt(D, w)
        with pytest.raises(_lib.SeirError, match="seir_sampler_rt_keep") as e:              # no store
            s.rt_order_stats([0])
        assert e.value.code == _lib.ERR_STATE
        with pytest.raises(ValueError):
            s.keep_rt_draws(-1)
        for cap in (-1, (1 << 20) + 1):
            assert s._lib.seir_sampler_rt_keep(s._s, cap) == _lib.ERR_INVALID
        s.keep_rt_draws(n - 1)                                 # one draw short of what the run folds
        with pytest.raises(_lib.SeirError, match="no draws kept") as e:
            s.rt_order_stats([0])
        assert e.value.code == _lib.ERR_STATE
        s.reset_trace()
        s.run(n)
        with pytest.raises(_lib.SeirError, match=rf"0 draws per chain .* and {n} more: the draw store holds {n - 1}") as e:
            s.rt(0, n)
        assert e.value.code == _lib.ERR_INVALID
        s.rt(0, n - 1)                                         # up to the cap it goes
        with pytest.raises(_lib.SeirError, match=rf"{n - 1} draws per chain .* and 1 more: the draw store holds {n - 1}"):
            s.rt(n - 1, 1)
        with pytest.raises(_lib.SeirError, match="first seir_sampler_rt") as e:             # sized after the first call
            s.keep_rt_draws(n)
        assert e.value.code == _lib.ERR_STATE
        cnt = n - 1
        for ranks, pooled in (([cnt], False), ([2 * cnt], True), ([-1], False), ([1, 1], False), ([2, 1], True),
                              (list(range(17)), True), ([], False)):
            with pytest.raises(_lib.SeirError) as e:
                s.rt_order_stats(ranks, pooled=pooled)
            assert e.value.code == _lib.ERR_INVALID, ranks
        assert s.rt_order_stats([2 * cnt - 1], pooled=True).shape == (1, D, s.M)           # the last pooled rank is one
        s.keep_rt_draws(0)                                     # frees it, at any time
        with pytest.raises(_lib.SeirError, match="seir_sampler_rt_keep"):
            s.rt_order_stats([0])


def test_a_store_above_half_of_the_free_memory_is_refused_and_a_restore_keeps_the_counts_together(api):
    """The UK-380 x 8 shape, D = 14: 2^20 draws would take 357 GB, more than half of any device's free memory; nothing is
    allocated and the sampler goes on.  Then a restore of the snapshot taken before the burst brings the device's count and
    the library's own copy of it back together: the selection's refusal of counts that differ from the store's guards that
    pairing and cannot be reached through the public calls, so what is held here is that they stay paired."""
    import torch
    case, u, ev, cfg, eps = _case("uk380", 8)
    w = _weight(case)
    n, D = 2, 14
    model, s = _sampler(api, case, cfg, u, ev, eps, n, record_events="u16")
    with model, s:
        s.reset_rt(D, w)
        free0 = torch.cuda.mem_get_info(0)[0]
        need = 8 * D * s.M * (1 << 20) * 8
        with pytest.raises(_lib.SeirError, match=rf"needs {need} bytes .* more than half of the \d+ bytes free") as e:
            s.keep_rt_draws(1 << 20)
        assert e.value.code == _lib.ERR_INVALID
        assert abs(torch.cuda.mem_get_info(0)[0] - free0) < (64 << 20)                    # nothing of 357 GB was taken
        s.keep_rt_draws(n)
        tr = s.sample(n, rt=True)
        full = s.rt_order_stats([0, n - 1])
        assert full.shape == (2, 8, D, s.M) and tr.rt.shape == (n, 8, D)
        s.restore(0)                                           # the snapshot sample() took before the burst: count 0
        with pytest.raises(_lib.SeirError, match="no draws kept"):
            s.rt_order_stats([0])
        s.rt(0, n)                                             # folded again into the same positions; not refused as past the cap
        assert np.array_equal(s.rt_summary().count, np.full(8, n))
        assert np.array_equal(_bits(s.rt_order_stats([0, n - 1])), _bits(full))


# ---- CLI end to end -------------------------------------------------------------------------------------------------------
def test_cli_rt_quantiles(api, tmp_path):
    """`--rt 7 --rt-quantiles 0.05,0.5,0.95` on an NI-11 data set: the new datasets equal np.quantile of the stateless kernel
    on the file's own draws; with `--summaries only --thin 2 --forecast 7 --rt 7 --check 7 --within-between 7` it works
    without samples/seir; `--rt 7` alone writes none of them."""
    tmp_path = str(tmp_path)
    cov = synth.make_covariates("ni11")
    events, init, _ = synth.simulate_epidemic(cov)
    data = os.path.join(tmp_path, "data.npz")
    inf.write_inference_data(data, cov, events[..., 2])
    q_path, q_log = _cli(tmp_path, "rtq", data, ["--rt", "7", "--rt-quantiles", "0.05,0.5,0.95"])
    q = _datasets(q_path)
    both = _datasets(_cli(tmp_path, "both", data, ["--summaries", "only", "--thin", "2", "--forecast", "7", "--rt", "7", "--check", "7",
                                                   "--within-between", "7", "--rt-quantiles", "0.5"])[0])
    rt_path, rt_log = _cli(tmp_path, "rt", data, ["--rt", "7"])
    rt = _datasets(rt_path)
    old = {"rt/days", "rt/first_day", "rt/count", "rt/R_it_mean", "rt/R_it_var", "rt/R_it_prob_gt1", "samples/R_t"}
    new = {"rt/quantile_probs", "rt/pooled_chains", "rt/R_it_quantiles", "rt/pooled_R_it_quantiles", "rt/R_t_quantiles",
           "rt/pooled_R_t_quantiles"}
    assert set(rt) == PLAIN | old and "R_t quantiles" not in rt_log
    assert set(q) == PLAIN | old | new and q_log.count("R_t quantiles:") == 1
    for k in rt:
        if rt[k].dtype.kind in "fiub":
            assert np.array_equal(rt[k], q[k], equal_nan=rt[k].dtype.kind == "f"), k
    M, T, D, ns = cov.M, cov.T, 7, 2 * 6
    assert "samples/seir" not in both and new | old <= set(both) and "check/count" in both and "within_between/count" in both
    assert np.array_equal(both["rt/quantile_probs"], [0.5]) and both["rt/R_it_quantiles"].shape == (1, D, M)
    assert np.all(np.isfinite(both["rt/R_it_quantiles"])) and np.array_equal(both["rt/pooled_R_it_quantiles"], both["rt/R_it_quantiles"])
    probs = [0.05, 0.5, 0.95]
    assert np.array_equal(q["rt/quantile_probs"], probs) and np.array_equal(q["rt/pooled_chains"], [0])
    # the reference from the file's own draws: the sampling phase is the last ns rows
    cov2, _, _ = inf.read_inference_data(data)
    seir = q["samples/seir"][-ns:]
    theta = np.concatenate([q[f"samples/{k}"][-ns:].reshape(ns, -1) for k in
                            ("psi", "sigma_space", "beta_area", "gamma0", "gamma1", "alpha_0", "alpha_t", "spatial_effect")], axis=1)
    with api[0](cov2, q["initial_state"], max_chains=ns) as model:
        R = model.reproduction_number(theta, seir)[:, T - D:]
    assert q["rt/R_it_quantiles"].shape == (3, D, M) and q["rt/R_it_quantiles"].dtype == np.float64
    np.testing.assert_allclose(q["rt/R_it_quantiles"], np.quantile(R, probs, axis=0), rtol=1e-12, atol=0.0)
    assert np.array_equal(q["rt/pooled_R_it_quantiles"], q["rt/R_it_quantiles"])            # one chain: the pool is the chain
    np.testing.assert_allclose(q["rt/R_t_quantiles"], np.quantile(q["samples/R_t"], probs, axis=0), rtol=1e-12, atol=0.0)
    assert np.array_equal(q["rt/pooled_R_t_quantiles"], q["rt/R_t_quantiles"])

"""Forecast intervals on the device (include/seir_hip.h, "Forecast intervals on the device"): k_forecast_keep fills the
draw store keep[B][3][M][H][cap] behind the forecast's fold, k_order_stats selects exact order statistics from it.

The selection alone is held to np.sort through `seir_order_stats` on values no simulation produces.  The store plus the
selection are held to test_forecast_gpu.py's oracle: `tr.theta` and `tr.events` are read back, `SeirModel.simulate` is
called per chain with `first_draw_id = chain << 20`, the three planes (cases, cumulative cases, prevalence) are formed with
NumPy in int64 and `np.sort(..., axis=0)[ranks]` is the expected result.  Every comparison of order statistics is
`np.array_equal`."""
import os

import numpy as np
import pytest

from covid19uk_amd import _lib, synth
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.posterior import predict
from tests import helpers as H
from tests import test_check_gpu as CG
from tests import test_forecast_gpu as FG
from tests.test_forecast_quantiles_host import INT_MIN, value_families
from tests.test_recovery_gpu import _case, _same_bits
from tests.test_sampler_gpu import api  # noqa: F401  (fixture)
from tests.test_summary_gpu import _cli, _datasets, _sampler

pytestmark = pytest.mark.gpu

PLANES = ("cases", "cum_cases", "prevalence")


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def _ranks(n):
    """Every rank while n <= 16; otherwise 16 of them with 0, n - 1 and the median's two."""
    if n <= 16:
        return np.arange(n, dtype=np.int64)
    fixed = {0, n - 1, (n - 1) // 2, n // 2}
    rest = [r for r in range(n) if r not in fixed]
    take = np.linspace(0, len(rest) - 1, 16 - len(fixed)).astype(np.int64)
    picked = sorted(fixed | {rest[i] for i in take})
    assert len(picked) == 16
    return np.array(picked, dtype=np.int64)


def _planes(case, events, sim):
    """events [n,B,M,T,3] recorded, sim [n,B,M,H,3] the oracle's forecast -> the store's planes [n,B,3,M,H] int64."""
    out = []
    for b in range(sim.shape[1]):
        st0 = FG._state_at_T(case["init"], events[:, b])
        x = FG._quantities(sim[:, b], st0)
        out.append(np.stack([sim[:, b, :, :, 2], np.cumsum(sim[:, b, :, :, 2], axis=2), x[..., 5]], axis=1))
    p = np.stack(out, axis=1)
    assert p.min() >= 0 and p.max() < 2 ** 31
    return p


def _want(planes, ranks, pooled=False):
    x = planes.reshape((-1,) + planes.shape[2:]) if pooled else planes
    return np.sort(x, axis=0)[ranks]


def _same_stats(s, planes):
    """Per-chain and pooled order statistics of sampler `s` against the planes [n,B,3,M,H] of its draws."""
    n, B = planes.shape[:2]
    r = _ranks(n)
    got = s.forecast_order_stats(r)
    assert got.dtype == np.int32 and got.shape == (len(r), B) + planes.shape[2:]
    assert np.array_equal(got, _want(planes, r))
    rp = _ranks(n * B)
    gp = s.forecast_order_stats(rp, pooled=True)
    assert gp.dtype == np.int32 and gp.shape == (len(rp),) + planes.shape[2:]
    assert np.array_equal(gp, _want(planes, rp, pooled=True))
    return got, gp


def _start(s, case, Hn, cap, seed=FG.SEED):
    FG._reset(s, case, Hn, seed)
    s.keep_forecast_draws(cap)


# ---- 1. the selection alone ------------------------------------------------------------------------------------------------
def _lay_out(cells_values, segs, seg_len, pad):
    """cells_values [cells][segs * seg_len] -> the flat array with seg_stride = seg_len + pad, gaps filled with a value
    that would show (INT_MIN), and the strides."""
    cells = len(cells_values)
    seg_stride = seg_len + pad
    cell_stride = segs * seg_stride + 3
    flat = np.full(cells * cell_stride, INT_MIN, np.int32)
    for c, vals in enumerate(cells_values):
        v = np.asarray(vals, np.int64).astype(np.int32).reshape(segs, seg_len)
        for g in range(segs):
            flat[c * cell_stride + g * seg_stride:c * cell_stride + g * seg_stride + seg_len] = v[g]
    return flat, seg_stride, cell_stride


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 5000])
def test_order_stats_equal_numpy_sort_on_every_array_family(api, n):
    case = H.build_case("micro_3x1", 43)
    with api[0](case["cov"], case["init"], max_chains=1) as model:
        for segs in (1, 3, 8):
            total = segs * n
            for name, xs in value_families(total, seed=segs).items():
                flat, ss, cs = _lay_out([xs], segs, n, pad=5)
                want = np.sort(np.asarray(xs, np.int64))
                r16 = _ranks(total)
                got = model.order_stats(flat, r16, cells=1, segs=segs, seg_len=n, seg_stride=ss, cell_stride=cs)
                assert got.dtype == np.int32 and got.shape == (len(r16), 1)
                assert 0 in r16 and total - 1 in r16
                assert np.array_equal(got[:, 0], want[r16]), (name, segs)
                for r1 in {0, total - 1}:                      # R = 1
                    one = model.order_stats(flat, [r1], cells=1, segs=segs, seg_len=n, seg_stride=ss, cell_stride=cs)
                    assert one.shape == (1, 1) and one[0, 0] == want[r1], (name, segs, r1)


@pytest.mark.parametrize("cells,n,segs", [(2, 5000, 3), (700, 65, 3), (700, 257, 1), (2, 1, 8), (700, 2, 1)])
def test_order_stats_of_many_cells_in_one_launch_each_with_its_own_values(api, cells, n, segs):
    case = H.build_case("micro_3x1", 43)
    total = segs * n
    vals = []
    for c in range(cells):
        fam = value_families(total, seed=100 + c)
        vals.append(fam[sorted(fam)[c % len(fam)]])
    flat, ss, cs = _lay_out(vals, segs, n, pad=2)
    want = np.sort(np.asarray(vals, np.int64), axis=1)         # [cells, total]
    assert len({tuple(w[:4]) for w in want}) > 1
    with api[0](case["cov"], case["init"], max_chains=1) as model:
        for r in (_ranks(total), np.array([total - 1]), np.array([0])):
            got = model.order_stats(flat, r, cells=cells, segs=segs, seg_len=n, seg_stride=ss, cell_stride=cs)
            assert got.shape == (len(r), cells) and np.array_equal(got, want[:, r].T)
        # refusals of the stateless entry point
        for ranks in ([total], [-1], [0, 0], [1, 0][:total], list(range(17)), []):
            if len(ranks) == 2 and total == 1:
                continue
            with pytest.raises(_lib.SeirError) as e:
                model.order_stats(flat, ranks, cells=cells, segs=segs, seg_len=n, seg_stride=ss, cell_stride=cs)
            assert e.value.code == _lib.ERR_INVALID, ranks


# ---- 2. the store plus the selection against the oracle --------------------------------------------------------------------
@pytest.mark.parametrize("case_id", list(FG.CASES))
def test_order_stats_of_the_kept_draws_equal_numpy_sort_of_the_oracles(api, case_id):
    name, cfg, eps, B, record, n, Hn = FG.CASES[case_id]
    case = H.build_case(name, 43, alpha_t_sd=0.005)
    u = synth.jitter_params(case["u"], B, scale=0.002 if name == "uk380" else 0.01, seed=3, T=case["k"].T)
    ev = np.stack([case["events"]] * B)
    model, s = _sampler(api, case, cfg, u, ev, eps, n, record_events=record)
    with model, s:
        FG._reset(s, case, Hn)
        # a store larger than half of what is free is refused before anything is allocated, with both figures
        import torch
        need, free = B * 3 * case["k"].M * Hn * (1 << 20) * 4, torch.cuda.mem_get_info()[0]
        if need > free:                                        # (between free / 2 and free another process may move the line)
            with pytest.raises(_lib.SeirError, match=rf"needs {need} bytes .* more than half of the \d+ bytes free") as e:
                s.keep_forecast_draws(1 << 20)
            assert e.value.code == _lib.ERR_INVALID
        assert name != "uk380" or need > free                  # UK-380 x 8, H = 56, 2^20 draws: 2.1 TB
        s.keep_forecast_draws(n)
        tr = s.sample(n, forecast=True)
        assert tr.events.dtype == (np.uint16 if record == "u16" else np.int32)
        want = FG._oracle(model, case, tr.theta, tr.events, Hn)
        FG._same_moments(s.forecast_summary(), want)           # the forecast itself is what it was
        planes = _planes(case, tr.events, want["sim"])
        assert planes.shape == (n, B, 3, case["k"].M, Hn)
        cases = planes[:, :, 0]
        assert (cases.max(axis=0) != cases.min(axis=0)).any(), "no cell of `cases` differs between draws"
        if name.startswith("micro"):
            srt = np.sort(cases, axis=0)
            assert (srt[1:] == srt[:-1]).any(), "no ties among the draws of a cell"
        _same_stats(s, planes)
        # the quantiles are NumPy's on the same draws
        probs = (0.05, 0.5, 0.95)
        q = s.forecast_quantiles(probs)
        assert q.dtype == np.float64 and q.shape == (3, B, 3, case["k"].M, Hn)
        np.testing.assert_allclose(q, np.quantile(planes, probs, axis=0), rtol=1e-12, atol=0)
        qp = s.forecast_quantiles(probs, pooled=True)
        np.testing.assert_allclose(qp, np.quantile(planes.reshape((-1,) + planes.shape[2:]), probs, axis=0), rtol=1e-12, atol=0)
        assert not s.pair_timeouts().any()


# ---- 3. cuts ---------------------------------------------------------------------------------------------------------------
def test_cutting_a_burst_into_calls_or_halves_does_not_matter(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    n, Hn = 11, 9
    model, s = _sampler(api, case, cfg, u, ev, eps, 2 * n)
    with model, s:
        _start(s, case, Hn, 2 * n)
        for first in (0, n):                                   # two bursts in the two halves of the buffer
            s.reset_trace(at=first)
            s.run(n)
            s.forecast(first, n)
        tr = s.read_trace(2 * n)
        planes = _planes(case, tr.events, FG._oracle(model, case, tr.theta, tr.events, Hn)["sim"])
        halves = _same_stats(s, planes)
        _start(s, case, Hn, 2 * n)
        s.forecast(0, 2 * n)                                   # one call over everything
        one = _same_stats(s, planes)
        _start(s, case, Hn, 2 * n)
        for first, count in ((0, 3), (3, 1), (4, 9), (13, 2 * n - 13)):
            s.forecast(first, count)
        cut = _same_stats(s, planes)
        for a, b in zip(one + cut, halves + halves):
            assert np.array_equal(a, b)


def test_a_call_of_two_host_batches_fills_one_run_per_cell(api):
    """130 slots: two batches of the host's cut (128 and 2), two k_forecast_keep launches into the same cells."""
    case, u, ev, cfg, eps = _case("micro_5x24", 2)
    n, Hn = 130, 3
    model, s = _sampler(api, case, cfg, u, ev, 0.002, n)
    with model, s:
        _start(s, case, Hn, n)
        tr = s.sample(n, forecast=True)
        planes = _planes(case, tr.events, FG._oracle(model, case, tr.theta, tr.events, Hn)["sim"])
        whole = _same_stats(s, planes)
        _start(s, case, Hn, n)
        for first in range(0, n, 26):
            s.forecast(first, 26)
        for a, b in zip(_same_stats(s, planes), whole):
            assert np.array_equal(a, b)


# ---- 4. further runs, each equal to the first --------------------------------------------------------------------------------
@pytest.mark.parametrize("skew", [1, 2, 3])
def test_the_statistics_do_not_depend_on_workgroup_timing_and_repeat(api, skew):
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    n, Hn = 6, 10
    res = {}
    for tag, sk in (("a", 0), ("b", 0), ("skew", skew)):
        if tag == "b" and skew != 1:
            continue                                           # the repeat of the plain run is checked once
        model, s = _sampler(api, case, cfg, u, ev, eps, n, skew=sk, record_events="u16")
        with model, s:
            _start(s, case, Hn, n)
            tr = s.sample(n, forecast=True)
            res[tag] = (s.forecast_order_stats(_ranks(n)), s.forecast_order_stats(_ranks(5 * n), pooled=True), tr.events)
            if tag == "a":
                _same_stats(s, _planes(case, tr.events, FG._oracle(model, case, tr.theta, tr.events, Hn)["sim"]))
    for tag in res:
        for a, b in zip(res[tag], res["a"]):
            assert np.array_equal(a, b), tag


def test_chains_keep_their_statistics_however_they_are_sharded(api):
    """Chains 0, 1 and 2, 3 in two samplers against 4 chains in one: per chain the same; the 4-chain sampler's pooled
    statistics are np.sort over the union."""
    case, u, ev, cfg, eps = _case("micro_20x60", 4)
    n, Hn = 5, 8
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        _start(s, case, Hn, n)
        tr4 = s.sample(n, forecast=True)
        planes4 = _planes(case, tr4.events, FG._oracle(model, case, tr4.theta, tr4.events, Hn)["sim"])
        own4, pooled4 = _same_stats(s, planes4)
    parts = []
    for c0 in (0, 2):
        model, s = _sampler(api, case, cfg, u[c0:c0 + 2], ev[c0:c0 + 2], eps, n, first_chain_id=c0)
        with model, s:
            _start(s, case, Hn, n)
            tr2 = s.sample(n, forecast=True)
            assert np.array_equal(tr2.events, tr4.events[:, c0:c0 + 2])
            parts.append(s.forecast_order_stats(_ranks(n)))
            assert np.array_equal(s.forecast_order_stats(_ranks(2 * n), pooled=True),
                                  _want(planes4[:, c0:c0 + 2], _ranks(2 * n), pooled=True))
    assert np.array_equal(np.concatenate(parts, axis=1), own4)
    assert np.array_equal(pooled4, np.sort(planes4.reshape((-1,) + planes4.shape[2:]), axis=0)[_ranks(4 * n)])


def test_with_thinning_the_statistics_are_those_of_the_kept_draws(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 4)
    n, Hn, k = 6, 5, 3
    model, s = _sampler(api, case, cfg, u, ev, eps, n, thin=k)
    with model, s:
        _start(s, case, Hn, n)
        kept = s.sample(n, forecast=True)
        stats = (s.forecast_order_stats(_ranks(n)), s.forecast_order_stats(_ranks(4 * n), pooled=True))
    model, s = _sampler(api, case, cfg, u, ev, eps, n * k)
    with model, s:
        every = s.sample(n * k)
        assert np.array_equal(every.events[k - 1::k], kept.events)
        planes = _planes(case, every.events[k - 1::k], FG._oracle(model, case, every.theta[k - 1::k], every.events[k - 1::k], Hn)["sim"])
    assert np.array_equal(stats[0], _want(planes, _ranks(n)))
    assert np.array_equal(stats[1], _want(planes, _ranks(4 * n), pooled=True))


def test_a_second_reset_empties_the_store(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 3)
    n, Hn = 5, 6
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        _start(s, case, Hn, n)
        tr = s.sample(n, forecast=True)
        want = FG._oracle(model, case, tr.theta, tr.events, Hn)
        _same_stats(s, _planes(case, tr.events, want["sim"]))
        FG._reset(s, case, Hn)                                 # the same horizon: the store stays, and is empty
        with pytest.raises(_lib.SeirError, match="no draws kept") as e:
            s.forecast_order_stats([0])
        assert e.value.code == _lib.ERR_STATE
        s.forecast(n - 1, 1)                                   # the last slot alone is draw 0 of every chain now
        one = FG._oracle(model, case, tr.theta[n - 1:], tr.events[n - 1:], Hn)
        _same_stats(s, _planes(case, tr.events[n - 1:], one["sim"]))
        FG._reset(s, case, Hn + 1)                             # another horizon frees it
        with pytest.raises(_lib.SeirError, match="seir_sampler_forecast_keep") as e:
            s.forecast_order_stats([0])
        assert e.value.code == _lib.ERR_STATE
        s.sample(n, forecast=True)                             # ... and the forecast goes on without it
        assert np.array_equal(s.forecast_summary().count, [n] * 3)


def test_a_burst_run_again_after_a_time_out_is_kept_once(api):
    """seir_sampler_debug_fail_handoff (the existing test hook, once) in the middle of overlapped bursts: the burst is
    restored -- the draw counter with it -- and run again; its draws overwrite their own positions of the store."""
    case, u, ev, cfg, eps = _case("micro_20x60", 8)
    B, nb, burst, Hn = 8, 6, 4, 5
    model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
    with model, s:
        got = {}
        _start(s, case, Hn, nb * burst)

        def consume(tr, i):
            got[i] = (tr.events.copy(), tr.theta.copy())
            if i == 1 and not s.recoveries:                    # while burst 2 or 3 is in flight
                _lib.check(s._lib.seir_sampler_debug_fail_handoff(s._s, B - 1))
        s.sample_bursts(nb, burst, consume, forecast=True)
        assert len(s.recoveries) == 1 and sorted(got) == list(range(nb))
        stats = (s.forecast_order_stats(_ranks(nb * burst)), s.forecast_order_stats(_ranks(B * nb * burst), pooled=True))
        assert np.array_equal(s.forecast_summary().count, [nb * burst] * B)
    theta, events = np.concatenate([got[i][1] for i in range(nb)]), np.concatenate([got[i][0] for i in range(nb)])
    with api[0](case["cov"], case["init"], max_chains=B) as model:
        planes = _planes(case, events, FG._oracle(model, case, theta, events, Hn)["sim"])
    assert np.array_equal(stats[0], _want(planes, _ranks(nb * burst)))
    assert np.array_equal(stats[1], _want(planes, _ranks(B * nb * burst), pooled=True))


# ---- 5. nothing else notices -------------------------------------------------------------------------------------------------
def test_chain_forecast_summaries_rt_and_check_do_not_notice_the_store(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    nb, burst, K = 4, 5, 6
    N = np.asarray(case["cov"].N, np.float64).reshape(-1)
    runs = {}
    for keep in (False, True):
        model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
        with model, s:
            got = {}
            FG._reset(s, case, K)
            if keep:
                s.keep_forecast_draws(nb * burst)
            s.reset_rt(K, N / N.sum())
            CG._reset(s, case, K)
            s.sample_bursts(nb, burst, lambda tr, i, got=got: got.__setitem__(i, CG._copy_burst(tr)), summarize=True,
                            forecast=True, rt=True, check=True)
            runs[keep] = (got, s.get_state() + s.get_kernel(), s.summary(), s.forecast_summary(), s.check_summary().moments,
                          s.rt_summary(), s.check_summary())
            if keep:
                theta, events = np.concatenate([got[i][0] for i in range(nb)]), np.concatenate([got[i][1] for i in range(nb)])
                _same_stats(s, _planes(case, events, FG._oracle(model, case, theta, events, K)["sim"]))
    from types import SimpleNamespace
    for i in range(nb):
        a, b = (SimpleNamespace(theta=x[0], events=x[1], hmc=x[2], moves=x[3]) for x in (runs[False][0][i], runs[True][0][i]))
        _same_bits(a, b)
        for j in (4, 5, 7):
            for k in runs[False][0][i][j]:
                assert np.array_equal(runs[False][0][i][j][k], runs[True][0][i][j][k]), k
        assert np.array_equal(runs[False][0][i][6], runs[True][0][i][6])
    for x, y in zip(runs[False][1], runs[True][1]):
        assert np.array_equal(x, y)
    for j in (2, 3, 4):
        for k in ("count", "ref", "sum", "sumsq"):
            assert np.array_equal(getattr(runs[False][j], k), getattr(runs[True][j], k)), (j, k)
    for k in ("count", "ref", "sum", "sumsq", "gt1"):
        assert np.array_equal(getattr(runs[False][5], k), getattr(runs[True][5], k)), k
    for k in ("observed", "lt", "eq", "location_lt", "location_eq", "day_lt", "day_eq", "total_lt", "total_eq"):
        assert np.array_equal(getattr(runs[False][6], k), getattr(runs[True][6], k)), k


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 2)
    n, Hn = 4, 5
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        for call in (lambda: s.keep_forecast_draws(4), lambda: s.forecast_order_stats([0])):
            with pytest.raises(_lib.SeirError, match="seir_sampler_forecast_reset") as e:      # before a reset
                call()
            assert e.value.code == _lib.ERR_STATE
        FG._reset(s, case, Hn)
        with pytest.raises(_lib.SeirError, match="seir_sampler_forecast_keep") as e:           # no store
            s.forecast_order_stats([0])
        assert e.value.code == _lib.ERR_STATE
        with pytest.raises(ValueError):
            s.keep_forecast_draws(-1)
        for cap in (-1, (1 << 20) + 1):
            assert s._lib.seir_sampler_forecast_keep(s._s, cap) == _lib.ERR_INVALID
        s.keep_forecast_draws(n - 1)                           # one draw short of what the run forecasts
        with pytest.raises(_lib.SeirError, match="no draws kept") as e:
            s.forecast_order_stats([0])
        assert e.value.code == _lib.ERR_STATE
        s.reset_trace()
        s.run(n)
        with pytest.raises(_lib.SeirError, match=rf"0 draws per chain forecast since the reset and {n} more: the draw store holds {n - 1}") as e:
            s.forecast(0, n)
        assert e.value.code == _lib.ERR_INVALID
        s.forecast(0, n - 1)                                   # what fits is taken
        with pytest.raises(_lib.SeirError, match=rf"{n - 1} draws per chain forecast since the reset and 1 more: the draw store holds {n - 1}"):
            s.forecast(n - 1, 1)
        with pytest.raises(_lib.SeirError, match="between") as e:                              # not once draws are kept
            s.keep_forecast_draws(n)
        assert e.value.code == _lib.ERR_STATE
        cnt = n - 1
        for ranks, pooled in (([cnt], False), ([-1], False), ([0, 0], False), ([2, 1], False), (list(range(17)), True),
                              ([], False), ([2 * cnt], True)):
            with pytest.raises(_lib.SeirError) as e:
                s.forecast_order_stats(ranks, pooled=pooled)
            assert e.value.code == _lib.ERR_INVALID, ranks
        assert s.forecast_order_stats([2 * cnt - 1], pooled=True).shape == (1, 3, s.M, Hn)      # the last pooled rank is one
        s.keep_forecast_draws(0)                               # frees it, at any time
        with pytest.raises(_lib.SeirError, match="seir_sampler_forecast_keep"):
            s.forecast_order_stats([0])
        s.forecast(n - 1, 1)                                   # and the forecast is no longer bounded by it
        assert np.array_equal(s.forecast_summary().count, [n, n])


# ---- 7. CLI end to end -------------------------------------------------------------------------------------------------------
def test_cli_forecast_quantiles(api, tmp_path):
    """`--forecast 14 --forecast-quantiles 0.05,0.5,0.95` on an NI-11 data set against np.quantile of the oracle's draws from
    the file's own samples; the same with `--summaries only --thin 2 --rt 7 --check 7` gives the datasets without
    samples/seir; without the option the file has no forecast/*quantiles dataset."""
    tmp_path = str(tmp_path)
    cov = synth.make_covariates("ni11")
    events, init, _ = synth.simulate_epidemic(cov)
    data = os.path.join(tmp_path, "data.npz")
    inf.write_inference_data(data, cov, events[..., 2])
    probs = (0.05, 0.5, 0.95)
    fq_path, fq_log = _cli(tmp_path, "fq", data, ["--forecast", "14", "--forecast-quantiles", "0.05,0.5,0.95"])
    fq = _datasets(fq_path)
    plain = _datasets(_cli(tmp_path, "plain", data, ["--forecast", "14"])[0])
    new = {"forecast/quantile_probs", "forecast/pooled_chains"} | \
        {f"forecast/{pre}{name}_quantiles" for pre in ("", "pooled_") for name in PLANES}
    assert set(fq) - set(plain) == new and set(plain) <= set(fq)
    assert not any("quantile" in k for k in plain)
    for k in plain:
        if plain[k].dtype.kind in "fiub":
            assert np.array_equal(plain[k], fq[k], equal_nan=plain[k].dtype.kind == "f"), k
    assert fq_log.count("Forecast quantiles:") == 1
    M, T, Hn, ns = cov.M, cov.T, 14, 2 * 6
    cov2, _, dates = inf.read_inference_data(data)
    W, wd = predict.forecast_calendar(cov2, dates, T, Hn)
    seir = fq["samples/seir"][-ns:]
    theta = np.concatenate([fq[f"samples/{k}"][-ns:].reshape(ns, -1) for k in
                            ("psi", "sigma_space", "beta_area", "gamma0", "gamma1", "alpha_0", "alpha_t", "spatial_effect")], axis=1)
    init_f = fq["initial_state"]
    par, a_path, spatial, st0 = FG._inputs(theta, seir.astype(np.int64), init_f, T, Hn)
    with api[0](cov2, init_f, max_chains=1) as model:
        sim = model.simulate(par, a_path, spatial, W, wd, st0.astype(np.float64), seed=0, first_draw_id=0).astype(np.int64)
    assert sim.any()
    x = FG._quantities(sim, st0)
    planes = dict(cases=sim[..., 2], cum_cases=np.cumsum(sim[..., 2], axis=2), prevalence=x[..., 5])
    assert np.array_equal(fq["forecast/quantile_probs"], probs) and np.array_equal(fq["forecast/pooled_chains"], [0])
    for name in PLANES:
        want = np.quantile(planes[name], probs, axis=0)
        for pre in ("", "pooled_"):                            # one chain: pooled over the process is that chain
            got = fq[f"forecast/{pre}{name}_quantiles"]
            assert got.shape == (3, M, Hn) and got.dtype == np.float64
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    assert (planes["cases"].max(axis=0) != planes["cases"].min(axis=0)).any()
    # with everything else on and no event tensor in the file
    only = _datasets(_cli(tmp_path, "only", data, ["--forecast", "14", "--forecast-quantiles", "0.05,0.5,0.95", "--summaries",
                                                   "only", "--thin", "2", "--rt", "7", "--check", "7"])[0])
    assert "samples/seir" not in only and new <= set(only)
    for name in PLANES:
        assert only[f"forecast/{name}_quantiles"].shape == (3, M, Hn)
        assert np.array_equal(only[f"forecast/{name}_quantiles"], only[f"forecast/pooled_{name}_quantiles"])
    q = only["forecast/cases_quantiles"]
    assert (q[0] <= q[1]).all() and (q[1] <= q[2]).all() and (q >= 0).all()
    cum = only["forecast/cum_cases_quantiles"]
    assert (np.diff(cum, axis=2) >= 0).all()                   # a cumulative count's quantiles do not fall over the days

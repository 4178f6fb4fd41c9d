"""Scoring the forecast against later data on the device (include/seir_hip.h, "Scoring the forecast against later data";
covid19uk_amd/csrc/verify_kernels.h): k_pair_abs alone (`SeirModel.pair_abs_sums`) and the fold riding on the sampler's
forecast, held to the NumPy definitions of `posterior.verify`.  Every comparison is `np.array_equal` on integers.

The sampler's oracle is tests/test_forecast_gpu.py's: the same run's recorded draws, `SeirModel.simulate` per chain.  The
truth is draw 0 of chain 0 of that simulation, perturbed (+1 / -1 on a third of the cells each), with cells knocked out."""
import numpy as np
import pytest

from covid19uk_amd import _lib, synth
from covid19uk_amd.posterior import verify as V
from tests import helpers as H
from tests import test_forecast_gpu as FG
from tests.test_recovery_gpu import _case
from tests.test_sampler_gpu import CFG_REF, CFG_SMALL, api  # noqa: F401  (fixture)
from tests.test_summary_gpu import _sampler

pytestmark = pytest.mark.gpu

C = _lib.PAIR_ABS_CHUNK
I32 = np.iinfo(np.int32)


@pytest.fixture(scope="module")
def model(api):
    case = H.build_case("micro_3x1", 43)
    with api[0](case["cov"], case["init"], max_chains=1) as m:
        yield m


def _family(rng, name, shape):
    n = shape[-1]
    if name == "all_equal":
        return np.full(shape, 12345, np.int32)
    if name == "two_valued":
        return rng.choice(np.array([-7, 1000003], np.int32), size=shape)
    if name == "zeros_but_one":
        x = np.zeros(shape, np.int32)
        x[..., n // 2] = 77
        return x
    if name == "extremes":
        return rng.choice(np.array([I32.min, -1, 0, I32.max], np.int32), size=shape)
    if name == "lowest_digit":
        return rng.integers(0, 256, size=shape, dtype=np.int64).astype(np.int32)
    if name == "highest_digit":
        return (rng.integers(-128, 128, size=shape, dtype=np.int64) << 24).astype(np.int32)
    if name == "random":
        return rng.integers(I32.min, I32.max, size=shape, dtype=np.int64, endpoint=True).astype(np.int32)
    if name == "zero_heavy":
        return (rng.poisson(0.3, size=shape) * rng.integers(0, 3, size=shape)).astype(np.int32)
    raise KeyError(name)


FAMILIES = ("all_equal", "two_valued", "zeros_but_one", "extremes", "lowest_digit", "highest_digit", "random", "zero_heavy")


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, C - 1, C, C + 1, 2 * C + 1, 5000])
def test_pair_sums_equal_the_definition_at_the_chunk_and_round_edges(model, n):
    """One value; one pair; 255 / 256 / 257 (a round of the block); one short of, exactly and one past a chunk (no cross
    phase / the first cross phase of one value); three chunks; a 5000-draw cell.  Every family, two cells each."""
    rng = np.random.default_rng(n)
    for fam in FAMILIES:
        x = _family(rng, fam, (2, n))
        got = model.pair_abs_sums(x, cells=2)
        assert got.dtype == np.int64 and np.array_equal(got, V.pair_sum(x)), fam


@pytest.mark.parametrize("segs", [1, 3, 8])
@pytest.mark.parametrize("cells", [1, 2, 700])
def test_segments_a_stride_apart_and_many_cells(model, segs, cells):
    """The pooled addressing: `segs` runs of seg_len values seg_stride apart, cells cell_stride apart, as a draw store lays
    them out ([seg][cell][cap] with cap > seg_len: the gaps hold values that must not be read)."""
    rng = np.random.default_rng([segs, cells])
    seg_len, cap = (700, 720) if cells < 700 else (37, 40)
    store = _family(rng, "random", (segs, cells, cap))
    for fam, c in (("zero_heavy", 0), ("extremes", cells - 1)):
        store[:, c, :seg_len] = _family(rng, fam, (segs, seg_len))
    got = model.pair_abs_sums(store, cells=cells, segs=segs, seg_len=seg_len, seg_stride=cells * cap, cell_stride=cap)
    want = V.pair_sum(np.moveaxis(store[:, :, :seg_len], 0, 1).reshape(cells, segs * seg_len))
    assert np.array_equal(got, want)


def test_the_largest_cell_is_exact_and_one_past_it_is_refused(model):
    """Half INT32_MIN and half INT32_MAX at n = 92 681: D = floor(n/2) ceil(n/2) (2^32 - 1), the largest value there is,
    against Python integers; n + 1 is refused."""
    n = _lib.PAIR_ABS_MAX_N
    x = np.full(n, I32.min, np.int32)
    x[::2] = I32.max
    want = (n // 2) * (n - n // 2) * (2 ** 32 - 1)
    assert want < 2 ** 63 and ((n + 1) ** 2 // 4) * (2 ** 32 - 1) >= 2 ** 63
    assert int(model.pair_abs_sums(x)[0]) == want
    assert int(model.pair_abs_sums(x, segs=7, seg_len=n // 7)[0]) == V.pair_sum(x[:n // 7 * 7])
    with pytest.raises(_lib.SeirError, match="2\\^63") as e:
        model.pair_abs_sums(np.zeros(n + 1, np.int32))
    assert e.value.code == _lib.ERR_INVALID


def test_pair_sums_do_not_depend_on_workgroup_timing(api):
    case = H.build_case("micro_3x1", 43)
    rng = np.random.default_rng(3)
    x = _family(rng, "random", (5, 2 * C + 17))
    want = V.pair_sum(x)
    for skew in (1, 2, 3):
        with api[0](case["cov"], case["init"], max_chains=1) as m:
            m.set_option(debug_skew=skew)
            assert np.array_equal(m.pair_abs_sums(x, cells=5), want)


def test_pair_sum_refusals(model):
    x = np.zeros(12, np.int32)
    with pytest.raises(ValueError, match="do not lie within"):
        model.pair_abs_sums(x, cells=2, seg_len=7)
    with pytest.raises(ValueError, match="do not lie within"):
        model.pair_abs_sums(x, cells=0)
    ip = _lib.ctypes.POINTER(_lib.ctypes.c_int32)
    out, flag = np.zeros(4, np.int64), _lib.ctypes.c_uint32(0)

    def call(ctx, values, cells, segs, seg_len, seg_stride, cell_stride, o=out):
        return model._lib.seir_pair_abs_sums(ctx, values, cells, segs, seg_len, seg_stride, cell_stride,
                                             None if o is None else o.ctypes.data_as(_lib.c_int64_p), _lib.ctypes.byref(flag))
    p = x.ctypes.data_as(ip)
    assert call(None, p, 1, 1, 12, 12, 12) != 0                          # a null handle
    for args, word in (((None, 1, 1, 12, 12, 12), "null pointer"), ((p, 0, 1, 12, 12, 12), "at least one"),
                       ((p, 1, 0, 12, 12, 12), "at least one"), ((p, 1, 1, 0, 12, 12), "at least one"),
                       ((p, 1, 1, 12, -1, 12), "negative stride"), ((p, 1, 2, 6, 5, 12), "do not overlap")):
        assert call(model._ctx, *args) == _lib.ERR_INVALID
        assert word in model._lib.seir_last_error().decode(), word
    assert call(model._ctx, p, 1, 1, 12, 12, 12, o=None) == _lib.ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------------
# riding on the sampler's forecast
# ---------------------------------------------------------------------------------------------------------------------
def _truth(sim, rng, knock=True):
    """truth [M, H] from draw 0 of chain 0: a third of the cells one above, a third one below (not below zero); with `knock`
    the last day missing everywhere (a partial horizon), single cells missing, and a gap in the middle of row 0."""
    t = sim[0, 0, :, :, 2].astype(np.int64)
    t = np.maximum(t + rng.integers(-1, 2, size=t.shape), 0).astype(np.int32)
    M, Hn = t.shape
    if knock and Hn > 2:
        t[:, -1] = -1
        t[0, Hn // 2] = -1
        t[rng.random(t.shape) < 0.05] = -1
    return t


def _holds(s, sim, truth, store=True):
    """The accumulators, and with the store the pair sums per chain and pooled, against NumPy on the simulated planes."""
    n, B = sim.shape[:2]
    y, valid = V.truth_targets(truth)
    x = V.targets(sim)                                       # [n, B, M, H, 2]
    got = s.verify_summary()
    assert np.array_equal(got["count"], np.full(B, n, np.uint64))
    for b in range(B):
        want = V.fold(x[:, b], y, valid)
        for k in ("lt", "eq", "abs_sum"):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k][b], want[k]), (b, k)
    if store:
        per = s.forecast_pair_sums()
        assert per.shape == (B, 2) + truth.shape and per.dtype == np.int64
        assert np.array_equal(per, np.moveaxis(V.pair_sum(np.moveaxis(x, 0, -1)), -1, 1))
        pooled = s.forecast_pair_sums(pooled=True)
        assert np.array_equal(pooled, np.moveaxis(V.pair_sum(np.moveaxis(x.reshape((n * B,) + x.shape[2:]), 0, -1)), -1, 0))
    return got


# name, cfg, eps, B, record, n, H: the shapes of tests/test_forecast_quantiles_gpu.py
VERIFY_CASES = {
    "M=1,H=1": ("micro_1x70", CFG_SMALL, 0.002, 3, "u16", 6, 1),
    "T=1,H=7": ("micro_3x1", CFG_SMALL, 0.002, 1, True, 4, 7),
    "9x64,H=64": ("micro_9x64", CFG_SMALL, 0.0004, 3, "u16", 5, 64),
    "9x64,H=65,B=8": ("micro_9x64", CFG_SMALL, 0.0004, 8, True, 4, 65),
    "M=65,H=7": ("micro_65x70", CFG_SMALL, 0.0001, 1, "u16", 9, 7),
    "M=520,H=128": ("slow_520x70", CFG_SMALL, 3e-5, 2, True, 3, 128),
    "uk380x8,12,H=14": ("uk380", CFG_REF, 1.2e-5, 8, "u16", 12, 14),
}


@pytest.mark.parametrize("case_id", list(VERIFY_CASES))
def test_the_fold_and_the_pair_sums_equal_numpy_on_the_recorded_draws(api, case_id):
    """The run forecasts its recorded draws once to learn the simulated planes, then again from a reset with the truth set:
    the same draw ids, the same counts.  Cells with draws below, at and above the truth each occur wherever there is more than
    a handful of cells (M = 1, H = 1 is one cell of six draws: it is there for the indexing)."""
    name, cfg, eps, B, record, n, Hn = VERIFY_CASES[case_id]
    case = H.build_case(name, 43, alpha_t_sd=0.005)
    u = synth.jitter_params(case["u"], B, scale=0.002 if name == "uk380" else 0.01, seed=3, T=case["k"].T)
    ev = np.stack([case["events"]] * B)
    model, s = _sampler(api, case, cfg, u, ev, eps, n, record_events=record)
    with model, s:
        FG._reset(s, case, Hn)
        tr = s.sample(n, forecast=True)
        sim = FG._oracle(model, case, tr.theta, tr.events, Hn)["sim"]
        truth = _truth(sim, np.random.default_rng(7))
        FG._reset(s, case, Hn)
        s.keep_forecast_draws(n)
        s.set_verify(truth)
        assert s.verify_state() == dict(on=True, H=Hn, j=0, store=True)
        s.forecast(0, n)
        assert s.verify_state()["j"] == n
        got = _holds(s, sim, truth)
        lt, eq = got["lt"].astype(np.int64), got["eq"].astype(np.int64)
        _, valid = V.truth_targets(truth)
        gt = np.where(valid, n - lt - eq, 0)
        print("cells with draws below / at / above:", (lt > 0).sum(), (eq > 0).sum(), (gt > 0).sum())
        if truth.size >= 7:
            assert (lt > 0).any() and (eq > 0).any() and (gt > 0).any()
        assert not lt[:, ~valid].any() and not eq[:, ~valid].any() and not got["abs_sum"][:, ~valid].any()
        assert not s.pair_timeouts().any()


def test_cuts_batches_resets_and_refusals(api):
    """Two calls in the buffer's halves, one call, uneven calls: the same integers.  A second reset empties and keeps the
    truth; another horizon frees it; None turns it off; a set without a forecast or behind the first forecast is refused."""
    case, u, ev, cfg, eps = _case("micro_20x60", 3)
    n, Hn = 11, 9
    model, s = _sampler(api, case, cfg, u, ev, eps, 2 * n)
    with model, s:
        off = dict(on=False, H=0, j=0, store=False)
        assert s.verify_state() == off
        with pytest.raises(_lib.SeirError, match="seir_sampler_forecast_reset") as e:
            s.set_verify(np.zeros((case["k"].M, Hn), np.int32))
        assert e.value.code == _lib.ERR_STATE
        FG._reset(s, case, Hn)
        for first in (0, n):
            s.reset_trace(at=first)
            s.run(n)
            s.forecast(first, n)
        tr = s.read_trace(2 * n)
        sim = FG._oracle(model, case, tr.theta, tr.events, Hn)["sim"]
        truth = _truth(sim, np.random.default_rng(1))
        with pytest.raises(_lib.SeirError, match="first seir_sampler_forecast") as e:
            s.set_verify(truth)
        assert e.value.code == _lib.ERR_STATE and s.verify_state() == off
        with pytest.raises(ValueError, match="need integers"):
            s.set_verify(truth[:, :-1])
        with pytest.raises(ValueError, match="need integers"):
            s.set_verify(truth.astype(np.float64))
        FG._reset(s, case, Hn)
        s.keep_forecast_draws(2 * n)
        s.set_verify(truth)
        want = None
        for cuts in (((0, 2 * n),), ((0, n), (n, n)), ((0, 3), (3, 1), (4, 9), (13, 2 * n - 13))):
            for first, count in cuts:
                s.forecast(first, count)
            got = _holds(s, sim, truth)
            want = want or got
            for k in ("lt", "eq", "abs_sum"):
                assert np.array_equal(got[k], want[k]), k
            FG._reset(s, case, Hn)                             # empties, keeps the truth
            assert s.verify_state() == dict(on=True, H=Hn, j=0, store=True)
            assert not any(s.verify_summary()[k].any() for k in ("lt", "eq", "abs_sum", "count"))
        assert want["abs_sum"].any() and want["lt"].any()
        FG._reset(s, case, Hn + 1)                             # another horizon frees it
        assert s.verify_state() == off
        with pytest.raises(_lib.SeirError, match="no truth is set") as e:
            s.verify_summary()
        assert e.value.code == _lib.ERR_STATE
        FG._reset(s, case, Hn)
        s.set_verify(truth)
        s.set_verify(None)
        assert s.verify_state() == off
        with pytest.raises(_lib.SeirError, match="draw store is not enabled"):
            s.forecast_pair_sums()
        assert not s.pair_timeouts().any()


def test_a_call_of_two_host_batches_and_workgroup_skew(api):
    """130 slots: two batches of the host's cut.  The same integers under every debug skew."""
    case, u, ev, cfg, eps = _case("micro_5x24", 2)
    n, Hn = 130, 3
    res = {}
    truth = None
    for skew in (0, 1, 2, 3):
        model, s = _sampler(api, case, cfg, u, ev, 0.002, n, skew=skew)
        with model, s:
            FG._reset(s, case, Hn)
            tr = s.sample(n, forecast=True)
            if skew == 0:
                sim = FG._oracle(model, case, tr.theta, tr.events, Hn)["sim"]
                truth = _truth(sim, np.random.default_rng(2), knock=False)
            FG._reset(s, case, Hn)
            s.keep_forecast_draws(n)
            s.set_verify(truth)
            s.forecast(0, n)
            if skew == 0:
                _holds(s, sim, truth)
            res[skew] = (s.verify_summary(), s.forecast_pair_sums(), s.forecast_pair_sums(pooled=True), tr.events)
    for skew in (1, 2, 3):
        assert np.array_equal(res[skew][3], res[0][3])
        for k in ("lt", "eq", "abs_sum"):
            assert np.array_equal(res[skew][0][k], res[0][0][k]), (skew, k)
        assert np.array_equal(res[skew][1], res[0][1]) and np.array_equal(res[skew][2], res[0][2])


def test_a_burst_run_again_after_a_time_out_is_counted_once(api):
    """tests/test_forecast_gpu.py's disturbance (the existing hook, once) with the truth set: the re-run burst is counted once."""
    case, u, ev, cfg, eps = _case("micro_20x60", 8)
    B, nb, burst, Hn = 8, 6, 4, 5
    model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
    with model, s:
        got = {}
        FG._reset(s, case, Hn)
        s.keep_forecast_draws(nb * burst)
        truth = np.full((case["k"].M, Hn), 1, np.int32)
        truth[3, 2] = -1
        s.set_verify(truth)

        def consume(tr, i):
            got[i] = (tr.events.copy(), tr.theta.copy())
            if i == 1 and not s.recoveries:
                _lib.check(s._lib.seir_sampler_debug_fail_handoff(s._s, B - 1))
        s.sample_bursts(nb, burst, consume, forecast=True)
        assert len(s.recoveries) == 1 and sorted(got) == list(range(nb))
        theta, events = np.concatenate([got[i][1] for i in range(nb)]), np.concatenate([got[i][0] for i in range(nb)])
        sim = FG._oracle(model, case, theta, events, Hn)["sim"]
        _holds(s, sim, truth)


def test_nothing_else_notices_the_truth(api):
    """The chain, the summaries, the forecast's moments, marginals, draw store and quantiles: bit for bit those of the same
    run without a truth."""
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    nb, burst, Hn = 3, 5, 6
    runs = {}
    for on in (False, True):
        model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
        with model, s:
            got = {}
            FG._reset(s, case, Hn)
            s.keep_forecast_draws(nb * burst)
            if on:
                s.set_verify(np.full((case["k"].M, Hn), 2, np.int32))

            def consume(tr, i, got=got):
                got[i] = (tr.theta.copy(), tr.events.copy(), {k: v.copy() for k, v in tr.marginals.items()},
                          {k: v.copy() for k, v in tr.forecast.items()})
            s.sample_bursts(nb, burst, consume, summarize=True, forecast=True)
            runs[on] = (got, s.get_state() + s.get_kernel(), s.summary(), s.forecast_summary(),
                        s.forecast_order_stats([0, nb * burst - 1]), s.forecast_quantiles([0.05, 0.5, 0.95], pooled=True))
            if on:
                assert s.verify_summary()["abs_sum"].any()
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


def test_a_block_above_half_of_the_free_memory_is_refused_and_the_forecast_runs_on_unscored(api, monkeypatch):
    """The accumulators are 32 B per cell: no device refuses them, and a test that held the rest of a device's memory would take
    it from whoever shares the device.  The library's hook caps the free figure its policy sees instead (csrc/dev_mem.h):
    with 64 KiB "free" the block of 3 chains x 20 locations x 9 days is above half of it.  The refusal clears what was in
    force, the forecast completes as the forecast it is without a truth, and with the hook gone the set is accepted again."""
    case, u, ev, cfg, eps = _case("micro_20x60", 3)
    n, Hn = 5, 9
    truth = np.full((case["k"].M, Hn), 1, np.int32)
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        FG._reset(s, case, Hn)
        s.set_verify(truth)
        assert s.verify_state()["on"]
        monkeypatch.setenv("SEIR_DEBUG_FREE_BYTES", str(64 * 1024))
        with pytest.raises(_lib.SeirError, match=r"the verification needs \d+ bytes .* more than half of the 65536 bytes free") as e:
            s.set_verify(truth)
        assert e.value.code == _lib.ERR_INVALID and s.verify_state() == dict(on=False, H=0, j=0, store=False)
        tr = s.sample(n, forecast=True)                        # the forecast runs on, unscored
        want = FG._oracle(model, case, tr.theta, tr.events, Hn)
        FG._same_moments(s.forecast_summary(), want)
        FG._same_marginals(tr.forecast, want)
        with pytest.raises(_lib.SeirError, match="no truth is set"):
            s.verify_summary()
        monkeypatch.delenv("SEIR_DEBUG_FREE_BYTES")
        FG._reset(s, case, Hn)
        s.set_verify(truth)
        s.forecast(0, n)
        _holds(s, want["sim"], truth, store=False)
        s.set_verify(None)
    # turning it off needs no forecast
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        s.set_verify(None)
        assert s.verify_state() == dict(on=False, H=0, j=0, store=False)


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


def test_no_other_product_notices_the_truth(api):
    """Every product on at once -- summaries, the forecast with its draw store, its group sums and two scenarios, R_t, the check,
    within / between, the group sums of all three sources and both group curves -- with and without the truth: every field of
    every burst's trace and every product's accumulators bit for bit, the scenarios' among them.  The fold is launched in the
    forecast's hook right behind the scenarios' batch, on the same staging tensor."""
    from covid19uk_amd.inference import inference as inf
    from covid19uk_amd.posterior import groups as G
    from covid19uk_amd.posterior import predict
    from covid19uk_amd.posterior import scenarios as SC
    from covid19uk_amd.sampler import Trace
    case, u, ev, cfg, eps = _case("micro_20x60", 3)
    B, nb, burst, Hn, K, D = 3, 3, 4, 6, 5, 4
    cov, T, M = case["cov"], case["k"].T, case["k"].M
    N = np.asarray(cov.N, np.float64).reshape(-1)
    tab = G.parse_groups({"all": list(range(M)), "low": list(range(0, M, 2)), "one": [M - 1]}, M)
    sc = SC.parse_scenarios(dict(a=dict(transmission=0.5), b=dict(commute=0.0, from_day=2)), Hn)
    truth = np.full((M, Hn), 1, np.int32)
    truth[5, 2] = truth[0, Hn - 1] = -1
    kw = dict(summarize=True, forecast=inf.forecast_steps_fn(7, list(range(B)), Hn), rt=True, check=True, within_between=True, groups=True)
    fields = tuple(f for f in Trace.__dataclass_fields__ if f not in ("hmc", "moves"))
    runs = {}
    for on in (False, True):
        model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
        with model, s:
            s.set_groups(tab.offsets, tab.members)
            s.set_group_rt(G.rt_weights(tab, N))
            s.set_group_within_between(True)
            s.reset_forecast(Hn, *predict.forecast_calendar(cov, None, T, Hn), 5)
            s.keep_forecast_draws(nb * burst)
            s.set_scenarios(sc.log_shift, sc.commute, nb * burst)
            if on:
                s.set_verify(truth)
            s.reset_check(K, *predict.check_calendar(cov, None, T, K), 6)
            s.reset_rt(D, N / N.sum())
            s.reset_within_between(D)
            got = {}

            def consume(tr, i, got=got):
                got[i] = {f: ({k: np.array(a) for k, a in getattr(tr, f).items()} if isinstance(getattr(tr, f), dict)
                              else np.array(getattr(tr, f))) for f in fields if getattr(tr, f) is not None}
            s.sample_bursts(nb, burst, consume, **kw)
            scen = dict(diffs={k: v for k, v in s.scenario_diffs().items() if k != "count"}, draws=s.read_scenario_draws(),
                        moments={str(k): dict(count=m.count, ref=m.ref, sum=m.sum, sumsq=m.sumsq) for k, m in enumerate(s.scenario_summary())})
            runs[on] = (got, _flat(dict(summary=s.summary(), forecast=s.forecast_summary(), rt=s.rt_summary(), check=s.check_summary(),
                                        wb=s.within_between_summary(), scenarios=scen,
                                        store=dict(order=s.forecast_order_stats([0, nb * burst - 1]),
                                                   q=s.forecast_quantiles([0.05, 0.5, 0.95], pooled=True)))), s.get_state())
            if on:
                acc = s.verify_summary()
                assert s.verify_state()["j"] == nb * burst and acc["abs_sum"].any() and not acc["abs_sum"][:, 5, 2].any()
    a, b = runs[False], runs[True]
    for i in range(nb):
        assert set(a[0][i]) == set(b[0][i]) >= {"theta", "events", "marginals", "forecast", "rt", "check", "wb", "groups", "group_curves"}
        for f in a[0][i]:
            for k, v in _flat({f: a[0][i][f]}).items():
                assert np.array_equal(v, _flat({f: b[0][i][f]})[k], equal_nan=True), (i, k)
    assert set(a[1]) == set(b[1]) and any(k.startswith("scenarios.diffs.") for k in a[1]) and any(k.startswith("wb.") for k in a[1])
    for k in a[1]:
        assert np.array_equal(a[1][k], b[1][k], equal_nan=True), k
    for x, y in zip(a[2], b[2]):
        assert np.array_equal(x, y)


def test_repeated_runs_chain_sharding_and_thinning(api):
    """The same run twice gives the same integers.  Chains 2 and 3 of a 4-chain sampler against a 2-chain sampler created with
    first_chain_id = 2, held to the oracle with chain0 = 2.  With thin = 3 the scores are those of the kept draws."""
    case, u, ev, cfg, eps = _case("micro_20x60", 4)
    n, Hn = 5, 8
    truth = np.full((case["k"].M, Hn), 1, np.int32)
    truth[4, 3] = truth[7, 0] = -1
    truth[::3] += 1

    def live(s, **kw):
        FG._reset(s, case, Hn)
        s.keep_forecast_draws(n)
        s.set_verify(truth)
        tr = s.sample(n, forecast=True, **kw)
        return tr, s.verify_summary(), s.forecast_pair_sums(), s.forecast_pair_sums(pooled=True)
    res = []
    for rep in range(2):
        model, s = _sampler(api, case, cfg, u, ev, eps, n)
        with model, s:
            res.append(live(s))
    tr4, acc4, per4, _ = res[0]
    assert np.array_equal(res[1][0].events, tr4.events) and np.array_equal(res[1][2], per4) and np.array_equal(res[1][3], res[0][3])
    for k in ("lt", "eq", "abs_sum"):
        assert np.array_equal(res[1][1][k], acc4[k]), k
    model, s = _sampler(api, case, cfg, u[2:], ev[2:], eps, n, first_chain_id=2)
    with model, s:
        tr2, acc2, per2, _ = live(s)
        assert np.array_equal(tr4.events[:, 2:], tr2.events)
        _holds(s, FG._oracle(model, case, tr2.theta, tr2.events, Hn, chain0=2)["sim"], truth)
    assert acc2["abs_sum"].any() and np.array_equal(per4[2:], per2)
    for k in ("lt", "eq", "abs_sum"):
        assert np.array_equal(acc4[k][2:], acc2[k]), k
    k = 3
    model, s = _sampler(api, case, cfg, u, ev, eps, n, thin=k)
    with model, s:
        kept, acc, per, pooled = live(s)
    model, s = _sampler(api, case, cfg, u, ev, eps, n * k)
    with model, s:
        every = s.sample(n * k)
        assert np.array_equal(every.events[k - 1::k], kept.events)
        x = V.targets(FG._oracle(model, case, every.theta[k - 1::k], every.events[k - 1::k], Hn)["sim"])
    y, valid = V.truth_targets(truth)
    for b in range(x.shape[1]):
        want = V.fold(x[:, b], y, valid)
        for key in ("lt", "eq", "abs_sum"):
            assert np.array_equal(acc[key][b], want[key]), (b, key)
    assert np.array_equal(per, np.moveaxis(V.pair_sum(np.moveaxis(x, 0, -1)), -1, 1))
    assert np.array_equal(pooled, np.moveaxis(V.pair_sum(np.moveaxis(x.reshape((-1,) + x.shape[2:]), 0, -1)), -1, 0))


def test_the_command_lines_with_verify(api, tmp_path):
    """The inference command line on NI-11, two chains, with --forecast 14 --forecast-quantiles 0.05,0.5,0.95 --verify FILE (a
    later file: the fitted days and ten more, one cell missing), and the replay command line on its two files with the same flags:
    every verify/* dataset equal.  Both command lines without the flag write every other dataset as with it."""
    import os

    import yaml
    from covid19uk_amd.inference import inference as inf
    from tests.test_replay_gpu import _run
    from tests.test_summary_gpu import _datasets
    tmp = str(tmp_path)
    cov = synth.make_covariates("ni11")
    events, _, _ = synth.simulate_epidemic(cov)
    cases = events[..., 2]
    M, T = cases.shape
    data, later = os.path.join(tmp, "data.h5"), os.path.join(tmp, "later.h5")
    inf.write_inference_data(data, cov, cases)
    more = 10
    rng = np.random.default_rng(3)
    lc = np.concatenate([cases, rng.poisson(np.maximum(cases[:, -more:].mean(axis=1, keepdims=True), 0.5), size=(M, more))], axis=1).astype(float)
    lc[2, T + 4] = np.nan
    lc[0, 3] += 1                                            # a revised cell of the fitted days: logged, not refused
    import dataclasses
    cov2 = dataclasses.replace(cov, W=np.concatenate([cov.W, cov.W[-more:]]), weekday=np.concatenate([cov.weekday, cov.weekday[-more:]]))
    inf.write_inference_data(later, cov2, lc)
    cfg = os.path.join(tmp, "config.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump(dict(Mcmc=dict(dmax=84, nmax=25, m=2, occult_nmax=15, num_event_time_updates=5, num_bursts=2,
                                      num_burst_samples=6, thin=1)), f)
    gpath = os.path.join(tmp, "groups.yaml")
    with open(gpath, "w") as f:
        yaml.safe_dump({"north": list(range(5)), "rest": list(range(5, M)), "third": [2]}, f, sort_keys=False)
    flags = ["--forecast", "14", "--forecast-quantiles", "0.05,0.5,0.95", "--groups", gpath]
    outs = {}
    for tag, extra in (("with", flags + ["--verify", later]), ("without", flags)):
        out = os.path.join(tmp, f"{tag}.h5")
        log = _run("covid19uk_amd.inference.inference", ["-c", cfg, "-o", out, "--seed", "4", "--chains", "2", data] + extra, tmp)
        assert ("Verify: national cumulative cases to forecast day 4:" in log and "1 cell(s) of the" in log) == (tag == "with")
        files = [inf.chain_file_name(out, c, 2) for c in range(2)]
        rout = os.path.join(tmp, f"{tag}_replay.h5")
        rlog = _run("covid19uk.posterior.replay", ["-c", cfg, "-o", rout, "--seed", "4", data] + files + extra, tmp)
        assert ("Verify: national" in rlog) == (tag == "with")
        outs[tag] = ([_datasets(f) for f in files], [_datasets(inf.chain_file_name(rout, c, 2)) for c in range(2)])
    for c in range(2):
        live, rep = outs["with"][0][c], outs["with"][1][c]
        plain, prep = outs["without"][0][c], outs["without"][1][c]
        new = {k for k in live if k.startswith("verify/")}
        assert {"verify/truth", "verify/valid", "verify/lt", "verify/abs_sum", "verify/pit", "verify/crps", "verify/pooled_crps",
                "verify/national_crps", "verify/coverage", "verify/pooled_coverage", "verify/group_truth", "verify/group_valid",
                "verify/group_pit", "verify/group_crps"} <= new and len(new) == 36
        assert set(plain) == set(live) - new and set(prep) == set(rep) - new
        for k in plain:
            assert plain[k].tobytes() == live[k].tobytes(), k
        for k in prep:
            if k != "replay/source":
                assert prep[k].tobytes() == rep[k].tobytes(), k
        for k in new:                                           # the replay re-creates the forecast bit for bit: the same scores
            assert live[k].tobytes() == rep[k].tobytes(), k
        truth = live["verify/truth"]
        assert truth.shape == (M, 14) and (truth[:, more:] == -1).all() and truth[2, 4] == -1 and (truth[:, :4] >= 0).all()
        assert np.isfinite(live["verify/crps"][:, :4]).all() and np.isnan(live["verify/crps"][2, 4:, 1]).all()
        assert (live["verify/crps"][np.isfinite(live["verify/crps"])] >= 0).all()
        # the groups' scores: the truth summed over the members where every member is observed, the draws samples/forecast_by_group
        tt = truth.astype(np.int64)
        want_t = np.stack([np.where((tt[r] >= 0).all(0), np.where(tt[r] >= 0, tt[r], 0).sum(0), -1) for r in (range(5), range(5, M), [2])])
        assert np.array_equal(live["verify/group_truth"], want_t) and want_t[0, 4] == -1 and want_t[2, 4] == -1 and want_t[1, 4] >= 0
        yg, vg = V.truth_targets(want_t)
        grp = V.score_draws(V.targets(live["samples/forecast_by_group"]), yg, vg)
        for k in ("lt", "eq", "abs_sum", "pair_sum", "pit", "mae", "crps"):
            assert np.array_equal(live[f"verify/group_{k}"], grp[k], equal_nan=True), k
        # the one-member group is its location
        assert np.array_equal(live["verify/group_abs_sum"][2], live["verify/abs_sum"][2])

"""Host side of the forecast on the device (include/seir_hip.h, "Forecast on the device"): the symbols, the configuration
and the command line, run_mcmc's call sequence with a stub sampler, the calendar helper against what `predict` builds,
the draw-id rule, the datasets written, and the compiler's account of the new kernels.  No GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from covid19uk_amd import _lib, hdf5io, model_spec
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.posterior import predict
from covid19uk_amd.sampler import FORECAST_KEYS, Summary, forecast_draw_id
from tests import helpers as H
from tests.abi_lib import check_symbols
from tests.test_summary_host import CFG, StubSampler, _read

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARG3 = "int64_t *forecast_by_day, int64_t *forecast_by_location, int64_t *forecast_state_by_day"
NEW = {
    "seir_sampler_forecast_reset": "seir_sampler *s, int32_t horizon, const double *W, const double *weekday_c, uint64_t seed",
    "seir_sampler_forecast": "seir_sampler *s, int32_t first_slot, int32_t count, const double *log_baseline_steps",
    "seir_sampler_read_forecast_marginals": "seir_sampler *s, int32_t first, int32_t count, " + MARG3,
    "seir_sampler_read_forecast_marginals_async": "seir_sampler *s, int32_t first, int32_t count, " + MARG3,
    "seir_sampler_read_forecast": "seir_sampler *s, uint64_t *count, int32_t *ref, int64_t *sum, uint64_t *sumsq",
}


# ---- 1. the symbols ------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound_with_the_headers_types():
    lib = check_symbols(NEW)
    raw = open(os.path.join(ROOT, "include", "seir_hip.h")).read()
    assert int(re.search(r"#define SEIR_FORECAST_MAX_H (\d+)", raw).group(1)) == _lib.FORECAST_MAX_H == 128
    # a null sampler is refused before anything touches a device
    one = (ctypes.c_double * 1)(0.0)
    assert lib.seir_sampler_forecast_reset(None, 5, one, one, 0) == _lib.ERR_INVALID
    assert lib.seir_sampler_forecast(None, 0, 1, None) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_forecast_marginals(None, 0, 1, None, None, None) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_forecast_marginals_async(None, 0, 1, None, None, None) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_forecast(None, None, None, None, None) == _lib.ERR_INVALID


# ---- 2. configuration and command line -----------------------------------------------------------------------------------
def test_forecast_value_is_parsed_and_bad_ones_refused_before_any_gpu_call(tmp_path):
    assert inf.forecast_mode({}) == (0, False)
    assert inf.forecast_mode(dict(CFG, forecast=14)) == (14, False)
    assert inf.forecast_mode(dict(CFG, forecast=14, forecast_walk="on")) == (14, True)
    assert inf.forecast_mode(dict(CFG, forecast=14, forecast_walk=True), 7) == (7, True)      # the command line overrides
    assert inf.forecast_mode(CFG, 1, True) == (1, True) and inf.forecast_mode(CFG, 128) == (128, False)
    assert inf.forecast_mode(dict(CFG, forecast="off")) == (0, False) and inf.forecast_mode(dict(CFG, forecast="28")) == (28, False)
    for bad in (0, 129, -3, "soon", True, 2.5):
        with pytest.raises(ValueError, match="forecast"):
            inf.forecast_mode(dict(CFG, forecast=bad))
    for cfg, kw in ((dict(CFG, forecast_walk="on"), {}), (CFG, dict(walk=True)), (dict(CFG, forecast="off"), dict(walk=True))):
        with pytest.raises(ValueError, match="no effect"):                      # a walk with nothing to walk is not dropped in silence
            inf.forecast_mode(cfg, **kw)
    # mcmc() refuses all of it before it reads the data file or opens a device: the file named here does not exist
    nofile, out = str(tmp_path / "no_such_file.nc"), str(tmp_path / "out.hd5")
    with pytest.raises(ValueError, match="forecast"):
        inf.mcmc(nofile, out, dict(CFG, forecast=0))
    with pytest.raises(ValueError, match="forecast"):
        inf.mcmc(nofile, out, CFG, forecast=129)
    with pytest.raises(ValueError, match="no effect"):
        inf.mcmc(nofile, out, CFG, forecast_walk=True)
    assert not os.path.exists(out)


def test_the_cli_flags_parse(tmp_path, monkeypatch):
    import yaml
    cpath = str(tmp_path / "c.yaml")
    with open(cpath, "w") as f:
        yaml.safe_dump(dict(Mcmc=CFG), f)
    seen = {}
    monkeypatch.setattr(inf, "mcmc", lambda *a, **kw: seen.update(kw))
    inf.main(["-c", cpath, "-o", "x", "--forecast", "14", "--forecast-walk", "data.nc"])
    assert seen["forecast"] == 14 and seen["forecast_walk"] is True
    inf.main(["-c", cpath, "-o", "x", "data.nc"])
    assert seen["forecast"] is None and seen["forecast_walk"] is None
    with pytest.raises(SystemExit):
        inf.main(["-c", cpath, "-o", "x", "--forecast", "soon", "data.nc"])


# ---- 3. the calendar helper and the draw id --------------------------------------------------------------------------------
@pytest.mark.parametrize("dates", [["2020-10-%02d" % d for d in range(1, 12)], None])
def test_the_calendar_is_what_predict_builds_for_initial_step_T(dates):
    """Weekday by date, and the fallback without dates: predict() replaces the covariate's weekday by
    prediction_weekday(dates, initial_step + num_steps, ...) and predicted_incidence centres and clips it."""
    T, Hn, M = 11, 9, 2
    rng = np.random.default_rng(1)
    cov = model_spec.Covariates(C=np.zeros((M, M)), W=rng.uniform(0.5, 1.5, T), N=np.ones(M), adjacency=np.zeros((M, M)),
                                weekday=(np.arange(T) % 7 < 5).astype(float), area=np.ones(M))
    W, wd = predict.forecast_calendar(cov, dates, T, Hn)
    weekday, days = predict.prediction_weekday(dates, T + Hn, cov.weekday)       # predict(), line by line
    assert (days is None) == (dates is None)
    want_wd = predict.clipped(weekday - weekday.mean(), T, Hn)
    want_W = predict.clipped(cov.W, T, Hn)
    assert W.shape == wd.shape == (Hn,) and np.array_equal(W, want_W) and np.array_equal(wd, want_wd)
    assert np.array_equal(W, np.full(Hn, cov.W[-1]))                             # the reference's clip
    if dates is not None:                                                        # 2020-10-12 was a Monday
        assert np.array_equal(wd + weekday.mean(), [1, 1, 1, 1, 1, 0, 0, 1, 1])
    else:
        assert np.array_equal(wd, np.full(Hn, cov.weekday[-1] - cov.weekday.mean()))
    # ... and predicted_incidence goes through the same helper
    W2, wd2 = predict.prediction_calendar(cov.W, weekday, T, Hn)
    assert np.array_equal(W2, W) and np.array_equal(wd2, wd)


def test_the_draw_id_rule_and_its_two_limits():
    assert forecast_draw_id(0, 0) == 0 and forecast_draw_id(3, 5) == (3 << 20) + 5
    assert forecast_draw_id(2047, (1 << 20) - 1) == 2 ** 31 - 1                  # the largest id fits seir_simulate's int32
    for c, j in ((2048, 0), (-1, 0), (0, 1 << 20), (0, -1)):
        with pytest.raises(ValueError):
            forecast_draw_id(c, j)
    assert _lib.FORECAST_ID_SHIFT == 20 and _lib.FORECAST_MAX_CHAIN == 2048
    # the steps of the walk are keyed the same way: by global chain id and draw number, not by the cut into bursts
    a = inf.forecast_steps_fn(9, [4, 5], 6)
    whole = a(0, 5)
    assert whole.shape == (5, 2, 6)
    assert np.array_equal(np.concatenate([a(0, 2), a(2, 3)]), whole)
    assert np.array_equal(inf.forecast_steps_fn(9, [5], 6)(3, 1)[0, 0], whole[3, 1])
    assert np.array_equal(whole[1, 0], np.random.default_rng([9, 4, 1]).normal(0.0, predict.ALPHA_T_SCALE, 6))
    assert predict.ALPHA_T_SCALE == 0.005


# ---- 4. run_mcmc with a stub sampler --------------------------------------------------------------------------------------
class ForecastStub(StubSampler):
    """StubSampler with the forecast: what is reset and forecast is recorded; a draw's forecast is its sweep number."""
    first_chain_id = 6

    def reset_forecast(self, horizon, W, weekday_c, seed):
        self.calls.append(("reset_forecast", horizon, np.asarray(W).copy(), np.asarray(weekday_c).copy(), seed))
        self.H, self.forecast_rows, self.steps = horizon, [], []

    def _trace(self, n, events=True, summarize=False, forecast=False):
        tr = super()._trace(n, events=events, summarize=summarize)
        if forecast:
            idx = self.sweeps - n + np.arange(n)
            self.calls.append(("forecast", n, len(self.forecast_rows)))
            if callable(forecast):
                self.steps.append(forecast(len(self.forecast_rows), n))
            self.forecast_rows.extend(idx)
            f = np.broadcast_to(idx[:, None, None, None], (n, self.B, self.H, 3)).astype(np.int64)
            tr.forecast = dict(forecast_by_day=f, forecast_by_location=np.broadcast_to(
                idx[:, None, None, None], (n, self.B, self.M, 3)).astype(np.int64), forecast_state_by_day=-f)
        return tr

    def forecast_summary(self):
        self.calls.append(("forecast_summary",))
        x = np.broadcast_to(np.asarray(self.forecast_rows, np.int64)[:, None, None, None, None],
                            (len(self.forecast_rows), self.B, self.M, self.H, 6))
        d = x - x[:1]
        return Summary(count=np.full(self.B, len(x), np.uint64), ref=x[0].astype(np.int32), sum=d.sum(axis=0),
                       sumsq=(d * d).sum(axis=0).astype(np.uint64))


def _run(tmp_path, tag, config, ext=".npz", cap=800, calendar=True):
    s = ForecastStub()
    s.cap = cap
    nb, ns = config["num_bursts"], config["num_burst_samples"]
    Hn, _ = inf.forecast_mode(config)
    names = [str(tmp_path / f"{tag}_{c}{ext}") for c in range(s.B)]
    kw = {} if config.get("summaries", "off") == "off" else dict(summaries=config["summaries"])
    if Hn:
        kw["forecast"] = (Hn, nb * ns)
    posts = [inf.Posterior(name, s.M, s.T, 2, inf.warmup_size() + nb * ns, **kw) for name in names]
    logname = str(tmp_path / f"{tag}.log")
    fkw = dict(forecast_calendar=(np.arange(Hn) + 0.5, np.arange(Hn) - 1.0), seed=21) if Hn and calendar else {}
    with open(logname, "w") as log:
        inf.run_mcmc(s, config, posts, log=log, **fkw)
    for p in posts:
        p.close()
    return s, [_read(n) for n in names], open(logname).read()


NEW_SETS = {"forecast/horizon", "forecast/first_day", "forecast/count", "forecast/seir_mean", "forecast/seir_var",
            "forecast/state_mean", "forecast/state_var"} | {f"samples/{k}" for k in FORECAST_KEYS}


def test_off_calls_nothing_new_and_writes_todays_datasets(tmp_path):
    s0 = StubSampler()                                        # a sampler that has never heard of the forecast
    posts = [inf.Posterior(str(tmp_path / f"ref_{c}.npz"), s0.M, s0.T, 2, inf.warmup_size() + 8) for c in range(2)]
    inf.run_mcmc(s0, CFG, posts, log=open(os.devnull, "w"))
    for p in posts:
        p.close()
    plain, pf, log = _run(tmp_path, "plain", CFG)
    assert plain.calls == s0.calls and "orecast" not in log
    assert not any(c[0] in ("reset_forecast", "forecast", "forecast_summary") for c in plain.calls)
    assert all(c[2] == {} for c in plain.calls if c[0] in ("sample", "burst"))
    ref = _read(str(tmp_path / "ref_1.npz"))
    assert set(pf[1]) == set(ref) and not (NEW_SETS & set(pf[1]))
    for k in ref:
        assert np.array_equal(pf[1][k], ref[k]), k
    with pytest.raises(ValueError, match="forecast_calendar"):
        _run(tmp_path, "nocal", dict(CFG, forecast=3), calendar=False)


@pytest.mark.parametrize("summaries,walk,overlap,ext", [("off", False, True, ".npz"), ("on", True, True, ".hd5"),
                                                        ("only", False, False, ".npz")])
def test_on_resets_once_forecasts_every_burst_and_writes_the_group(tmp_path, summaries, walk, overlap, ext):
    if ext == ".hd5" and not hdf5io.available():
        ext = ".npz"
    nb, ns, Hn = 3, 4, 5
    cfg = dict(CFG, num_bursts=nb, num_burst_samples=ns, summaries=summaries, forecast=Hn, **(dict(forecast_walk="on") if walk else {}))
    s, files, log = _run(tmp_path, "on", cfg, ext=ext, cap=800 if overlap else ns)
    names = [c[0] for c in s.calls]
    # reset once, after the last warm-up window and before the first burst; nothing during the warm-up
    assert names.count("reset_forecast") == 1 and names.count("forecast_summary") == 1
    r = names.index("reset_forecast")
    burst_name = "burst" if overlap else "sample"
    warm = [c for c in s.calls[:r] if c[0] == "sample"]
    assert len(warm) == 8 and all("forecast" not in c[2] for c in warm)
    assert not any(c[0] == "forecast" for c in s.calls[:r])
    reset = s.calls[r]
    assert reset[1] == Hn and np.array_equal(reset[2], np.arange(Hn) + 0.5) and np.array_equal(reset[3], np.arange(Hn) - 1.0) and reset[4] == 21
    # one forecast per burst, behind it (the stub records a burst, then what its kwargs made it do), j going on
    after = [c for c in s.calls[r:] if c[0] in (burst_name, "forecast")]
    assert [c[0] for c in after] == [burst_name, "forecast"] * nb
    assert [c[2] for c in after if c[0] == "forecast"] == [0, ns, 2 * ns]
    for c in after:
        if c[0] == burst_name:
            assert (callable(c[2]["forecast"]) if walk else c[2]["forecast"] is True)
            assert c[2].get("summarize", False) == (summaries != "off")
    if walk:                                                   # the steps: keyed by the stub's first_chain_id = 6
        got = np.concatenate(s.steps)
        assert got.shape == (nb * ns, s.B, Hn)
        assert np.array_equal(got[5, 1], np.random.default_rng([21, 7, 5]).normal(0.0, 0.005, Hn))
    # the files: today's datasets for this `summaries`, plus the group and the three per-draw datasets
    base, bf, _ = _run(tmp_path, "base", {k: v for k, v in cfg.items() if not k.startswith("forecast")}, ext=ext,
                       cap=800 if overlap else ns)
    w = inf.warmup_size()
    sweeps = w + np.arange(nb * ns)
    for c, f in enumerate(files):
        assert set(f) == set(bf[c]) | NEW_SETS
        for k in bf[c]:
            assert np.array_equal(f[k], bf[c][k], equal_nan=True), k
        assert f["samples/forecast_by_day"].shape == (nb * ns, Hn, 3) and f["samples/forecast_by_location"].shape == (nb * ns, s.M, 3)
        assert f["samples/forecast_state_by_day"].shape == (nb * ns, Hn, 3)
        for k in FORECAST_KEYS:
            assert f[f"samples/{k}"].dtype == np.int64
        assert np.array_equal(f["samples/forecast_by_day"][:, 0, 0], sweeps)      # one row per kept draw of the sampling phase
        assert np.array_equal(f["samples/forecast_state_by_day"][:, 2, 1], -sweeps)
        assert f["forecast/horizon"].reshape(-1)[0] == Hn and f["forecast/first_day"].reshape(-1)[0] == s.T
        assert f["forecast/count"].reshape(-1)[0] == nb * ns
        for k in ("seir_mean", "seir_var", "state_mean", "state_var"):
            assert f[f"forecast/{k}"].shape == (s.M, Hn, 3) and f[f"forecast/{k}"].dtype == np.float64
        np.testing.assert_allclose(f["forecast/seir_mean"], sweeps.mean(), rtol=1e-15)
        np.testing.assert_allclose(f["forecast/state_var"], sweeps.var(ddof=1), rtol=1e-13)
    assert log.count("Forecast:") == 1 and f"{Hn} day(s) from day {s.T}" in log


# ---- 5. the compiler's account of the new kernels -------------------------------------------------------------------------
def test_the_forecast_kernels_fit_and_contraction_and_fold_have_no_scratch():
    res = H.kernel_account("base")
    new = ["k_forecast_prepare<0>", "k_forecast_prepare<1>", "k_forecast_day", "k_forecast_fold", "k_forecast_finish"]
    assert all(k in res for k in new), sorted(res)
    for k in ("k_gemm<64>", "k_forecast_fold", "k_forecast_finish", "k_forecast_prepare<0>", "k_forecast_prepare<1>"):
        assert res[k]["scratch_bytes_per_lane"] == 0 and res[k]["vgpr_spill"] == 0, (k, res[k])
    # static + dynamic LDS at M = 1280, H = 128: no forecast launch's LDS depends on M or H (the draws of a batch bound
    # the fold's carries); the contraction asks for its two panels, 64 x (80 + 80) doubles
    dynamic = dict.fromkeys(new, 0)
    dynamic["k_gemm<64>"] = 64 * (80 + 80) * 8
    for k, dyn in dynamic.items():
        assert res[k]["lds_bytes_per_block"] + dyn <= 160 * 1024, (k, res[k])
    assert res["k_forecast_fold"]["lds_bytes_per_block"] == 16 * 64 * 3 * 8 + 8 * 128 * 3 * 4
    # k_simulate shares its per-cell expressions with k_forecast_day now; what it needs is what it needed
    parent = json.load(open(os.path.join(ROOT, "profiles", "r08_kernel_resources.json")))
    for k in ("scratch_bytes_per_lane", "lds_bytes_per_block", "vgpr_spill", "sgpr_spill", "occupancy_waves_per_simd"):
        assert res["k_simulate"][k] == parent["k_simulate"][k], k
    for k in ("k_summarize<0,0>", "k_summarize<1,0>", "k_summarize<0,1>", "k_summarize<1,1>", "k_gemm<64>"):
        assert res[k] == parent[k], k

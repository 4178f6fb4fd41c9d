"""Host side of the reproduction number on the device (include/seir_hip.h, "Reproduction number on the device"): the
symbols, the configuration and the command line, run_mcmc's call sequence with a stub sampler, ChainSampler's own order
of calls inside a burst, the host's formulas against exact rationals, the datasets written, and the compiler's account of
the new kernels.  No GPU."""
import ctypes
import json
import os
import warnings
from fractions import Fraction

import numpy as np
import pytest

from covid19uk_amd import _lib, hdf5io
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.sampler import ChainSampler, ProductState, RtSummary, Trace
from tests import helpers as H
from tests.abi_lib import check_symbols
from tests.test_forecast_host import ForecastStub
from tests.test_summary_host import CFG, StubSampler, _read

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "seir_sampler_rt_reset": "seir_sampler *s, int32_t days, const double *weight",
    "seir_sampler_rt": "seir_sampler *s, int32_t first_slot, int32_t count",
    "seir_sampler_read_rt_draws": "seir_sampler *s, int32_t first, int32_t count, double *R_t",
    "seir_sampler_read_rt_draws_async": "seir_sampler *s, int32_t first, int32_t count, double *R_t",
    "seir_sampler_read_rt": "seir_sampler *s, uint64_t *count, double *ref, double *sum, double *sumsq, uint32_t *gt1",
}


# ---- 1. the symbols ------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound_with_the_headers_types():
    lib = check_symbols(NEW)
    # a null sampler is refused before anything touches a device
    one = (ctypes.c_double * 1)(1.0)
    assert lib.seir_sampler_rt_reset(None, 1, one) == _lib.ERR_INVALID
    assert lib.seir_sampler_rt(None, 0, 1) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_rt_draws(None, 0, 1, one) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_rt_draws_async(None, 0, 1, one) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_rt(None, None, None, None, None, None) == _lib.ERR_INVALID


# ---- 2. configuration and command line -----------------------------------------------------------------------------------
def test_rt_value_is_parsed_and_bad_ones_refused_before_any_gpu_call(tmp_path):
    T = 5
    assert inf.rt_mode({}) == 0 and inf.rt_mode(CFG, T=T) == 0
    assert inf.rt_mode(dict(CFG, rt=3), T=T) == 3 and inf.rt_mode(dict(CFG, rt=3), 4, T=T) == 4      # the command line overrides
    assert inf.rt_mode(dict(CFG, rt=1), T=T) == 1 and inf.rt_mode(dict(CFG, rt=T), T=T) == T
    assert inf.rt_mode(dict(CFG, rt="off")) == 0 and inf.rt_mode(dict(CFG, rt="4"), T=T) == 4
    assert inf.rt_mode(dict(CFG, rt=400)) == 400                               # without T only the lower end can be held
    for bad in (0, T + 1, -2, 2.5, "soon", True):
        with pytest.raises(ValueError, match="rt="):
            inf.rt_mode(dict(CFG, rt=bad), T=T)
    with pytest.raises(ValueError, match="rt="):
        inf.rt_mode(CFG, 0, T=T)
    # mcmc() refuses what does not need the data before it reads the data file or opens a device: the file does not exist
    nofile, out = str(tmp_path / "no_such_file.nc"), str(tmp_path / "out.hd5")
    for kw, cfg in ((dict(rt=0), CFG), ({}, dict(CFG, rt=2.5)), ({}, dict(CFG, rt="soon"))):
        with pytest.raises(ValueError, match="rt="):
            inf.mcmc(nofile, out, cfg, **kw)
    assert not os.path.exists(out)
    # ... and run_mcmc holds the window to the sampler's T before it calls the sampler at all
    s = StubSampler()
    with pytest.raises(ValueError, match="rt="):
        inf.run_mcmc(s, dict(CFG, rt=s.T + 1), [], log=open(os.devnull, "w"), rt_weight=np.ones(s.M) / s.M)
    with pytest.raises(ValueError, match="rt_weight"):
        inf.run_mcmc(s, dict(CFG, rt=2), [], log=open(os.devnull, "w"))
    assert s.calls == []


def test_the_cli_flag_parses(tmp_path, monkeypatch):
    import yaml
    cpath = str(tmp_path / "c.yaml")
    with open(cpath, "w") as f:
        yaml.safe_dump(dict(Mcmc=CFG), f)
    seen = {}
    monkeypatch.setattr(inf, "mcmc", lambda *a, **kw: seen.update(kw))
    inf.main(["-c", cpath, "-o", "x", "--rt", "7", "data.nc"])
    assert seen["rt"] == 7
    inf.main(["-c", cpath, "-o", "x", "data.nc"])
    assert seen["rt"] is None
    for bad in ("2.5", "soon"):
        with pytest.raises(SystemExit):
            inf.main(["-c", cpath, "-o", "x", "--rt", bad, "data.nc"])


# ---- 3. the host's formulas -------------------------------------------------------------------------------------------------
def test_mean_variance_and_probability_against_exact_rationals():
    rng = np.random.default_rng(11)
    B, D, M = 2, 3, 4
    n = np.array([5, 7], np.uint64)
    draws = [rng.integers(0, 1 << 20, (int(n[b]), D, M)) / float(1 << 18) for b in range(B)]   # dyadic: every step below is exact
    ref = np.stack([d[0] for d in draws])
    sm = np.stack([(d - d[0]).sum(axis=0) for d in draws])
    sq = np.stack([((d - d[0]) ** 2).sum(axis=0) for d in draws])
    g1 = np.stack([(d > 1.0).sum(axis=0) for d in draws]).astype(np.uint32)
    rs = RtSummary(count=n, ref=ref, sum=sm, sumsq=sq, gt1=g1)
    mean, var, prob = rs.mean, rs.var, rs.prob_gt1
    assert mean.shape == var.shape == prob.shape == (B, D, M)
    for b in range(B):
        nb = int(n[b])
        for t in range(D):
            for j in range(M):
                x = [Fraction(float(v)) for v in draws[b][:, t, j]]
                m = sum(x) / nb
                v = sum((xi - m) ** 2 for xi in x) / (nb - 1)
                assert abs(Fraction(float(mean[b, t, j])) - m) <= abs(m) * Fraction(1, 2 ** 50)
                assert abs(Fraction(float(var[b, t, j])) - v) <= v * Fraction(1, 2 ** 40)
                assert Fraction(float(prob[b, t, j])) == Fraction(float(np.float64(sum(xi > 1 for xi in x)) / nb))
    # one draw: the mean is the draw, the variance NaN without a warning; no draw: NaN all round
    one = RtSummary(count=np.array([1, 0], np.uint64), ref=ref, sum=np.zeros_like(sm), sumsq=np.zeros_like(sq),
                    gt1=(ref > 1.0).astype(np.uint32))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        mean, var, prob = one.mean, one.var, one.prob_gt1
    assert np.array_equal(mean[0], ref[0]) and np.all(np.isnan(var)) and np.array_equal(prob[0], (ref[0] > 1.0).astype(float))
    assert np.all(np.isnan(mean[1])) and np.all(np.isnan(prob[1]))


# ---- 4. run_mcmc with a stub sampler --------------------------------------------------------------------------------------
class RtStub(ForecastStub):
    """ForecastStub with the reproduction number: a draw's R_t is its sweep number (plus the day), R_it likewise."""

    def reset_rt(self, days, weight):
        self.calls.append(("reset_rt", days, np.asarray(weight).copy()))
        self.D, self.rt_rows = days, []

    def _trace(self, n, events=True, summarize=False, forecast=False, rt=False):
        tr = super()._trace(n, events=events, summarize=summarize, forecast=forecast)
        if rt:
            idx = self.sweeps - n + np.arange(n)
            self.calls.append(("rt", n, len(self.rt_rows)))
            self.rt_rows.extend(idx)
            tr.rt = idx[:, None, None] + np.arange(self.D)[None, None, :] / 8.0 + np.zeros((n, self.B, self.D))
        return tr

    def rt_summary(self):
        self.calls.append(("rt_summary",))
        x = np.broadcast_to(np.asarray(self.rt_rows, np.float64)[:, None, None, None], (len(self.rt_rows), self.B, self.D, self.M))
        d = x - x[:1]
        return RtSummary(count=np.full(self.B, len(x), np.uint64), ref=x[0].copy(), sum=d.sum(axis=0), sumsq=(d * d).sum(axis=0),
                         gt1=(x > 1.0).sum(axis=0).astype(np.uint32))


def _run(tmp_path, tag, config, ext=".npz", cap=800):
    s = RtStub()
    s.cap = cap
    nb, ns = config["num_bursts"], config["num_burst_samples"]
    Hn, _ = inf.forecast_mode(config)
    D = inf.rt_mode(config)
    names = [str(tmp_path / f"{tag}_{c}{ext}") for c in range(s.B)]
    kw = {} if config.get("summaries", "off") == "off" else dict(summaries=config["summaries"])
    if Hn:
        kw["forecast"] = (Hn, nb * ns)
    if D:
        kw["rt"] = (D, nb * ns)
    posts = [inf.Posterior(name, s.M, s.T, 2, inf.warmup_size() + nb * ns, **kw) for name in names]
    logname = str(tmp_path / f"{tag}.log")
    fkw = dict(forecast_calendar=(np.arange(Hn) + 0.5, np.arange(Hn) - 1.0), seed=21) if Hn else {}
    if D:
        fkw["rt_weight"] = np.arange(1, s.M + 1) / (s.M * (s.M + 1) / 2)
    with open(logname, "w") as log:
        inf.run_mcmc(s, config, posts, log=log, **fkw)
    for p in posts:
        p.close()
    return s, [_read(n) for n in names], open(logname).read()


NEW_SETS = {"rt/days", "rt/first_day", "rt/count", "rt/R_it_mean", "rt/R_it_var", "rt/R_it_prob_gt1", "samples/R_t"}


def test_off_calls_nothing_new_and_writes_todays_datasets(tmp_path):
    s0 = StubSampler()                                        # a sampler that has never heard of the reproduction number
    posts = [inf.Posterior(str(tmp_path / f"ref_{c}.npz"), s0.M, s0.T, 2, inf.warmup_size() + 8) for c in range(2)]
    inf.run_mcmc(s0, CFG, posts, log=open(os.devnull, "w"))
    for p in posts:
        p.close()
    plain, pf, log = _run(tmp_path, "plain", CFG)
    assert plain.calls == s0.calls and "R_t" not in log
    assert not any(c[0] in ("reset_rt", "rt", "rt_summary") for c in plain.calls)
    assert all(c[2] == {} for c in plain.calls if c[0] in ("sample", "burst"))
    ref = _read(str(tmp_path / "ref_1.npz"))
    assert set(pf[1]) == set(ref) and not (NEW_SETS & set(pf[1]))
    for k in ref:
        assert np.array_equal(pf[1][k], ref[k]), k


@pytest.mark.parametrize("summaries,forecast,overlap,ext", [("off", 0, True, ".npz"), ("on", 4, True, ".hd5"),
                                                            ("only", 4, False, ".npz")])
def test_on_resets_once_runs_once_per_burst_and_writes_the_group(tmp_path, summaries, forecast, overlap, ext):
    if ext == ".hd5" and not hdf5io.available():
        ext = ".npz"
    nb, ns, D = 3, 4, 3
    cfg = dict(CFG, num_bursts=nb, num_burst_samples=ns, summaries=summaries, rt=D, **(dict(forecast=forecast) if forecast else {}))
    s, files, log = _run(tmp_path, "on", cfg, ext=ext, cap=800 if overlap else ns)
    names = [c[0] for c in s.calls]
    # reset once, after the last warm-up window and before the first burst; nothing during the warm-up
    assert names.count("reset_rt") == 1 and names.count("rt_summary") == 1
    r = names.index("reset_rt")
    burst_name = "burst" if overlap else "sample"
    warm = [c for c in s.calls[:r] if c[0] == "sample"]
    assert len(warm) == 8 and all("rt" not in c[2] for c in warm)
    assert not any(c[0] == "rt" for c in s.calls[:r])
    assert s.calls[r][1] == D and np.array_equal(s.calls[r][2], np.arange(1, s.M + 1) / 6.0)
    # one rt per burst, behind it and behind its forecast (the stub records a burst, then what its kwargs made it do)
    after = [c for c in s.calls[r:] if c[0] in (burst_name, "forecast", "rt")]
    assert [c[0] for c in after] == ([burst_name, "forecast", "rt"] if forecast else [burst_name, "rt"]) * nb
    assert [c[2] for c in after if c[0] == "rt"] == [0, ns, 2 * ns]
    for c in after:
        if c[0] == burst_name:
            assert c[2]["rt"] is True and c[2].get("summarize", False) == (summaries != "off")
    # the files: today's datasets for this configuration, plus the group and the per-draw curve
    base, bf, _ = _run(tmp_path, "base", {k: v for k, v in cfg.items() if k != "rt"}, ext=ext, cap=800 if overlap else ns)
    sweeps = inf.warmup_size() + np.arange(nb * ns)
    for c, f in enumerate(files):
        assert set(f) == set(bf[c]) | NEW_SETS
        for k in bf[c]:
            assert np.array_equal(f[k], bf[c][k], equal_nan=True), k
        assert f["samples/R_t"].shape == (nb * ns, D) and f["samples/R_t"].dtype == np.float64
        assert np.array_equal(f["samples/R_t"], sweeps[:, None] + np.arange(D)[None, :] / 8.0)   # one row per kept draw of the sampling phase
        assert f["rt/days"].reshape(-1)[0] == D and f["rt/first_day"].reshape(-1)[0] == s.T - D
        assert f["rt/count"].reshape(-1)[0] == nb * ns
        for k in ("R_it_mean", "R_it_var", "R_it_prob_gt1"):
            assert f[f"rt/{k}"].shape == (D, s.M) and f[f"rt/{k}"].dtype == np.float64
        np.testing.assert_allclose(f["rt/R_it_mean"], sweeps.mean(), rtol=1e-15)
        np.testing.assert_allclose(f["rt/R_it_var"], sweeps.var(ddof=1), rtol=1e-13)
        assert np.array_equal(f["rt/R_it_prob_gt1"], np.ones((D, s.M)))
    # one line: the last day's national value with its quantiles, and the share of locations above one
    assert log.count("R_t:") == 1
    last = (sweeps[:, None] + (D - 1) / 8.0 + np.zeros((nb * ns, s.B))).reshape(-1)
    lo, hi = np.quantile(last, [0.05, 0.95])
    assert f"day {s.T - 1} national mean {last.mean():.3f} (0.05 / 0.95 quantiles {lo:.3f} / {hi:.3f})" in log
    assert "100.0 % of locations" in log and f"window of {D} day(s) from day {s.T - D}" in log


# ---- 5. ChainSampler's own order of calls inside a burst ------------------------------------------------------------------
class Recorder(ChainSampler):
    """ChainSampler without a device: every call that would reach the library is recorded instead."""
    B, P, M, T, cap, mmax = 2, 13, 3, 5, 16, 2
    record_events, events_dtype, auto_recover = True, np.int32, True

    def __init__(self):
        self.calls = []
        self.state = ProductState(summary_on=1, forecast_H=2, rt_D=3)
        self._fallback_level = 0

    def _state(self):
        return self.state

    def __getattribute__(self, name):
        if name in ("snapshot", "reset_trace", "run", "summarize", "forecast", "rt", "trace_wait", "read_trace_async",
                    "read_marginals_async", "read_forecast_marginals_async", "read_rt_draws_async"):
            calls = object.__getattribute__(self, "calls")
            return lambda *a, **kw: calls.append((name,) + a)
        return object.__getattribute__(self, name)

    def close(self):
        pass

    def read_trace(self, n, events=True):
        self.calls.append(("read_trace", n))
        return Trace(theta=np.zeros((n, self.B, self.P)), events=None, hmc={}, moves={})

    def read_marginals(self, n):
        self.calls.append(("read_marginals", n))

    def read_forecast_marginals(self, n):
        self.calls.append(("read_forecast_marginals", n))

    def read_rt_draws(self, n, first=0):
        self.calls.append(("read_rt_draws", n))
        return np.zeros((n, self.B, self.state.rt_D))


def test_a_burst_is_folded_behind_its_summary_and_forecast_and_not_at_all_when_off(monkeypatch):
    s = Recorder()
    tr = s.sample(4, summarize=True, forecast=True, rt=True)
    assert [c[0] for c in s.calls] == ["snapshot", "reset_trace", "run", "summarize", "forecast", "rt", "read_trace",
                                       "read_marginals", "read_forecast_marginals", "read_rt_draws"]
    assert s.calls[5] == ("rt", 0, 4) and tr.rt.shape == (4, s.B, 3)
    s = Recorder()
    s.sample(4, summarize=True, forecast=True)
    assert not any("rt" in c[0] for c in s.calls)
    # the overlapped bursts: the same order in each half of the buffer, the curves on the copy stream with the trace
    import covid19uk_amd.sampler as sm

    class NoPin:
        def __init__(self, sampler, count, events=True, **kw):
            self.count, self.kw = count, kw
            self.theta = np.zeros((count, sampler.B, sampler.P))
            self.hmc, self.moves = np.zeros((count, sampler.B, 3)), np.zeros((count, sampler.B, 4, _lib.MOVE_TRACE))
            self.events = self.marginals = self.forecast = None
            self.rt = np.zeros((count, sampler.B, kw["rt"])) if kw.get("rt") else None

        def close(self):
            pass
    monkeypatch.setattr(sm, "PinnedTrace", NoPin)
    for on in (True, False):
        s = Recorder()
        got = []
        s.sample_bursts(2, 4, lambda tr, i: got.append(tr.rt), events=False, summarize=True, forecast=True, rt=on)
        names = [c[0] for c in s.calls]
        if on:
            assert names[:6] == ["snapshot", "reset_trace", "run", "summarize", "forecast", "rt"]
            assert [c for c in s.calls if c[0] == "rt"] == [("rt", 0, 4), ("rt", 4, 4)]
            assert [c[:3] for c in s.calls if c[0] == "read_rt_draws_async"] == [("read_rt_draws_async", 4, 0), ("read_rt_draws_async", 4, 4)]
            assert all(g is not None and g.shape == (4, s.B, 3) for g in got) and s._pinned[0].kw["rt"] == 3
        else:
            assert not any("rt" in n for n in names) and got == [None, None] and "rt" not in s._pinned[0].kw


# ---- 6. the compiler's account of the new kernels -------------------------------------------------------------------------
def test_the_new_kernels_have_no_scratch_and_fit_the_lds():
    res = H.kernel_account("base")
    new = ["k_rt_prepare<0>", "k_rt_prepare<1>", "k_rt_trace<4>", "k_rt_finish"]
    assert all(k in res for k in new), sorted(res)
    for k in new:
        assert res[k]["scratch_bytes_per_lane"] == 0 and res[k]["vgpr_spill"] == 0 and res[k]["sgpr_spill"] == 0, (k, res[k])
    # static + dynamic LDS at Mp = 2048: only k_rt_trace asks for any, E and S of its 4 days and the four waves' partials
    dynamic = dict.fromkeys(new, 0)
    dynamic["k_rt_trace<4>"] = (2 * 4 * 2048 + 4 * 4 * 64) * 8
    for k, dyn in dynamic.items():
        assert res[k]["lds_bytes_per_block"] + dyn <= 160 * 1024, (k, res[k])
    assert res["k_rt_trace<4>"]["lds_bytes_per_block"] == 0
    # at UK-380 (Mp = 384) five workgroups of 32 KiB share a CU's LDS: the registers must not allow fewer
    assert res["k_rt_trace<4>"]["occupancy_waves_per_simd"] >= 5
    # k_rt and its table kernel are what they were
    parent = json.load(open(os.path.join(ROOT, "profiles", "r10_kernel_resources.json")))
    for k in ("k_rt<16>", "k_rt<4>", "k_rt_tables"):
        assert res[k] == parent[k], k

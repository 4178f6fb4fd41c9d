"""Host side of the within/between pressure shares on the device (include/seir_hip.h, "Within/between pressure shares on
the device"): the symbols, the configuration and the command line, run_mcmc's call sequence with a stub sampler,
ChainSampler's own order of calls inside a burst, the host's formulas against exact rationals, the datasets written, the
csv tool pooled over chain files, and the compiler's account of the new kernels.  No GPU."""
import ctypes
import os
import re
import warnings
from fractions import Fraction

import numpy as np
import pytest

from covid19uk_amd import _lib, hdf5io
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.posterior import within_between as wbtool
from covid19uk_amd.sampler import WB_KEYS, WbSummary
from tests import helpers as H
from tests.abi_lib import check_symbols
from tests.test_check_host import CheckRecorder, CheckStub
from tests.test_summary_host import CFG, StubSampler, _read

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "seir_sampler_wb_reset": "seir_sampler *s, int32_t days",
    "seir_sampler_wb": "seir_sampler *s, int32_t first_slot, int32_t count",
    "seir_sampler_read_wb": "seir_sampler *s, uint64_t *count, uint32_t *n, double *ref_w, double *sum_w, double *sumsq_w, "
                            "double *ref_b, double *sum_b, uint32_t *gt",
    "seir_sampler_read_wb_draws": "seir_sampler *s, int32_t first, int32_t count, double *within_pressure, "
                                  "double *between_pressure",
    "seir_sampler_read_wb_draws_async": "seir_sampler *s, int32_t first, int32_t count, double *within_pressure, "
                                        "double *between_pressure",
}


# ---- 1. the symbols ------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound_with_the_headers_types():
    lib = check_symbols(NEW)
    # a null sampler is refused before anything touches a device
    one = (ctypes.c_double * 1)(1.0)
    assert lib.seir_sampler_wb_reset(None, 1) == _lib.ERR_INVALID
    assert lib.seir_sampler_wb(None, 0, 1) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_wb_draws(None, 0, 1, one, one) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_wb_draws_async(None, 0, 1, one, one) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_wb(None, None, None, None, None, None, None, None, None) == _lib.ERR_INVALID


# ---- 2. configuration and command line -----------------------------------------------------------------------------------
def test_the_value_is_parsed_and_bad_ones_refused_before_any_gpu_call(tmp_path):
    T = 5
    mode = inf.within_between_mode
    assert mode({}) == 0 and mode(CFG, T=T) == 0
    assert mode(dict(CFG, within_between=3), T=T) == 3 and mode(dict(CFG, within_between=3), 4, T=T) == 4   # the command line overrides
    assert mode(dict(CFG, within_between=1), T=T) == 1 and mode(dict(CFG, within_between=T), T=T) == T
    assert mode(dict(CFG, within_between="off")) == 0 and mode(dict(CFG, within_between="4"), T=T) == 4
    assert mode(dict(CFG, within_between=400)) == 400          # without T only the lower end can be held
    for bad in (0, T + 1, -2, 2.5, "soon", True):
        with pytest.raises(ValueError, match="within_between="):
            mode(dict(CFG, within_between=bad), T=T)
    with pytest.raises(ValueError, match="within_between="):
        mode(CFG, 0, T=T)
    # mcmc() refuses what does not need the data before it reads the data file or opens a device: the file does not exist
    nofile, out = str(tmp_path / "no_such_file.nc"), str(tmp_path / "out.hd5")
    for kw, cfg in ((dict(within_between=0), CFG), ({}, dict(CFG, within_between=2.5)), ({}, dict(CFG, within_between="soon"))):
        with pytest.raises(ValueError, match="within_between="):
            inf.mcmc(nofile, out, cfg, **kw)
    assert not os.path.exists(out)
    # ... and run_mcmc holds the window to the sampler's T before it calls the sampler at all
    s = StubSampler()
    with pytest.raises(ValueError, match=r"within_between=6: the window is 1 .. T = 5"):
        inf.run_mcmc(s, dict(CFG, within_between=s.T + 1), [], log=open(os.devnull, "w"))
    assert s.calls == []


def test_the_cli_flag_parses(tmp_path, monkeypatch):
    import yaml
    cpath = str(tmp_path / "c.yaml")
    with open(cpath, "w") as f:
        yaml.safe_dump(dict(Mcmc=CFG), f)
    seen = {}
    monkeypatch.setattr(inf, "mcmc", lambda *a, **kw: (seen.clear(), seen.update(kw)))
    inf.main(["-c", cpath, "-o", "x", "--within-between", "7", "data.nc"])
    assert seen["within_between"] == 7
    inf.main(["-c", cpath, "-o", "x", "data.nc"])
    assert "within_between" not in seen                        # absent: mcmc is called as before the option existed
    for bad in ("2.5", "soon"):
        with pytest.raises(SystemExit):
            inf.main(["-c", cpath, "-o", "x", "--within-between", bad, "data.nc"])


# ---- 3. the host's formulas -------------------------------------------------------------------------------------------------
def _summary_of(w, b, defined):
    """w, b [n,B,D,M] shares, defined [n,B,D,M] bool -> WbSummary by the fold the header states."""
    n_, B, D, M = w.shape
    shape = (B, D, M)
    n, gt = np.zeros(shape, np.uint32), np.zeros(shape, np.uint32)
    ref_w, sum_w, sumsq_w, ref_b, sum_b = (np.zeros(shape) for _ in range(5))
    for j in range(n_):
        d = defined[j]
        first = d & (n == 0)
        ref_w, ref_b = np.where(first, w[j], ref_w), np.where(first, b[j], ref_b)
        dw, db = w[j] - ref_w, b[j] - ref_b
        sum_w, sumsq_w, sum_b = np.where(d, sum_w + dw, sum_w), np.where(d, sumsq_w + dw * dw, sumsq_w), np.where(d, sum_b + db, sum_b)
        gt = gt + (d & (w[j] > b[j])).astype(np.uint32)
        n = n + d.astype(np.uint32)
    return WbSummary(count=np.full(B, n_, np.uint64), defined=n, ref_w=ref_w, sum_w=sum_w, sumsq_w=sumsq_w, ref_b=ref_b,
                     sum_b=sum_b, gt=gt)


def test_means_variance_and_probability_against_exact_rationals():
    rng = np.random.default_rng(11)
    n_, B, D, M = 7, 2, 3, 4
    w = rng.integers(0, 1 << 20, (n_, B, D, M)) / float(1 << 20)      # dyadic: every step of the fold is exact
    b = 1.0 - w
    defined = rng.random((n_, B, D, M)) < 0.7
    defined[:, 0, 0, 0] = False                                       # a cell with no defined draw
    defined[:, 0, 0, 1] = np.arange(n_) == 3                          # ... and one with exactly one, not the first
    defined[:2, 1, 2, 3] = False                                      # the reference value is the first DEFINED draw's
    ws = _summary_of(w, b, defined)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        wm, wv, bm, pg = ws.within_mean, ws.within_var, ws.between_mean, ws.p_within_gt_between
    assert wm.shape == wv.shape == bm.shape == pg.shape == (B, D, M) and wm.dtype == np.float64
    assert np.array_equal(ws.defined, defined.sum(axis=0))
    assert ws.ref_w[1, 2, 3] == w[np.argmax(defined[:, 1, 2, 3]), 1, 2, 3]
    for c in range(B):
        for t in range(D):
            for m in range(M):
                sel = defined[:, c, t, m]
                k = int(sel.sum())
                xs = [Fraction(float(v)) for v in w[sel, c, t, m]]
                ys = [Fraction(float(v)) for v in b[sel, c, t, m]]
                if k == 0:
                    assert np.isnan(wm[c, t, m]) and np.isnan(wv[c, t, m]) and np.isnan(bm[c, t, m]) and np.isnan(pg[c, t, m])
                    continue
                mw, mb = sum(xs) / k, sum(ys) / k
                assert abs(Fraction(float(wm[c, t, m])) - mw) <= abs(mw) * Fraction(1, 2 ** 50)
                assert abs(Fraction(float(bm[c, t, m])) - mb) <= abs(mb) * Fraction(1, 2 ** 50)
                assert Fraction(float(pg[c, t, m])) == Fraction(float(np.float64(sum(x > y for x, y in zip(xs, ys))) / k))
                if k == 1:
                    assert np.isnan(wv[c, t, m]) and wm[c, t, m] == float(xs[0])
                else:
                    v = sum((x - mw) ** 2 for x in xs) / (k - 1)
                    assert abs(Fraction(float(wv[c, t, m])) - v) <= v * Fraction(1, 2 ** 40)
    assert defined[:, 0, 0, 0].sum() == 0 and defined[:, 0, 0, 1].sum() == 1


# ---- 4. run_mcmc with a stub sampler --------------------------------------------------------------------------------------
class WbStub(CheckStub):
    """CheckStub with the within/between shares: a draw's national pressures are its sweep number (plus the day), its within
    share is 3/4 in location 0 and 1/4 elsewhere, and chain 1 defines no draw at all in the last location."""

    def reset_within_between(self, days):
        self.calls.append(("reset_within_between", days))
        self.Dw, self.wb_rows = days, []

    def _trace(self, n, events=True, summarize=False, forecast=False, rt=False, check=False, within_between=False):
        tr = super()._trace(n, events=events, summarize=summarize, forecast=forecast, rt=rt, check=check)
        if within_between:
            idx = self.sweeps - n + np.arange(n)
            self.calls.append(("within_between", n, len(self.wb_rows)))
            self.wb_rows.extend(idx)
            wn = idx[:, None, None] + np.arange(self.Dw)[None, None, :] / 8.0 + np.zeros((n, self.B, self.Dw))
            tr.wb = dict(within_pressure=3.0 * wn, between_pressure=wn)
        return tr

    def within_between_summary(self):
        self.calls.append(("within_between_summary",))
        n, B, D, M = len(self.wb_rows), self.B, self.Dw, self.M
        w = np.full((n, B, D, M), 0.25)
        w[..., 0] = 0.75
        defined = np.ones((n, B, D, M), bool)
        defined[:, 1, :, M - 1] = False
        return _summary_of(w, 1.0 - w, defined)


def _run(tmp_path, tag, config, ext=".npz", cap=800):
    s = WbStub()
    s.cap = cap
    nb, ns = config["num_bursts"], config["num_burst_samples"]
    Hn, _ = inf.forecast_mode(config)
    D, K, Dw = inf.rt_mode(config), inf.check_mode(config), inf.within_between_mode(config)
    names = [str(tmp_path / f"{tag}_{c}{ext}") for c in range(s.B)]
    kw = {} if config.get("summaries", "off") == "off" else dict(summaries=config["summaries"])
    for key, v in (("forecast", Hn), ("rt", D), ("check", K), ("within_between", Dw)):
        if v:
            kw[key] = (v, nb * ns)
    posts = [inf.Posterior(name, s.M, s.T, 2, inf.warmup_size() + nb * ns, **kw) for name in names]
    logname = str(tmp_path / f"{tag}.log")
    fkw = dict(seed=21)
    if Hn:
        fkw["forecast_calendar"] = (np.arange(Hn) + 0.5, np.arange(Hn) - 1.0)
    if D:
        fkw["rt_weight"] = np.arange(1, s.M + 1) / (s.M * (s.M + 1) / 2)
    if K:
        fkw["check_calendar"] = (np.arange(K) + 0.25, np.arange(K) - 2.0)
    with open(logname, "w") as log:
        inf.run_mcmc(s, config, posts, log=log, **fkw)
    for p in posts:
        p.close()
    return s, [_read(n) for n in names], open(logname).read(), names


NEW_SETS = {f"within_between/{k}" for k in ("days", "first_day", "count", "defined", "within_mean", "within_var", "between_mean",
                                            "p_within_gt_between")} | {f"samples/{k}" for k in WB_KEYS}


def test_off_calls_nothing_new_and_writes_todays_datasets(tmp_path):
    s0 = StubSampler()                                        # a sampler that has never heard of the shares
    posts = [inf.Posterior(str(tmp_path / f"ref_{c}.npz"), s0.M, s0.T, 2, inf.warmup_size() + 8) for c in range(2)]
    inf.run_mcmc(s0, CFG, posts, log=open(os.devnull, "w"))
    for p in posts:
        p.close()
    plain, pf, log, _ = _run(tmp_path, "plain", CFG)
    assert plain.calls == s0.calls and "Within/between" not in log
    assert not any(c[0] in ("reset_within_between", "within_between", "within_between_summary") for c in plain.calls)
    assert all(c[2] == {} for c in plain.calls if c[0] in ("sample", "burst"))
    ref = _read(str(tmp_path / "ref_1.npz"))
    assert set(pf[1]) == set(ref) and not (NEW_SETS & set(pf[1]))
    for k in ref:
        assert np.array_equal(pf[1][k], ref[k]), k
    # the other products on and this one absent: their keyword sets are what they were
    full, _, log, _ = _run(tmp_path, "others", dict(CFG, summaries="only", thin=2, forecast=4, rt=3, check=5))
    assert "Within/between" not in log
    for c in full.calls:
        if c[0] in ("sample", "burst"):
            assert "within_between" not in c[2]


@pytest.mark.parametrize("summaries,others,overlap,ext", [("off", False, True, ".npz"), ("on", True, True, ".hd5"),
                                                          ("only", True, False, ".npz")])
def test_on_resets_once_folds_every_burst_behind_the_others_and_writes_the_group(tmp_path, summaries, others, overlap, ext):
    if ext == ".hd5" and not hdf5io.available():
        ext = ".npz"
    nb, ns, D = 3, 4, 3
    cfg = dict(CFG, num_bursts=nb, num_burst_samples=ns, summaries=summaries, within_between=D,
               **(dict(forecast=4, rt=2, check=5, thin=2) if others else {}))
    s, files, log, _ = _run(tmp_path, "on", cfg, ext=ext, cap=800 if overlap else ns)
    names = [c[0] for c in s.calls]
    # reset once, after the last warm-up window and before the first burst; nothing during the warm-up
    assert names.count("reset_within_between") == 1 and names.count("within_between_summary") == 1
    r = names.index("reset_within_between")
    burst_name = "burst" if overlap else "sample"
    warm = [c for c in s.calls[:r] if c[0] == "sample"]
    assert len(warm) == 8 and all("within_between" not in c[2] for c in warm)
    assert not any(c[0] == "within_between" for c in s.calls[:r])
    assert s.calls[r] == ("reset_within_between", D)
    if others:                                                 # the resets of the others come first
        assert all(names.index(k) < r for k in ("reset_forecast", "reset_rt", "reset_check"))
    # one call per burst, behind the burst's forecast, R_t and check (the stub records a burst, then what its kwargs made it do)
    after = [c for c in s.calls[r:] if c[0] in (burst_name, "forecast", "rt", "check", "within_between")]
    assert [c[0] for c in after] == ([burst_name, "forecast", "rt", "check", "within_between"] if others
                                     else [burst_name, "within_between"]) * nb
    assert [c[2] for c in after if c[0] == "within_between"] == [0, ns, 2 * ns]
    for c in after:
        if c[0] == burst_name:
            assert c[2]["within_between"] is True and c[2].get("summarize", False) == (summaries != "off")
            assert set(c[2]) == {"within_between"} | ({"events", "summarize"} if summaries != "off" else set()) | \
                ({"forecast", "rt", "check"} if others else set())
    # the files: today's datasets for this configuration, plus the group and the two per-draw datasets
    base, bf, _, _ = _run(tmp_path, "base", {k: v for k, v in cfg.items() if k != "within_between"}, ext=ext,
                          cap=800 if overlap else ns)
    sweeps = inf.warmup_size() + np.arange(nb * ns)
    n = nb * ns
    for c, f in enumerate(files):
        assert set(f) == set(bf[c]) | NEW_SETS
        for k in bf[c]:
            assert np.array_equal(f[k], bf[c][k], equal_nan=True), k
        for k, scale in (("within_pressure", 3.0), ("between_pressure", 1.0)):
            assert f[f"samples/{k}"].shape == (n, D) and f[f"samples/{k}"].dtype == np.float64
            assert np.array_equal(f[f"samples/{k}"], scale * (sweeps[:, None] + np.arange(D)[None, :] / 8.0))   # a row per kept draw
        g = {k: f[f"within_between/{k}"] for k in ("days", "first_day", "count")}
        assert g["days"].reshape(-1)[0] == D and g["first_day"].reshape(-1)[0] == s.T - D and g["count"].reshape(-1)[0] == n
        for k in ("defined", "within_mean", "within_var", "between_mean", "p_within_gt_between"):
            assert f[f"within_between/{k}"].shape == (D, s.M) and f[f"within_between/{k}"].dtype == np.float64
        live = np.ones(s.M, bool)
        live[s.M - 1] = c == 0
        assert np.array_equal(f["within_between/defined"], np.broadcast_to(np.where(live, float(n), 0.0), (D, s.M)))
        want_w = np.where(np.arange(s.M) == 0, 0.75, 0.25)
        assert np.array_equal(f["within_between/within_mean"][:, live], np.broadcast_to(want_w[live], (D, int(live.sum()))))
        assert np.array_equal(f["within_between/between_mean"][:, live], np.broadcast_to(1.0 - want_w[live], (D, int(live.sum()))))
        assert np.array_equal(f["within_between/p_within_gt_between"][:, live],
                              np.broadcast_to((want_w > 0.5).astype(float)[live], (D, int(live.sum()))))
        assert np.all(f["within_between/within_var"][:, live] == 0.0)
        for k in ("within_mean", "within_var", "between_mean", "p_within_gt_between"):
            assert np.all(np.isnan(f[f"within_between/{k}"][:, ~live]))
    # one line: the last day's national within share 3 / (3 + 1) with its quantiles, and the share of locations above one half
    assert log.count("Within/between:") == 1
    assert f"day {s.T - 1} national within share mean 0.750 (0.05 / 0.95 quantiles 0.750 / 0.750) over {n * s.B} kept draw(s)" in log
    assert f"P(within > between) > 0.5 in {100.0 / s.M:.1f} % of locations" in log
    assert f"window of {D} day(s) from day {s.T - D}" in log


# ---- 5. ChainSampler's own order of calls inside a burst ------------------------------------------------------------------
class WbRecorder(CheckRecorder):
    def __init__(self):
        super().__init__()
        self.state = self.state._replace(wb_D=3)

    def __getattribute__(self, name):
        if name in ("within_between", "read_wb_draws_async"):
            calls = object.__getattribute__(self, "calls")
            return lambda *a, **kw: calls.append((name,) + a)
        return CheckRecorder.__getattribute__(self, name)

    def read_wb_draws(self, n, first=0):
        self.calls.append(("read_wb_draws", n))
        return {k: np.zeros((n, self.B, self.state.wb_D)) for k in WB_KEYS}


def test_a_burst_is_folded_behind_summary_forecast_rt_and_check_and_not_at_all_when_off(monkeypatch):
    s = WbRecorder()
    tr = s.sample(4, summarize=True, forecast=True, rt=True, check=True, within_between=True)
    assert [c[0] for c in s.calls] == ["snapshot", "reset_trace", "run", "summarize", "forecast", "rt", "check", "within_between",
                                       "read_trace", "read_marginals", "read_forecast_marginals", "read_rt_draws",
                                       "read_check_marginals", "read_wb_draws"]
    assert s.calls[7] == ("within_between", 0, 4) and tr.wb["within_pressure"].shape == (4, s.B, 3)
    s = WbRecorder()
    tr = s.sample(4, summarize=True, forecast=True, rt=True, check=True)
    assert not any("within_between" in c[0] or "wb" in c[0] for c in s.calls) and tr.wb is None
    s = WbRecorder()
    s.state = s.state._replace(wb_D=0)
    with pytest.raises(ValueError, match="before reset_within_between"):
        s.sample(4, within_between=True)
    import covid19uk_amd.sampler as sm

    class NoPin:
        def __init__(self, sampler, count, events=True, **kw):
            self.count, self.kw = count, kw
            self.theta = np.zeros((count, sampler.B, sampler.P))
            self.hmc, self.moves = np.zeros((count, sampler.B, 3)), np.zeros((count, sampler.B, 4, _lib.MOVE_TRACE))
            self.events = self.marginals = self.forecast = self.rt = self.check = None
            self.wb = {k: np.zeros((count, sampler.B, kw["wb"])) for k in WB_KEYS} if kw.get("wb") else None

        def close(self):
            pass
    monkeypatch.setattr(sm, "PinnedTrace", NoPin)
    for on in (True, False):
        s = WbRecorder()
        got = []
        s.sample_bursts(2, 4, lambda tr, i: got.append(tr.wb), events=False, summarize=True, forecast=True, rt=True, check=True,
                        **(dict(within_between=True) if on else {}))
        names = [c[0] for c in s.calls]
        if on:
            assert names[:8] == ["snapshot", "reset_trace", "run", "summarize", "forecast", "rt", "check", "within_between"]
            assert [c for c in s.calls if c[0] == "within_between"] == [("within_between", 0, 4), ("within_between", 4, 4)]
            assert [c[:3] for c in s.calls if c[0] == "read_wb_draws_async"] == \
                [("read_wb_draws_async", 4, 0), ("read_wb_draws_async", 4, 4)]
            assert all(g is not None and g["between_pressure"].shape == (4, s.B, 3) for g in got) and s._pinned[0].kw["wb"] == 3
        else:
            assert not any("within_between" in n or "wb" in n for n in names) and got == [None, None]
            assert "wb" not in s._pinned[0].kw


# ---- 6. the csv tool ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [".npz", ".hd5"])
def test_the_csv_tool_pools_the_files_with_the_weights_defined(tmp_path, ext, monkeypatch):
    if ext == ".hd5" and not hdf5io.available():
        pytest.skip("no HDF5 library")
    nb, ns, D = 2, 4, 3
    cfg = dict(CFG, num_bursts=nb, num_burst_samples=ns, within_between=D)
    s, files, _, names = _run(tmp_path, "csv", cfg, ext=ext)
    # make the two files differ, so that the weights matter: chain 1 saw a quarter of the draws in location 0, with other values
    rng = np.random.default_rng(5)
    chains = [wbtool.read_chain_file(n) for n in names]
    for c in chains:
        for k in ("within_mean", "between_mean", "p_within_gt_between"):
            c[k] = np.where(np.isnan(c[k]), np.nan, rng.random(c[k].shape))
    chains[1]["defined"] = chains[1]["defined"].copy()
    chains[1]["defined"][:, 0] = 2.0
    for day in (-1, 0, D - 1, -D):
        got = wbtool.pool_posterior(chains, day)
        w = np.stack([c["defined"][day] for c in chains])
        for x, k in enumerate(("within_mean", "between_mean", "p_within_gt_between")):
            v = np.stack([c[k][day] for c in chains])
            want = np.array([np.nan if w[:, m].sum() == 0 else
                             sum(w[f, m] * v[f, m] for f in range(2) if w[f, m] > 0) / w[:, m].sum() for m in range(s.M)])
            np.testing.assert_allclose(got[:, x], want, rtol=1e-15, equal_nan=True)
    with pytest.raises(ValueError, match="--day"):
        wbtool.pool_posterior(chains, D)
    # end to end through the command line, from the files as written: chain 1 defines nothing in the last location
    out = str(tmp_path / "wb.csv")
    rows = wbtool.main(["--posterior", *names, "--day", "-1", "-o", out])
    lines = open(out).read().splitlines()
    assert lines[0] == "location,within_mean,between_mean,p_within_gt_between" and len(lines) == s.M + 1
    assert [ln.split(",")[0] for ln in lines[1:]] == [str(m) for m in range(s.M)]
    want_w = np.where(np.arange(s.M) == 0, 0.75, 0.25)
    assert np.array_equal(rows, np.stack([want_w, 1.0 - want_w, (want_w > 0.5).astype(float)], axis=1))
    assert [float(x) for x in lines[-1].split(",")[1:]] == [0.25, 0.75, 0.0]
    # a file of a run without the key says so
    _, _, _, plain = _run(tmp_path, "plaincsv", CFG, ext=ext)
    with pytest.raises(ValueError, match="within_between"):
        wbtool.main(["--posterior", plain[0], "-o", out])
    # the reference's argument form still parses and goes where it went
    seen = []
    monkeypatch.setattr(wbtool, "within_between", lambda files, output, device=0: seen.append((files, output)))
    wbtool.main(["-d", "data.nc", "-s", "samples.pkl", "-o", "o.csv"])
    wbtool.main(["--datafile", "data.nc", "--samples", "samples.pkl", "--output", "o.csv"])
    assert seen == [(["data.nc", "samples.pkl"], "o.csv")] * 2
    for bad in (["-d", "data.nc", "-o", "o.csv"], ["-s", "samples.pkl"], ["--posterior", names[0], "-d", "data.nc", "-o", out]):
        with pytest.raises(SystemExit):
            wbtool.main(bad)


# ---- 7. the compiler's account of the new kernels -------------------------------------------------------------------------
def test_the_new_kernels_are_these_instances_without_scratch_or_static_lds():
    res = H.kernel_account("wb")
    new = ["k_wb_prepare<0>", "k_wb_prepare<1>", "k_wb_trace<4>", "k_wb_finish"]
    assert sorted(res) == sorted(new), sorted(res)
    for k in new:
        assert res[k]["scratch_bytes_per_lane"] == 0 and res[k]["vgpr_spill"] == 0 and res[k]["sgpr_spill"] == 0, (k, res[k])
    # LDS as the constexpr says: no static part anywhere, and k_wb_trace's dynamic part -- x of its 4 days and the four waves'
    # partials -- fits a workgroup at Mp = 2048 (csrc/wb_kernels.h: k_wb_trace_lds_bytes, WB_DT = 4)
    for k in new:
        assert res[k]["lds_bytes_per_block"] == 0, (k, res[k])
    text = open(os.path.join(ROOT, "covid19uk_amd", "csrc", "wb_kernels.h")).read()
    assert re.search(r"constexpr int WB_DT = 4;", text)
    assert re.search(r"return sizeof\(double\) \* \(\(size_t\)DT \* Mp \+ 4 \* DT \* WAVE\);", text)
    assert (4 * 2048 + 4 * 4 * 64) * 8 == 72 * 1024 <= 160 * 1024
    # at UK-380 (Mp = 384) a workgroup takes 20 KiB and the LDS would hold eight: the registers must allow at least six
    assert res["k_wb_trace<4>"]["occupancy_waves_per_simd"] >= 6

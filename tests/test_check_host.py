"""Host side of the in-sample predictive check (include/seir_hip.h, "In-sample predictive check on the device"): the
symbols, the configuration and the command line, run_mcmc's call sequence with a stub sampler, ChainSampler's own order
inside a burst, the datasets written, the shared compare update (covid19uk_amd/csrc/check_update.h) compiled as plain C++
against Python integers, the mid-p value against fractions.Fraction, the calendar and baseline helpers against what
`predict` builds for initial_step = T - K, and the compiler's account of the new kernels.  No GPU."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import warnings
from fractions import Fraction

import numpy as np
import pytest

import __graft_entry__ as entry
from covid19uk_amd import _lib, hdf5io, model_spec
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.posterior import predict
from covid19uk_amd.sampler import CHECK_KEYS, CheckSummary, Summary, mid_p
from tests import helpers as H
from tests.abi_lib import check_symbols
from tests.test_rt_device_host import Recorder, RtStub
from tests.test_summary_host import CFG, StubSampler, _read

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARG3 = "int64_t *check_by_day, int64_t *check_by_location, int64_t *check_state_by_day"
NEW = {
    "seir_sampler_check_reset": "seir_sampler *s, int32_t days, const double *W, const double *weekday_c, uint64_t seed",
    "seir_sampler_check": "seir_sampler *s, int32_t first_slot, int32_t count",
    "seir_sampler_read_check": "seir_sampler *s, uint64_t *count, int32_t *ref, int64_t *sum, uint64_t *sumsq",
    "seir_sampler_read_check_marginals": "seir_sampler *s, int32_t first, int32_t count, " + MARG3,
    "seir_sampler_read_check_marginals_async": "seir_sampler *s, int32_t first, int32_t count, " + MARG3,
    "seir_sampler_read_check_counts": "seir_sampler *s, int32_t *obs, uint32_t *lt, uint32_t *eq, uint32_t *loc_lt, "
                                      "uint32_t *loc_eq, uint32_t *day_lt, uint32_t *day_eq, uint32_t *all_lt, uint32_t *all_eq",
}


# ---- 1. the symbols ------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound_with_the_headers_types():
    lib = check_symbols(NEW)
    raw = open(os.path.join(ROOT, "include", "seir_hip.h")).read()
    assert int(re.search(r"#define SEIR_CHECK_MAX_DAYS (\d+)", raw).group(1)) == _lib.CHECK_MAX_DAYS == 128
    # a null sampler is refused before anything touches a device
    one = (ctypes.c_double * 1)(0.0)
    assert lib.seir_sampler_check_reset(None, 5, one, one, 0) == _lib.ERR_INVALID
    assert lib.seir_sampler_check(None, 0, 1) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_check(None, None, None, None, None) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_check_marginals(None, 0, 1, None, None, None) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_check_marginals_async(None, 0, 1, None, None, None) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_check_counts(None, *([None] * 9)) == _lib.ERR_INVALID


# ---- 2. configuration and command line -----------------------------------------------------------------------------------
def test_check_value_is_parsed_and_bad_ones_refused_before_any_gpu_call(tmp_path):
    assert inf.check_mode({}) == 0 and inf.check_mode(dict(CFG, check="off")) == 0
    assert inf.check_mode(dict(CFG, check=14)) == 14 and inf.check_mode(dict(CFG, check="28")) == 28
    assert inf.check_mode(dict(CFG, check=14), 7) == 7                           # the command line overrides
    assert inf.check_mode(CFG, 1) == 1 and inf.check_mode(CFG, 128) == 128 and inf.check_mode(CFG, 70, T=70) == 70
    for bad in (0, 129, -3, "all", True, 2.5):
        with pytest.raises(ValueError, match="check"):
            inf.check_mode(dict(CFG, check=bad))
    with pytest.raises(ValueError, match=r"min\(T = 70, 128\)"):
        inf.check_mode(CFG, 71, T=70)
    # mcmc() refuses 0, 129 and a non-integer before it reads the data file or opens a device: the file does not exist
    nofile, out = str(tmp_path / "no_such_file.nc"), str(tmp_path / "out.npz")
    for kw, cfg in ((dict(check=0), CFG), (dict(check=129), CFG), ({}, dict(CFG, check=2.5)), ({}, dict(CFG, check=0))):
        with pytest.raises(ValueError, match="check"):
            inf.mcmc(nofile, out, cfg, **kw)
    # T + 1 is refused once the data have been read and before a device is opened: the device named does not exist
    from covid19uk_amd import synth
    cov = synth.make_covariates("ni11")
    events, _, _ = synth.simulate_epidemic(cov)
    data = str(tmp_path / "data.npz")
    inf.write_inference_data(data, cov, events[..., 2])
    assert cov.T < 128
    with pytest.raises(ValueError, match=rf"check={cov.T + 1}: the window is 1 .. min\(T = {cov.T}, 128\)"):
        inf.mcmc(data, out, CFG, check=cov.T + 1, device=10 ** 6)
    assert not os.path.exists(out)


def test_the_cli_flag_parses(tmp_path, monkeypatch):
    import yaml
    cpath = str(tmp_path / "c.yaml")
    with open(cpath, "w") as f:
        yaml.safe_dump(dict(Mcmc=CFG), f)
    seen = {}
    monkeypatch.setattr(inf, "mcmc", lambda *a, **kw: (seen.clear(), seen.update(kw)))
    inf.main(["-c", cpath, "-o", "x", "--check", "7", "--summaries", "only", "--thin", "2", "--forecast", "7", "--rt", "7", "data.nc"])
    assert seen["check"] == 7 and seen["forecast"] == 7 and seen["rt"] == 7 and seen["thin"] == 2 and seen["summaries"] == "only"
    inf.main(["-c", cpath, "-o", "x", "data.nc"])
    assert "check" not in seen                                 # without the flag mcmc() is called as before
    with pytest.raises(SystemExit):
        inf.main(["-c", cpath, "-o", "x", "--check", "2.5", "data.nc"])


# ---- 3. the calendar and baseline helpers ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dates", [["2020-10-%02d" % d for d in range(1, 12)], None])
@pytest.mark.parametrize("K", [1, 4, 11])
def test_the_calendar_is_what_predict_builds_for_initial_step_T_minus_K(dates, K):
    T, M = 11, 2
    rng = np.random.default_rng(1)
    cov = model_spec.Covariates(C=np.zeros((M, M)), W=rng.uniform(0.5, 1.5, T), N=np.ones(M), adjacency=np.zeros((M, M)),
                                weekday=(np.arange(T) % 7 < 5).astype(float), area=np.ones(M))
    W, wd = predict.check_calendar(cov, dates, T, K)
    weekday, days = predict.prediction_weekday(dates, (T - K) + K, cov.weekday)    # predict(), line by line
    assert (days is None) == (dates is None)
    assert np.array_equal(wd, predict.clipped(weekday - weekday.mean(), T - K, K))
    assert np.array_equal(W, predict.clipped(cov.W, T - K, K)) and np.array_equal(W, cov.W[T - K:])
    assert W.shape == wd.shape == (K,)
    if dates is not None:                                      # 2020-10-01 was a Thursday; centred over the T observed days
        full = np.array([1, 1, 0, 0, 1, 1, 1, 1, 1, 0, 0], float)
        assert np.array_equal(wd, (full - full.mean())[T - K:])
    else:
        assert np.array_equal(wd, (cov.weekday - cov.weekday.mean())[T - K:])


def _baseline_sequential(alpha_0, alpha_t, T, K):
    """The header's rule, one float64 operation at a time: what k_check_prepare does for one draw."""
    out = np.empty(K)
    t0 = T - K
    if t0 == 0:
        out[0] = alpha_0
    cs = 0.0
    for i in range(T - 1):
        cs = float(alpha_t[i]) if i == 0 else cs + float(alpha_t[i])
        if i + 1 - t0 >= 0:
            out[i + 1 - t0] = alpha_0 + cs
    return out


@pytest.mark.parametrize("T,K", [(1, 1), (2, 1), (2, 2), (65, 1), (65, 2), (65, 64), (65, 65), (200, 128)])
def test_the_baseline_rule_restates_log_baseline_path_to_the_bit(T, K):
    rng = np.random.default_rng(T * 1000 + K)
    n = 3
    a0, at = rng.normal(-1.0, 0.3, n), rng.normal(0.0, 0.05, (n, T - 1))
    want = predict.log_baseline_path(a0, at, T - K, K)
    assert want.shape == (n, K)
    for i in range(n):
        assert np.array_equal(_baseline_sequential(a0[i], at[i], T, K), want[i])
    if K == T:
        assert np.array_equal(want[:, 0], a0)


# ---- 4. the shared compare update, as plain C++ ---------------------------------------------------------------------------
DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include "check_update.h"
// one cell and one total.  "c sim seen": a draw's cell; "t sim obs": a draw's total; "r 0 0": reset.
int main() {
    int32_t obs = 0; uint32_t lt = 0, eq = 0, tl = 0, te = 0; bool first = true, moved = false;
    char op[8]; long long a, b;
    while (std::scanf("%7s %lld %lld", op, &a, &b) == 3) {
        if (op[0] == 'r') { obs = 0; lt = eq = tl = te = 0; first = true; moved = false; continue; }
        if (op[0] == 'c') {
            moved |= seir::check_cell_update(obs, lt, eq, (int32_t)a, (int32_t)b, first);
            first = false;
            std::printf("%" PRId32 " %" PRIu32 " %" PRIu32 " %d\n", obs, lt, eq, moved ? 1 : 0);
        } else {
            seir::check_total_update(tl, te, (int64_t)a, (int64_t)b);
            std::printf("%" PRIu32 " %" PRIu32 "\n", tl, te);
        }
    }
}
"""


@pytest.fixture(scope="module")
def compare(tmp_path_factory):
    cxx = None
    try:
        cxx = [entry._hipcc(), "-x", "c++"]
    except RuntimeError:
        for cand in ("g++", "c++", "clang++"):
            if shutil.which(cand):
                cxx = [cand]
                break
    assert cxx, "no C++ compiler"
    d = tmp_path_factory.mktemp("check_update")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run(cxx + ["-std=c++17", "-O1", "-Wall", "-Werror", "-I", entry.CSRC, "-o", str(exe), str(src)],
                   check=True, capture_output=True, text=True)

    def run(lines):
        text = "".join(f"{op} {int(a)} {int(b)}\n" for op, a, b in lines)
        out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.split("\n")
        return [tuple(int(v) for v in row.split()) for row in out if row]
    return run


def test_the_cell_update_counts_below_and_at_the_first_draws_count_and_flags_a_moved_one(compare):
    rng = np.random.default_rng(4)
    sims = [int(v) for v in rng.integers(0, 9, 200)] + [0, 2 ** 31 - 1]
    seen = [4] * len(sims)
    seen[120] = 5                                              # one later draw carries other data: sticky from there on
    got = compare([("c", s, o) for s, o in zip(sims, seen)])
    obs, lt, eq, moved = seen[0], 0, 0, 0
    for i, (s, o) in enumerate(zip(sims, seen)):
        lt += s < obs
        eq += s == obs
        moved |= o != obs
        assert got[i] == (obs, lt, eq, moved), i
    assert got[119][3] == 0 and got[120][3] == 1 and got[-1][3] == 1 and 0 < got[-1][1] < len(sims) and got[-1][2] > 0
    # a reset starts again: the next draw's count becomes obs, the flag is down
    got = compare([("c", 1, 3), ("r", 0, 0), ("c", 7, 7), ("c", 6, 7), ("c", 8, 7)])
    assert got == [(3, 1, 0, 0), (7, 0, 1, 0), (7, 1, 1, 0), (7, 1, 1, 0)]


def test_the_total_update_compares_64_bit_sums(compare):
    pairs = [(5, 6), (6, 6), (7, 6), (2 ** 40, 2 ** 40 + 1), (2 ** 40 + 1, 2 ** 40), (2 ** 40, 2 ** 40), (0, 0)]
    got = compare([("t", a, b) for a, b in pairs])
    lt = eq = 0
    for i, (a, b) in enumerate(pairs):
        lt += a < b
        eq += a == b
        assert got[i] == (lt, eq)
    assert got[-1] == (2, 3)


# ---- 5. the mid-p value ----------------------------------------------------------------------------------------------------
def test_mid_p_is_the_correctly_rounded_fraction_and_nan_without_a_warning_for_no_draw():
    rng = np.random.default_rng(2)
    count = np.array([0, 1, 7, 1000, (1 << 20) - 1], np.uint64)
    lt = np.stack([rng.integers(0, int(c) + 1, (3, 4)) for c in count]).astype(np.uint32)
    eq = rng.integers(0, count.astype(np.int64)[:, None, None] - lt + 1).astype(np.uint32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        p = mid_p(count, lt, eq)
        tot = mid_p(count, lt[:, 0, 0], eq[:, 0, 0])
        none = mid_p(np.uint64(0), np.uint32(0), np.uint32(0))
    assert p.shape == lt.shape and p.dtype == np.float64 and np.all(np.isnan(p[0])) and np.isnan(none)
    for b in range(1, len(count)):
        for idx in np.ndindex(3, 4):
            want = (Fraction(int(lt[b][idx])) + Fraction(int(eq[b][idx]), 2)) / int(count[b])
            assert p[b][idx] == float(want), (b, idx)
            assert 0.0 <= p[b][idx] <= 1.0
    assert np.array_equal(tot[1:], p[1:, 0, 0])
    assert mid_p(np.uint64(4), np.uint32(4), np.uint32(0)) == 1.0 and mid_p(np.uint64(4), np.uint32(0), np.uint32(0)) == 0.0
    assert mid_p(np.uint64(3), np.uint32(1), np.uint32(1)) == 0.5


# ---- 6. run_mcmc with a stub sampler --------------------------------------------------------------------------------------
class CheckStub(RtStub):
    """RtStub with the check: a draw's check marginals are its sweep number; the counts are simple functions of the rows."""

    def reset_check(self, days, W, weekday_c, seed):
        self.calls.append(("reset_check", days, np.asarray(W).copy(), np.asarray(weekday_c).copy(), seed))
        self.K, self.check_rows = days, []

    def _trace(self, n, events=True, summarize=False, forecast=False, rt=False, check=False):
        tr = super()._trace(n, events=events, summarize=summarize, forecast=forecast, rt=rt)
        if check:
            idx = self.sweeps - n + np.arange(n)
            self.calls.append(("check", n, len(self.check_rows)))
            self.check_rows.extend(idx)
            f = np.broadcast_to(idx[:, None, None, None], (n, self.B, self.K, 3)).astype(np.int64)
            tr.check = dict(check_by_day=f, check_by_location=np.broadcast_to(
                idx[:, None, None, None], (n, self.B, self.M, 3)).astype(np.int64), check_state_by_day=-f)
        return tr

    def check_summary(self):
        self.calls.append(("check_summary",))
        n, B, M, K = len(self.check_rows), self.B, self.M, self.K
        x = np.broadcast_to(np.asarray(self.check_rows, np.int64)[:, None, None, None, None], (n, B, M, K, 6))
        d = x - x[:1]
        mom = Summary(count=np.full(B, n, np.uint64), ref=x[0].astype(np.int32), sum=d.sum(axis=0),
                      sumsq=(d * d).sum(axis=0).astype(np.uint64))
        u = lambda shape, v: np.full(shape, v, np.uint32)      # noqa: E731
        return CheckSummary(mom, np.full((B, M, K), 9, np.int32), u((B, M, K), 3), u((B, M, K), 2),
                            np.stack([np.arange(M), np.full(M, n)]).astype(np.uint32), u((B, M), 0),
                            u((B, K), 1), u((B, K), 1), np.array([n, 0], np.uint32), np.array([0, n], np.uint32))


def _run(tmp_path, tag, config, ext=".npz", cap=800, calendar=True):
    s = CheckStub()
    s.cap = cap
    nb, ns = config["num_bursts"], config["num_burst_samples"]
    Hn, _ = inf.forecast_mode(config)
    D, K = inf.rt_mode(config), inf.check_mode(config)
    names = [str(tmp_path / f"{tag}_{c}{ext}") for c in range(s.B)]
    kw = {} if config.get("summaries", "off") == "off" else dict(summaries=config["summaries"])
    for key, v in (("forecast", Hn), ("rt", D), ("check", K)):
        if v:
            kw[key] = (v, nb * ns)
    posts = [inf.Posterior(name, s.M, s.T, 2, inf.warmup_size() + nb * ns, **kw) for name in names]
    logname = str(tmp_path / f"{tag}.log")
    fkw = dict(seed=21)
    if Hn:
        fkw["forecast_calendar"] = (np.arange(Hn) + 0.5, np.arange(Hn) - 1.0)
    if D:
        fkw["rt_weight"] = np.arange(1, s.M + 1) / (s.M * (s.M + 1) / 2)
    if K and calendar:
        fkw["check_calendar"] = (np.arange(K) + 0.25, np.arange(K) - 2.0)
    with open(logname, "w") as log:
        inf.run_mcmc(s, config, posts, log=log, **fkw)
    for p in posts:
        p.close()
    return s, [_read(n) for n in names], open(logname).read()


NEW_SETS = {f"check/{k}" for k in ("days", "first_day", "count", "seir_mean", "seir_var", "state_mean", "state_var", "observed",
                                   "lt", "eq", "location_lt", "location_eq", "day_lt", "day_eq", "total_lt", "total_eq", "pit",
                                   "location_pit", "day_pit", "total_pit")} | {f"samples/{k}" for k in CHECK_KEYS}


def test_off_calls_nothing_new_and_writes_todays_datasets(tmp_path):
    s0 = StubSampler()                                        # a sampler that has never heard of the check
    posts = [inf.Posterior(str(tmp_path / f"ref_{c}.npz"), s0.M, s0.T, 2, inf.warmup_size() + 8) for c in range(2)]
    inf.run_mcmc(s0, CFG, posts, log=open(os.devnull, "w"))
    for p in posts:
        p.close()
    plain, pf, log = _run(tmp_path, "plain", CFG)
    assert plain.calls == s0.calls and "Check" not in log
    assert not any(c[0] in ("reset_check", "check", "check_summary") for c in plain.calls)
    assert all(c[2] == {} for c in plain.calls if c[0] in ("sample", "burst"))
    ref = _read(str(tmp_path / "ref_1.npz"))
    assert set(pf[1]) == set(ref) and not (NEW_SETS & set(pf[1]))
    for k in ref:
        assert np.array_equal(pf[1][k], ref[k]), k
    with pytest.raises(ValueError, match="check_calendar"):
        _run(tmp_path, "nocal", dict(CFG, check=3), calendar=False)
    with pytest.raises(ValueError, match=r"check=6: the window is 1 .. min\(T = 5, 128\)"):
        _run(tmp_path, "long", dict(CFG, check=6))             # the stub's series has 5 days


@pytest.mark.parametrize("summaries,others,overlap,ext", [("off", False, True, ".npz"), ("on", True, True, ".hd5"),
                                                          ("only", True, False, ".npz")])
def test_on_resets_once_checks_every_burst_behind_the_others_and_writes_the_group(tmp_path, summaries, others, overlap, ext):
    if ext == ".hd5" and not hdf5io.available():
        ext = ".npz"
    nb, ns, K = 3, 4, 5
    cfg = dict(CFG, num_bursts=nb, num_burst_samples=ns, summaries=summaries, check=K, **(dict(forecast=4, rt=3) if others else {}))
    s, files, log = _run(tmp_path, "on", cfg, ext=ext, cap=800 if overlap else ns)
    names = [c[0] for c in s.calls]
    # reset once, after the last warm-up window and before the first burst; nothing during the warm-up
    assert names.count("reset_check") == 1 and names.count("check_summary") == 1
    r = names.index("reset_check")
    burst_name = "burst" if overlap else "sample"
    warm = [c for c in s.calls[:r] if c[0] == "sample"]
    assert len(warm) == 8 and all("check" not in c[2] for c in warm)
    assert not any(c[0] == "check" for c in s.calls[:r])
    reset = s.calls[r]
    assert reset[1] == K and np.array_equal(reset[2], np.arange(K) + 0.25) and np.array_equal(reset[3], np.arange(K) - 2.0)
    # the check's key is derived from the run's seed with the one named constant: never the forecast's key
    assert reset[4] == inf.check_seed(21) == (21 ^ inf.CHECK_SEED_SALT) and reset[4] != 21 and 0 <= reset[4] < 2 ** 64
    if others:
        assert [c for c in s.calls if c[0] == "reset_forecast"][0][4] == 21
    # one check per burst, behind the burst's forecast and R_t (the stub records a burst, then what its kwargs made it do)
    after = [c for c in s.calls[r:] if c[0] in (burst_name, "forecast", "rt", "check")]
    assert [c[0] for c in after] == ([burst_name, "forecast", "rt", "check"] if others else [burst_name, "check"]) * nb
    assert [c[2] for c in after if c[0] == "check"] == [0, ns, 2 * ns]
    for c in after:
        if c[0] == burst_name:
            assert c[2]["check"] is True and c[2].get("summarize", False) == (summaries != "off")
    # the files: today's datasets for this configuration, plus the group and the three per-draw datasets
    base, bf, _ = _run(tmp_path, "base", {k: v for k, v in cfg.items() if k != "check"}, ext=ext, cap=800 if overlap else ns)
    sweeps = inf.warmup_size() + np.arange(nb * ns)
    n = nb * ns
    for c, f in enumerate(files):
        assert set(f) == set(bf[c]) | NEW_SETS
        for k in bf[c]:
            assert np.array_equal(f[k], bf[c][k], equal_nan=True), k
        assert f["samples/check_by_day"].shape == (n, K, 3) and f["samples/check_by_location"].shape == (n, s.M, 3)
        assert f["samples/check_state_by_day"].shape == (n, K, 3)
        for k in CHECK_KEYS:
            assert f[f"samples/{k}"].dtype == np.int64
        assert np.array_equal(f["samples/check_by_day"][:, 0, 0], sweeps)         # one row per kept draw of the sampling phase
        assert np.array_equal(f["samples/check_state_by_day"][:, 2, 1], -sweeps)
        assert f["check/days"].reshape(-1)[0] == K and f["check/first_day"].reshape(-1)[0] == s.T - K
        assert f["check/count"].reshape(-1)[0] == n
        for k in ("seir_mean", "seir_var", "state_mean", "state_var"):
            assert f[f"check/{k}"].shape == (s.M, K, 3) and f[f"check/{k}"].dtype == np.float64
        np.testing.assert_allclose(f["check/seir_mean"], sweeps.mean(), rtol=1e-15)
        for k, shape in (("observed", (s.M, K)), ("lt", (s.M, K)), ("eq", (s.M, K)), ("pit", (s.M, K)), ("location_lt", (s.M,)),
                         ("location_eq", (s.M,)), ("location_pit", (s.M,)), ("day_lt", (K,)), ("day_eq", (K,)), ("day_pit", (K,)),
                         ("total_lt", (1,)), ("total_eq", (1,)), ("total_pit", (1,))):
            assert f[f"check/{k}"].shape == shape, k
        assert np.all(f["check/observed"] == 9) and np.all(f["check/lt"] == 3) and np.all(f["check/eq"] == 2)
        assert np.array_equal(f["check/pit"], np.full((s.M, K), 4.0 / n)) and np.array_equal(f["check/day_pit"], np.full(K, 1.5 / n))
        assert np.array_equal(f["check/location_lt"], [np.arange(s.M), np.full(s.M, n)][c])
        assert f["check/total_pit"].reshape(-1)[0] == (1.0, 0.5)[c] and f["check/total_lt"].reshape(-1)[0] == (n, 0)[c]
    # the log: pooled over the two chains, total (n + n / 2) / 2n; location totals (m + n) / 2n lie in [0.05, 0.95]
    assert log.count("Check:") == 1 and f"last {K} day(s) from day {s.T - K}" in log
    assert "national total mid-p 0.750" in log and "100.0 %" in log


# ---- 7. ChainSampler's own order of calls inside a burst ------------------------------------------------------------------
class CheckRecorder(Recorder):
    def __init__(self):
        super().__init__()
        self.state = self.state._replace(check_K=2)

    def __getattribute__(self, name):
        if name in ("check", "read_check_marginals_async"):
            calls = object.__getattribute__(self, "calls")
            return lambda *a, **kw: calls.append((name,) + a)
        return Recorder.__getattribute__(self, name)

    def read_check_marginals(self, n, first=0):
        self.calls.append(("read_check_marginals", n))
        return {k: np.zeros((n, self.B, e, 3), np.int64) for k, e in zip(CHECK_KEYS, (2, self.M, 2))}


def test_a_burst_is_checked_behind_its_summary_forecast_and_rt_and_not_at_all_when_off(monkeypatch):
    s = CheckRecorder()
    tr = s.sample(4, summarize=True, forecast=True, rt=True, check=True)
    assert [c[0] for c in s.calls] == ["snapshot", "reset_trace", "run", "summarize", "forecast", "rt", "check", "read_trace",
                                       "read_marginals", "read_forecast_marginals", "read_rt_draws", "read_check_marginals"]
    assert s.calls[6] == ("check", 0, 4) and tr.check["check_by_day"].shape == (4, s.B, 2, 3)
    s = CheckRecorder()
    tr = s.sample(4, summarize=True, forecast=True, rt=True)
    assert not any("check" in c[0] for c in s.calls) and tr.check is None
    s = CheckRecorder()
    s.state = s.state._replace(check_K=0)
    with pytest.raises(ValueError, match="before reset_check"):
        s.sample(4, check=True)
    import covid19uk_amd.sampler as sm

    class NoPin:
        def __init__(self, sampler, count, events=True, **kw):
            self.count, self.kw = count, kw
            self.theta = np.zeros((count, sampler.B, sampler.P))
            self.hmc, self.moves = np.zeros((count, sampler.B, 3)), np.zeros((count, sampler.B, 4, _lib.MOVE_TRACE))
            self.events = self.marginals = self.forecast = self.rt = None
            self.check = {k: np.zeros((count, sampler.B, 2, 3), np.int64) for k in CHECK_KEYS} if kw.get("check") else None

        def close(self):
            pass
    monkeypatch.setattr(sm, "PinnedTrace", NoPin)
    for on in (True, False):
        s = CheckRecorder()
        got = []
        s.sample_bursts(2, 4, lambda tr, i: got.append(tr.check), events=False, summarize=True, forecast=True, rt=True, check=on)
        names = [c[0] for c in s.calls]
        if on:
            assert names[:7] == ["snapshot", "reset_trace", "run", "summarize", "forecast", "rt", "check"]
            assert [c for c in s.calls if c[0] == "check"] == [("check", 0, 4), ("check", 4, 4)]
            assert [c[:3] for c in s.calls if c[0] == "read_check_marginals_async"] == \
                [("read_check_marginals_async", 4, 0), ("read_check_marginals_async", 4, 4)]
            assert all(g is not None for g in got) and s._pinned[0].kw["check"] == 2
        else:
            assert not any("check" in n for n in names) and got == [None, None] and "check" not in s._pinned[0].kw


# ---- 8. the compiler's account of the new kernels -------------------------------------------------------------------------
def test_the_new_kernels_have_no_scratch_and_fit_the_lds_and_the_old_ones_are_what_they_were():
    res = H.kernel_account("base")
    new = ["k_check_prepare<0>", "k_check_prepare<1>", "k_check_compare<0>", "k_check_compare<1>", "k_check_totals"]
    assert all(k in res for k in new), sorted(res)
    for k in new:
        assert res[k]["scratch_bytes_per_lane"] == 0 and res[k]["vgpr_spill"] == 0 and res[k]["sgpr_spill"] == 0, (k, res[k])
    # no new launch asks for dynamic LDS; the totals hold 128 day sums, the window's sum and two counters
    for k in new[:4]:
        assert res[k]["lds_bytes_per_block"] == 0, (k, res[k])
    assert res["k_check_totals"]["lds_bytes_per_block"] == 128 * 8 + 8 + 2 * 4
    # the compare keeps a (row, chain)'s counts in registers without costing occupancy
    assert res["k_check_compare<0>"]["occupancy_waves_per_simd"] == 8 and res["k_check_compare<1>"]["occupancy_waves_per_simd"] == 8
    # kernels were added: every instance of the parent is what it was
    parent = json.load(open(os.path.join(ROOT, "profiles", "r11_kernel_resources.json")))
    assert set(res) - set(parent) == set(new) and set(parent) <= set(res)
    for k in parent:
        if k.startswith(("k_forecast_", "k_summarize", "k_summary_finish", "k_gemm", "k_simulate")):
            assert res[k] == parent[k], k

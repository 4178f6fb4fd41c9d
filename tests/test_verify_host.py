"""Scoring the forecast against later data (include/seir_hip.h, "Scoring the forecast against later data"), on the host:
the entry points; the shared cell update (covid19uk_amd/csrc/verify_update.h) compiled as plain C++ against Python integers;
the NumPy definitions of `posterior.verify` against plain loops and `fractions.Fraction`; the truth's extraction and every
refusal; the options' resolution of its own; `run_mcmc` and the replay driver with a stub sampler; the kernels' account."""
import ctypes
import os
import shutil
import subprocess
import warnings
from fractions import Fraction

import numpy as np
import pytest

import __graft_entry__ as entry
from covid19uk_amd import _lib, hdf5io, kernel_resources
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.inference import options
from covid19uk_amd.posterior import replay as R
from covid19uk_amd.posterior import verify as V
from tests import abi_lib
from tests import helpers as H
from tests.test_forecast_host import ForecastStub
from tests.test_forecast_host import _run as _forecast_run
from tests.test_summary_host import CFG, _read

NEW = {
    "seir_sampler_verify_set": "seir_sampler *s, const int32_t *truth",
    "seir_sampler_verify_state": "seir_sampler *s, int64_t out[4]",
    "seir_sampler_read_verify": "seir_sampler *s, uint64_t *count, uint32_t *lt, uint32_t *eq, uint64_t *abs_sum",
    "seir_sampler_forecast_pair_sums": "seir_sampler *s, int32_t pooled, int64_t *out",
    "seir_pair_abs_sums": "seir_ctx *ctx, const int32_t *values, int64_t cells, int32_t segs, int64_t seg_len, int64_t seg_stride, "
                          "int64_t cell_stride, int64_t *out, uint32_t *overflow",
}


# ---- 1. the entry points ----------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound_with_the_headers_types():
    lib = abi_lib.check_symbols(NEW)
    text = open(abi_lib.HEADER).read()
    assert f"#define SEIR_PAIR_ABS_CHUNK {_lib.PAIR_ABS_CHUNK}" in text and f"#define SEIR_PAIR_ABS_MAX_N {_lib.PAIR_ABS_MAX_N}" in text
    # the largest n whose D cannot reach 2^63, and a chunk that is a power of two
    n = _lib.PAIR_ABS_MAX_N
    assert (n * n // 4) * (2 ** 32 - 1) < 2 ** 63 <= ((n + 1) ** 2 // 4) * (2 ** 32 - 1)
    assert _lib.PAIR_ABS_CHUNK & (_lib.PAIR_ABS_CHUNK - 1) == 0
    out = (ctypes.c_int64 * 4)()
    for call in (lambda: lib.seir_sampler_verify_set(None, None), lambda: lib.seir_sampler_verify_state(None, out),
                 lambda: lib.seir_sampler_read_verify(None, None, None, None, None),
                 lambda: lib.seir_sampler_forecast_pair_sums(None, 0, None)):
        assert call() == _lib.ERR_INVALID and b"null sampler" in lib.seir_last_error()
    assert lib.seir_pair_abs_sums(None, None, 1, 1, 1, 1, 1, None, None) == _lib.ERR_INVALID


# ---- 2. verify_update.h as plain C++ ------------------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include "verify_update.h"
// one cell: "y" first, then a draw x per line.  After every draw: lt eq abs_sum.
int main() {
    long long y, x;
    if (scanf("%lld", &y) != 1) return 1;
    uint32_t lt = 0, eq = 0; uint64_t ab = 0;
    while (scanf("%lld", &x) == 1) {
        seir::verify_cell_update(lt, eq, ab, (int64_t)x, (int64_t)y);
        printf("%u %u %llu\n", lt, eq, (unsigned long long)ab);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def update(tmp_path_factory):
    cxx = None
    for cand in ("g++", "c++", "clang++"):
        if shutil.which(cand):
            cxx = [cand]
            break
    if cxx is None:
        cxx = [entry._hipcc(), "-x", "c++"]
    d = tmp_path_factory.mktemp("verify_update")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run(cxx + ["-std=c++17", "-O1", "-Wall", "-Werror", "-I", entry.CSRC, "-o", str(exe), str(src)],
                   check=True, capture_output=True, text=True)

    def run(y, xs):
        text = "\n".join([str(y)] + [str(x) for x in xs]) + "\n"
        out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.split("\n")
        return [tuple(int(v) for v in row.split()) for row in out if row]
    return run


@pytest.mark.parametrize("y", [0, 1, 2 ** 31 - 1, 2 ** 31, 5 * 2 ** 31 + 3, -1])
def test_the_cell_update_equals_python_integers(update, y):
    """y at the extremes of int32, a running total past 2^31 (compared in int64), and -1: no truth, the cell keeps its zeros."""
    rng = np.random.default_rng(abs(y) % 1000)
    xs = [0, 2 ** 31 - 1, 2 ** 31, 7 * 2 ** 31, max(y, 0), max(y - 1, 0), y + 1] + [int(v) for v in rng.integers(0, 2 ** 34, 30)]
    lt = eq = ab = 0
    want = []
    for x in xs:
        if y >= 0:
            lt, eq, ab = lt + (x < y), eq + (x == y), ab + abs(x - y)
        want.append((lt, eq, ab))
    assert update(y, xs) == want


# ---- 3. the definitions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 64, 257])
def test_pair_sum_equals_a_plain_double_loop(n):
    rng = np.random.default_rng(n)
    for x in (rng.integers(-2 ** 31, 2 ** 31, n), rng.poisson(0.5, n), np.full(n, -2 ** 31), rng.choice([-2 ** 31, 2 ** 31 - 1], n)):
        want = sum(abs(int(x[i]) - int(x[j])) for i in range(n) for j in range(i + 1, n))
        got = V.pair_sum(x)
        assert got.dtype == np.int64 and int(got) == want
        assert int(V.pair_sum(x[::-1])) == want                            # no dependence on the draws' order
    x2 = rng.integers(-50, 50, size=(3, 4, n))
    assert np.array_equal(V.pair_sum(x2), [[V.pair_sum(r) for r in p] for p in x2])


def test_scores_equal_fractions_and_the_degenerate_samples():
    rng = np.random.default_rng(4)
    n = 23
    x = rng.poisson(3.0, size=(n, 5, 7, 2))
    y = rng.poisson(3.0, size=(5, 7, 2)).astype(np.int64)
    valid = np.ones(y.shape, bool)
    sc = V.score_draws(x, y, valid)
    for idx in np.ndindex(y.shape):
        xs, yy = [int(v) for v in x[(slice(None),) + idx]], int(y[idx])
        lt, eq = sum(v < yy for v in xs), sum(v == yy for v in xs)
        ab = sum(abs(v - yy) for v in xs)
        D = sum(abs(a - b) for i, a in enumerate(xs) for b in xs[i + 1:])
        assert (sc["lt"][idx], sc["eq"][idx], sc["abs_sum"][idx], sc["pair_sum"][idx]) == (lt, eq, ab, D)
        assert sc["pit"][idx] == float(Fraction(2 * lt + eq, 2 * n)) and sc["mae"][idx] == float(Fraction(ab, n))
        # the energy form with denominators n and n^2: E|X - y| - E|X - X'| / 2 over the empirical distribution
        crps = Fraction(ab, n) - Fraction(D, n * n)
        assert abs(sc["crps"][idx] - float(crps)) <= 4 * np.finfo(float).eps * max(float(Fraction(ab, n)), 1.0)
        assert crps == Fraction(ab, n) - Fraction(sum(abs(a - b) for a in xs for b in xs), 2 * n * n)
    # one draw, and all-equal draws: |x - y|
    one = V.score_draws(x[:1], y, valid)
    assert np.array_equal(one["crps"], np.abs(x[0] - y)) and not one["pair_sum"].any()
    same = V.score_draws(np.broadcast_to(x[:1], x.shape), y, valid)
    assert np.array_equal(same["crps"], np.abs(x[0] - y)) and np.array_equal(same["mae"], same["crps"])


def test_a_cell_without_truth_has_zeros_and_nan_scores_without_a_warning():
    x = np.arange(24).reshape(3, 2, 2, 2)
    truth = np.array([[4, -1], [-1, 5]], np.int32)
    y, valid = V.truth_targets(truth)
    assert np.array_equal(valid[..., 0], truth >= 0) and np.array_equal(valid[..., 1], [[True, False], [False, False]])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sc = V.score_draws(x, y, valid)
        none = V.scores(0, sc["lt"], sc["eq"], sc["abs_sum"], valid, sc["pair_sum"])
    for k in ("lt", "eq", "abs_sum", "pair_sum"):
        assert not sc[k][~valid].any(), k
    for k in ("pit", "mae", "crps"):
        assert np.isnan(sc[k][~valid]).all() and np.isfinite(sc[k][valid]).all() and np.isnan(none[k]).all(), k


def test_the_cum_mask_stops_at_the_first_gap_per_location_and_targets_are_the_stores_planes():
    truth = np.array([[1, 2, -1, 4, 5], [3, 0, 0, 1, 2], [-1, 1, 1, 1, 1]], np.int32)
    y, valid = V.truth_targets(truth)
    assert np.array_equal(valid[..., 1], [[1, 1, 0, 0, 0], [1, 1, 1, 1, 1], [0, 0, 0, 0, 0]])
    assert np.array_equal(y[..., 1], [[1, 3, -1, -1, -1], [3, 3, 3, 4, 6], [-1, -1, -1, -1, -1]])
    assert np.array_equal(y[..., 0], truth)
    ev = np.random.default_rng(0).integers(0, 9, size=(4, 3, 5, 3))
    t = V.targets(ev)
    assert np.array_equal(t[..., 0], ev[..., 2]) and np.array_equal(t[..., 1], np.cumsum(ev[..., 2], axis=-1))


def test_coverage_against_a_hand_case():
    probs = [0.05, 0.25, 0.5, 0.75, 0.9]
    assert V.interval_pairs(probs) == [(1, 3, 0.25)]
    assert V.interval_pairs([0.05, 0.5, 0.95]) == [(0, 2, 0.05)] and V.interval_pairs([0.5]) == []
    # three locations, two days, one target: y inside at (0,0), on the upper edge at (1,0), outside at (2,0); day 1: one valid cell, outside
    lo = np.array([[1.0, 0.0], [2.0, 0.0], [3.0, 0.0]])[..., None]
    hi = np.array([[5.0, 1.0], [4.0, 1.0], [4.0, 1.0]])[..., None]
    y = np.array([[3, 7], [4, 0], [9, 0]])[..., None]
    valid = np.array([[1, 1], [1, 0], [1, 0]], bool)[..., None]
    assert np.array_equal(V.coverage(lo, hi, y, valid), [[2 / 3], [0.0]])
    assert np.isnan(V.coverage(lo, hi, y, np.zeros_like(valid))).all()


# ---- 4. the truth and every refusal -------------------------------------------------------------------------------------
def _files(tmp_path, T=6, M=3, more=4, ext=".npz", revise=False, shift=False, cases_later=None):
    case = H.build_case("micro_3x1", 43)
    cov = case["cov"]
    rng = np.random.default_rng(0)
    cases = rng.poisson(5.0, size=(M, T + more)).astype(np.float64)
    dates = [str(np.datetime64("2021-01-01") + np.timedelta64(i + (1 if shift else 0), "D")) for i in range(T + more)]
    fitted, later = str(tmp_path / f"fit{ext}"), str(tmp_path / f"later{ext}")
    fit_dates = [str(np.datetime64("2021-01-01") + np.timedelta64(i, "D")) for i in range(T)]
    np.savez(fitted, C=cov.C, W=np.ones(T), N=cov.N, adjacency=cov.adjacency, weekday=np.zeros(T), area=cov.area,
             cases=cases[:, :T], time=np.array(fit_dates))
    lc = cases.copy() if cases_later is None else cases_later(cases.copy())
    if revise:
        lc[0, 1] += 2
        lc[2, 3] -= 1
    np.savez(later, C=cov.C, W=np.ones(T + more), N=cov.N, adjacency=cov.adjacency, weekday=np.zeros(T + more), area=cov.area,
             cases=lc, time=np.array(dates))
    return fitted, later, cases


def test_truth_extraction_partial_horizon_nan_negative_and_revised_history(tmp_path):
    def hole(c):
        c[1, 7] = np.nan
        c[2, 8] = -3
        return c
    fitted, later, cases = _files(tmp_path, revise=True, cases_later=hole)
    import io
    log = io.StringIO()
    tr = V.load_truth(later, fitted, 7, log=log)                # 4 of the 7 days are in the file
    assert tr.truth.dtype == np.int32 and tr.truth.shape == (3, 7) and tr.revised == 2
    want = np.full((3, 7), -1, np.int64)
    want[:, :4] = cases[:, 6:10]
    want[1, 1] = want[2, 2] = -1
    assert np.array_equal(tr.truth, want)
    assert "2 cell(s)" in log.getvalue() and "not refused" in log.getvalue()
    assert np.array_equal(V.load_truth(later, fitted, 2).truth, want[:, :2])


def _replay_refuses(tmp_path, monkeypatch, fitted, config, overrides, word):
    """`replay_files` on a readable posterior file refuses with `word` before a model, a sampler or an output file exists."""
    from covid19uk_amd import sampler as sampler_mod
    from covid19uk_amd import seir as seir_mod
    from tests.test_replay_host import _posterior_file

    def no_gpu(*a, **k):
        raise AssertionError("a GPU call before the refusal")
    monkeypatch.setattr(seir_mod, "SeirModel", no_gpu)
    monkeypatch.setattr(sampler_mod, "ChainSampler", no_gpu)
    M, T = np.load(fitted)["cases"].shape
    src, out = str(tmp_path / "src.npz"), str(tmp_path / "replay_out.npz")
    _posterior_file(src, M, T, 4)
    with pytest.raises(ValueError, match=word):
        R.replay_files(fitted, [src], out, config, first=0, log=open(os.devnull, "w"), **overrides)
    assert not os.path.exists(inf.chain_file_name(out, 0, 1)) and not os.path.exists(out)


@pytest.mark.parametrize("kind,word", [("fraction", "not integers"), ("rows", "locations"), ("dates", "dates"), ("empty", "no valid cell"),
                                       ("short", "dates")])
def test_every_refusal_of_the_truth_comes_with_no_gpu_call(tmp_path, monkeypatch, kind, word):
    def later(c):
        if kind == "fraction":
            c[0, 7] = 2.5
        if kind == "empty":
            c[:, 6:] = np.nan
        return c
    fitted, path, cases = _files(tmp_path, shift=kind == "dates", cases_later=later)
    d = dict(np.load(path))
    if kind == "rows":
        d["cases"] = d["cases"][:2]
    if kind == "short":
        d["cases"], d["time"] = d["cases"][:, :5], d["time"][:5]
    np.savez(path, **d)
    with pytest.raises(ValueError, match=word):
        V.load_truth(path, fitted, 3)
    # inference.mcmc and the replay: before any GPU call (neither gets as far as a model or a posterior file)
    out = str(tmp_path / "out.npz")
    with pytest.raises(ValueError, match=word):
        inf.mcmc(fitted, out, dict(CFG, forecast=3, verify=path))
    with pytest.raises(ValueError, match=word):
        inf.mcmc(fitted, out, dict(CFG, forecast=3), verify=path)
    assert not os.path.exists(out)
    _replay_refuses(tmp_path, monkeypatch, fitted, dict(CFG, forecast=3, verify=path), {}, word)
    _replay_refuses(tmp_path, monkeypatch, fitted, dict(CFG, forecast=3), dict(verify=path), word)


def test_the_resolution_is_its_own_and_verify_without_forecast_is_refused(tmp_path, monkeypatch):
    cfg = dict(num_bursts=2, num_burst_samples=4, forecast=5, verify="later.nc")
    section, opt = options.resolve_products(cfg)
    plain, opt0 = options.resolve_products({k: v for k, v in cfg.items() if k != "verify"})
    assert opt == opt0 and {k: v for k, v in section.items() if k != "verify"} == plain
    assert "verify" not in options.PRODUCT_KEYS and not hasattr(opt, "verify")
    assert options.resolve_verify(section, opt.horizon) == "later.nc" and options.resolve_verify(plain, opt.horizon) is None
    assert options.resolve_verify(section, opt.horizon, override="other.hd5") == "other.hd5"
    with pytest.raises(ValueError, match="needs a forecast"):
        options.resolve_verify(section, 0)
    with pytest.raises(ValueError, match="the path"):
        options.resolve_verify(dict(verify=3), 5)
    nofile, out = str(tmp_path / "no_such_file.nc"), str(tmp_path / "out.npz")
    with pytest.raises(ValueError, match="needs a forecast"):    # inference.mcmc: before the data file is opened
        inf.mcmc(nofile, out, dict(CFG, verify="later.nc"))
    fitted, later, _ = _files(tmp_path)
    _replay_refuses(tmp_path, monkeypatch, fitted, dict(CFG, verify=later), {}, "needs a forecast")      # the replay likewise
    s = ForecastStub()
    with pytest.raises(ValueError, match="needs a forecast"):
        inf.run_mcmc(s, dict(CFG, verify="later.nc"), [], log=open(os.devnull, "w"))
    with pytest.raises(ValueError, match="run_mcmc needs verify"):
        inf.run_mcmc(s, dict(CFG, forecast=3, verify="later.nc"), [], log=open(os.devnull, "w"), forecast_calendar=(np.ones(3), np.ones(3)))
    assert s.calls == []


# ---- 5. the compiler's account ------------------------------------------------------------------------------------------
def test_the_kernels_account_owner_verify_no_scratch_no_spills():
    res = H.kernel_account("verify")
    assert sorted(res) == ["k_pair_abs<256>", "k_verify_fold<2>"]
    assert kernel_resources.OWNERS["verify"] == ("k_verify_fold", "k_pair_abs")
    for k, v in res.items():
        assert v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch_bytes_per_lane"] == 0, (k, v)
    # keys 16 KB + int64 prefix sums 32 KB + the block's reduction words: under the 64 KB of a static allocation
    C = _lib.PAIR_ABS_CHUNK
    assert 12 * C <= res["k_pair_abs<256>"]["lds_bytes_per_block"] <= 12 * C + 128
    assert res["k_verify_fold<2>"]["lds_bytes_per_block"] == 2 * 128 * 8


# ---- 6. run_mcmc and the replay driver with a stub sampler; the datasets --------------------------------------------------
READS = ("verify_summary", "forecast_pair_sums")
BASE_SETS = {f"verify/{k}" for k in ("truth", "valid", "horizon", "first_day", "count", "lt", "eq", "abs_sum", "pit", "mae",
                                      "national_truth", "national_valid", "national_lt", "national_eq", "national_abs_sum",
                                      "national_pair_sum", "national_pit", "national_mae", "national_crps")}
STORE_SETS = {f"verify/{k}" for k in ("pair_sum", "crps", "pooled_pair_sum", "pooled_crps", "pooled_chains", "coverage_probs",
                                       "coverage", "pooled_coverage")}


class VerifyCalls:
    """The verification's calls on a stub sampler: a draw's every cell is its sweep number modulo 5 (cases) and that times
    s + 1 (cum_cases); the accumulators are the NumPy fold of those draws."""

    def set_verify(self, truth):
        self.calls.append(("set_verify", np.array(truth)))
        self.truth = np.array(truth)

    def draws(self):
        r = np.asarray(self.forecast_rows, np.int64) % 5
        ev = np.zeros((len(r), self.B, self.M, self.H, 3), np.int64)
        ev[..., 2] = r[:, None, None, None]
        return V.targets(ev)                                    # [n,B,M,H,2]

    def verify_summary(self):
        self.calls.append(("verify_summary",))
        y, valid = V.truth_targets(self.truth)
        x = self.draws()
        f = [V.fold(x[:, b], y, valid) for b in range(self.B)]
        return dict(count=np.full(self.B, len(x), np.uint64), **{k: np.stack([p[k] for p in f]) for k in ("lt", "eq", "abs_sum")})

    def forecast_pair_sums(self, pooled=False):
        self.calls.append(("forecast_pair_sums", pooled))
        x = self.draws()
        if pooled:
            return np.moveaxis(V.pair_sum(np.moveaxis(x.reshape((-1,) + x.shape[2:]), 0, -1)), -1, 0)
        return np.moveaxis(V.pair_sum(np.moveaxis(x, 0, -1)), -1, 1)

    def replay(self, theta, events, **kw):
        n = theta[0].shape[0]
        self.calls.append(("replay", n, kw))
        tr = self._trace(n, events=False, **kw)
        tr.theta = np.stack(theta, axis=1)
        return tr


class VerifyStub(VerifyCalls, ForecastStub):
    """ForecastStub with the draw store and the verification."""

    def keep_forecast_draws(self, cap):
        self.calls.append(("keep_forecast_draws", cap))

    def forecast_quantiles(self, probs, pooled=False):
        self.calls.append(("forecast_quantiles", pooled))
        q = np.array(probs)[(slice(None),) + (None,) * (3 if pooled else 4)] * 8.0
        return np.broadcast_to(q, (len(probs),) + (() if pooled else (self.B,)) + (3, self.M, self.H)).copy()


def _truth(s, Hn):
    t = np.full((s.M, Hn), 2, np.int32)
    t[0, Hn - 1] = -1
    t[s.M - 1, 1] = -1
    return V.Truth(truth=t, revised=0, path="later.npz")


def _run(tmp_path, tag, config, ext=".npz", truth=None):
    s = VerifyStub()
    s.cap = 800
    nb, ns = config["num_bursts"], config["num_burst_samples"]
    Hn, _ = inf.forecast_mode(config)
    names = [str(tmp_path / f"{tag}_{c}{ext}") for c in range(s.B)]
    posts = [inf.Posterior(name, s.M, s.T, 2, inf.warmup_size() + nb * ns, **(dict(forecast=(Hn, nb * ns)) if Hn else {})) for name in names]
    logname = str(tmp_path / f"{tag}.log")
    kw = dict(forecast_calendar=(np.arange(Hn) + 0.5, np.arange(Hn) - 1.0), seed=21) if Hn else {}
    if truth is not None:
        kw["verify"] = truth
    with open(logname, "w") as log:
        inf.run_mcmc(s, config, posts, log=log, **kw)
    for p in posts:
        p.close()
    return s, [_read(n) for n in names], open(logname).read()


def _same_calls(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x) == len(y) and x[0] == y[0]
        for u, v in zip(x[1:], y[1:]):
            if isinstance(u, dict):
                assert set(u) == set(v), (x[0], set(u), set(v))        # the products' keyword sets
            elif not callable(u):
                assert np.array_equal(u, v), x[0]


@pytest.mark.parametrize("ext,store", [(".npz", True), (".hd5", True), (".npz", False)])
def test_run_mcmc_sets_once_behind_reset_and_store_reads_once_and_writes_the_datasets(tmp_path, ext, store):
    assert hdf5io.available()
    Hn, nb, ns = 4, CFG["num_bursts"], CFG["num_burst_samples"]
    n = nb * ns
    cfg = dict(CFG, forecast=Hn, verify="later.npz", **(dict(forecast_quantiles=[0.25, 0.5, 0.75]) if store else {}))
    probe = VerifyStub()
    truth = _truth(probe, Hn)
    s, files, log = _run(tmp_path, "on", cfg, ext, truth)
    names = [c[0] for c in s.calls]
    # set once, behind the forecast's reset and its draw store, before the first burst; one read of each kind at the end
    i = names.index("set_verify")
    assert names.count("set_verify") == 1 and np.array_equal(s.calls[i][1], truth.truth) and "forecast" not in names[:i]
    assert names[i - 2:i] == (["reset_forecast", "keep_forecast_draws"] if store else names[i - 2:i]) and names[i - 1] != "sample"
    assert names.count("verify_summary") == 1
    assert [c[1] for c in s.calls if c[0] == "forecast_pair_sums"] == ([False, True] if store else [])
    last = max(j for j, nm in enumerate(names) if nm == "forecast")
    assert all(j > last for j, nm in enumerate(names) if nm in READS)
    # the same run without the key: nothing of it is called, every other call and the products' keyword sets are what they were
    plain = {k: v for k, v in cfg.items() if k != "verify"}
    base, bfiles, blog = _run(tmp_path, "base", plain, ext)
    assert not any(c[0] in READS + ("set_verify",) for c in base.calls) and "Verify" not in blog
    _same_calls([c for c in s.calls if c[0] not in READS + ("set_verify",)], base.calls)
    keep = lambda text, drop: [l for l in text.split("\n") if not l.startswith(drop)]      # noqa: E731  ("Sampling:" holds a timing)
    assert keep(log, ("Verify:", "Sampling:")) == keep(blog, ("Sampling:",))
    y, valid = V.truth_targets(truth.truth)
    x = s.draws()
    for c, f in enumerate(files):
        assert set(f) - set(bfiles[c]) == BASE_SETS | (STORE_SETS if store else set()) and set(bfiles[c]) <= set(f)
        for k in bfiles[c]:
            assert np.array_equal(f[k], bfiles[c][k]), k
        want = V.score_draws(x[:, c], y, valid)
        assert np.array_equal(f["verify/truth"], truth.truth) and np.array_equal(f["verify/valid"], valid)
        assert (f["verify/horizon"], f["verify/first_day"], f["verify/count"]) == ([Hn], [s.T], [n])
        for k in ("lt", "eq", "abs_sum"):
            assert f[f"verify/{k}"].shape == (s.M, Hn, 2) and np.array_equal(f[f"verify/{k}"], want[k]), k
        for k in ("pit", "mae"):
            assert np.array_equal(f[f"verify/{k}"], want[k], equal_nan=True), k
        assert np.isnan(f["verify/pit"][0, Hn - 1]).all() and np.isnan(f["verify/mae"][s.M - 1, 1:, 1]).all()
        # the national scores, from the per-draw curves that are in the file
        nat_t = np.where((truth.truth >= 0).all(0), np.where(truth.truth >= 0, truth.truth, 0).sum(0), -1)[None]
        yn, vn = V.truth_targets(nat_t)
        nat = V.score_draws(V.targets(f["samples/forecast_by_day"][:, None]), yn, vn)
        for k in ("lt", "eq", "abs_sum", "pair_sum", "pit", "mae", "crps"):
            assert np.array_equal(f[f"verify/national_{k}"], nat[k][0], equal_nan=True), k
        if store:
            assert np.array_equal(f["verify/pair_sum"], want["pair_sum"]) and np.array_equal(f["verify/crps"], want["crps"], equal_nan=True)
            pooled = V.score_draws(x.reshape((-1,) + x.shape[2:]), y, valid)
            assert np.array_equal(f["verify/pooled_pair_sum"], pooled["pair_sum"])
            assert np.array_equal(f["verify/pooled_crps"], pooled["crps"], equal_nan=True)
            assert np.array_equal(f["verify/pooled_chains"], [6, 7][:s.B] if s.B <= 2 else f["verify/pooled_chains"])
            # quantiles 2, 4, 6 everywhere: y = 2 of cases is inside [2, 6]; of cum_cases 2 (s + 1) only on days 0..2
            assert np.array_equal(f["verify/coverage_probs"], [0.25]) and f["verify/coverage"].shape == (1, Hn, 2)
            assert np.array_equal(f["verify/coverage"][0, :, 0], np.ones(Hn))
            assert np.array_equal(f["verify/coverage"][0, :, 1], [1.0, 1.0, 1.0, 0.0][:Hn])
            assert np.array_equal(f["verify/coverage"], f["verify/pooled_coverage"])
    lines = [l for l in log.split("\n") if l.startswith("Verify:")]
    assert len(lines) == 1 and "mid-p within [0.05, 0.95]" in lines[0] and "forecast day 1: observed 6," in lines[0]      # day 1 of row M - 1 is missing
    assert ("mean CRPS over" in lines[0]) == store and ("no draw store: set forecast_quantiles for CRPS" in lines[0]) != store


def test_the_pooled_rule_over_two_files_is_a_sum_and_the_pair_sum_is_not(tmp_path):
    Hn = 3
    cfg = dict(CFG, forecast=Hn, verify="later.npz", forecast_quantiles=[0.25, 0.75])
    probe = VerifyStub()
    truth = _truth(probe, Hn)
    s, files, _ = _run(tmp_path, "two", cfg, ".npz", truth)
    assert len(files) >= 2
    n = int(files[0]["verify/count"][0])
    parts = [dict(count=n, **{k: f[f"verify/{k}"] for k in ("lt", "eq", "abs_sum")}) for f in files]
    pooled = V.pool(parts)
    y, valid = V.truth_targets(truth.truth)
    x = s.draws()
    want = V.score_draws(x.reshape((-1,) + x.shape[2:]), y, valid)
    for k in ("lt", "eq", "abs_sum"):
        assert np.array_equal(pooled[k], want[k]), k
    assert pooled["count"] == n * len(files)
    sc = V.scores(pooled["count"], pooled["lt"], pooled["eq"], pooled["abs_sum"], valid, files[0]["verify/pooled_pair_sum"])
    assert np.array_equal(sc["crps"], want["crps"], equal_nan=True) and np.array_equal(sc["pit"], want["pit"], equal_nan=True)
    # the chains' own pair sums do not add up to the pooled one: the cross pairs are missing
    assert (sum(f["verify/pair_sum"] for f in files) < files[0]["verify/pooled_pair_sum"])[valid].all()


def test_the_key_absent_calls_nothing(tmp_path):
    s0, ref, log0 = _forecast_run(tmp_path, "ref", dict(CFG, forecast=3))       # a sampler that has never heard of verify
    s1, got, log1 = _run(tmp_path, "plain", dict(CFG, forecast=3))
    assert [c[0] for c in s1.calls] == [c[0] for c in s0.calls]
    assert [l for l in log1.split("\n") if not l.startswith("Sampling:")] == [l for l in log0.split("\n") if not l.startswith("Sampling:")]
    assert set(got[1]) == set(ref[1]) and all(np.array_equal(got[1][k], ref[1][k]) for k in ref[1])


@pytest.mark.parametrize("store", [False, True])
def test_the_replay_driver_sets_once_and_reads_once(tmp_path, store):
    Hn, n, burst = 3, 7, 3
    cfg = dict(CFG, forecast=Hn, verify="later.npz", num_burst_samples=burst, num_bursts=3, thin=1,
               **(dict(forecast_quantiles=[0.25, 0.75]) if store else {}))

    class Source:
        def __init__(self, c, P, M, T):
            rng = np.random.default_rng(c)
            self.path, self.theta, self.events = f"c{c}", rng.standard_normal((n, P)), rng.integers(0, 3, size=(n, M, T, 3)).astype(np.float64)

        def draws(self, rows):
            return self.theta[rows], self.events[rows]
    runs = {}
    for on in (True, False):
        s = VerifyStub()
        config = cfg if on else {k: v for k, v in cfg.items() if k != "verify"}
        names = [str(tmp_path / f"rp{int(on)}_{c}.npz") for c in range(s.B)]
        posts = [inf.Posterior(name, s.M, s.T, 2, n, burst=burst, results=False, forecast=(Hn, n)) for name in names]
        with open(os.devnull, "w") as log:
            pr = inf.product_records(s, config, posts, log=log, seed=21, forecast_calendar=(np.ones(Hn), np.zeros(Hn)), total=n, results=False,
                                     **(dict(verify=_truth(s, Hn)) if on else {}))
            R.replay_bursts(s, [Source(c, s.P, s.M, s.T) for c in range(s.B)], np.arange(n), burst, pr, log=log)
        for p in posts:
            p.close()
        runs[on] = (s, [_read(name) for name in names])
    s, files = runs[True]
    names = [c[0] for c in s.calls]
    i = names.index("set_verify")
    assert names.count("set_verify") == 1 and names[i - 1] == ("keep_forecast_draws" if store else "reset_forecast")
    assert "replay" not in names[:i] and (not store or names[i - 2] == "reset_forecast")
    assert names.count("verify_summary") == 1 and names.count("replay") == 3
    assert [c[1] for c in s.calls if c[0] == "forecast_pair_sums"] == ([False, True] if store else [])      # one read of each kind
    last = max(j for j, nm in enumerate(names) if nm == "replay")
    assert all(j > last for j, nm in enumerate(names) if nm in READS)
    _same_calls([c for c in s.calls if c[0] not in READS + ("set_verify",)], runs[False][0].calls)
    assert set(files[0]) - set(runs[False][1][0]) == BASE_SETS | (STORE_SETS if store else set())
    assert files[0]["verify/count"] == [n]


def test_the_flag_is_on_both_command_lines_and_absent_it_passes_nothing(tmp_path, monkeypatch):
    import yaml
    cpath = str(tmp_path / "c.yaml")
    with open(cpath, "w") as f:
        yaml.safe_dump(dict(Mcmc=CFG), f)
    seen = {}
    monkeypatch.setattr(inf, "mcmc", lambda *a, **kw: seen.update(kw=kw))
    inf.main(["-c", cpath, "-o", "x", "--forecast", "14", "--forecast-quantiles", "0.05,0.5,0.95", "--verify", "later.nc", "data.nc"])
    assert seen["kw"]["verify"] == "later.nc" and seen["kw"]["forecast"] == 14
    inf.main(["-c", cpath, "-o", "x", "--forecast", "14", "data.nc"])
    assert "verify" not in seen["kw"]
    monkeypatch.setattr(R, "replay_files", lambda *a, **kw: seen.update(kw=kw))
    R.main(["-c", cpath, "-o", "x", "--forecast", "14", "--verify", "later.nc", "data.nc", "p0.hd5"])
    assert seen["kw"]["verify"] == "later.nc"
    R.main(["-c", cpath, "-o", "x", "--forecast", "14", "data.nc", "p0.hd5"])
    assert "verify" not in seen["kw"]


# ---- 7. the groups' scores; the pooled pair sum's bound ---------------------------------------------------------------------
from covid19uk_amd.posterior import groups as G  # noqa: E402
from tests.test_groups_host import GroupStub  # noqa: E402

TABLE = G.parse_groups({"all": [0, 1, 2], "ends": [0, 2]}, 3)
GROUP_SETS = {f"verify/group_{k}" for k in ("truth", "valid", "lt", "eq", "abs_sum", "pair_sum", "pit", "mae", "crps")}


class VerifyGroupStub(VerifyCalls, GroupStub):
    """GroupStub (the draw store, the group sums of every forecast draw) with the verification."""


@pytest.mark.parametrize("ext", [".npz", ".hd5"])
def test_with_groups_the_group_scores_are_written_from_the_group_curves(tmp_path, ext):
    Hn = 4
    cfg = dict(CFG, forecast=Hn, forecast_quantiles=[0.25, 0.75], verify="later.npz")
    runs = {}
    for on in (True, False):
        s = VerifyGroupStub()
        s.cap = 800
        nb, ns = cfg["num_bursts"], cfg["num_burst_samples"]
        truth = _truth(s, Hn)
        names = [str(tmp_path / f"g{int(on)}_{c}{ext}") for c in range(s.B)]
        posts = [inf.Posterior(name, s.M, s.T, 2, inf.warmup_size() + nb * ns, forecast=(Hn, nb * ns), groups=TABLE.G) for name in names]
        for p in posts:
            p.write_groups(TABLE, np.array([10.0, 20.0, 40.0]), np.arange(12.0).reshape(3, 4))
        with open(os.devnull, "w") as log:
            inf.run_mcmc(s, cfg if on else {k: v for k, v in cfg.items() if k != "verify"}, posts, log=log, seed=21, groups=TABLE,
                         forecast_calendar=(np.arange(Hn) + 0.5, np.arange(Hn) - 1.0), **(dict(verify=truth) if on else {}))
        for p in posts:
            p.close()
        runs[on] = (s, [_read(n) for n in names])
    s, files = runs[True]
    assert s.M == 3
    t = truth.truth.astype(np.int64)
    # a group's truth: the sum over its members where every member is observed ("all": rows 0, 1, 2; "ends": rows 0, 2)
    want_t = np.stack([np.where((t[r] >= 0).all(0), np.where(t[r] >= 0, t[r], 0).sum(0), -1) for r in ([0, 1, 2], [0, 2])])
    yg, vg = V.truth_targets(want_t)
    assert (want_t[:, Hn - 1] == -1).all() and want_t[0, 1] == -1 and want_t[1, 1] == -1 and (want_t[:, 0] == [6, 4]).all()
    for c, f in enumerate(files):
        assert set(f) - set(runs[False][1][c]) == BASE_SETS | STORE_SETS | GROUP_SETS
        assert np.array_equal(f["verify/group_truth"], want_t) and np.array_equal(f["verify/group_valid"], vg)
        want = V.score_draws(V.targets(f["samples/forecast_by_group"]), yg, vg)
        assert want["abs_sum"].any() and f["verify/group_crps"].shape == (2, Hn, 2)
        for k in ("lt", "eq", "abs_sum", "pair_sum", "pit", "mae", "crps"):
            assert np.array_equal(f[f"verify/group_{k}"], want[k], equal_nan=True), k


def test_a_pooled_cell_above_the_pair_sums_bound_is_skipped_with_a_line_and_a_chain_above_it_refused(tmp_path, monkeypatch):
    """10 chains x 10 000 kept draws are above `PAIR_ABS_MAX_N` values per pooled cell: known before the first GPU call.  The
    pooled pair sum is then not asked for (the library would refuse it at the end of the run), the chains' own are; a run whose
    chains alone are above the bound is refused before any call.  The bound is lowered here in the place of a long run."""
    Hn = 3
    cfg = dict(CFG, forecast=Hn, forecast_quantiles=[0.25, 0.75], verify="later.npz")
    n = cfg["num_bursts"] * cfg["num_burst_samples"]
    probe = VerifyStub()
    assert probe.B >= 2
    monkeypatch.setattr(_lib, "PAIR_ABS_MAX_N", n * probe.B - 1)
    s, files, log = _run(tmp_path, "skip", cfg, ".npz", _truth(probe, Hn))
    assert [c[1] for c in s.calls if c[0] == "forecast_pair_sums"] == [False]
    assert f"{probe.B} chain(s) x {n} kept draws are {probe.B * n} values per pooled cell" in log
    for f in files:
        assert set(f) >= (BASE_SETS | STORE_SETS) - {"verify/pooled_pair_sum", "verify/pooled_crps"}
        assert "verify/pooled_pair_sum" not in f and "verify/pooled_crps" not in f and np.isfinite(f["verify/crps"][0, 0]).all()
    line = [l for l in log.split("\n") if l.startswith("Verify: national")]
    assert len(line) == 1 and "mean CRPS over" in line[0]
    monkeypatch.setattr(_lib, "PAIR_ABS_MAX_N", n * probe.B)         # exactly at the bound: pooled
    s, files, log = _run(tmp_path, "at", cfg, ".npz", _truth(probe, Hn))
    assert [c[1] for c in s.calls if c[0] == "forecast_pair_sums"] == [False, True] and "verify/pooled_crps" in files[0]
    monkeypatch.setattr(_lib, "PAIR_ABS_MAX_N", n - 1)
    s = VerifyStub()
    with pytest.raises(ValueError, match="kept draws per chain"):
        inf.run_mcmc(s, cfg, [], log=open(os.devnull, "w"), forecast_calendar=(np.ones(Hn), np.ones(Hn)), verify=_truth(probe, Hn))
    assert s.calls == []

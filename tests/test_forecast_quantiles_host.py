"""Host side of the forecast intervals (include/seir_hip.h, "Forecast intervals on the device"), no GPU: the symbols, the
narrowing step of the radix select (covid19uk_amd/csrc/order_select.h, the one definition k_order_stats calls) compiled as
plain C++ and driven against Python's sorted(), the rank rule against fractions.Fraction and np.quantile, the
configuration and the command line, run_mcmc's call sequence with a stub sampler, the datasets written, and the
compiler's account of the two new kernels."""
import ctypes
import json
import math
import os
import re
import shutil
import subprocess
import warnings
from fractions import Fraction

import numpy as np
import pytest

import __graft_entry__ as entry
from covid19uk_amd import _lib, hdf5io
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.posterior import quantiles as Q
from covid19uk_amd.sampler import FORECAST_QUANTILE_PLANES, ChainSampler
from tests import helpers as H
from tests.abi_lib import check_symbols
from tests.test_forecast_host import ForecastStub
from tests.test_summary_host import CFG, _read

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "seir_sampler_forecast_keep": "seir_sampler *s, int64_t cap",
    "seir_sampler_forecast_order_stats": "seir_sampler *s, const int64_t *ranks, int32_t R, int32_t pooled, int32_t *out",
    "seir_order_stats": "seir_ctx *ctx, const int32_t *values, int64_t cells, int32_t segs, int64_t seg_len, "
                        "int64_t seg_stride, int64_t cell_stride, const int64_t *ranks, int32_t R, int32_t *out",
}


# ---- 1. the symbols ------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound_with_the_headers_types():
    lib = check_symbols(NEW)
    raw = open(os.path.join(ROOT, "include", "seir_hip.h")).read()
    assert int(re.search(r"#define SEIR_ORDER_STATS_MAX_RANKS (\d+)", raw).group(1)) == _lib.ORDER_STATS_MAX_RANKS == 16
    assert 2 * Q.MAX_PROBS == _lib.ORDER_STATS_MAX_RANKS
    # a null sampler / context is refused before anything touches a device
    one = (ctypes.c_int64 * 1)(0)
    out = (ctypes.c_int32 * 1)(0)
    assert lib.seir_sampler_forecast_keep(None, 5) == _lib.ERR_INVALID
    assert lib.seir_sampler_forecast_order_stats(None, one, 1, 0, out) == _lib.ERR_INVALID
    assert lib.seir_order_stats(None, out, 1, 1, 1, 1, 1, one, 1, out) == _lib.ERR_INVALID
    for name in ("keep_forecast_draws", "forecast_order_stats", "forecast_quantiles"):
        assert callable(getattr(ChainSampler, name))
    assert FORECAST_QUANTILE_PLANES == ("cases", "cum_cases", "prevalence")


# ---- 2. the narrowing step, as plain C++ -----------------------------------------------------------------------------------
DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include <unordered_map>
#include <vector>
#include "order_select.h"
// stdin: n, then n values.  stdout: for every rank 0 .. n-1 the value the four-pass select arrives at, one per line.
// As in k_order_stats, ranks whose prefixes agree share a histogram, and a value is counted under the prefix it matches.
int main() {
    long long n;
    if (std::scanf("%lld", &n) != 1 || n < 1) return 2;
    std::vector<int32_t> v((size_t)n);
    for (auto &x : v) { long long t; if (std::scanf("%lld", &t) != 1) return 2; x = (int32_t)t; }
    std::vector<uint32_t> prefix((size_t)n, 0u), rem((size_t)n);
    for (long long r = 0; r < n; ++r) rem[(size_t)r] = (uint32_t)r;
    static_assert(seir::ORDER_PASSES == 4 && seir::ORDER_BINS == 256 && seir::ORDER_MAX_RANKS == 16, "8-bit digits, four passes");
    for (int pass = 0; pass < seir::ORDER_PASSES; ++pass) {
        std::unordered_map<uint32_t, std::vector<uint32_t>> hist;
        for (uint32_t p : prefix) if (!hist.count(p)) hist[p] = std::vector<uint32_t>(seir::ORDER_BINS, 0u);
        const int sh = seir::order_shift<uint32_t>(pass);
        for (int32_t x : v) {
            const uint32_t key = seir::order_key(x);
            if (seir::order_value(key) != x) return 3;
            const uint32_t high = pass == 0 ? 0u : key & ~((1u << (sh + seir::ORDER_DIGIT_BITS)) - 1u);
            auto it = hist.find(high);
            if (it == hist.end()) continue;
            if (!seir::order_matches(key, it->first, pass)) return 4;
            it->second[seir::order_digit(key, pass)] += 1u;
        }
        for (long long r = 0; r < n; ++r)
            if (!seir::order_select_narrow(hist[prefix[(size_t)r]].data(), pass, prefix[(size_t)r], rem[(size_t)r])) return 5;
    }
    for (long long r = 0; r < n; ++r) {
        if (rem[(size_t)r] >= (uint32_t)n) return 6;
        std::printf("%" PRId32 "\n", seir::order_value(prefix[(size_t)r]));
    }
    // a rank past the count is refused, and the state is left alone
    std::vector<uint32_t> h(seir::ORDER_BINS, 0u);
    h[7] = 3;
    uint32_t p = 0x12000000u, k = 3;
    if (seir::order_select_narrow(h.data(), 1, p, k) || p != 0x12000000u || k != 3) return 7;
    k = 2;
    if (!seir::order_select_narrow(h.data(), 1, p, k) || p != 0x12070000u || k != 2) return 8;
    return 0;
}
"""
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
SIZES = (1, 2, 3, 255, 256, 257, 5000)


def value_families(n, seed=0):
    """The arrays both test files hold the select to: name -> n Python ints in int32."""
    rng = np.random.default_rng([seed, n])
    one = [0] * n
    one[n // 2] = 9
    mix = [(INT_MIN, -1, 0, INT_MAX)[i % 4] for i in range(n)]
    rng.shuffle(mix)
    return {
        "all_equal": [123456] * n,
        "two_valued": [int(v) for v in rng.choice([5, -70000], size=n)],
        "zeros_but_one": one,
        "extremes": [int(v) for v in mix],
        "lowest_digit": [int(v) for v in 0x01020300 + rng.integers(0, 256, size=n)],
        "highest_digit": [int(v) for v in ((rng.integers(0, 256, size=n) << 24) - 2 ** 31) | 0x00ABCDEF],
        "random": [int(v) for v in rng.integers(INT_MIN, INT_MAX, size=n, endpoint=True)],
        "zero_heavy_counts": [int(v) for v in rng.poisson(0.4, size=n)],
    }


@pytest.fixture(scope="module")
def select(tmp_path_factory):
    cxx = None
    try:
        cxx = [entry._hipcc(), "-x", "c++"]
    except RuntimeError:
        for cand in ("g++", "c++", "clang++"):
            if shutil.which(cand):
                cxx = [cand]
                break
    assert cxx, "no C++ compiler"
    d = tmp_path_factory.mktemp("order_select")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run(cxx + ["-std=c++17", "-O1", "-Wall", "-Werror", "-I", entry.CSRC, "-o", str(exe), str(src)],
                   check=True, capture_output=True, text=True)

    def run(xs):
        text = f"{len(xs)}\n" + " ".join(str(int(v)) for v in xs) + "\n"
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr)
        return [int(v) for v in r.stdout.split()]
    return run


@pytest.mark.parametrize("n", SIZES)
def test_the_four_pass_select_equals_sorted_for_every_rank(select, n):
    for name, xs in value_families(n).items():
        assert len(xs) == n and min(xs) >= INT_MIN and max(xs) <= INT_MAX
        assert select(xs) == sorted(xs), name
    fam = value_families(max(n, 4))
    assert set(fam["extremes"]) == {INT_MIN, -1, 0, INT_MAX}
    assert len({v >> 8 for v in fam["lowest_digit"]}) == 1 and len({v & 0xFFFFFF for v in fam["highest_digit"]}) == 1
    if n >= 255:
        assert len(set(fam["lowest_digit"])) > 100 and len(set(fam["highest_digit"])) > 100


# ---- 3. the rank rule ------------------------------------------------------------------------------------------------------
PROBS = (0.0, 0.05, 0.5, 0.95, 1.0, 1.0 / 3.0)


@pytest.mark.parametrize("n", [1, 2, 7, 100, 5000])
def test_ranks_are_floor_and_ceil_of_p_n_minus_1(n):
    for p in PROBS:
        h = Fraction(p * (n - 1))                            # the fp64 product NumPy forms, as an exact number
        assert abs(h - Fraction(p) * (n - 1)) <= Fraction(n, 2 ** 52)
        want = sorted({math.floor(h), math.ceil(h)})
        got = Q.quantile_ranks(n, [p])
        assert got.dtype == np.int64 and got.tolist() == want, (n, p)
        assert 0 <= want[0] <= want[-1] <= n - 1
    allr = Q.quantile_ranks(n, PROBS)
    want = sorted({f(Fraction(p * (n - 1))) for p in PROBS for f in (math.floor, math.ceil)})
    assert allr.tolist() == want and len(set(allr.tolist())) == len(allr) <= 2 * len(PROBS)
    if n == 5000:                                            # the example configuration: 0.05 x 4999 = 249.95
        assert Q.quantile_ranks(n, [0.05, 0.5, 0.95]).tolist() == [249, 250, 2499, 2500, 4749, 4750]
    for bad in ([-0.1], [1.5]):
        with pytest.raises(ValueError):
            Q.quantile_ranks(n, bad)
    with pytest.raises(ValueError):
        Q.quantile_ranks(0, [0.5])


@pytest.mark.parametrize("n", [1, 2, 7, 100, 5000])
def test_interpolate_equals_numpy_quantile(n):
    rng = np.random.default_rng(n)
    x = np.concatenate([rng.poisson(0.7, size=(n, 5)), rng.integers(0, 2 ** 31 - 1, size=(n, 4))], axis=1).astype(np.int64)
    srt = np.sort(x, axis=0)
    ranks = Q.quantile_ranks(n, PROBS)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = Q.interpolate(srt[ranks].astype(np.int32), ranks, n, PROBS)
    assert got.dtype == np.float64 and got.shape == (len(PROBS), 9)
    np.testing.assert_allclose(got, np.quantile(x, PROBS, axis=0), rtol=1e-12, atol=0)
    for k, p in enumerate(PROBS):
        h = Fraction(p * (n - 1))
        if h.denominator == 1:                               # an integer index: the order statistic itself
            assert np.array_equal(got[k], srt[int(h)].astype(np.float64)), (n, p)
    if n == 1:
        assert all(np.array_equal(got[k], x[0].astype(np.float64)) for k in range(len(PROBS)))


# ---- 4. configuration and command line -------------------------------------------------------------------------------------
def test_probabilities_are_parsed_and_bad_ones_refused_before_any_gpu_call(tmp_path):
    mode = inf.forecast_quantiles_mode
    assert mode({}) == () and mode(dict(CFG, forecast=14)) == ()
    assert mode(dict(CFG, forecast=14, forecast_quantiles=[0.05, 0.5, 0.95]), horizon=14) == (0.05, 0.5, 0.95)
    assert mode(dict(CFG, forecast_quantiles=[0.5]), "0.05,0.5,0.95", horizon=7) == (0.05, 0.5, 0.95)   # the command line overrides
    assert mode(CFG, "0, 1") == (0.0, 1.0) and mode(CFG, [0.25]) == (0.25,) and mode(CFG, 0.5) == (0.5,)
    assert mode(dict(CFG, forecast_quantiles="off")) == ()
    assert len(mode(CFG, [i / 8 for i in range(8)])) == 8
    for bad in ([], "", [0.5, 0.5], [0.9, 0.1], [-0.01], [1.01], ["soon"], "0.1,,0.2", [float("nan")], [True],
                [i / 9 for i in range(9)], {"a": 1}, True):
        with pytest.raises(ValueError, match="forecast_quantiles"):
            mode(dict(CFG, forecast=14, forecast_quantiles=bad), horizon=14)
    with pytest.raises(ValueError, match="no effect"):       # quantiles of nothing are not dropped in silence
        mode(dict(CFG, forecast_quantiles=[0.5]), horizon=0)
    # mcmc() refuses all of it before it reads the data file or opens a device: the file named here does not exist
    nofile, out = str(tmp_path / "no_such_file.nc"), str(tmp_path / "out.hd5")
    with pytest.raises(ValueError, match="no effect"):
        inf.mcmc(nofile, out, dict(CFG, forecast_quantiles=[0.5]))
    with pytest.raises(ValueError, match="no effect"):
        inf.mcmc(nofile, out, CFG, forecast_quantiles="0.5")
    with pytest.raises(ValueError, match="no effect"):
        inf.mcmc(nofile, out, dict(CFG, forecast="off"), forecast_quantiles="0.5")
    for bad in ("", "0.5,0.5", "0.9,0.1", "2", "soon", "nan"):
        with pytest.raises(ValueError, match="forecast_quantiles"):
            inf.mcmc(nofile, out, dict(CFG, forecast=14), forecast_quantiles=bad)
    with pytest.raises(ValueError, match="forecast_quantiles"):
        inf.mcmc(nofile, out, dict(CFG, forecast=14, forecast_quantiles=[]))
    assert not os.path.exists(out)


def test_the_cli_flag_parses(tmp_path, monkeypatch):
    import yaml
    cpath = str(tmp_path / "c.yaml")
    with open(cpath, "w") as f:
        yaml.safe_dump(dict(Mcmc=CFG), f)
    seen = {}
    monkeypatch.setattr(inf, "mcmc", lambda *a, **kw: (seen.clear(), seen.update(kw)))
    inf.main(["-c", cpath, "-o", "x", "--forecast", "14", "--forecast-quantiles", "0.05,0.5,0.95", "data.nc"])
    assert seen["forecast"] == 14 and seen["forecast_quantiles"] == "0.05,0.5,0.95"
    inf.main(["-c", cpath, "-o", "x", "data.nc"])
    assert "forecast_quantiles" not in seen                  # absent: mcmc is called as before the option existed


# ---- 5. run_mcmc with a stub sampler ---------------------------------------------------------------------------------------
class QuantileStub(ForecastStub):
    """ForecastStub with the draw store: what is kept and asked for is recorded; a cell's draws are the sweep numbers."""

    def keep_forecast_draws(self, cap):
        self.calls.append(("keep_forecast_draws", cap))

    def forecast_quantiles(self, probs, pooled=False):
        self.calls.append(("forecast_quantiles", tuple(probs), pooled))
        x = np.asarray(self.forecast_rows, np.float64)
        q = np.quantile(x, probs)                            # pooling B identical chains leaves these quantiles alone
        cell = q[:, None, None, None] + np.arange(3.0)[None, :, None, None] + np.zeros((1, 1, self.M, self.H))
        return cell + 100.0 if pooled else np.repeat(cell[:, None], self.B, axis=1)


def _run(tmp_path, tag, config, ext=".npz", cap=800, stub=QuantileStub):
    s = stub()
    s.cap = cap
    nb, ns = config["num_bursts"], config["num_burst_samples"]
    Hn, _ = inf.forecast_mode(config)
    names = [str(tmp_path / f"{tag}_{c}{ext}") for c in range(s.B)]
    kw = {} if config.get("summaries", "off") == "off" else dict(summaries=config["summaries"])
    if Hn:
        kw["forecast"] = (Hn, nb * ns)
    posts = [inf.Posterior(name, s.M, s.T, 2, inf.warmup_size() + nb * ns, **kw) for name in names]
    logname = str(tmp_path / f"{tag}.log")
    fkw = dict(forecast_calendar=(np.arange(Hn) + 0.5, np.arange(Hn) - 1.0), seed=21) if Hn else {}
    with open(logname, "w") as log:
        inf.run_mcmc(s, config, posts, log=log, **fkw)
    for p in posts:
        p.close()
    return s, [_read(n) for n in names], open(logname).read()


def _untimed(log):
    return [ln for ln in log.splitlines() if not ln.startswith("Sampling: ")]      # that line carries a wall-clock rate


NEW_SETS = {"forecast/quantile_probs", "forecast/pooled_chains"} | \
    {f"forecast/{pre}{name}_quantiles" for pre in ("", "pooled_") for name in FORECAST_QUANTILE_PLANES}


def test_absent_calls_nothing_new_and_writes_todays_datasets(tmp_path):
    cfg = dict(CFG, forecast=5)
    s0, f0, log0 = _run(tmp_path, "parent", cfg, stub=ForecastStub)       # a sampler that has never heard of the store
    s1, f1, log1 = _run(tmp_path, "absent", cfg)
    assert len(s1.calls) == len(s0.calls) and [c[0] for c in s1.calls] == [c[0] for c in s0.calls]
    assert not any(c[0] in ("keep_forecast_draws", "forecast_quantiles") for c in s1.calls)
    assert "uantiles" not in log1 and _untimed(log1) == _untimed(log0)
    for c in range(2):
        assert set(f1[c]) == set(f0[c]) and not (NEW_SETS & set(f1[c]))
        for k in f0[c]:
            assert np.array_equal(f1[c][k], f0[c][k], equal_nan=True), k
    with pytest.raises(ValueError, match="no effect"):
        _run(tmp_path, "nofc", dict(CFG, forecast_quantiles=[0.5]))


@pytest.mark.parametrize("summaries,overlap,ext", [("off", True, ".npz"), ("only", True, ".hd5"), ("on", False, ".npz")])
def test_on_keeps_once_behind_the_reset_asks_twice_at_the_end_and_writes_the_datasets(tmp_path, summaries, overlap, ext):
    if ext == ".hd5" and not hdf5io.available():
        ext = ".npz"
    nb, ns, Hn, probs = 3, 4, 5, (0.05, 0.5, 0.95)
    cfg = dict(CFG, num_bursts=nb, num_burst_samples=ns, summaries=summaries, forecast=Hn, forecast_quantiles=list(probs))
    s, files, log = _run(tmp_path, "on", cfg, ext=ext, cap=800 if overlap else ns)
    names = [c[0] for c in s.calls]
    # once, right behind the reset, with the number of draws the sampling phase keeps; nothing during the warm-up
    assert names.count("keep_forecast_draws") == 1 and names.count("reset_forecast") == 1
    r = names.index("reset_forecast")
    assert s.calls[r + 1] == ("keep_forecast_draws", nb * ns)
    assert not any(n in ("keep_forecast_draws", "forecast_quantiles", "forecast") for n in names[:r])
    # one per-chain and one pooled call, behind the last burst and the forecast's moments
    asked = [c for c in s.calls if c[0] == "forecast_quantiles"]
    assert asked == [("forecast_quantiles", probs, False), ("forecast_quantiles", probs, True)]
    last_burst = max(i for i, n in enumerate(names) if n in ("burst", "sample", "forecast"))
    assert names.index("forecast_quantiles") > max(last_burst, names.index("forecast_summary"))
    # the files: the datasets of the same run without the key, plus the new ones
    base, bf, blog = _run(tmp_path, "base", {k: v for k, v in cfg.items() if k != "forecast_quantiles"}, ext=ext,
                          cap=800 if overlap else ns)
    assert [c[0] for c in s.calls if c[0] not in ("keep_forecast_draws", "forecast_quantiles")] == [c[0] for c in base.calls]
    sweeps = inf.warmup_size() + np.arange(nb * ns)
    want = np.quantile(sweeps.astype(np.float64), probs)
    for c, f in enumerate(files):
        assert set(f) == set(bf[c]) | NEW_SETS
        for k in bf[c]:
            assert np.array_equal(f[k], bf[c][k], equal_nan=True), k
        assert np.array_equal(f["forecast/quantile_probs"], probs) and f["forecast/quantile_probs"].shape == (3,)
        assert np.array_equal(f["forecast/pooled_chains"], [6, 7])            # the stub's first_chain_id = 6, global ids
        for x, name in enumerate(FORECAST_QUANTILE_PLANES):
            own, pooled = f[f"forecast/{name}_quantiles"], f[f"forecast/pooled_{name}_quantiles"]
            assert own.shape == pooled.shape == (3, s.M, Hn) and own.dtype == pooled.dtype == np.float64
            assert np.array_equal(own, np.broadcast_to(want[:, None, None] + x, own.shape)), name
            assert np.array_equal(pooled, own + 100.0), name
    assert log.count("Forecast quantiles:") == 1 and "0.05, 0.5, 0.95" in log
    assert [ln for ln in _untimed(log) if not ln.startswith("Forecast quantiles:")] == _untimed(blog)   # one line more


# ---- 6. the compiler's account of the new kernels --------------------------------------------------------------------------
def test_the_new_kernels_have_no_scratch_and_the_others_are_what_they_were():
    """The compiler's account of the kernels this product owns (covid19uk_amd/kernel_resources.py), and of the parent's."""
    res = H.kernel_account("base")
    added = H.kernel_account("forecast_quantiles")
    new = ["k_forecast_keep", "k_order_stats<1>", "k_order_stats<4>"]
    assert sorted(added) == new and not set(added) & set(res)
    for k in new:
        assert added[k]["scratch_bytes_per_lane"] == 0 and added[k]["vgpr_spill"] == 0 and added[k]["sgpr_spill"] == 0, (k, added[k])
    # k_forecast_keep: the padded tile [rows 2][planes 3][days 64][draws 32 + 1] and the carries [2][32][2], int32
    assert added["k_forecast_keep"]["lds_bytes_per_block"] == 2 * 3 * 64 * 33 * 4 + 2 * 32 * 2 * 4
    # k_order_stats: 16 histograms of 256 bins and the ranks' state (prefix, rank, distinct prefixes, group: 16 words each)
    for k in new[1:]:
        assert 16 * 256 * 4 <= added[k]["lds_bytes_per_block"] <= 16 * 256 * 4 + 4 * 16 * 4 + 16, (k, added[k])
    # three workgroups of the keep kernel fit a CU's 160 KiB
    assert 3 * added["k_forecast_keep"]["lds_bytes_per_block"] <= 160 * 1024
    # every kernel of the parent is in the library as it was
    parent = json.load(open(os.path.join(ROOT, "profiles", "r12_kernel_resources.json")))
    assert set(parent) <= set(res)
    for k in ("k_forecast_fold", "k_forecast_day", "k_forecast_prepare<0>", "k_forecast_prepare<1>", "k_forecast_finish",
              "k_summarize<0,0>", "k_summarize<1,0>", "k_summarize<0,1>", "k_summarize<1,1>", "k_summary_finish", "k_gemm<64>"):
        for f in ("scratch_bytes_per_lane", "lds_bytes_per_block", "vgpr_spill", "sgpr_spill", "vgpr", "occupancy_waves_per_simd"):
            assert res[k][f] == parent[k][f], (k, f, res[k], parent[k])

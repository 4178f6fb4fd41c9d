"""Scenario forecasts, the parts that need no GPU: the new entry points declared, exported and bound with the header's types;
the shared cell update (covid19uk_amd/csrc/scenario_update.h) compiled as plain C++ against Python integers; the NumPy
definition of the four differences against a plain Python loop; the statistics against fractions.Fraction; the
specification parser and every refusal; the options' resolution of its own; the compiler's account of the kernels."""
import ctypes
import shutil
import subprocess
import warnings
from fractions import Fraction

import numpy as np
import pytest

import __graft_entry__ as entry
from covid19uk_amd import _lib, kernel_resources
from covid19uk_amd.inference import options
from covid19uk_amd.posterior import scenarios as SC
from tests import abi_lib
from tests import helpers as H

NEW = {
    "seir_sampler_scenarios_set": "seir_sampler *s, int32_t K, const double *log_shift, const double *commute, int64_t cap",
    "seir_sampler_scenario_state": "seir_sampler *s, int64_t out[4]",
    "seir_sampler_read_scenarios": "seir_sampler *s, uint64_t *count, int32_t *ref, int64_t *sum, uint64_t *sumsq",
    "seir_sampler_read_scenario_diffs": "seir_sampler *s, int32_t *ref, int64_t *sum, uint64_t *sumsq, uint32_t *lt, uint32_t *eq",
    "seir_sampler_read_scenario_draws": "seir_sampler *s, int64_t first, int64_t count, int64_t *by_day, int64_t *state_by_day",
    "seir_scenario_diffs": "seir_ctx *ctx, const int32_t *base_events, const int32_t *scenario_events, int64_t n, int32_t B, "
                           "int32_t M, int32_t H, uint64_t folded, int32_t *ref, int64_t *sum, uint64_t *sumsq, uint32_t *lt, "
                           "uint32_t *eq, uint32_t *overflow",
}


# ---- 1. the entry points ----------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound_with_the_headers_types():
    lib = abi_lib.check_symbols(NEW)
    text = open(abi_lib.HEADER).read()
    assert "#define SEIR_SCENARIO_MAX 4" in text and "#define SEIR_SCENARIO_Q 4" in text
    assert SC.MAX_SCENARIOS == 4 and SC.Q == 4 == len(SC.QUANTITIES)
    # null handles are refused without touching the GPU
    out = (ctypes.c_int64 * 4)()
    for call in (lambda: lib.seir_sampler_scenarios_set(None, 0, None, None, 0), lambda: lib.seir_sampler_scenario_state(None, out),
                 lambda: lib.seir_sampler_read_scenarios(None, None, None, None, None),
                 lambda: lib.seir_sampler_read_scenario_diffs(None, None, None, None, None, None),
                 lambda: lib.seir_sampler_read_scenario_draws(None, 0, 0, None, None)):
        assert call() == _lib.ERR_INVALID and b"null sampler" in lib.seir_last_error()
    assert lib.seir_scenario_diffs(None, None, None, 1, 1, 1, 1, 0, None, None, None, None, None, None) == _lib.ERR_INVALID


# ---- 2. scenario_update.h as plain C++ ---------------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include "scenario_update.h"
// one cell.  "u d_se d_ei d_ir ex_se ex_ei ex_ir": a draw's differences and their exclusive prefixes; "r": reset.
// After every draw: ovf, then per quantity ref sum sumsq lt eq.
int main() {
    using namespace seir;
    int32_t ref[SCENARIO_Q] = {0, 0, 0, 0}; int64_t sum[SCENARIO_Q] = {0, 0, 0, 0}; uint64_t sq[SCENARIO_Q] = {0, 0, 0, 0};
    uint32_t lt[SCENARIO_Q] = {0, 0, 0, 0}, eq[SCENARIO_Q] = {0, 0, 0, 0};
    bool first = true;
    char op;
    while (scanf(" %c", &op) == 1) {
        if (op == 'r') {
            for (int q = 0; q < SCENARIO_Q; ++q) { ref[q] = 0; sum[q] = 0; sq[q] = 0; lt[q] = 0; eq[q] = 0; }
            first = true;
            continue;
        }
        long long v[6];
        for (int i = 0; i < 6; ++i) if (scanf("%lld", &v[i]) != 1) return 1;
        const int32_t d[3] = {(int32_t)v[0], (int32_t)v[1], (int32_t)v[2]}, ex[3] = {(int32_t)v[3], (int32_t)v[4], (int32_t)v[5]};
        int32_t val[SCENARIO_Q];
        scenario_diff_values(d, ex, val);
        const bool ovf = scenario_cell_update(ref, sum, sq, lt, eq, val, first);
        first = false;
        printf("%d", ovf ? 1 : 0);
        for (int q = 0; q < SCENARIO_Q; ++q)
            printf(" %d %lld %llu %u %u", ref[q], (long long)sum[q], (unsigned long long)sq[q], lt[q], eq[q]);
        printf("\n");
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
    d = tmp_path_factory.mktemp("scenario_update")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run(cxx + ["-std=c++17", "-O1", "-Wall", "-Werror", "-I", entry.CSRC, "-o", str(exe), str(src)],
                   check=True, capture_output=True, text=True)

    def run(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.split("\n")
        return [tuple(int(v) for v in row.split()) for row in out if row]
    return run


def _python_cell(draws):
    """The same in Python integers: rows of (ovf, then per quantity ref sum sumsq lt eq), sumsq modulo 2^64 as uint64 holds it."""
    ref, sm, sq, lt, eq, ovf_rows = None, [0] * 4, [0] * 4, [0] * 4, [0] * 4, []
    for d_se, d_ei, d_ir, ex_se, ex_ei, ex_ir in draws:
        val = [d_ir, ex_ir + d_ir, ex_ei - ex_ir, ex_se + d_se]
        if ref is None:
            ref = list(val)
        ovf = False
        for q in range(4):
            dlt = val[q] - ref[q]
            sm[q] += dlt
            tot = sq[q] + dlt * dlt
            ovf |= tot >= 2 ** 63
            sq[q] = tot % 2 ** 64
            lt[q] += val[q] < 0
            eq[q] += val[q] == 0
        ovf_rows.append((int(ovf),) + tuple(x for q in range(4) for x in (ref[q], sm[q], sq[q], lt[q], eq[q])))
    return ovf_rows


def test_the_cell_update_takes_ref_from_the_first_draw_counts_below_and_equal_and_tests_overflow(update):
    rng = np.random.default_rng(1)
    draws = [tuple(int(v) for v in rng.integers(-1000, 1000, 6)) for _ in range(40)]
    draws[0] = (-5, 3, -7, 10, -2, 4)                      # negative differences in the first draw: ref is negative
    draws[3] = (0, 0, 0, 0, 0, 0)                          # every difference equal
    got = update(["u " + " ".join(map(str, d)) for d in draws])
    want = _python_cell(draws)
    assert got == want
    assert got[0][1] == -7 and got[0][6] == -3 and got[0][11] == -6 and got[0][16] == 5      # the four refs
    assert not any(r[0] for r in got) and any(r[4] for r in got) and any(r[5] for r in got)
    # a reset starts again: the next draw gives ref
    again = update(["u 1 2 3 4 5 6", "r", "u -1 -2 -3 -4 -5 -6"])
    assert again[1] == _python_cell([(-1, -2, -3, -4, -5, -6)])[0]
    # the overflow test: differences 2^30 apart add 2^60 each; the eighth reaches 2^63, and the flag is the caller's to keep
    big = [(0, 0, 0, 0, 0, 0)] + [(0, 0, 2 ** 30, 0, 0, 0)] * 9
    got = update(["u " + " ".join(map(str, d)) for d in big])
    assert got == _python_cell(big)
    assert [r[0] for r in got] == [0] * 8 + [1, 1]
    # the extremes of int32: |x - ref| = 2^32 - 1 squares to just under 2^64, no wrap of the product
    ext = [(0, 0, -2 ** 31, 0, 0, 0), (0, 0, 2 ** 31 - 1, 0, 0, 0)]
    assert update(["u " + " ".join(map(str, d)) for d in ext]) == _python_cell(ext)


# ---- 3. the NumPy definition --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hd", [1, 63, 64, 65, 128])
def test_the_four_differences_equal_a_plain_loop(Hd):
    rng = np.random.default_rng(Hd)
    base = rng.integers(0, 50, size=(3, 2, 4, Hd, 3))
    scen = rng.integers(0, 50, size=(3, 2, 4, Hd, 3))
    got = SC.differences(base, scen)
    assert got.dtype == np.int64 and got.shape == (3, 2, 4, Hd, 4)
    for j in range(3):
        for b in range(2):
            for m in range(4):
                c_se = c_ei = c_ir = 0
                for s in range(Hd):
                    d = [int(scen[j, b, m, s, x]) - int(base[j, b, m, s, x]) for x in range(3)]
                    want = [d[2], c_ir + d[2], c_ei - c_ir, c_se + d[0]]
                    assert list(got[j, b, m, s]) == want
                    c_se, c_ei, c_ir = c_se + d[0], c_ei + d[1], c_ir + d[2]
    assert not got[..., 0, 2].any()                        # the prevalence of day 0 is the common state's
    fold = SC.fold_differences(base, scen)
    dev = got - got[0]
    assert fold["count"] == 3 and np.array_equal(fold["ref"], got[0]) and np.array_equal(fold["sum"], dev.sum(0))
    assert np.array_equal(fold["sumsq"], (dev * dev).sum(0).astype(np.uint64)) and not fold["overflow"]
    assert np.array_equal(fold["lt"], (got < 0).sum(0)) and np.array_equal(fold["eq"], (got == 0).sum(0))
    two = SC.fold_differences(base[1:], scen[1:], acc=SC.fold_differences(base[:1], scen[:1]))
    for k in ("count", "ref", "sum", "sumsq", "lt", "eq", "overflow"):
        assert np.array_equal(two[k], fold[k]), k
    with pytest.raises(ValueError, match="does not fit int32"):
        SC.fold_differences(np.zeros((1, 1, 1, 2, 3), np.int64), np.full((1, 1, 1, 2, 3), 2 ** 31, np.int64))


# ---- 4. the statistics --------------------------------------------------------------------------------------------------
def test_the_statistics_are_the_fractions_and_nan_without_a_warning_for_one_draw():
    rng = np.random.default_rng(2)
    base, scen = rng.integers(0, 2000, size=(9, 1, 2, 5, 3)), rng.integers(0, 2000, size=(9, 1, 2, 5, 3))
    acc = SC.fold_differences(base, scen)
    st = SC.statistics(acc["count"], acc["ref"], acc["sum"], acc["sumsq"], acc["lt"], acc["eq"])
    n = 9
    for idx in np.ndindex(acc["ref"].shape):
        ref, sm, sq = int(acc["ref"][idx]), int(acc["sum"][idx]), int(acc["sumsq"][idx])
        mean, var = ref + Fraction(sm, n), (sq - Fraction(sm * sm, n)) / (n - 1)
        # the integers are below 2^53, exact in float64; every operation then rounds by at most 2^-53 of its result, which is
        # bounded by the operands' magnitudes (ref and sum / n may cancel, as may sumsq and sum^2 / n): 2 operations for the
        # mean, 4 for the variance
        assert abs(Fraction(float(st["mean"][idx])) - mean) <= (abs(ref) + abs(Fraction(sm, n))) * Fraction(2, 2 ** 53)
        assert abs(Fraction(float(st["var"][idx])) - var) <= (sq + Fraction(sm * sm, n)) / (n - 1) * Fraction(4, 2 ** 53)
        assert st["p_below"][idx] == int(acc["lt"][idx]) / n and st["p_equal"][idx] == int(acc["eq"][idx]) / n
    assert np.allclose(st["mean"], SC.differences(base, scen).mean(0)) and np.allclose(st["var"], SC.differences(base, scen).var(0, ddof=1))
    one = SC.fold_differences(base[:1], scen[:1])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        st1 = SC.statistics(one["count"], one["ref"], one["sum"], one["sumsq"], one["lt"], one["eq"])
    assert np.isnan(st1["var"]).all() and np.array_equal(st1["mean"], one["ref"].astype(np.float64))
    with pytest.raises(ValueError, match="no draw"):
        SC.statistics(0, one["ref"], one["sum"], one["sumsq"], one["lt"], one["eq"])
    line = SC.run_line("half", np.arange(2 * 3 * 3).reshape(2, 3, 3))
    assert line.startswith("Scenario half: cumulative cases at day 2 minus the baseline's: mean 28.5") and "over 2 draws" in line


# ---- 5. the parser --------------------------------------------------------------------------------------------------------
def test_the_specification_scalar_list_and_from_day():
    Hd = 5
    sc = SC.parse_scenarios({"half": {"transmission": 0.5}, "stay": {"commute": [1, 0.5, 0, 0, 2], "from_day": 1},
                             "both": {"transmission": [1.0, 2.0, 0.5, 0.5, 0.25], "commute": 0.0, "from_day": 3}, "same": None}, Hd)
    assert sc.names == ("half", "stay", "both", "same") and sc.K == 4 and sc.horizon == Hd and bool(sc)
    assert sc.log_shift.shape == sc.commute.shape == (4, Hd) and sc.log_shift.dtype == np.float64
    assert np.array_equal(sc.log_shift[0], np.log(np.full(Hd, 0.5))) and np.array_equal(sc.commute[0], np.ones(Hd))
    assert np.array_equal(sc.log_shift[1], np.zeros(Hd)) and np.array_equal(sc.commute[1], [1, 0.5, 0, 0, 2])
    assert np.array_equal(sc.log_shift[2], np.log([1, 1, 1, 0.5, 0.25])) and np.array_equal(sc.commute[2], [1, 1, 1, 0, 0])
    assert not sc.log_shift[3].any() and np.array_equal(sc.commute[3], np.ones(Hd))
    with pytest.raises(ValueError):
        sc.log_shift[0, 0] = 1.0                           # frozen, and its arrays read-only
    a, W = SC.scenario_inputs(np.arange(2 * Hd, dtype=float).reshape(2, Hd), np.full(Hd, 3.0), sc, 2)
    assert np.array_equal(a, np.arange(2 * Hd).reshape(2, Hd) + sc.log_shift[2]) and np.array_equal(W, [3, 3, 3, 0, 0])
    for off in (None, False, "off", {}):
        assert not SC.parse_scenarios(off, Hd) and SC.parse_scenarios(off, 0).K == 0


@pytest.mark.parametrize("spec,Hd,word", [
    ({"a": {"transmission": 0.5}}, 0, "without forecast"),
    ({str(i): {} for i in range(5)}, 3, "at most 4"),
    ({"": {"commute": 0.5}}, 3, "name is empty"),
    ([("a", {}), ("a", {})], 3, "given twice"),
    ({"a": {"transmission": [1, 1]}}, 3, "has 2 values, the forecast has 3 days"),
    ({"a": {"transmission": 0.0}}, 3, "> 0"),
    ({"a": {"transmission": -1.0}}, 3, "> 0"),
    ({"a": {"transmission": float("nan")}}, 3, "finite"),
    ({"a": {"commute": float("inf")}}, 3, "finite"),
    ({"a": {"commute": [1, -0.5, 1]}}, 3, ">= 0"),
    ({"a": {"commute": "half"}}, 3, "a number"),
    ({"a": {"from_day": 3}}, 3, r"from_day=3"),
    ({"a": {"from_day": -1}}, 3, r"from_day=-1"),
    ({"a": {"from_day": 1.5}}, 3, "from_day"),
    ({"a": {"local": 1}}, 3, "keys transmission, commute, from_day"),
    ("everything", 3, "a mapping name"),
])
def test_every_refusal_comes_from_the_parser_with_no_gpu_call(spec, Hd, word):
    with pytest.raises(ValueError, match=word):
        SC.parse_scenarios(spec, Hd)
    if isinstance(spec, dict):
        with pytest.raises(ValueError, match=word):
            options.resolve_scenarios({"scenarios": spec}, Hd)


def test_the_resolution_is_its_own_and_moves_nothing_of_the_products(tmp_path):
    cfg = dict(num_bursts=2, num_burst_samples=4, forecast=5, scenarios={"half": {"transmission": 0.5, "from_day": 2}})
    section, opt = options.resolve_products(cfg)
    plain, opt0 = options.resolve_products({k: v for k, v in cfg.items() if k != "scenarios"})
    assert opt == opt0 and {k: v for k, v in section.items() if k != "scenarios"} == plain
    assert "scenarios" not in options.PRODUCT_KEYS and not hasattr(opt, "scenarios")
    sc = options.resolve_scenarios(section, opt.horizon)
    assert sc.names == ("half",) and np.array_equal(sc.log_shift[0], np.log([1, 1, 0.5, 0.5, 0.5]))
    assert not options.resolve_scenarios(plain, opt.horizon)
    # the command line's file overrides the section
    import yaml
    path = tmp_path / "s.yaml"
    path.write_text(yaml.safe_dump({"scenarios": {"stay": {"commute": 0.5}}}))
    over = options.resolve_scenarios(section, opt.horizon, override=SC.load_spec(str(path)))
    assert over.names == ("stay",) and np.array_equal(over.commute[0], np.full(5, 0.5))
    with pytest.raises(ValueError, match="without forecast"):
        options.resolve_scenarios(section, 0)


# ---- 6. the compiler's account ------------------------------------------------------------------------------------------
def test_the_kernels_account_owner_scenarios_no_spills_and_the_day_kernel_is_the_forecasts():
    res = H.kernel_account("scenarios")
    assert sorted(res) == ["k_scenario_begin<256>", "k_scenario_day<4>", "k_scenario_diff<4>"]
    assert kernel_resources.OWNERS["scenarios"] == ("k_scenario_begin", "k_scenario_day", "k_scenario_diff")
    for k, v in res.items():
        assert v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
    assert res["k_scenario_begin<256>"]["scratch_bytes_per_lane"] == 0 and res["k_scenario_diff<4>"]["scratch_bytes_per_lane"] == 0
    # no static LDS beyond the fold's carries: 8 waves x 128 draws x 3 ints
    assert res["k_scenario_diff<4>"]["lds_bytes_per_block"] == 8 * 128 * 3 * 4
    assert res["k_scenario_begin<256>"]["lds_bytes_per_block"] == 0 and res["k_scenario_day<4>"]["lds_bytes_per_block"] == 0
    # the day kernel is k_forecast_day's arithmetic: the binomial sampler's 32 bytes of scratch, its registers, its occupancy
    day, fday = res["k_scenario_day<4>"], H.kernel_account()["k_forecast_day"]
    for key in ("scratch_bytes_per_lane", "vgpr", "occupancy_waves_per_simd", "agpr"):
        assert day[key] == fday[key], key


# ---- 7. run_mcmc and the replay driver with a stub sampler; the datasets --------------------------------------------------
import os  # noqa: E402

from covid19uk_amd import hdf5io  # noqa: E402
from covid19uk_amd.inference import inference as inf  # noqa: E402
from covid19uk_amd.posterior import replay as R  # noqa: E402
from covid19uk_amd.sampler import Summary  # noqa: E402
from tests.test_forecast_host import ForecastStub  # noqa: E402
from tests.test_forecast_host import _run as _forecast_run  # noqa: E402
from tests.test_summary_host import CFG, _read  # noqa: E402

SPEC = {"half": {"transmission": 0.5, "from_day": 1}, "stay": {"commute": 0.0}}
SCEN_SETS = ({f"scenarios/{k}" for k in ("names", "log_shift", "commute", "horizon", "first_day", "count", "seir_mean", "seir_var",
                                         "state_mean", "state_var", "diff_mean", "diff_var", "p_below", "p_equal", "diff_lt", "diff_eq")}
             | {f"samples/{k}" for k in ("scenario_by_day", "scenario_state_by_day", "scenario_diff_by_day")})
READS = ("scenario_summary", "scenario_diffs", "read_scenario_draws")


class ScenarioStub(ForecastStub):
    """ForecastStub with the scenarios: scenario k's by-day curve of a draw is the forecast's plus k + 1 (its state curve minus
    that); the accumulators are the NumPy fold of counts built the same way."""

    def keep_forecast_draws(self, cap):
        self.calls.append(("keep_forecast_draws", cap))

    def forecast_quantiles(self, probs, pooled=False):
        self.calls.append(("forecast_quantiles", pooled))
        return np.zeros((len(probs),) + (() if pooled else (self.B,)) + (3, self.M, self.H))

    def set_scenarios(self, log_shift, commute, cap):
        self.calls.append(("set_scenarios", np.array(log_shift), np.array(commute), cap))
        self.K = len(log_shift)

    def _rows(self):
        return np.asarray(self.forecast_rows, np.int64)

    def scenario_summary(self):
        self.calls.append(("scenario_summary",))
        out = []
        for k in range(self.K):
            x = np.broadcast_to((self._rows() + k + 1)[:, None, None, None, None], (len(self._rows()), self.B, self.M, self.H, 6))
            d = x - x[:1]
            out.append(Summary(count=np.full(self.B, len(x), np.uint64), ref=x[0].astype(np.int32), sum=d.sum(axis=0),
                               sumsq=(d * d).sum(axis=0).astype(np.uint64)))
        return out

    def _events(self, k):
        n = len(self._rows())
        return np.broadcast_to((self._rows() % 3 + (0 if k is None else k + 1))[:, None, None, None, None], (n, self.B, self.M, self.H, 3))

    def scenario_diffs(self):
        self.calls.append(("scenario_diffs",))
        folds = [SC.fold_differences(self._events(None), self._events(k)) for k in range(self.K)]
        out = {key: np.stack([f[key] for f in folds]) for key in ("ref", "sum", "sumsq", "lt", "eq")}
        out["count"] = len(self._rows())
        return out

    def read_scenario_draws(self, count=None, first=0):
        self.calls.append(("read_scenario_draws", count, first))
        f = np.broadcast_to(self._rows()[None, :, None, None, None], (self.K, len(self._rows()), self.B, self.H, 3)).astype(np.int64)
        add = (np.arange(self.K) + 1)[:, None, None, None, None]
        return dict(by_day=f + add, state_by_day=-f - add)

    def replay(self, theta, events, **kw):
        n = theta[0].shape[0]
        self.calls.append(("replay", n, kw))
        tr = self._trace(n, events=False, **kw)
        tr.theta = np.stack(theta, axis=1)
        return tr


def _run(tmp_path, tag, config, ext=".npz"):
    s = ScenarioStub()
    s.cap = 800
    nb, ns = config["num_bursts"], config["num_burst_samples"]
    Hn, _ = inf.forecast_mode(config)
    names = [str(tmp_path / f"{tag}_{c}{ext}") for c in range(s.B)]
    posts = [inf.Posterior(name, s.M, s.T, 2, inf.warmup_size() + nb * ns, **(dict(forecast=(Hn, nb * ns)) if Hn else {})) for name in names]
    logname = str(tmp_path / f"{tag}.log")
    with open(logname, "w") as log:
        inf.run_mcmc(s, config, posts, log=log, **(dict(forecast_calendar=(np.arange(Hn) + 0.5, np.arange(Hn) - 1.0), seed=21) if Hn else {}))
    for p in posts:
        p.close()
    return s, [_read(n) for n in names], open(logname).read()


def _without(calls):
    return [c for c in calls if c[0] not in READS + ("set_scenarios",)]


def _same_calls(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x) == len(y) and x[0] == y[0]
        for u, v in zip(x[1:], y[1:]):
            if isinstance(u, dict):
                assert set(u) == set(v), (x[0], set(u), set(v))        # the products' keyword sets
            elif not callable(u):
                assert np.array_equal(u, v), x[0]


@pytest.mark.parametrize("ext", [".npz", ".hd5"])
def test_run_mcmc_sets_once_behind_reset_and_store_reads_once_and_writes_the_datasets(tmp_path, ext):
    assert hdf5io.available()
    Hn, nb, ns = 4, CFG["num_bursts"], CFG["num_burst_samples"]
    n = nb * ns
    cfg = dict(CFG, forecast=Hn, forecast_quantiles=[0.25, 0.75], scenarios=SPEC)
    s, files, log = _run(tmp_path, "on", cfg, ext)
    names = [c[0] for c in s.calls]
    sc = SC.parse_scenarios(SPEC, Hn)
    # set once, right behind the forecast's reset and its draw store, before the first burst; one read of each kind at the end
    assert names.count("set_scenarios") == 1
    i = names.index("set_scenarios")
    assert names[i - 2:i] == ["reset_forecast", "keep_forecast_draws"] and not any(nm in ("sample", "burst", "forecast") for nm in names[i - 2:i])
    call = s.calls[i]
    assert np.array_equal(call[1], sc.log_shift) and np.array_equal(call[2], sc.commute) and call[3] == n
    assert "forecast" not in names[:i] and [names.count(r) for r in READS] == [1, 1, 1]
    assert all(names.index(r) > max(j for j, nm in enumerate(names) if nm == "forecast") for r in READS)
    # the same run without the key: nothing of it is called, every other call and the products' keyword sets are what they were
    base, bfiles, blog = _run(tmp_path, "base", {k: v for k, v in cfg.items() if k != "scenarios"}, ext)
    assert not any(c[0] in READS + ("set_scenarios",) for c in base.calls) and "Scenario" not in blog
    _same_calls(_without(s.calls), base.calls)
    keep = lambda text, drop: [l for l in text.split("\n") if not l.startswith(drop)]      # noqa: E731  ("Sampling:" holds a timing)
    assert keep(log, ("Scenario ", "Sampling:")) == keep(blog, ("Sampling:",))
    # the datasets: the baseline's, untouched, and the scenarios' beside them
    rows = np.asarray(s.forecast_rows, np.int64)
    for c, f in enumerate(files):
        assert set(f) - set(bfiles[c]) == SCEN_SETS | {"scenarios/national_diff_quantiles"} and set(bfiles[c]) <= set(f)
        for k in bfiles[c]:
            assert np.array_equal(f[k], bfiles[c][k]), k
        assert [x.decode() for x in f["scenarios/names"]] == ["half", "stay"]
        assert np.array_equal(f["scenarios/log_shift"], sc.log_shift) and np.array_equal(f["scenarios/commute"], sc.commute)
        assert (f["scenarios/horizon"], f["scenarios/first_day"], f["scenarios/count"]) == ([Hn], [s.T], [n])
        for k in range(2):
            want = np.broadcast_to((rows + k + 1)[:, None, None, None], (n, s.M, Hn, 3)).astype(np.float64)
            assert np.allclose(f["scenarios/seir_mean"][k], want.mean(0)) and np.allclose(f["scenarios/state_var"][k], want.var(0, ddof=1))
            assert f["samples/scenario_by_day"].shape == (n, 2, Hn, 3) and f["samples/scenario_by_day"].dtype == np.int64
            assert np.array_equal(f["samples/scenario_by_day"][:, k], np.broadcast_to((rows + k + 1)[:, None, None], (n, Hn, 3)))
            assert np.array_equal(f["samples/scenario_state_by_day"][:, k], -f["samples/scenario_by_day"][:, k])
            # the paired difference of the draws: the scenario's curve minus samples/forecast_by_day, formed on the host
            assert np.array_equal(f["samples/scenario_diff_by_day"][:, k], f["samples/scenario_by_day"][:, k] - f["samples/forecast_by_day"])
            assert np.all(f["samples/scenario_diff_by_day"][:, k] == k + 1)
        d = s.scenario_diffs()
        st = SC.statistics(n, d["ref"], d["sum"], d["sumsq"], d["lt"], d["eq"])
        for key, got in (("mean", "diff_mean"), ("var", "diff_var"), ("p_below", "p_below"), ("p_equal", "p_equal")):
            assert f[f"scenarios/{got}"].shape == (2, s.M, Hn, 4) and np.array_equal(f[f"scenarios/{got}"], st[key][:, c], equal_nan=True)
        assert np.array_equal(f["scenarios/diff_lt"], d["lt"][:, c]) and np.array_equal(f["scenarios/diff_eq"], d["eq"][:, c])
        assert f["scenarios/national_diff_quantiles"].shape == (2, 2, Hn, 3)
        assert np.array_equal(f["scenarios/national_diff_quantiles"], inf.draw_quantiles(f["samples/scenario_diff_by_day"], [0.25, 0.75]))
    # one line per scenario: national cumulative cases at H - 1 minus the baseline's
    lines = [l for l in log.split("\n") if l.startswith("Scenario ")]
    assert len(lines) == 2 and lines[0] == SC.run_line("half", np.ones((n * s.B, Hn, 3))) and "mean 8.0" in lines[1]


def test_the_key_absent_calls_nothing_and_refusals_come_before_any_call(tmp_path):
    s0, ref, log0 = _forecast_run(tmp_path, "ref", dict(CFG, forecast=3))       # a sampler that has never heard of scenarios
    s1, got, log1 = _run(tmp_path, "plain", dict(CFG, forecast=3))
    assert [c[0] for c in s1.calls] == [c[0] for c in s0.calls]
    assert [l for l in log1.split("\n") if not l.startswith("Sampling:")] == [l for l in log0.split("\n") if not l.startswith("Sampling:")]
    assert set(got[1]) == set(ref[1]) and all(np.array_equal(got[1][k], ref[1][k]) for k in ref[1])
    for bad, word in ((dict(CFG, scenarios=SPEC), "without forecast"), (dict(CFG, forecast=3, scenarios={"a": {"from_day": 3}}), "from_day=3"),
                      (dict(CFG, forecast=3, scenarios={str(i): {} for i in range(5)}), "at most 4")):
        s = ScenarioStub()
        with pytest.raises(ValueError, match=word):
            inf.run_mcmc(s, bad, [], log=open(os.devnull, "w"), forecast_calendar=(np.ones(3), np.ones(3)))
        assert s.calls == []
        nofile, out = str(tmp_path / "no_such_file.nc"), str(tmp_path / "out.npz")
        with pytest.raises(ValueError, match=word):             # inference.mcmc: before the data file is opened
            inf.mcmc(nofile, out, bad)
        assert not os.path.exists(out)


def test_the_replay_driver_sets_once_and_reads_once(tmp_path):
    Hn, n, burst = 3, 7, 3
    cfg = dict(CFG, forecast=Hn, scenarios=SPEC, num_burst_samples=burst, num_bursts=3, thin=1)

    class Source:
        def __init__(self, c, P, M, T):
            rng = np.random.default_rng(c)
            self.path, self.theta, self.events = f"c{c}", rng.standard_normal((n, P)), rng.integers(0, 3, size=(n, M, T, 3)).astype(np.float64)

        def draws(self, rows):
            return self.theta[rows], self.events[rows]
    runs = {}
    for on in (True, False):
        s = ScenarioStub()
        config = cfg if on else {k: v for k, v in cfg.items() if k != "scenarios"}
        names = [str(tmp_path / f"rp{int(on)}_{c}.npz") for c in range(s.B)]
        posts = [inf.Posterior(name, s.M, s.T, 2, n, burst=burst, results=False, forecast=(Hn, n)) for name in names]
        with open(os.devnull, "w") as log:
            pr = inf.product_records(s, config, posts, log=log, seed=21, forecast_calendar=(np.ones(Hn), np.zeros(Hn)), total=n, results=False)
            R.replay_bursts(s, [Source(c, s.P, s.M, s.T) for c in range(s.B)], np.arange(n), burst, pr, log=log)
        for p in posts:
            p.close()
        runs[on] = (s, [_read(name) for name in names])
    s, files = runs[True]
    names = [c[0] for c in s.calls]
    i = names.index("set_scenarios")
    assert names.count("set_scenarios") == 1 and names[i - 1] == "reset_forecast" and s.calls[i][3] == n and "replay" not in names[:i]
    assert [names.count(r) for r in READS] == [1, 1, 1] and names.count("replay") == 3
    _same_calls(_without(s.calls), runs[False][0].calls)
    assert set(files[0]) - set(runs[False][1][0]) == SCEN_SETS
    assert files[0]["samples/scenario_diff_by_day"].shape == (n, 2, Hn, 3)


def test_the_flag_is_on_both_command_lines_and_absent_it_passes_nothing(tmp_path, monkeypatch):
    import yaml
    cpath, spath = str(tmp_path / "c.yaml"), str(tmp_path / "s.yaml")
    with open(cpath, "w") as f:
        yaml.safe_dump(dict(Mcmc=CFG), f)
    with open(spath, "w") as f:
        yaml.safe_dump(SPEC, f)
    seen = {}
    monkeypatch.setattr(inf, "mcmc", lambda *a, **kw: seen.update(kw=kw))
    inf.main(["-c", cpath, "-o", "x", "--forecast", "14", "--scenarios", spath, "data.nc"])
    assert seen["kw"]["scenarios"] == SPEC and seen["kw"]["forecast"] == 14
    inf.main(["-c", cpath, "-o", "x", "--forecast", "14", "data.nc"])
    assert "scenarios" not in seen["kw"]
    monkeypatch.setattr(R, "replay_files", lambda *a, **kw: seen.update(kw=kw))
    R.main(["-c", cpath, "-o", "x", "--forecast", "14", "--scenarios", spath, "data.nc", "p0.hd5"])
    assert seen["kw"]["scenarios"] == SPEC
    R.main(["-c", cpath, "-o", "x", "--forecast", "14", "data.nc", "p0.hd5"])
    assert "scenarios" not in seen["kw"]

"""Host side of the device summaries (include/seir_hip.h, "Summaries of samples/seir on the device"), no GPU:
the new C-ABI symbols and their argument types, the shared per-cell update (covid19uk_amd/csrc/summary_update.h, the one
definition k_summarize calls) compiled as plain C++ and driven against Python integers up to the overflow flag, mean and
variance from the integer accumulators against NumPy, and the `summaries` option of the configuration, the command line
and the output file."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
from covid19uk_amd import _lib
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.sampler import MARGINAL_KEYS, SUMMARY_QUANTITIES, Summary, Trace, summary_mean, summary_var
from tests import helpers as H
from tests.abi_lib import check_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "seir_sampler_summary_reset": "seir_sampler *s",
    "seir_sampler_summarize": "seir_sampler *s, int32_t first_slot, int32_t count, int32_t accumulate",
    "seir_sampler_read_marginals": "seir_sampler *s, int32_t first, int32_t count, int64_t *events_by_day, "
                                   "int64_t *events_by_location, int64_t *state_by_day",
    "seir_sampler_read_marginals_async": "seir_sampler *s, int32_t first, int32_t count, int64_t *events_by_day, "
                                         "int64_t *events_by_location, int64_t *state_by_day",
    "seir_sampler_read_summary": "seir_sampler *s, uint64_t *count, int32_t *ref, int64_t *sum, uint64_t *sumsq",
}


# ---- 1. the symbols ------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound_with_the_headers_types():
    lib = check_symbols(NEW)
    # a null sampler is refused before anything touches a device
    assert lib.seir_sampler_summary_reset(None) == _lib.ERR_INVALID
    assert lib.seir_sampler_summarize(None, 0, 1, 1) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_summary(None, None, None, None, None) == _lib.ERR_INVALID


# ---- 2. the shared per-cell update, as plain C++ -------------------------------------------------------------------------
DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include "summary_update.h"
// one cell: lines "x" fold x; the line "r" resets.  After every fold: ref sum sumsq flag
int main() {
    int32_t ref = 0; int64_t sum = 0; uint64_t sumsq = 0; bool first = true;
    char op[8]; long long x;
    while (std::scanf("%7s %lld", op, &x) == 2) {
        if (op[0] == 'r') { ref = 0; sum = 0; sumsq = 0; first = true; continue; }
        if (op[0] == 's') { sum = (int64_t)x; continue; }                       // test set-up: start from given sums
        if (op[0] == 'q') { sumsq = (uint64_t)x; first = false; continue; }
        const bool flag = seir::summary_fold(ref, sum, sumsq, (int32_t)x, first);
        first = false;
        std::printf("%" PRId32 " %" PRId64 " %" PRIu64 " %d\n", ref, sum, sumsq, flag ? 1 : 0);
    }
    static_assert(seir::SUMMARY_Q == 6, "k_se, k_ei, k_ir, S, E, I");
}
"""


@pytest.fixture(scope="module")
def fold(tmp_path_factory):
    cxx = None
    try:
        cxx = [entry._hipcc(), "-x", "c++"]
    except RuntimeError:
        for cand in ("g++", "c++", "clang++"):
            if shutil.which(cand):
                cxx = [cand]
                break
    assert cxx, "no C++ compiler"
    d = tmp_path_factory.mktemp("summary_update")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run(cxx + ["-std=c++17", "-O1", "-Wall", "-Werror", "-I", entry.CSRC, "-o", str(exe), str(src)],
                   check=True, capture_output=True, text=True)

    def run(lines):
        text = "".join(f"{op} {int(v)}\n" for op, v in lines)
        out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.split("\n")
        return [tuple(int(v) for v in row.split()) for row in out if row]
    return run


def _model(xs):
    """Python integers: (ref, sum, sumsq, flag) after each draw."""
    ref, out = xs[0], []
    s = q = 0
    for x in xs:
        s += x - ref
        q += (x - ref) ** 2
        out.append((ref, s, q, int(q >= 2 ** 63)))
    return out


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fold_equals_python_integers_on_random_draws(fold, seed):
    rng = np.random.default_rng(seed)
    centre = int(rng.integers(0, 2_000_000))
    xs = [int(v) for v in rng.integers(max(centre - 5000, 0), centre + 5000, size=400)]
    got = fold([("x", v) for v in xs])
    assert got == _model(xs)
    assert got[0] == (xs[0], 0, 0, 0)                                          # the first draw sets ref
    assert any(x < xs[0] for x in xs) and any(x > xs[0] for x in xs)           # shifts of both signs occur


def test_first_draw_sets_ref_negative_shifts_and_reset(fold):
    got = fold([("x", 1_000_000), ("x", 999_990), ("x", 1_000_003), ("r", 0), ("x", 7), ("x", 0)])
    assert got == [(1_000_000, 0, 0, 0), (1_000_000, -10, 100, 0), (1_000_000, -7, 109, 0), (7, 0, 0, 0), (7, -7, 49, 0)]


def test_extreme_inputs(fold):
    lo, hi = -2 ** 31, 2 ** 31 - 1
    xs = [lo, hi, lo, 0, hi]
    got = fold([("x", v) for v in xs])
    want = _model(xs)
    assert got[:2] == want[:2] and got[1] == (lo, 2 ** 32 - 1, (2 ** 32 - 1) ** 2, 1)     # one step of 2^32 - 1 raises it
    xs = [hi, lo]
    assert fold([("x", v) for v in xs]) == [(hi, 0, 0, 0), (hi, -(2 ** 32 - 1), (2 ** 32 - 1) ** 2, 1)]


def test_the_flag_is_raised_exactly_when_sumsq_reaches_2_to_63(fold):
    # start one unit short: sumsq = 2^63 - 2 with ref = 0 (first draw 0), then a shift of 1 twice
    got = fold([("x", 0), ("q", 2 ** 63 - 2), ("x", 1), ("x", 1), ("x", 0)])
    assert [r[3] for r in got] == [0, 0, 1, 1]
    assert got[1][2] == 2 ** 63 - 1 and got[2][2] == 2 ** 63
    # with |d| = 2^31 - 1 per draw: the number of draws Python integers say, not one fewer
    d = 2 ** 31 - 1
    n = -(-(2 ** 63) // (d * d))                                               # first n with n d^2 >= 2^63
    got = fold([("x", 0), ("q", (n - 2) * d * d), ("s", (n - 2) * d), ("x", d), ("x", d)])
    assert got[1] == (0, (n - 1) * d, (n - 1) * d * d, 0)
    assert got[2] == (0, n * d, n * d * d, 1)
    # a wrap past 2^64 is caught as well (sumsq set to 2^64 - 1, then a shift of 2)
    got = fold([("x", 0), ("q", -1), ("x", 2)])
    assert [r[3] for r in got] == [0, 1] and got[1][2] == 3


# ---- 3. mean and variance from the integers ------------------------------------------------------------------------------
def _summary_of(x):
    """x [n, B, M, T, 6] integer draws -> Summary, by the definitions."""
    x = np.asarray(x, np.int64)
    d = x - x[:1]
    return Summary(count=np.full(x.shape[1], x.shape[0], np.uint64), ref=x[0].astype(np.int32), sum=d.sum(axis=0),
                   sumsq=(d * d).sum(axis=0).astype(np.uint64))


def test_mean_and_var_against_numpy():
    rng = np.random.default_rng(5)
    base = rng.integers(0, 1_200_000, size=(1, 3, 4, 9, 6))
    x = base + rng.integers(-40, 40, size=(200, 3, 4, 9, 6))
    sm = _summary_of(x)
    xf = x.astype(np.float64)
    np.testing.assert_allclose(sm.mean, xf.mean(axis=0), rtol=1e-14, atol=0.0)
    # the shift is what makes this accurate: S ~ 1e6 with a spread of tens
    np.testing.assert_allclose(sm.var, (xf - base).var(axis=0, ddof=1), rtol=1e-12, atol=1e-12)
    assert sm.mean.shape == sm.var.shape == (3, 4, 9, len(SUMMARY_QUANTITIES)) and sm.mean.dtype == np.float64


def test_variance_of_one_draw_is_nan_without_a_warning():
    import warnings
    x = np.arange(2 * 3 * 4 * 6).reshape(1, 2, 3, 4, 6)
    sm = _summary_of(x)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        var, mean = sm.var, sm.mean
        assert np.isnan(var).all()
        assert np.array_equal(mean, x[0].astype(np.float64))
        # no draw at all: both undefined, still no warning
        empty = Summary(count=np.zeros(2, np.uint64), ref=sm.ref * 0, sum=sm.sum * 0, sumsq=sm.sumsq * 0)
        assert np.isnan(empty.mean).all() and np.isnan(empty.var).all()
        # chains with different counts
        cnt = np.array([1, 5], np.uint64)
        v = summary_var(cnt, np.zeros((2, 3)), np.full((2, 3), 8.0))
        assert np.isnan(v[0]).all() and np.array_equal(v[1], np.full(3, 2.0))
        assert np.array_equal(summary_mean(cnt, np.ones((2, 3)), np.full((2, 3), 5.0)), [[6.0] * 3, [2.0] * 3])


# ---- 4. configuration, command line, output file ---------------------------------------------------------------------------
CFG = dict(dmax=84, nmax=25, m=2, occult_nmax=15, num_event_time_updates=5, num_bursts=2, num_burst_samples=4)


def test_summaries_value_is_parsed_and_an_unknown_one_refused_before_any_gpu_call(tmp_path):
    assert inf.summaries_mode({}) == "off"
    assert inf.summaries_mode(dict(summaries="only")) == "only"
    assert inf.summaries_mode(dict(summaries="only"), "on") == "on"          # the command line overrides
    assert inf.summaries_mode(dict(summaries=True)) == "on" and inf.summaries_mode(dict(summaries=False)) == "off"
    with pytest.raises(ValueError, match="summaries"):
        inf.summaries_mode(dict(summaries="sometimes"))
    # mcmc() refuses it before it reads the data file or opens a device: the file named here does not exist
    with pytest.raises(ValueError, match="summaries"):
        inf.mcmc(str(tmp_path / "no_such_file.nc"), str(tmp_path / "out.hd5"), dict(CFG, summaries="sometimes"))
    with pytest.raises(ValueError, match="summaries"):
        inf.mcmc(str(tmp_path / "no_such_file.nc"), str(tmp_path / "out.hd5"), CFG, summaries="maybe")
    # ... and the command line's parser before it opens the configuration
    with pytest.raises(SystemExit):
        inf.main(["-c", str(tmp_path / "no_such.yaml"), "-o", "x", "--summaries", "maybe", "data.nc"])
    assert not os.path.exists(tmp_path / "out.hd5")


class StubSampler:
    """What run_mcmc calls, recorded; draws carry the sweep they were taken at."""
    B, P, M, T, cap = 2, 6 + 4 + 3, 3, 5, 800

    def __init__(self):
        self.calls, self.sweeps, self.folded = [], 0, None

    def set_thin(self, k):
        self.calls.append(("set_thin", k))

    def set_adaptation(self, **kw):
        pass

    def set_kernel(self, **kw):
        pass

    def get_kernel(self):
        return np.ones(self.B), np.ones((self.B, self.P))

    def reset_summary(self):
        self.calls.append(("reset_summary",))
        self.folded = []

    def _trace(self, n, events=True, summarize=False):
        idx = self.sweeps + np.arange(n)
        self.sweeps += n
        ev = np.broadcast_to(idx[:, None, None, None, None], (n, self.B, self.M, self.T, 3)).astype(np.int32)
        marg = None
        if summarize:
            marg = dict(events_by_day=ev.sum(axis=2, dtype=np.int64), events_by_location=ev.sum(axis=3, dtype=np.int64),
                        state_by_day=-ev.sum(axis=2, dtype=np.int64))
            if summarize is True:
                self.folded.extend(idx)
        hmc = dict(is_accepted=np.ones((n, self.B), bool), target_log_prob=np.zeros((n, self.B)), step_size=np.ones((n, self.B)))
        moves = {k: dict(is_accepted=np.ones((n, self.B), bool), target_log_prob=np.zeros((n, self.B)),
                         proposed_delta=np.zeros((n, self.B, 4, 2), np.int64)) for k in inf.MOVE_KEYS}
        return Trace(theta=np.ones((n, self.B, self.P)), events=ev if events else None, hmc=hmc, moves=moves, marginals=marg)

    def sample(self, n, **kw):
        self.calls.append(("sample", n, kw))
        return self._trace(n, **kw)

    def sample_bursts(self, nb, n, consume, **kw):
        for i in range(nb):
            self.calls.append(("burst", n, kw))
            consume(self._trace(n, **kw), i)

    def summary(self):
        self.calls.append(("summary",))
        n = len(self.folded)
        x = np.broadcast_to(np.asarray(self.folded, np.int64)[:, None, None, None, None], (n, self.B, self.M, self.T, 6))
        return _summary_of(x)


def _run(mode, tmp_path, ext):
    s = StubSampler()
    names = [str(tmp_path / f"{mode}_{c}{ext}") for c in range(s.B)]
    kw = {} if mode is None else dict(summaries=mode)
    num = inf.warmup_size() + 8
    posts = [inf.Posterior(name, s.M, s.T, 2, num, **kw) for name in names]
    log = open(str(tmp_path / f"{mode}{ext}.log"), "w")
    n = inf.run_mcmc(s, CFG if mode is None else dict(CFG, summaries=mode), posts, log=log)
    log.close()
    for p in posts:
        p.close()
    assert n == num
    return s, names, open(str(tmp_path / f"{mode}{ext}.log")).read()


def _read(name):
    if name.endswith(".npz"):
        d = np.load(name)
        return {k.replace("__", "/"): d[k] for k in d.files}
    from covid19uk_amd import hdf5io
    out = {}
    with hdf5io.File(name, "r") as f:
        def walk(group):
            for link in f._links(group or "/"):
                path = f"{group}/{link}"
                if f._links(path):
                    walk(path)
                else:
                    out[path[1:]] = f.read(path)
        walk("")
    return out


NEW_SETS = {"samples/seir_by_day", "samples/seir_by_location", "samples/state_by_day", "summaries/count",
            "summaries/seir_mean", "summaries/seir_var", "summaries/state_mean", "summaries/state_var"}


@pytest.mark.parametrize("ext", [".npz", ".hd5"])
def test_off_creates_todays_datasets_only_leaves_out_the_tensor_and_on_adds_the_summaries(tmp_path, ext):
    from covid19uk_amd import hdf5io
    if ext == ".hd5" and not hdf5io.available():
        ext = ".npz"
    runs = {mode: _run(mode, tmp_path, ext) for mode in (None, "off", "on", "only")}
    files = {mode: _read(r[1][1]) for mode, r in runs.items()}
    # off: the calls and the file of a run that has never heard of the option
    assert runs["off"][0].calls == runs[None][0].calls
    assert all(c[0] != "sample" or c[2] == {} for c in runs["off"][0].calls)
    assert set(files["off"]) == set(files[None])
    for k in files[None]:
        assert np.array_equal(files["off"][k], files[None][k]), k
    assert "samples/seir" in files["off"] and not (NEW_SETS & set(files["off"]))
    # on: today's datasets and the new ones
    assert set(files["on"]) == set(files["off"]) | NEW_SETS
    # only: no samples/seir, and the events were never asked for
    assert set(files["only"]) == set(files["on"]) - {"samples/seir"}
    assert all(c[2]["events"] is False for c in runs["only"][0].calls if c[0] in ("sample", "burst"))
    assert all(c[2]["events"] is True for c in runs["on"][0].calls if c[0] in ("sample", "burst"))
    for word in ("samples/seir", "thin_posterior", "predict", "reproduction_number"):
        assert word in runs["only"][2] and word not in runs["on"][2]
    for mode in ("on", "only"):
        s, f = runs[mode][0], files[mode]
        # the warm-up gets marginals without folding; the moments are reset after the last window and cover the bursts
        warm = [c for c in s.calls if c[0] == "sample"]
        assert warm and all(c[2]["summarize"] == "marginals" for c in warm)
        assert [c[0] for c in s.calls if c[0] in ("reset_summary", "burst", "summary")] == ["reset_summary", "burst", "burst", "summary"]
        assert s.calls.index(("reset_summary",)) > max(i for i, c in enumerate(s.calls) if c[0] == "sample")
        assert all(c[2]["summarize"] is True for c in s.calls if c[0] == "burst")
        w = inf.warmup_size()
        sweeps = np.arange(w + 8)
        assert f["samples/seir_by_day"].shape == (w + 8, s.T, 3) and f["samples/seir_by_location"].shape == (w + 8, s.M, 3)
        assert np.array_equal(f["samples/seir_by_day"][:, 0, 0], sweeps * s.M)
        assert np.array_equal(f["samples/seir_by_location"][:, 0, 0], sweeps * s.T)
        assert np.array_equal(f["samples/state_by_day"][:, 0, 0], -sweeps * s.M)
        assert int(np.asarray(f["summaries/count"]).reshape(-1)[0]) == 8
        for k in ("seir_mean", "state_mean"):
            assert f[f"summaries/{k}"].shape == (s.M, s.T, 3)
            np.testing.assert_allclose(f[f"summaries/{k}"], np.mean(sweeps[w:]), rtol=1e-15)
        for k in ("seir_var", "state_var"):
            np.testing.assert_allclose(f[f"summaries/{k}"], np.var(sweeps[w:], ddof=1), rtol=1e-14)
    assert set(MARGINAL_KEYS) == {"events_by_day", "events_by_location", "state_by_day"}


# ---- the compiler's account of the kernels that share the fold's pieces and the finish body --------------------------------
MOMENT_KERNELS = [f"k_summarize<{ev16},{diag}>" for ev16 in (0, 1) for diag in (0, 1)] + \
    ["k_summary_finish", "k_forecast_fold", "k_forecast_finish"]


@pytest.mark.parametrize("kernel", MOMENT_KERNELS)
def test_the_kernels_built_from_shared_pieces_keep_the_resources_they_had_on_their_own(kernel):
    """Against the build before the pieces were shared (profiles/r09_kernel_resources.json): scratch, spills and LDS equal,
    occupancy not lower, and the register count within the few that move with the compiler's mood."""
    import json
    r = H.kernel_account("base")[kernel]
    was = json.load(open(os.path.join(ROOT, "profiles", "r09_kernel_resources.json")))[kernel]
    for k in ("scratch_bytes_per_lane", "vgpr_spill", "sgpr_spill", "lds_bytes_per_block"):
        assert r[k] == was[k], (kernel, k, r, was)
    assert r["occupancy_waves_per_simd"] >= was["occupancy_waves_per_simd"], (kernel, r, was)
    assert r["vgpr"] <= was["vgpr"] + 4, (kernel, r, was)

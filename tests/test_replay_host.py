"""Stored draws into trace slots and the replay of the products from posterior files (include/seir_hip.h, "Stored draws
into trace slots"): everything that needs no GPU -- the symbols, `load_classify` of csrc/trace_load.h as plain C++ against a
Python restatement, the NumPy definition of the status words against hand cases and plain loops, theta assembly as the
inverse of `draws_to_dict`, the row selection and every refusal, the driver's calls and datasets with a stub sampler,
run_mcmc's call list after the factoring, and the compiler's account of the new kernels."""
import ctypes
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
from covid19uk_amd import _lib, hdf5io
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.posterior import replay as R
from covid19uk_amd.sampler import BURST_PRODUCTS, ChainSampler
from tests import helpers as H
from tests.abi_lib import check_symbols
from tests.test_group_curves_host import FULL, POP, TABLE, _read
from tests.test_group_curves_host import _run as _run_mcmc
from tests.test_ngm_host import NgmStub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "seir_sampler_load_trace": "seir_sampler *s, int32_t chain, int32_t first, int32_t count, const double *theta, const double *events",
    "seir_sampler_load_status": "seir_sampler *s, uint64_t out[8], int32_t clear",
}


# ---- 1. the symbols ------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound_with_the_headers_types():
    lib = check_symbols(NEW)
    # a null sampler is refused before anything touches a device
    one = (ctypes.c_double * 2)(0.0, 1.0)
    out = (ctypes.c_uint64 * 8)()
    assert lib.seir_sampler_load_trace(None, 0, 0, 1, one, one) == _lib.ERR_INVALID and b"null sampler" in lib.seir_last_error()
    assert lib.seir_sampler_load_status(None, out, 0) == _lib.ERR_INVALID
    for name in ("load_trace", "load_status", "replay"):
        assert callable(getattr(ChainSampler, name))
    # the table of burst products and the draws' signatures are what they were: a replay is `sample` without the sweeps
    import inspect
    want = [p.request for p in BURST_PRODUCTS if p.request]
    sig = inspect.signature(ChainSampler.replay).parameters
    assert list(sig)[:4] == ["self", "theta", "events", "events_out"] and list(sig)[4:] == want
    assert list(inspect.signature(ChainSampler.sample).parameters)[3:] == want
    assert len(_lib.LOAD_CODES) == 6


# ---- 2. load_classify: csrc/trace_load.h as plain C++ ------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include <cstring>
#include <cinttypes>
#include "trace_load.h"
int main() {
    unsigned long long bits;
    int width;
    while (std::scanf("%llx %d", &bits, &width) == 2) {
        double x;
        std::memcpy(&x, &bits, 8);
        const seir::LoadCell r = seir::load_classify(x, width);
        std::printf("%" PRId64 " %d %d\n", r.value, r.code, (int)seir::load_theta_bad(bits));
    }
    const int64_t s0[3] = {5, 0, 2};
    std::printf("%d %d %d %d\n", seir::load_state_below_zero(s0, 5, 5, 7), seir::load_state_below_zero(s0, 6, 5, 7),
                seir::load_state_below_zero(s0, 5, 6, 7), seir::load_state_below_zero(s0, 5, 5, 8));
    std::printf("%" PRIu64 "\n", seir::load_key(((uint64_t)1 << 40) - 1, seir::LOAD_BAD_THETA));
    return 0;
}
"""


def _classify(x, width):
    """The table of csrc/trace_load.h, restated with exact rationals: the first row that applies."""
    top = 65535 if width == 16 else 2 ** 31 - 1
    if math.isnan(x) or math.isinf(x) or abs(x) >= 2 ** 53 or x != math.floor(x):
        return 0, R.LOAD_NOT_INTEGER
    if x < 0:
        return 0, R.LOAD_NEGATIVE
    if x > top:
        return 0, R.LOAD_OVER_WIDTH
    return int(x), R.LOAD_OK


VALUES = [0.0, -0.0, 0.5, 1.0 - 2.0 ** -53, 65535.0, 65536.0, 2.0 ** 31 - 1, 2.0 ** 31, 2.0 ** 53 - 1, 2.0 ** 53, 1e300, 5e-324,
          float("nan"), -float("nan"), float("inf"), -float("inf"), -1.0, -0.5, 1.0, 7.0, 65534.5, -(2.0 ** 53), -1e300, 2.0 ** 52 + 0.5]


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_load_classify_as_plain_cxx_against_the_table():
    cxx = None
    try:
        cxx = [entry._hipcc(), "-x", "c++"]
    except RuntimeError:
        for cand in ("g++", "c++", "clang++"):
            if shutil.which(cand):
                cxx = [cand]
                break
    assert cxx, "no C++ compiler"
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "driver.cpp"), os.path.join(d, "driver")
        open(src, "w").write(DRIVER)
        subprocess.run(cxx + ["-std=c++17", "-O1", "-Wall", "-Werror", "-I", entry.CSRC, "-o", exe, src], check=True,
                       capture_output=True, text=True)
        cases = [(x, w) for w in (16, 32) for x in VALUES]
        text = "".join(f"{_bits(x):x} {w}\n" for x, w in cases)
        out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.split("\n")
    rows = [tuple(int(v) for v in row.split()) for row in out if row]
    assert len(rows) == len(cases) + 2
    seen = set()
    for (x, w), (value, code, bad) in zip(cases, rows):
        assert (value, code) == _classify(x, w), (x, w, value, code)
        assert bool(bad) == (math.isnan(x) or math.isinf(x)), x
        nv, nc = R.classify(np.array([x]), w)                  # the NumPy definition says the same
        assert (int(nv[0]), int(nc[0])) == (value, code), (x, w)
        seen.add(code)
    assert seen == {0, 1, 2, 3}
    by = {(x, w): r[:2] for (x, w), r in zip(cases, rows) if not math.isnan(x)}
    assert by[(-0.0, 16)] == (0, 0) and by[(65535.0, 16)] == (65535, 0) and by[(65536.0, 16)] == (0, 3) and by[(65536.0, 32)] == (65536, 0)
    assert by[(2.0 ** 31 - 1, 32)] == (2 ** 31 - 1, 0) and by[(2.0 ** 31, 32)] == (0, 3) and by[(2.0 ** 53 - 1, 32)] == (0, 3)
    assert by[(2.0 ** 53, 32)] == (0, 1) and by[(-0.5, 16)] == (0, 1) and by[(-1.0, 32)] == (0, 2) and by[(5e-324, 16)] == (0, 1)
    assert rows[-2] == (0, 1, 2, 4)                            # S, E, I one below zero, each alone
    assert rows[-1] == ((2 ** 40 - 1) * 8 + 5,) and rows[-1][0] < 2 ** 43


# ---- 3. the NumPy definition of the status words ---------------------------------------------------------------------
def _loop(theta, events, init, width):
    """check_draws, plainly: Python integers, a cell at a time."""
    n, M, T, _ = events.shape
    out, keys = [0] * 5, []
    for j in range(n):
        for m in range(M):
            st = [int(init[m][x]) for x in range(3)]
            for t in range(T):
                k = []
                for x in range(3):
                    value, code = _classify(float(events[j, m, t, x]), width)
                    k.append(value)
                    if code:
                        out[code - 1] += 1
                        keys.append((((j * M + m) * T + t) * 3 + x) * 8 + code)
                st = [st[0] - k[0], st[1] + k[0] - k[1], st[2] + k[1] - k[2]]
                for x in range(3):
                    if st[x] < 0:
                        out[3] += 1
                        keys.append((((j * M + m) * T + t) * 3 + x) * 8 + R.LOAD_NEG_STATE)
    for j in range(theta.shape[0]):
        for p in range(theta.shape[1]):
            if not math.isfinite(theta[j, p]):
                out[4] += 1
                keys.append((j * theta.shape[1] + p) * 8 + R.LOAD_BAD_THETA)
    return out + [min(keys) if keys else 0]


def test_check_draws_hand_cases():
    init = np.array([[5.0, 1.0, 2.0, 0.0], [3.0, 0.0, 0.0, 0.0]])
    T = 4
    theta = np.zeros((1, 3))
    ev = np.zeros((1, 2, T, 3))
    assert not R.check_draws(theta, ev, init, 16).any()
    # S one below zero at boundary 1: six leave five
    e = ev.copy()
    e[0, 0, 0, 0] = 6
    got = R.check_draws(theta, e, init, 16)
    assert got.tolist() == [0, 0, 0, T, 0, 0 * 8 + 4]          # ... and it stays below at every later boundary
    # S below zero at boundary T only
    e = ev.copy()
    e[0, 1, :, 0] = [1, 1, 1, 1]
    got = R.check_draws(theta, e, init, 16)
    assert got.tolist() == [0, 0, 0, 1, 0, (((0 * 2 + 1) * T + T - 1) * 3 + 0) * 8 + 4]
    # E one below zero at boundary T only: two leave the one that is there
    e = ev.copy()
    e[0, 0, T - 1, 1] = 2
    got = R.check_draws(theta, e, init, 32)
    assert got.tolist() == [0, 0, 0, 1, 0, ((T - 1) * 3 + 1) * 8 + 4]
    # I one below zero at boundary 2, back at zero behind day 2
    e = ev.copy()
    e[0, 0, 1, 2], e[0, 0, 2, 1] = 3, 1
    got = R.check_draws(theta, e, init, 32)
    assert got.tolist() == [0, 0, 0, 1, 0, (1 * 3 + 2) * 8 + 4]
    # a bad cell counts 0 in the state; the smallest key wins whatever its category
    e = ev.copy()
    e[0, 1, 3, 2] = 0.5
    th = theta.copy()
    th[0, 2] = np.inf
    got = R.check_draws(th, e, init, 16)
    assert got.tolist() == [1, 0, 0, 0, 1, 2 * 8 + 5]
    assert np.array_equal(R.check_draws(th, e, init, 16), np.array(_loop(th, e, init, 16), np.uint64))


@pytest.mark.parametrize("width", [16, 32])
def test_check_draws_against_a_plain_loop_on_random_data_with_every_category(width):
    rng = np.random.default_rng(width)
    n, M, T, P = 3, 4, 9, 7
    top = 65535 if width == 16 else 2 ** 31 - 1
    init = np.stack([rng.integers(20, 60, M), rng.integers(0, 5, M), rng.integers(0, 5, M), np.zeros(M, np.int64)], axis=1).astype(np.float64)
    ev = rng.integers(0, 3, size=(n, M, T, 3)).astype(np.float64)
    pick = rng.random(ev.shape) < 0.1
    ev[pick] = rng.choice([0.5, -3.0, np.nan, float(top) + 1.0, float(top), 1e300, -0.0, -np.inf], size=int(pick.sum()))
    theta = rng.standard_normal((n, P))
    theta[1, 2], theta[2, 6] = np.nan, -np.inf
    got = R.check_draws(theta, ev, init, width)
    assert got.dtype == np.uint64 and got[:5].all()
    assert got.tolist() == _loop(theta, ev, init, width)


# ---- 4. theta, rows and the refusals ---------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("T", [1, 2, 5])
def test_theta_assembly_is_the_inverse_of_draws_to_dict(M, T):
    rng = np.random.default_rng([M, T])
    n, P = 4, 6 + (T - 1) + M
    theta = rng.standard_normal((n, 2, P))
    theta[0, 1, 0] = -0.0
    ev = np.zeros((n, 2, M, T, 3), np.int32)
    for c in range(2):
        d = inf.draws_to_dict(theta, ev, c)
        back = R.theta_from_samples({k: d[k] for k in R.PARAMETER_KEYS}, M, T)
        assert back.shape == (n, P) and back.tobytes() == np.ascontiguousarray(theta[:, c]).tobytes()
        assert inf.theta_to_dict(theta[:, c], M, T).keys() == {k: 0 for k in R.PARAMETER_KEYS}.keys()
        for k in R.PARAMETER_KEYS:
            assert np.array_equal(inf.theta_to_dict(theta[:, c], M, T)[k], d[k])


def test_row_selection():
    assert R.select_rows(10, 4).tolist() == [4, 5, 6, 7, 8, 9]
    assert R.select_rows(10, 4, 9, 2).tolist() == [4, 6, 8]
    assert R.select_rows(10, 9).tolist() == [9] and R.select_rows(10, 0, 1).tolist() == [0]
    for args, msg in (((10, 10), "first=10"), ((10, -1), "first=-1"), ((10, 4, 11), "stop=11"), ((10, 4, 4), "nothing to replay"),
                      ((10, 4, 3), "nothing to replay"), ((10, 4, None, 0), "every=0")):
        with pytest.raises(ValueError, match=msg):
            R.select_rows(*args)


def _posterior_file(path, M, T, n, seed=0, seir=True, chain=0):
    rng = np.random.default_rng(seed)
    theta = rng.standard_normal((n, 1, 6 + T - 1 + M))
    ev = rng.integers(0, 2, size=(n, 1, M, T, 3)).astype(np.int32)
    post = inf.Posterior(path, M, T, 2, n, **({} if seir else dict(summaries="only")))
    d = inf.draws_to_dict(theta, ev, 0)
    if not seir:
        d.pop("seir")
    post.write_samples({k: v for k, v in d.items() if f"samples/{k}" in post.shapes}, 0)
    post.create_dataset("initial_state", np.tile([50.0, 2.0, 2.0, 0.0], (M, 1)))
    post.close()
    return theta[:, 0], ev[:, 0]


@pytest.mark.parametrize("ext", [".hd5", ".npz"])
def test_the_files_are_read_by_rows_and_every_refusal_comes_before_any_gpu_call(tmp_path, ext, monkeypatch):
    assert hdf5io.available(), "the HDF5 reader is part of what this project needs"
    M, T, n = 3, 5, 9
    a, b = str(tmp_path / f"a{ext}"), str(tmp_path / f"b{ext}")
    ta, ea = _posterior_file(a, M, T, n, 1)
    tb, eb = _posterior_file(b, M, T, n, 2)
    sources, rows = R.open_sources([a, b], M, T, first=2, every=3)
    assert rows.tolist() == [2, 5, 8]
    for src, th, ev in zip(sources, (ta, tb), (ea, eb)):
        got_th, got_ev = src.draws(rows)
        assert got_th.tobytes() == np.ascontiguousarray(th[rows]).tobytes()
        assert got_ev.dtype == np.float64 and np.array_equal(got_ev, ev[rows])
        one_th, one_ev = src.draws(rows[1:2])
        assert np.array_equal(one_th, th[5:6]) and np.array_equal(one_ev, ev[5:6])
        assert np.array_equal(src.initial_state(), np.tile([50.0, 2.0, 2.0, 0.0], (M, 1)))
        src.close()
    # --first defaults to the warm-up's length: these files are shorter
    with pytest.raises(ValueError, match=f"first={inf.warmup_size()}: the file holds 9"):
        R.open_sources([a], M, T)
    only, short, other = str(tmp_path / f"only{ext}"), str(tmp_path / f"short{ext}"), str(tmp_path / f"other{ext}")
    _posterior_file(only, M, T, n, seir=False)
    _posterior_file(short, M, T, n - 1)
    _posterior_file(other, M + 1, T, n)
    for files, kw, msg in (([a, only], {}, "no samples/seir -- an output of `summaries: only`"), ([a, short], {}, "files of one job have one length"),
                           ([a, other], {}, "samples/seir is for M = 4"), ([a], dict(first=9), "first=9"),
                           ([a], dict(first=3, stop=3), "nothing to replay"), ([], {}, "no posterior file")):
        with pytest.raises(ValueError, match=msg):
            R.open_sources(files, M, T, **dict(dict(first=0), **kw))
    # the driver refuses before it opens a device: a model or a sampler here would be an error of its own
    from covid19uk_amd import sampler as sampler_mod, seir as seir_mod, synth

    def no_gpu(*a, **k):
        raise AssertionError("a GPU call before the refusal")
    monkeypatch.setattr(seir_mod, "SeirModel", no_gpu)
    monkeypatch.setattr(sampler_mod, "ChainSampler", no_gpu)
    cov = synth.make_covariates("ni11")
    events, _, _ = synth.simulate_epidemic(cov)
    data = str(tmp_path / "data.npz")
    inf.write_inference_data(data, cov, events[..., 2])
    good = str(tmp_path / f"good{ext}")
    _posterior_file(good, cov.M, cov.T, n)
    cfg = dict(dmax=84, nmax=25, m=2, occult_nmax=15, num_event_time_updates=5, num_bursts=2, num_burst_samples=4)
    out = str(tmp_path / "out.hd5")
    for files, kw, msg in (([a], dict(first=0), "samples/seir is for M = 3"), ([good], {}, "first=1825"),
                           ([good], dict(first=0, forecast=999), "forecast"), ([good], dict(first=0, rt=cov.T + 1), "rt"),
                           ([good], dict(first=0, groups_rt=True), "groups_rt given without groups"),
                           ([good], dict(first=0, summaries="sometimes"), "summaries"),
                           ([good], dict(first=0, forecast_quantiles="0.5"), "forecast"),
                           ([good], dict(first=0, diagnostics="on", burst=9), "diagnostics"),
                           ([good], dict(first=0, diagnostics="on", burst=4), "whole bursts"),
                           ([good], dict(first=0, burst=0), "burst=0")):
        with pytest.raises(ValueError, match=msg):
            R.replay_files(data, files, out, cfg, **kw)
    assert not os.path.exists(out)


def test_the_cli_parses_and_the_forwarder_resolves(tmp_path, monkeypatch):
    import covid19uk.posterior.replay as fwd
    assert fwd.main is R.main and fwd.replay_files is R.replay_files
    seen = {}
    monkeypatch.setattr(R, "replay_files", lambda *a, **k: seen.update(args=a, kw=k))
    cfg = tmp_path / "c.yaml"
    cfg.write_text("Mcmc:\n  num_burst_samples: 4\n  num_bursts: 2\n")
    R.main(["-c", str(cfg), "-o", "out.hd5", "data.nc", "p0.hd5", "p1.hd5", "--first", "5", "--stop", "20", "--every", "3", "--burst", "2",
            "--first-chain-id", "4", "--seed", "7", "--events-dtype", "int32", "--summaries", "only", "--forecast", "14",
            "--forecast-quantiles", "0.1,0.9", "--rt", "7", "--rt-quantiles", "0.5", "--check", "3", "--within-between", "2",
            "--groups", "nations", "--groups-rt", "--groups-within-between", "--groups-ngm", "--diagnostics", "on",
            "--diagnostics-batch", "2", "--forecast-walk"])
    assert seen["args"] == ("data.nc", ["p0.hd5", "p1.hd5"], "out.hd5", dict(num_burst_samples=4, num_bursts=2))
    assert seen["kw"] == dict(seed=7, device=None, first=5, stop=20, every=3, burst=2, first_chain_id=4, events_dtype="int32",
                              summaries="only", forecast=14, forecast_quantiles="0.1,0.9", rt=7, rt_quantiles="0.5", check=3,
                              within_between=2, groups="nations", groups_rt=True, groups_within_between=True, groups_ngm=True,
                              diagnostics="on", diagnostics_batch=2, forecast_walk=True)
    R.main(["-c", str(cfg), "-o", "out.hd5", "data.nc", "p0.hd5"])
    assert seen["kw"] == dict(seed=0, device=None, first=None, stop=None, every=1, burst=None, first_chain_id=0, events_dtype="auto")


# ---- 5. the driver with a stub sampler -------------------------------------------------------------------------------
FORBIDDEN = ("run", "reset_trace", "set_adaptation", "set_kernel", "sample", "sample_bursts", "set_thin", "snapshot", "restore")


class ReplayStub(NgmStub):
    """NgmStub with `replay`: the products of a replayed burst are those its `sample` would give; what a replay must never
    call is recorded as such."""

    def replay(self, theta, events, **kw):
        n = theta[0].shape[0]
        self.calls.append(("replay", n, kw))
        tr = self._trace(n, events=False, **kw)
        tr.theta = np.stack(theta, axis=1)
        tr.hmc = {k: np.zeros_like(v) for k, v in tr.hmc.items()}
        self.loaded.append((np.stack(theta, axis=1), np.stack(events, axis=1)))
        return tr

    def mark(self, which):
        self.calls.append(("mark", which, self.sweeps))


for _name in FORBIDDEN:
    setattr(ReplayStub, _name, (lambda name: lambda self, *a, **k: self.calls.append(("forbidden", name)))(_name))


class StubSource:
    def __init__(self, c, n, P, M, T):
        self.path, self.reads = f"posterior_chain{c}.hd5", []
        rng = np.random.default_rng(c)
        self.theta, self.events = rng.standard_normal((n, P)), rng.integers(0, 3, size=(n, M, T, 3)).astype(np.float64)

    def draws(self, rows):
        self.reads.append(np.asarray(rows).tolist())
        return self.theta[rows], self.events[rows]


def _replay(tmp_path, tag, config, rows, burst, ext=".npz", stub=ReplayStub):
    s = stub()
    s.loaded = []
    n = len(rows)
    config = dict(config, num_burst_samples=burst, num_bursts=-(-n // burst), thin=1)
    config, opt = inf.resolve_products(config)
    names = [str(tmp_path / f"{tag}_{c}{ext}") for c in range(s.B)]
    posts = [inf.Posterior(name, s.M, s.T, 2, n, burst=burst, results=False, **inf.posterior_kwargs(config, opt, TABLE, n)) for name in names]
    for p in posts:
        p.write_groups(TABLE, POP, np.arange(12.0).reshape(3, 4))
    sources = [StubSource(c, 40, s.P, s.M, s.T) for c in range(s.B)]
    logname = str(tmp_path / f"{tag}.log")
    with open(logname, "w") as log:
        pr = inf.product_records(s, config, posts, log=log, seed=21, rt_weight=POP / POP.sum(), groups=TABLE, population=POP, total=n,
                                 results=False)
        got = R.replay_bursts(s, sources, np.asarray(rows), burst, pr, log=log)
    for c, p in enumerate(posts):
        p.create_dataset("replay/rows", np.asarray(rows), dtype=np.int64)
        p.close()
    return s, sources, [_read(name) for name in names], open(logname).read(), got


@pytest.mark.parametrize("ext", [".npz", ".hd5"])
def test_the_driver_resets_once_replays_per_burst_and_finishes_once(tmp_path, ext):
    assert hdf5io.available()
    cfg = dict(FULL, groups_rt="on", groups_ngm="on", summaries="on")
    rows = list(range(7, 37, 3))                                # 10 rows: bursts of 4, 4, 2
    s, sources, files, log, (n, dt, waited) = _replay(tmp_path, "replay", cfg, rows, 4, ext=ext)
    live, live_files, _ = _run_mcmc(tmp_path, "live", dict(cfg, num_bursts=3, num_burst_samples=4), ext=ext, stub=NgmStub, groups=TABLE)
    names = [c[0] for c in s.calls]
    assert "forbidden" not in names and n == 10 and 0.0 <= waited <= dt
    # the resets and the stores: once, in run_mcmc's order
    setup = [x for x in names if x not in ("replay", "mark")]
    live_setup = [c[0] for c in live.calls if c[0] not in ("sample", "burst", "mark", "set_thin")]
    assert setup == live_setup
    sizes = {c[0]: c for c in s.calls}
    assert sizes["set_group_ngm"][2] == 10 and sizes["keep_rt_draws"][1] == 10 and sizes["read_group_ngm"][1:] == (10, 0)
    # per burst one replay, with the sampling phase's keyword set (a replay returns no event tensor)
    replays = [c for c in s.calls if c[0] == "replay"]
    live_kw = [c[2] for c in live.calls if c[0] == "burst"][0]
    assert [c[1] for c in replays] == [4, 4, 2]
    assert all(c[2] == {k: v for k, v in live_kw.items() if k != "events"} for c in replays)
    assert names.index("replay") > max(i for i, x in enumerate(names) if x.startswith(("reset_", "set_", "keep_")))
    # every file is read by bursts, each burst once, in order; what was read is what was loaded
    for c, src in enumerate(sources):
        assert src.reads == [rows[0:4], rows[4:8], rows[8:10]]
        assert np.array_equal(np.concatenate([th[:, c] for th, _ in s.loaded]), src.theta[rows])
        assert np.array_equal(np.concatenate([ev[:, c] for _, ev in s.loaded]), src.events[rows])
    assert [ln for ln in log.splitlines() if ln.startswith("  burst")] == ["  burst 1/3", "  burst 2/3", "  burst 3/3"]
    # the datasets: a live run's for its sampling phase, without results/ and samples/seir, with replay/
    for c, f in enumerate(files):
        want = {k for k in live_files[c] if not k.startswith("results/") and k != "samples/seir"}
        assert set(f) == want | {"replay/rows"}
        assert np.array_equal(f["replay/rows"], rows)
        assert f["samples/psi"].shape == (10,) and np.array_equal(f["samples/psi"], sources[c].theta[rows, 0])
        assert np.array_equal(f["samples/spatial_effect"], sources[c].theta[rows][:, -s.M:])
        assert f["samples/seir_by_day"].shape == (10, s.T, 3) and f["samples/R_t"].shape == (10, 3)
        assert f["samples/ngm_by_group"].shape == (10, s.G, s.G, 3) and f["ngm/count"][0] == 10


def test_the_marks_fall_where_diagnostics_marks_puts_them(tmp_path):
    from tests.test_diagnostics_host import DiagStub

    class DiagReplayStub(DiagStub):
        def replay(self, theta, events, **kw):
            n = theta[0].shape[0]
            self.calls.append(("replay", n, kw))
            return self._trace(n, events=False, **kw)

    for nb in (2, 3, 5):
        s = DiagReplayStub()
        ns = 4
        n = nb * ns                                             # half-chains of one length: whole bursts
        config, opt = inf.resolve_products(dict(FULL, rt=None, rt_quantiles=None, within_between=None, summaries="off", diagnostics="on",
                                                num_bursts=nb, num_burst_samples=ns))
        posts = [inf.Posterior(str(tmp_path / f"d{nb}_{c}.npz"), s.M, s.T, 2, n, results=False, **inf.posterior_kwargs(config, opt, None, n))
                 for c in range(s.B)]
        sources = [StubSource(c, n, s.P, s.M, s.T) for c in range(s.B)]
        with open(os.devnull, "w") as log:
            pr = inf.product_records(s, config, posts, log=log, total=n, results=False)
            R.replay_bursts(s, sources, np.arange(n), ns, pr, log=log)
        seq = [c[:2] for c in s.calls if c[0] in ("replay", "mark")]
        want = []
        for i in range(nb):
            want.append(("replay", ns))
            if i in inf.diagnostics_marks(nb):
                want.append(("mark", inf.diagnostics_marks(nb)[i]))
        assert seq == want and [c[0] for c in s.calls].count("diagnostics") == 1
        assert all(c[2] == dict(summarize=True) for c in s.calls if c[0] == "replay")


# ---- 6. run_mcmc after the factoring -----------------------------------------------------------------------------------
PARENT_CALLS = ["set_groups", "set_group_rt", "set_thin"] + ["sample"] * 8 + \
    ["set_thin", "reset_summary", "reset_rt", "keep_rt_draws", "set_group_ngm", "reset_within_between"] + \
    ["burst", "rt", "within_between"] * 3 + \
    ["summary", "rt_summary", "rt_quantiles", "rt_quantiles", "read_group_ngm", "within_between_summary"]


def test_run_mcmc_makes_the_parents_call_list(tmp_path):
    """The list below was recorded on the parent commit with this stub and this configuration."""
    cfg = dict(FULL, groups_rt="on", groups_ngm="on", summaries="on")
    s, files, log = _run_mcmc(tmp_path, "parent", cfg, stub=NgmStub, groups=TABLE)
    assert [c[0] for c in s.calls] == PARENT_CALLS
    kws = [c[2] for c in s.calls if c[0] in ("sample", "burst")]
    assert all(kw == dict(events=True, summarize="marginals", groups=("trace",)) for kw in kws[:8])
    assert all(kw == dict(events=True, summarize=True, rt=True, groups=("trace",), within_between=True) for kw in kws[8:])
    assert [c[1] for c in s.calls if c[0] == "set_thin"] == [1, 1]
    assert any(k.startswith("results/") for k in files[0]) and "samples/seir" in files[0]


# ---- 7. the compiler's account of the new kernels ----------------------------------------------------------------------
def test_the_new_kernels_are_these_instances_without_scratch_or_lds_at_the_summarys_occupancy():
    res = H.kernel_account("replay")
    assert sorted(res) == ["k_trace_load<0>", "k_trace_load<1>", "k_trace_load_theta<256>"], sorted(res)
    base = H.kernel_account("base")
    for name, k in res.items():
        assert k["scratch_bytes_per_lane"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, name
        assert k["lds_bytes_per_block"] == 0, name              # the carry lives in the wave's registers: no LDS at all
        assert k["occupancy_waves_per_simd"] >= base["k_summarize<1,0>"]["occupancy_waves_per_simd"], name

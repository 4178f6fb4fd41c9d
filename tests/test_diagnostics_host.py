"""Host side of the convergence diagnostics (include/seir_hip.h, "Convergence diagnostics"), no GPU: the new C-ABI symbols,
the batch update of covid19uk_amd/csrc/summary_update.h compiled as plain C++ against Python integers, the host's formulas
(covid19uk_amd/posterior/diagnostics.py) against `fractions.Fraction`, seeded sanity brackets of the two estimators, the
pooling tool on files written by `Posterior`, the configuration, and the compiler's account of the new kernel instances.

`accumulate` below is the NumPy restatement of the accumulators' definitions that the GPU tests compare the device with."""
import json
import math
import os
import shutil
import subprocess
import warnings
from fractions import Fraction

import numpy as np
import pytest

import __graft_entry__ as entry
from covid19uk_amd import _lib, hdf5io
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.posterior import diagnostics as dm
from tests import helpers as H
from tests.abi_lib import check_symbols
from tests.test_summary_host import CFG, StubSampler, _read

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "seir_sampler_diag_reset": "seir_sampler *s, int32_t batch_len",
    "seir_sampler_diag_mark": "seir_sampler *s, int32_t which",
    "seir_sampler_read_diag": "seir_sampler *s, uint64_t *nbatch, int64_t *bsum, uint64_t *bsumsq",
    "seir_sampler_read_diag_mark": "seir_sampler *s, int32_t which, uint64_t *count, int64_t *sum, uint64_t *sumsq",
}


def accumulate(x, L, marks=None):
    """x [n, B, ...] integer draws -> `Diagnostics` by the definitions, in int64 (the caller keeps the sums inside it).
    `marks` {number of draws folded when the mark is taken: which}."""
    x = np.asarray(x, np.int64)
    n, B = x.shape[:2]
    d = x - x[:1]
    a = n // L
    closed = d[:a * L].reshape((a, L) + d.shape[1:]).sum(axis=1)
    z = np.zeros_like(d[0])
    mc, ms, mq = np.zeros((2, B), np.uint64), np.stack([z, z]), np.stack([z, z]).astype(np.uint64)
    for at, which in (marks or {}).items():
        mc[which] = at
        ms[which] = d[:at].sum(axis=0)
        mq[which] = (d[:at] * d[:at]).sum(axis=0).astype(np.uint64)
    return dm.Diagnostics(batch_length=L, count=np.full(B, n, np.uint64), ref=x[0].astype(np.int32), sum=d.sum(axis=0),
                          sumsq=(d * d).sum(axis=0).astype(np.uint64), bsum=d[a * L:].sum(axis=0),
                          bsumsq=(closed * closed).sum(axis=0).astype(np.uint64), nbatch=np.full(B, a, np.uint64),
                          mark_count=mc, mark_sum=ms, mark_sumsq=mq)


def same_accumulators(got, want):
    for f in ("count", "ref", "sum", "sumsq", "bsum", "bsumsq", "nbatch", "mark_count", "mark_sum", "mark_sumsq"):
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape, (f, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), f
    assert got.batch_length == want.batch_length


# ---- 1. the symbols ------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound_with_the_headers_types():
    lib = check_symbols(NEW)
    # a null sampler is refused before anything touches a device
    assert lib.seir_sampler_diag_reset(None, 5) == _lib.ERR_INVALID
    assert lib.seir_sampler_diag_mark(None, 0) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_diag(None, None, None, None) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_diag_mark(None, 0, None, None, None) == _lib.ERR_INVALID


# ---- 2. the batch update, as plain C++ -------------------------------------------------------------------------------------
DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include "summary_update.h"
// one cell.  "L v": batch length; "x v": a draw of the call being collected; "e 0": the call ends -- its draws are folded
// the way a launch folds them (count is read at its start and moves at its end) and the state is printed; "r 0": reset;
// "b v" / "q v": set bsum / bsumsq (test set-up); "c 0": close the batch now and print.
// Printed: ref sum sumsq bsum bsumsq count flag
int main() {
    int32_t ref = 0; int64_t sum = 0, bsum = 0; uint64_t sumsq = 0, bsumsq = 0, count = 0, L = 1; bool flag = false;
    static int32_t call[4096]; int n = 0;
    char op[8]; long long v;
    while (std::scanf("%7s %lld", op, &v) == 2) {
        switch (op[0]) {
        case 'L': L = (uint64_t)v; continue;
        case 'x': call[n++] = (int32_t)v; continue;
        case 'r': ref = 0; sum = bsum = 0; sumsq = bsumsq = count = 0; flag = false; n = 0; continue;
        case 'b': bsum = (int64_t)v; continue;
        case 'q': bsumsq = (uint64_t)v; continue;
        case 'c': flag |= seir::summary_batch_close(bsum, bsumsq); break;
        case 'e':
            for (int j = 0; j < n; ++j) {
                flag |= seir::summary_fold(ref, sum, sumsq, call[j], count == 0 && j == 0);
                seir::summary_batch_add(bsum, ref, call[j]);
                if (seir::summary_batch_closes(count, (uint64_t)j, L)) flag |= seir::summary_batch_close(bsum, bsumsq);
            }
            count += (uint64_t)n; n = 0;
            break;
        default: return 2;
        }
        std::printf("%" PRId32 " %" PRId64 " %" PRIu64 " %" PRId64 " %" PRIu64 " %" PRIu64 " %d\n", ref, sum, sumsq, bsum, bsumsq,
                    count, flag ? 1 : 0);
    }
}
"""


@pytest.fixture(scope="module")
def batch(tmp_path_factory):
    cxx = None
    try:
        cxx = [entry._hipcc(), "-x", "c++"]
    except RuntimeError:
        for cand in ("g++", "c++", "clang++"):
            if shutil.which(cand):
                cxx = [cand]
                break
    assert cxx, "no C++ compiler"
    d = tmp_path_factory.mktemp("summary_batch")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run(cxx + ["-std=c++17", "-O1", "-Wall", "-Werror", "-I", entry.CSRC, "-o", str(exe), str(src)],
                   check=True, capture_output=True, text=True)

    def run(lines):
        text = "".join(f"{op} {int(v)}\n" for op, v in lines)
        out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.split("\n")
        return [tuple(int(v) for v in row.split()) for row in out if row]
    return run


def _model(xs, L):
    """Python integers: (ref, sum, sumsq, bsum, bsumsq, count, flag) after all of xs."""
    ref, s, q, bs, bq, flag = xs[0], 0, 0, 0, 0, False
    for j, x in enumerate(xs):
        s += x - ref
        q += (x - ref) ** 2
        bs += x - ref
        flag |= q >= 2 ** 63
        if (j + 1) % L == 0:
            if abs(bs) >= 2 ** 32:
                flag = True
            else:
                bq += bs * bs
                flag |= bq >= 2 ** 63
            bs = 0
    return (ref, s, q, bs, bq, len(xs), int(flag))


def _calls(xs, cuts):
    lines, at = [], 0
    for c in list(cuts) + [len(xs) - sum(cuts)]:
        lines += [("x", v) for v in xs[at:at + c]] + [("e", 0)]
        at += c
    return lines


@pytest.mark.parametrize("L", [1, 7, 50, 100, 1000])
def test_batch_sums_equal_python_integers_however_the_stream_is_cut(batch, L):
    rng = np.random.default_rng(L)
    centre = int(rng.integers(0, 2_000_000))
    xs = [int(v) for v in rng.integers(max(centre - 5000, 0), centre + 5000, size=437)]
    want = _model(xs, L)
    assert want[6] == 0 and (want[4] > 0 or L > len(xs)) and (want[3] != 0 or len(xs) % L == 0)
    whole = batch([("L", L)] + _calls(xs, []))[-1]
    assert whole == want
    for seed in range(4):                                     # calls of arbitrary lengths, single draws among them
        cuts, left = [], len(xs)
        r = np.random.default_rng([L, seed])
        while left > 1 and len(cuts) < 40:
            c = int(r.integers(1, max(2, min(left, 3 * L, 128))))
            cuts.append(c)
            left -= c
        got = batch([("L", L)] + _calls(xs, cuts))
        assert got[-1] == want, (cuts, got[-1], want)
        at = 0
        for c, row in zip(cuts, got):                         # ... and after every call, not only at the end
            at += c
            assert row == _model(xs[:at], L)


def test_closing_a_batch_raises_the_flag_at_2_to_32_and_at_2_to_63(batch):
    # |bsum| = 2^32 - 1 is the largest whose square fits 64 bits: it is added exactly (and, being past 2^63, raises the flag
    # by that rule); 2^32 itself raises the flag and leaves bsumsq alone; both signs.  The largest batch sum that closes
    # cleanly from zero is floor(sqrt(2^63 - 1))
    for sign in (1, -1):
        top = batch([("b", sign * (2 ** 32 - 1)), ("c", 0)])[0]
        assert top[3:5] == (0, (2 ** 32 - 1) ** 2) and top[6] == 1
        bad = batch([("q", 5), ("b", sign * 2 ** 32), ("c", 0)])[0]
        assert bad[3:5] == (0, 5) and bad[6] == 1
        r = math.isqrt(2 ** 63 - 1)
        assert batch([("b", sign * r), ("c", 0)])[0][3:7] == (0, r * r, 0, 0)
        assert batch([("b", sign * (r + 1)), ("c", 0)])[0][3:7] == (0, (r + 1) ** 2, 0, 1)
    assert batch([("b", -2 ** 63), ("c", 0)])[0][6] == 1
    # bsumsq reaching exactly 2^63: one unit short holds, the unit that reaches it raises
    assert batch([("q", 2 ** 63 - 2), ("b", 1), ("c", 0)])[0][4:7:2] == (2 ** 63 - 1, 0)
    assert batch([("q", 2 ** 63 - 1), ("b", 1), ("c", 0)])[0][4:7:2] == (2 ** 63, 1)
    assert batch([("q", 2 ** 63 - 9), ("b", -3), ("c", 0)])[0][4:7:2] == (2 ** 63, 1)
    # a wrap past 2^64 is caught as well, and the flag is sticky
    got = batch([("q", -1), ("b", 2), ("c", 0), ("b", 1), ("c", 0)])
    assert [r[6] for r in got] == [1, 1] and got[0][4] == 3
    # through draws, L = 2: two draws 2^31 - 1 above ref close a batch of 2^32 - 2, squared exactly; with ref = -2^31 the
    # batch sum is 2^33 - 2, which cannot be squared
    d = 2 ** 31 - 1
    got = batch([("L", 2)] + _calls([0, 0, d, d], []))[-1]
    assert got == _model([0, 0, d, d], 2) and got[4] == (2 * d) ** 2 and got[6] == 1
    got = batch([("L", 2)] + _calls([-2 ** 31, -2 ** 31, d, d], []))[-1]
    assert got[3:] == _model([-2 ** 31, -2 ** 31, d, d], 2)[3:] == (0, 0, 4, 1)       # (sumsq itself has wrapped by then)


def test_the_host_accumulator_does_not_care_about_cuts_either_and_agrees_with_the_restatement():
    rng = np.random.default_rng(3)
    x = rng.integers(-300, 300, size=(120, 3, 5))
    for L in (1, 7, 40, 240):
        want = accumulate(x, L, {50: 0, 70: 1})
        for cuts in ([10] * 12, [50, 20, 50], [1, 49, 13, 7, 50], [5] * 10 + [17, 3] + [2] * 25):
            acc, at = dm.DrawAccumulator(L), 0
            for c in cuts:
                acc.fold(x[at:at + c])
                at += c
                if at in (50, 70):
                    acc.mark({50: 0, 70: 1}[at])
            got = acc.result()
            for f in ("sum", "sumsq", "bsum", "bsumsq", "mark_sum", "mark_sumsq", "count", "nbatch", "mark_count"):
                assert np.array_equal(np.asarray(getattr(got, f), np.float64), np.asarray(getattr(want, f), np.float64)), (L, f)
            assert np.array_equal(got.ess, want.ess, equal_nan=True) and np.array_equal(got.rhat, want.rhat, equal_nan=True)


# ---- 3. the host's formulas against exact rationals ---------------------------------------------------------------------
def _exact_ess(x, L):
    n, a = len(x), len(x) // L
    d = [Fraction(int(v) - int(x[0])) for v in x]
    s2 = (sum(v * v for v in d) - sum(d) ** 2 / n) / (n - 1)
    B = [sum(d[k * L:(k + 1) * L]) for k in range(a)]
    sig = (sum(b * b for b in B) - sum(B) ** 2 / a) / ((a - 1) * L)
    return n * s2 / sig


def _exact_var(x):
    n = len(x)
    f = [Fraction(int(v)) for v in x]
    mu = sum(f) / n
    return mu, sum((v - mu) ** 2 for v in f) / (n - 1)


def test_ess_and_rhat_agree_with_fractions_to_the_stated_tolerance():
    """rtol 1e-9 is DESIGN section 0's figure for summed fp64 quantities.  The shifted float64 subtraction
    sumsq - sum^2 / n loses log10(mean square about ref / variance about ref) digits: the inputs keep that ratio below
    1e3 (checked), so 1e-16 x 1e3 stays far inside the bound."""
    rng = np.random.default_rng(11)
    n, B, C, L = 60, 3, 4, 7             # 8 closed batches and 4 draws in the open one
    base = rng.integers(0, 1_000_000, size=(1, B, C))
    x = base + rng.integers(-50, 50, size=(n, B, C)) + (np.arange(n)[:, None, None] // 10) * rng.integers(-9, 9, size=(1, B, C))
    half = 24                                                 # 60 draws: halves of 24, the middle 12 in neither
    dg = accumulate(x, L, {half: 0, n - half: 1})
    for b in range(B):
        for c in range(C):
            for seg in (x[:, b, c], x[:half, b, c], x[n - half:, b, c]):
                d = seg.astype(np.float64) - float(x[0, b, c])
                assert d.var(ddof=1) >= 1e-3 * np.mean(d * d)
    ess, hc, hm, hv, rhat = dg.ess, dg.half_count, dg.half_mean, dg.half_var, dg.rhat
    assert ess.shape == (B, C) and hm.shape == hv.shape == (2, B, C) and rhat.shape == (C,)
    assert np.array_equal(hc, np.full((2, B), half))
    for c in range(C):
        means, vars_ = [], []
        for b in range(B):
            assert ess[b, c] == pytest.approx(float(_exact_ess(x[:, b, c], L)), rel=1e-9)
            for h, seg in enumerate((x[:half, b, c], x[n - half:, b, c])):
                mu, var = _exact_var(seg)
                assert hm[h, b, c] == pytest.approx(float(mu), rel=1e-9) and hv[h, b, c] == pytest.approx(float(var), rel=1e-9)
                means.append(mu)
                vars_.append(var)
        k = len(means)
        W = sum(vars_) / k
        centre = sum(means) / k
        Bn = sum((m - centre) ** 2 for m in means) / (k - 1)
        want = math.sqrt(float((Fraction(half - 1, half) * W + Bn) / W))
        assert rhat[c] == pytest.approx(want, rel=1e-9)
    # without mark 1 the second half starts at mark 0
    dg0 = accumulate(x, L, {30: 0})
    assert np.array_equal(dg0.half_count, np.full((2, B), 30))
    assert dg0.half_mean[1, 1, 2] == pytest.approx(float(_exact_var(x[30:, 1, 2])[0]), rel=1e-9)
    assert dg0.half_var[1, 1, 2] == pytest.approx(float(_exact_var(x[30:, 1, 2])[1]), rel=1e-9)
    # a parameter-like float series through the host accumulator: the same formulas
    acc = dm.DrawAccumulator(L)
    acc.fold(x[:half].astype(np.float64))
    acc.mark(0)
    acc.fold(x[half:n - half].astype(np.float64))
    acc.mark(1)
    acc.fold(x[n - half:].astype(np.float64))
    th = acc.result()
    np.testing.assert_allclose(th.ess, ess, rtol=1e-12)
    np.testing.assert_allclose(th.rhat, rhat, rtol=1e-12)


def test_undefined_results_are_nan_without_a_warning():
    rng = np.random.default_rng(2)
    x = rng.integers(0, 50, size=(12, 2, 4))
    x[:, :, 0] = 17                                           # a cell that never changes
    x[:, 1, 1] = 3                                            # ... in one chain only
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        dg = accumulate(x, 4, {6: 0})                         # a = 3
        ess, rhat = dg.ess, dg.rhat
        assert np.isnan(ess[:, 0]).all() and np.isnan(ess[1, 1]) and np.isfinite(ess[0, 1:]).all() and np.isfinite(ess[1, 2:]).all()
        assert np.isnan(rhat[0]) and np.isfinite(rhat[1:]).all()           # W = 0 only where every half-chain is constant
        one = accumulate(x, 8, {6: 0})                        # a = 1 < 2
        assert np.isnan(one.ess).all() and np.isfinite(one.rhat[1:]).all()
        none = accumulate(x, 100, {6: 0})                     # a = 0
        assert np.isnan(none.ess).all()
        short = accumulate(x[:2], 1, {1: 0})                  # half-chains of one draw: n < 2
        assert np.isnan(short.rhat).all() and np.isnan(short.half_var).all() and np.isfinite(short.half_mean).all()
        single = accumulate(x[:1], 1)                         # one draw, no mark
        assert np.isnan(single.ess).all() and np.isnan(single.half_var).all()
        line = dm.summary_line(rhat, np.full((2, 3), np.nan), ess[0], np.full(4, np.nan), ["a", "b", "c", "d"])
        assert "no non-constant latent cell" in line and "undefined" in line
        assert np.isnan(dm.sum_ess(ess)[0]) and dm.sum_ess(ess)[1] == ess[0, 1]
    with pytest.raises(ValueError, match="one length"):
        dm.split_rhat(np.array([[5, 5], [5, 6]]), np.zeros((2, 2, 3)), np.ones((2, 2, 3)))


# ---- 4. the estimators do what they are for (seeded) --------------------------------------------------------------------
def test_ess_of_independent_draws_is_about_n():
    """a = 100 batches: sigma^2_bm has a relative standard deviation of about sqrt(2 / 99) = 0.14; [0.3, 1.7] is +-5 of them."""
    rng = np.random.default_rng(101)
    a, L = 100, 50
    x = rng.integers(0, 1000, size=(a * L, 4, 6))
    ratio = accumulate(x, L).ess / (a * L)
    print("iid ESS / n:", np.sort(ratio.reshape(-1)))
    assert ratio.min() > 0.3 and ratio.max() < 1.7


def test_ess_of_an_ar1_series_is_within_a_factor_of_two_of_theory():
    rng = np.random.default_rng(202)
    rho, a, L, C = 0.9, 100, 200, 8
    n = a * L
    e = rng.normal(size=(n, 1, C)) * math.sqrt(1 - rho * rho) * 100.0
    y = np.empty_like(e)
    y[0] = rng.normal(size=(1, C)) * 100.0
    for j in range(1, n):
        y[j] = rho * y[j - 1] + e[j]
    ess = accumulate(np.rint(y).astype(np.int64), L).ess
    want = n * (1 - rho) / (1 + rho)
    print("AR(1) ESS:", ess.reshape(-1), "theory", want)
    assert (ess > want / 2).all() and (ess < want * 2).all()


def test_rhat_is_near_one_for_equal_chains_and_large_for_a_shifted_one():
    rng = np.random.default_rng(303)
    n, B, C = 1000, 4, 10
    x = rng.integers(0, 200, size=(n, B, C)) + 10_000
    same = accumulate(x, 50, {n // 2: 0}).rhat
    sd = float(x[:, 0].std())
    x[:, 2] += int(round(2 * sd))                             # one chain two standard deviations away
    moved = accumulate(x, 50, {n // 2: 0}).rhat
    print("R-hat equal:", same, "one chain shifted:", moved)
    assert (same < 1.05).all() and (same > 0.99).all()
    assert (moved > 1.2).all()


# ---- 5. the pooling tool on files written by Posterior -------------------------------------------------------------------
def _latent_and_theta(seed, B, n=40, M=3, T=5, L=5, marks=None):
    rng = np.random.default_rng(seed)
    P = 6 + T - 1 + M
    x = rng.integers(0, 30, size=(n, B, M, T, 6)) + rng.integers(0, 3, size=(1, B, 1, 1, 6))
    x[:, :, 0, 0] = 4                                         # a constant cell
    theta = rng.normal(size=(n, B, P)) + 0.3 * np.arange(B)[None, :, None]
    marks = marks or {n // 2: 0}
    acc = dm.DrawAccumulator(L)
    at = 0
    for cut in sorted(marks) + [n]:
        acc.fold(theta[at:cut])
        if cut in marks:
            acc.mark(marks[cut])
        at = cut
    return accumulate(x, L, marks), acc.result(), (M, T, P)


@pytest.mark.parametrize("ext", [".hd5", ".npz"])
def test_pooling_two_chain_files_equals_rhat_over_both_chains_at_once(tmp_path, ext, capsys):
    if ext == ".hd5" and not hdf5io.available():
        ext = ".npz"
    lat, th, (M, T, P) = _latent_and_theta(7, 2)
    both = dm.evaluate(lat, th)
    names = []
    for c in range(2):                                        # each chain as a process of its own: one file each
        one = lambda d: dm.Diagnostics(d.batch_length, *(getattr(d, f)[c:c + 1] for f in ("count", "ref", "sum", "sumsq", "bsum", "bsumsq", "nbatch")),  # noqa: E731,E501
                                       *(getattr(d, f)[:, c:c + 1] for f in ("mark_count", "mark_sum", "mark_sumsq")))
        ev = dm.evaluate(one(lat), one(th))
        name = str(tmp_path / f"posterior_chain{c}{ext}")
        post = inf.Posterior(name, M, T, 2, 4)
        post.write_diagnostics(dm.chain_datasets(ev, 0))
        post.close()
        names.append(name)
        f = _read(name)
        assert {k for k in f if k.startswith("diagnostics/")} == {f"diagnostics/{k}" for k in dm.NAMES}
        assert f["diagnostics/seir_half_mean"].shape == (2, M, T, 3) and f["diagnostics/state_ess"].shape == (M, T, 3)
        assert f["diagnostics/theta_half_var"].shape == (2, P) and f["diagnostics/half_count"].shape == (2,)
    out = str(tmp_path / f"diagnostics{ext}")
    pooled = dm.main(names + ["-o", out])
    line = capsys.readouterr().out
    assert "2 chain(s)" in line and "largest theta R-hat" in line and "non-constant latent cells" in line and "smallest ESS" in line
    assert np.array_equal(pooled["seir_rhat"], both["latent_rhat"][..., :3], equal_nan=True)
    assert np.array_equal(pooled["state_rhat"], both["latent_rhat"][..., 3:], equal_nan=True)
    assert np.array_equal(pooled["theta_rhat"], both["theta_rhat"])
    assert np.isnan(pooled["seir_rhat"][0, 0]).all() and np.isfinite(pooled["seir_rhat"][1:]).all()
    np.testing.assert_allclose(pooled["theta_ess"], both["theta_ess"].sum(axis=0), rtol=1e-14)
    assert np.array_equal(pooled["seir_ess"], dm.sum_ess(both["latent_ess"][..., :3]), equal_nan=True)
    # ... and the file it wrote holds the same
    disk = _read(out)
    for k, v in pooled.items():
        assert np.array_equal(np.asarray(disk[k]).reshape(np.shape(v)), v, equal_nan=True), k
    # the forwarder serves the same entry point; a file without the group is refused by name
    import covid19uk.posterior.diagnostics as fwd
    assert fwd.main is dm.main
    bare = str(tmp_path / f"bare{ext}")
    inf.Posterior(bare, M, T, 2, 4).close()
    with pytest.raises(ValueError, match="diagnostics on"):
        dm.main([bare, "-o", out])


# ---- 6. configuration, command line, run_mcmc ---------------------------------------------------------------------------
def test_diagnostics_value_is_parsed_and_bad_ones_refused_before_any_gpu_call(tmp_path):
    assert inf.diagnostics_mode({}) == ("off", 0)
    assert inf.diagnostics_mode(dict(CFG, diagnostics="on")) == ("on", 4)                 # one burst is one batch
    assert inf.diagnostics_mode(dict(CFG, diagnostics=True)) == ("on", 4) and inf.diagnostics_mode(dict(CFG, diagnostics=False))[0] == "off"
    assert inf.diagnostics_mode(dict(CFG, diagnostics="on"), "off") == ("off", 0)         # the command line overrides
    assert inf.diagnostics_mode(CFG, "on", 2) == ("on", 2) and inf.diagnostics_mode(dict(CFG, diagnostics_batch=8), "on") == ("on", 8)
    for bad in (3, 6, 0, -4):                                 # neither a divisor nor a multiple of the burst's 4 draws
        with pytest.raises(ValueError, match="batch"):
            inf.diagnostics_mode(CFG, "on", bad)
    with pytest.raises(ValueError, match="diagnostics"):
        inf.diagnostics_mode(dict(CFG, diagnostics="sometimes"))
    with pytest.raises(ValueError, match="num_bursts"):
        inf.diagnostics_mode(dict(CFG, num_bursts=1), "on")
    for cfg, kw in ((CFG, dict(batch=4)), (dict(CFG, diagnostics_batch=4), {}), (dict(CFG, diagnostics="on"), dict(override="off", batch=4))):
        with pytest.raises(ValueError, match="no effect"):                      # a batch length with nothing to cut is not dropped in silence
            inf.diagnostics_mode(cfg, **kw)
    # mcmc() refuses all of it before it reads the data file or opens a device: the file named here does not exist
    nofile, out = str(tmp_path / "no_such_file.nc"), str(tmp_path / "out.hd5")
    with pytest.raises(ValueError, match="diagnostics"):
        inf.mcmc(nofile, out, dict(CFG, diagnostics="sometimes"))
    with pytest.raises(ValueError, match="num_bursts"):
        inf.mcmc(nofile, out, dict(CFG, num_bursts=1), diagnostics="on")
    with pytest.raises(ValueError, match="num_bursts"):
        inf.mcmc(nofile, out, dict(CFG, num_bursts=1, diagnostics="on"))
    with pytest.raises(ValueError, match="batch"):
        inf.mcmc(nofile, out, CFG, diagnostics="on", diagnostics_batch=3)
    with pytest.raises(ValueError, match="no effect"):
        inf.mcmc(nofile, out, CFG, diagnostics_batch=4)
    with pytest.raises(ValueError, match="no effect"):
        inf.mcmc(nofile, out, dict(CFG, diagnostics_batch=4))
    with pytest.raises(SystemExit):
        inf.main(["-c", str(tmp_path / "no_such.yaml"), "-o", "x", "--diagnostics", "maybe", "data.nc"])
    assert not os.path.exists(out)
    assert inf.diagnostics_marks(2) == {0: 0} and inf.diagnostics_marks(4) == {1: 0}
    assert inf.diagnostics_marks(3) == {0: 0, 1: 1} and inf.diagnostics_marks(5) == {1: 0, 2: 1}     # the middle burst in neither half


class DiagStub(StubSampler):
    """StubSampler with the diagnostics: what is folded and where the marks fall is recorded; `diagnostics()` is the NumPy
    restatement over the folded draws.  The parameter draws vary so that their R-hat is defined."""

    def reset_diagnostics(self, L):
        self.calls.append(("reset_diagnostics", L))
        self.folded, self.L, self.marks = [], L, {}

    def mark(self, which):
        self.calls.append(("mark", which, len(self.folded)))
        self.marks[len(self.folded)] = which

    def _trace(self, n, events=True, summarize=False):
        tr = super()._trace(n, events=events, summarize=summarize)
        idx = (self.sweeps - n + np.arange(n)).astype(np.float64)
        tr.theta = np.sin(idx)[:, None, None] * (1.0 + np.arange(self.B))[None, :, None] + np.arange(self.P)[None, None, :]
        return tr

    def sample_bursts(self, nb, n, consume, marks=None, **kw):
        for i in range(nb):
            self.calls.append(("burst", n, kw))
            tr = self._trace(n, **kw)
            if marks and i in marks:
                self.mark(marks[i])
            consume(tr, i)

    def diagnostics(self):
        self.calls.append(("diagnostics",))
        n = len(self.folded)
        x = np.broadcast_to(np.asarray(self.folded, np.int64)[:, None, None, None, None], (n, self.B, self.M, self.T, 6))
        return accumulate(x, self.L, self.marks)

    def summary(self):
        assert not getattr(self, "L", 0), "with the diagnostics on the moments come with diagnostics()"
        return super().summary()


def _run(tmp_path, tag, config, ext=".npz", cap=800):
    s = DiagStub()
    s.cap = cap
    nb, ns = config["num_bursts"], config["num_burst_samples"]
    names = [str(tmp_path / f"{tag}_{c}{ext}") for c in range(s.B)]
    kw = {} if config.get("summaries", "off") == "off" else dict(summaries=config["summaries"])
    posts = [inf.Posterior(name, s.M, s.T, 2, inf.warmup_size() + nb * ns, **kw) for name in names]
    logname = str(tmp_path / f"{tag}.log")
    with open(logname, "w") as log:
        inf.run_mcmc(s, config, posts, log=log)
    for p in posts:
        p.close()
    return s, [_read(n) for n in names], open(logname).read()


def test_off_calls_nothing_new_and_writes_todays_datasets(tmp_path):
    plain, pf, _ = _run(tmp_path, "plain", CFG)
    off, of, log = _run(tmp_path, "off", dict(CFG, diagnostics="off"))
    assert off.calls == plain.calls and "diagnostics" not in log
    assert not any(c[0] in ("reset_diagnostics", "mark", "diagnostics") for c in off.calls)
    assert all(c[2] == {} for c in off.calls if c[0] in ("sample", "burst"))
    assert set(of[0]) == set(pf[0]) and not any(k.startswith("diagnostics/") for k in of[0])
    for k in pf[1]:
        assert np.array_equal(of[1][k], pf[1][k]), k
    # with summaries on as well: the parent's sequence, reset_summary and summary included
    son, _, _ = _run(tmp_path, "son", dict(CFG, summaries="on", diagnostics="off"))
    ref = StubSampler()
    posts = [inf.Posterior(str(tmp_path / f"ref_{c}.npz"), ref.M, ref.T, 2, inf.warmup_size() + 8, summaries="on") for c in range(2)]
    inf.run_mcmc(ref, dict(CFG, summaries="on"), posts, log=open(os.devnull, "w"))
    assert son.calls == ref.calls


@pytest.mark.parametrize("nb,summaries,overlap", [(2, "off", True), (5, "on", True), (4, "only", True), (3, "off", False)])
def test_on_marks_the_halves_and_adds_the_group(tmp_path, nb, summaries, overlap):
    ns = 4
    cfg = dict(CFG, num_bursts=nb, num_burst_samples=ns, diagnostics="on", summaries=summaries)
    s, files, log = _run(tmp_path, f"on{nb}", cfg, cap=800 if overlap else ns)
    h = nb // 2
    seq = [c for c in s.calls if c[0] in ("reset_diagnostics", "mark", "diagnostics", "reset_summary", "burst")]
    want_marks = [("mark", 0, h * ns)] + ([("mark", 1, (nb - h) * ns)] if nb % 2 else [])
    assert [c for c in seq if c[0] == "mark"] == want_marks
    assert seq[0] == ("reset_diagnostics", ns) and seq[-1] == ("diagnostics",) and not any(c[0] == "reset_summary" for c in seq)
    if overlap:
        assert [c[0] for c in seq].count("burst") == nb
        assert all(c[2] == dict(events=summaries != "only", summarize=True) for c in seq if c[0] == "burst")
    warm = [c for c in s.calls if c[0] == "sample"][:8]
    assert all(c[2] == ({} if summaries == "off" else dict(events=summaries != "only", summarize="marginals")) for c in warm)
    # the files: today's datasets for this `summaries`, plus the group
    base, bf, _ = _run(tmp_path, f"base{nb}", dict(cfg, diagnostics="off"), cap=800 if overlap else ns)
    M, T, P, w = s.M, s.T, s.P, inf.warmup_size()
    for c, f in enumerate(files):
        assert set(f) == set(bf[c]) | {f"diagnostics/{k}" for k in dm.NAMES}
        for k in bf[c]:
            assert np.array_equal(f[k], bf[c][k], equal_nan=True), k
        d = {k: f[f"diagnostics/{k}"] for k in dm.NAMES}
        assert d["count"].reshape(-1)[0] == nb * ns and d["batch_length"].reshape(-1)[0] == ns and d["num_batches"].reshape(-1)[0] == nb
        assert np.array_equal(d["half_count"], [h * ns, h * ns])
        for k in ("seir", "state"):
            assert d[f"{k}_half_mean"].shape == d[f"{k}_half_var"].shape == (2, M, T, 3)
            assert d[f"{k}_ess"].shape == d[f"{k}_rhat"].shape == (M, T, 3)
        assert d["theta_half_mean"].shape == d["theta_half_var"].shape == (2, P) and d["theta_ess"].shape == d["theta_rhat"].shape == (P,)
        # the latent draws of the stub are the sweep's number: the halves are the first and last h bursts
        sweeps = w + np.arange(nb * ns)
        np.testing.assert_allclose(d["seir_half_mean"][0], sweeps[:h * ns].mean(), rtol=1e-14)
        np.testing.assert_allclose(d["state_half_mean"][1], sweeps[(nb - h) * ns:].mean(), rtol=1e-14)
        np.testing.assert_allclose(d["seir_half_var"][1], sweeps[(nb - h) * ns:].var(ddof=1), rtol=1e-12)
        # the parameters: this module's functions on the run's own draws, read back from samples/*
        theta = np.concatenate([np.stack([fc[f"samples/{k}"][w:] for k in dm.THETA_HEAD], axis=-1)
                                for fc in [f]], axis=0)
        acc = dm.DrawAccumulator(ns)
        acc.fold(theta[:h * ns, None])
        acc.mark(0)
        acc.fold(theta[h * ns:(nb - h) * ns, None])
        if nb % 2:
            acc.mark(1)
        acc.fold(theta[(nb - h) * ns:, None])
        np.testing.assert_allclose(d["theta_half_mean"][:, :6], acc.result().half_mean[:, 0], rtol=1e-13)
        np.testing.assert_allclose(d["theta_ess"][:6], acc.result().ess[0], rtol=1e-9)
    assert np.array_equal(files[0]["diagnostics/theta_rhat"], files[1]["diagnostics/theta_rhat"])    # over the process's chains
    assert "diagnostics: largest theta R-hat" in log and "smallest ESS" in log and f"batches of {ns}" in log


# ---- 7. the compiler's account of the new instances ---------------------------------------------------------------------
def test_the_diag_instances_have_no_scratch_and_the_others_are_the_parents():
    res = H.kernel_account("base")
    parent = json.load(open(os.path.join(ROOT, "profiles", "r07_kernel_resources.json")))
    for ev16 in (0, 1):
        r = res[f"k_summarize<{ev16},1>"]
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0, r
        assert r["lds_bytes_per_block"] == parent[f"k_summarize<{ev16}>"]["lds_bytes_per_block"]
        plain, was = res[f"k_summarize<{ev16},0>"], parent[f"k_summarize<{ev16}>"]
        for k in ("scratch_bytes_per_lane", "lds_bytes_per_block", "vgpr_spill", "sgpr_spill"):
            assert plain[k] == was[k], (ev16, k, plain, was)
        assert plain["vgpr"] <= was["vgpr"] + 4 and plain["occupancy_waves_per_simd"] >= was["occupancy_waves_per_simd"]
    assert res["k_summary_finish"]["scratch_bytes_per_lane"] == 0

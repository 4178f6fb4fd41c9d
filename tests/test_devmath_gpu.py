"""The scalar device functions (csrc/device_math.h), the delta log-ratios of the event updates (band_delta, the S->E piece of
own_rows_delta) and the wave / block primitives, each by itself on the GPU through the self-test hooks
(csrc/selftest_kernels.h), against mpmath on the grids and with the bounds of tests/devmath_lib.py; and the increments of the
sampler's running log-density per accepted event update against mpmath differences of the full density."""
import functools
import math

import numpy as np
import pytest

from tests import devmath_lib as D
from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as entry
    entry.build()
    from covid19uk_amd.seir import SeirModel
    case = H.build_case("micro_2x3", 13)
    with SeirModel(case["cov"], case["init"]) as m:
        yield m


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


LOG_FNS = ("fast_log", "fast_log_k", "mv_log", "fast_rcp")
SOFTPLUS_FNS = ("softplus_tab", "softplus_sigmoid_tab", "softplus")
LBINOM_FNS = ("lbinom_tab", "lbinom_const", "lbinom_bf")
L1ME_FNS = ("log1mexp_tab", "log1mexp", "log1mexp_series", "l1me_inv_series", "l1me_inv_k", "l1me_inv_series_k")


@functools.lru_cache(maxsize=None)
def _grid(name):
    """(x, y) of a function's grid; shared by the functions of a family, so is the reference"""
    if name in LOG_FNS:
        return D.cat(D.grid_log()), None
    if name in SOFTPLUS_FNS:
        return D.cat(D.grid_softplus()), None
    if name == "lfact_bf":
        return D.grid_lfact(), None
    if name in LBINOM_FNS:
        return D.grid_lbinom()
    if name in L1ME_FNS:
        return D.cat(D.grid_l1me()), None
    if name == "log1mexp_diff_slow":
        rows = np.concatenate(list(D.grid_band().values()))
        pairs = [(float(r0q) + float(aq), float(r0q)) for r0q, aq in map(D.band_exact, rows)]
        pairs = [p for p, row in zip(pairs, rows) if row[2] != 0 and D.band_parts(p[1], p[0] - p[1])[2] == "slow"]
        x = D.cat(D.grid_l1me())
        pairs += list(zip(x, x[::-1]))
        p = np.array(pairs)
        return p[:, 0].copy(), p[:, 1].copy()
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _reference(family):
    x, y = _grid(family)
    return D.reference(family, x, y)


def _values(model, name, x, y):
    out = model.selftest_fn(name, x, y)
    return out if isinstance(out, tuple) else (out,)


def _check_values(model, name, x, y, out):
    """the bounds of devmath_lib, function by function"""
    msg = []

    def hold(bound_name, got, refs, xs=x, ys=y):
        worst, at = D.worst_ratio(bound_name, got, refs, xs, ys)
        msg.append(f"{name}/{bound_name}: worst |err| / bound = {worst:.3f} at x = {float(xs[at])!r}")
        print(msg[-1])
        assert worst <= 1.0, msg[-1]

    if name in LOG_FNS[:3]:
        hold("fast_log", out[0], _reference("fast_log"))
        if name == "mv_log":
            assert (out[0][x == 1.0] == 0.0).all() and (x == 1.0).any()
        if name == "fast_log_k":
            assert np.array_equal(_bits(out[0]), _bits(model.selftest_fn("fast_log", x)))
    elif name == "fast_rcp":
        hold("fast_rcp", out[0], _reference("fast_rcp"))
    elif name in ("softplus_tab", "softplus"):
        hold(name, out[0], _reference("softplus_tab"))
    elif name == "softplus_sigmoid_tab":
        refs = _reference("softplus_sigmoid_tab")
        hold("softplus_tab", out[0], [r[0] for r in refs])
        hold("sigmoid", out[1], [r[1] for r in refs])
    elif name == "lfact_bf":
        hold("lfact_bf", out[0], _reference("lfact_bf"))
        assert np.array_equal(_bits(out[0]), _bits(model.selftest_math(x)[2]))            # lfact(n, tab): the same bits
    elif name in LBINOM_FNS:
        assert not np.isnan(out[0]).any()
        assert np.array_equal(np.isneginf(out[0]), (y < 0) | (y > x))
        hold(name, out[0], _reference("lbinom_tab"))
        if name == "lbinom_bf":
            assert np.array_equal(_bits(out[0]), _bits(model.selftest_fn("lbinom_tab", x, y)))
    elif name in ("log1mexp_tab", "log1mexp"):
        hold(name, out[0], _reference("log1mexp_tab"))
    elif name == "log1mexp_diff_slow":
        hold(name, out[0], _reference("log1mexp_diff_slow"))
    else:
        ins = np.array([D.in_series(float(v)) for v in x])
        refs = _reference("l1me_inv_series")
        if name == "log1mexp_series":
            assert np.array_equal(out[1], (~ins).astype(np.float64))                     # `odd` exactly outside the range
            hold("l1me_L", out[0][ins], [r[0] for r, i in zip(refs, ins) if i], x[ins])
        else:
            sel = ins if name != "l1me_inv_k" else x >= D.L1ME_SERIES_MIN
            hold("l1me_L", out[0][sel], [r[0] for r, i in zip(refs, sel) if i], x[sel])
            hold("l1me_inv", out[1][sel], [r[1] for r, i in zip(refs, sel) if i], x[sel])
            if name == "l1me_inv_series_k":
                ser = model.selftest_fn("l1me_inv_series", x[ins])
                assert np.array_equal(_bits(out[0][ins]), _bits(ser[0])) and np.array_equal(_bits(out[1][ins]), _bits(ser[1]))
            if name == "l1me_inv_k":
                # r < 0: never a finite value.  NaN where 1 - e^-r is a negative double; below 2^-54 in size e^-r rounds to
                # 1 and the libm branch's log(1 - e^-r) is log(0) = -inf (the accept tests reject both alike)
                neg = out[0][x < 0]
                assert (np.isnan(neg) | np.isneginf(neg)).all() and np.isnan(out[0][x <= -2.0 ** -52]).all() and (x < -0.5).any()
                nn = x >= 0                                                               # (l1me_inv's hook also takes lfact(floor x))
                L, inv, _ = model.selftest_math(x[nn])
                assert np.array_equal(_bits(out[0][nn]), _bits(L)) and np.array_equal(_bits(out[1][nn]), _bits(inv))


ALL_FNS = LOG_FNS + SOFTPLUS_FNS + ("lfact_bf",) + LBINOM_FNS + L1ME_FNS + ("log1mexp_diff_slow",)


@pytest.mark.parametrize("name", ALL_FNS)
def test_scalar_function_against_mpmath_on_its_grid(model, name):
    """Every element of the function's grid within the bound of devmath_lib's table; the same results bit for bit when the
    grid is permuted (no function depends on its neighbours in the wave) and in launches of 1, 255, 256 and 257 elements."""
    from covid19uk_amd import _lib
    assert set(ALL_FNS) == set(_lib.SELFTEST_FN)
    x, y = _grid(name)
    out = _values(model, name, x, y)
    _check_values(model, name, x, y, out)
    perm = np.random.default_rng(11).permutation(x.size)
    got = _values(model, name, x[perm], None if y is None else y[perm])
    for a, b in zip(out, got):
        assert np.array_equal(_bits(a)[perm], _bits(b)), name
    for n in (1, 255, 256, 257):
        got = _values(model, name, x[:n], None if y is None else y[:n])
        for a, b in zip(out, got):
            assert np.array_equal(_bits(a)[:n], _bits(b)), (name, n)


def test_self_test_hooks_refuse_arguments_outside_the_domains(model):
    from covid19uk_amd import _lib
    one = np.ones(4)

    def refused(fn, *a):
        with pytest.raises(_lib.SeirError) as e:
            fn(*a)
        assert e.value.code == _lib.ERR_INVALID

    for name in ("fast_log", "fast_log_k", "mv_log", "fast_rcp"):
        for bad in (0.0, -1.0, 5e-324, 2.0 ** -1030, np.inf, np.nan):
            refused(model.selftest_fn, name, np.array([1.0, bad]))
    for name in ("lfact_bf",) + LBINOM_FNS:
        for bad in (-1.0, 0.5, 2.0 ** 31, np.nan):
            refused(model.selftest_fn, name, np.array([3.0, bad]), one[:2])
    for name in LBINOM_FNS:
        refused(model.selftest_fn, name, np.array([3.0, 4.0]), np.array([0.5, 1.0]))
        refused(model.selftest_fn, name, np.array([3.0, 4.0]), np.array([np.inf, 1.0]))
        got = model.selftest_fn(name, np.array([3.0, 3.0, 3.0]), np.array([-1.0, 4.0, 3.0]))   # inside the domain
        assert np.isneginf(got[:2]).all() and got[2] == 0.0
    for name in SOFTPLUS_FNS + L1ME_FNS:
        refused(model.selftest_fn, name, np.array([1.0, np.nan]))
        refused(model.selftest_fn, name, np.array([np.inf]))
    refused(model.selftest_fn, "fast_log", np.empty(0))                                           # n < 1
    lib, ctx = model._lib, model._ctx
    assert lib.seir_selftest_fn(ctx, 99, 4, one.ctypes.data_as(_lib.c_double_p), None, one.ctypes.data_as(_lib.c_double_p), None) \
        == _lib.ERR_INVALID
    assert lib.seir_selftest_fn(ctx, _lib.SELFTEST_FN["lbinom_bf"][0], 4, one.ctypes.data_as(_lib.c_double_p), None,
                                one.ctypes.data_as(_lib.c_double_p), None) == _lib.ERR_INVALID
    cols = [one] * 7
    refused(model.selftest_delta, "band", *(cols[:3] + [np.array([1.0, np.nan, 1.0, 1.0])] + cols[4:]), 0.0, 1.0)
    refused(model.selftest_delta, "band", *cols, np.inf, 1.0)
    refused(model.selftest_delta, "own_ei", *[np.empty(0)] * 7, 0.0, 1.0)
    assert lib.seir_selftest_band_delta(ctx, 3, 4, *[one.ctypes.data_as(_lib.c_double_p)] * 7, 0.0, 1.0,
                                        one.ctypes.data_as(_lib.c_double_p)) == _lib.ERR_INVALID
    p = one.ctypes.data
    assert lib.seir_selftest_wave(ctx, 7, 0, 1, p, p, p) == _lib.ERR_INVALID
    assert lib.seir_selftest_wave(ctx, _lib.SELFTEST_WAVE["wave_min"][0], 1, 1, p, p, p) == _lib.ERR_INVALID   # no int32 form
    assert lib.seir_selftest_wave(ctx, 0, 0, 0, p, p, p) == _lib.ERR_INVALID
    assert lib.seir_selftest_wave(ctx, 0, 0, 1025, p, p, p) == _lib.ERR_INVALID
    with pytest.raises(ValueError):
        model.selftest_wave("wave_sum", np.ones(100))


# ---- the delta log-ratios ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _delta_case(which):
    rows = D.own_se_rows() if which == "own_se" else np.concatenate(list(D.grid_band().values()))
    if which == "own_se":
        refs = [D.own_se_reference(r) for r in rows]
    else:
        refs = [D.delta_reference(which, r) for r in rows]
    return rows, refs


def _delta(model, which, rows):
    return model.selftest_delta(which, *[rows[:, c].copy() for c in range(7)], 0.0, D.DT)


@pytest.mark.parametrize("which", ["band", "own_ei", "own_se"])
def test_delta_log_ratio_against_mpmath(model, which):
    """band_delta on every branch (series, |z| switch, slow, K0 = 0) and the S->E piece of own_rows_delta, per cell, within
    the bounds of devmath_lib; the E->I-type piece against exact r0 + a and against the rates as it is handed them."""
    rows, refs = _delta_case(which)
    got = _delta(model, which, rows)
    worst = {}
    for j, (g, (ref, b, branch)) in enumerate(zip(got, refs)):
        if which == "own_ei" and not D.own_ei_exact_applies(rows[j]):
            continue
        q = D.err_ratio(g, ref, b)
        if q > worst.get(branch, (0.0, -1))[0]:
            worst[branch] = (q, j)
    if which == "own_ei":
        for j, g in enumerate(got):
            ref, b, branch = D.delta_reference("own_ei_formed", rows[j])
            q = D.err_ratio(g, ref, b)
            if q > worst.get(branch + "/formed", (0.0, -1))[0]:
                worst[branch + "/formed"] = (q, j)
    print(which, {k: (round(q, 3), rows[j].tolist()) for k, (q, j) in worst.items()})
    assert all(q <= 1.0 for q, _ in worst.values()), worst
    perm = np.random.default_rng(12).permutation(len(rows))
    assert np.array_equal(_bits(got)[perm], _bits(_delta(model, which, rows[perm])))
    for n in (1, 255, 256, 257):
        assert np.array_equal(_bits(got)[:n], _bits(_delta(model, which, rows[:n]))), n


# ---- wave and block primitives ----------------------------------------------------------------------------------------------
WAVE_FORMS = [("wave_sum", np.float64), ("wave_sum", np.int32), ("wave_min", np.float64), ("wave_incl_scan", np.float64),
              ("wave_incl_scan", np.int32), ("wave_incl_suffix_scan", np.float64), ("block_excl_scan_256", np.float64),
              ("block_excl_scan_256", np.int32), ("block_incl_suffix_scan_256", np.float64), ("block_sum_256", np.float64)]


@pytest.mark.parametrize("name,dtype", WAVE_FORMS, ids=[f"{n}-{np.dtype(t).name}" for n, t in WAVE_FORMS])
def test_wave_and_block_primitives_on_exact_integer_inputs(model, name, dtype):
    """4 blocks (16 waves with different data) per input; integer-valued, so every sum is exact whatever its order: a single
    1 at each of the 64 lane positions and each of the 256 thread positions (names a missed lane or row), all ones, random
    integers of either sign below 2^20.  wave_sum hands the same value to all 64 lanes, block_* the right total to every
    thread."""
    from covid19uk_amd import _lib
    assert {n for n, _ in WAVE_FORMS} == set(_lib.SELFTEST_WAVE)
    inputs = D.wave_inputs(dtype)
    ids = list(inputs)
    for lo in range(0, len(ids), 256):                       # 256 inputs of 4 blocks per launch
        part = ids[lo:lo + 256]
        v = np.concatenate([inputs[i] for i in part])
        out, tot = model.selftest_wave(name, v)
        want, wtot = D.wave_expected(name, v)
        assert out.dtype == dtype and tot.dtype == dtype
        for j, i in enumerate(part):
            s = slice(j * 1024, (j + 1) * 1024)
            assert np.array_equal(out[s], want[s].astype(dtype)), (name, i, np.flatnonzero(out[s] != want[s])[:8])
            assert np.array_equal(tot[s], wtot[s].astype(dtype)), (name, i)


@pytest.mark.parametrize("name", [n for n, t in WAVE_FORMS if t is np.float64])
def test_wave_and_block_primitives_on_non_integer_doubles(model, name):
    """Against math.fsum within 8 eps sum|v| of the wave (7 additions deep), the block forms 3 more; wave_min exactly."""
    v = np.random.default_rng(13).normal(size=1024) * np.exp(np.random.default_rng(14).uniform(-3, 3, 1024))
    out, tot = model.selftest_wave(name, v)
    per = 64 if name.startswith("wave") else 256
    depth = 8 if per == 64 else 11
    for g in range(1024 // per):
        w = v[g * per:(g + 1) * per]
        tol = depth * D.EPS * math.fsum(abs(w))
        o = out[g * per:(g + 1) * per]
        for t in range(per):
            if name == "wave_min":
                want, tol_t = w.min(), 0.0
            elif name in ("wave_sum", "block_sum_256"):
                want, tol_t = math.fsum(w), tol
            elif name == "wave_incl_scan":
                want, tol_t = math.fsum(w[:t + 1]), tol
            elif name == "block_excl_scan_256":
                want, tol_t = math.fsum(w[:t]), tol
            else:
                want, tol_t = math.fsum(w[t:]), tol
            assert abs(o[t] - want) <= tol_t, (name, g, t, o[t], want)
        if name in ("block_excl_scan_256", "block_incl_suffix_scan_256"):
            assert (np.abs(tot[g * per:(g + 1) * per] - math.fsum(w)) <= tol).all()
        if name == "wave_sum":
            assert (o == o[0]).all()


# ---- the sampler's increments of the running log-density ----------------------------------------------------------------------
INC_CFG = dict(dmax=8, nmax=6, m=2, occult_nmax=5, num_event_time_updates=1)      # test_sampler_gpu.CFG_SMALL, one scan
INC_KEYS = ("move/S->E", "move/E->I", "occult/S->E", "occult/E->I")
INC_B, INC_SEED = 2, 77
INC_SWEEPS = {"micro_5x24": 30, "micro_17x70": 20}      # the mpmath reference of the larger case costs ~0.15 s per sweep and chain


@functools.lru_cache(maxsize=None)
def _increment_reference(name, seed):
    """The oracle chains replayed (same seed, HMC disabled: u stays the start value), and for every ACCEPTED update the
    mpmath difference of the full log-densities over the cells whose term changed, with the scale A of its tolerance."""
    import mpmath as mp
    from covid19uk_amd import synth
    from oracle import mcmc_oracle as mo
    from oracle import seir_oracle as so
    case = H.build_case(name, seed, alpha_t_sd=0.005)
    k = case["k"]
    u = synth.jitter_params(case["u"], INC_B, scale=0.05, seed=seed, T=k.T)
    ev0 = np.stack([case["events"]] * INC_B)
    decisions, refs = {}, {}
    n_sweeps = INC_SWEEPS[name]
    for b in range(INC_B):
        ch = mo.OracleChain(k, INC_CFG, u[b], ev0[b], seed=INC_SEED, chain_id=5 + b, disable=("hmc",))
        cur, cache = ev0[b].copy(), {}
        for i in range(n_sweeps):
            o = ch.sweep_once()
            for key in INC_KEYS:
                acc = bool(o[key]["is_accepted"])
                decisions[(i, b, key)] = acc
                if not acc:
                    continue
                new = o[key]["proposed_events"]
                cells = so.changed_cells(cur, new, k)
                old_t = so.likelihood_cells_mp(u[b], cur, k, cells, cache=cache)
                new_t = so.likelihood_cells_mp(u[b], new, k, cells, cache=cache)
                with mp.workdps(50):
                    moved = [c for c in cells if old_t[c][0] != new_t[c][0]]
                    inc = sum((new_t[c][0] - old_t[c][0] for c in moved), mp.mpf(0))
                    A = float(sum((new_t[c][1] + old_t[c][1] for c in moved), mp.mpf(0)))
                refs[(i, b, key)] = (inc, A)
                cur = new
            assert np.array_equal(cur, o["events"])
    return case, u, ev0, decisions, refs


@pytest.mark.parametrize("moves", ["default", "split"])
@pytest.mark.parametrize("name,seed", [("micro_5x24", 1), ("micro_17x70", 3)])
def test_accepted_updates_move_the_running_log_density_by_the_mpmath_difference(name, seed, moves):
    """For every accepted event update of 20 to 30 sweeps of 2 chains (HMC disabled, one scan of the four updates per sweep),
    the increment of the traced target_log_prob -- this update's value minus the previous update's -- equals the mpmath
    difference of the full log-densities at the fixed u, within 2e-15 A + 4 ulp(|lp|): A sums, over the cells whose term
    changed and both states, the absolute values of each log-factorial, each k L and each (n - k) r (2e-15 is the
    project's per-function bound); the second term covers the two roundings of the running sum.  A rejected update
    leaves the running value as it was, bit for bit; its log-ratio is seen by no trace, so the delta log-ratios of
    rejected proposals are pinned only through the scalar hooks above."""
    import mpmath as mp
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as entry
    entry.build()
    from covid19uk_amd.sampler import ChainSampler
    from covid19uk_amd.seir import SeirModel
    case, u, ev0, decisions, refs = _increment_reference(name, seed)
    per_kind = {key: sum(1 for (i, b, kk) in refs if kk == key) for key in INC_KEYS}
    assert min(per_kind.values()) >= 10, per_kind
    form = {} if moves == "default" else dict(moves=moves)
    with SeirModel(case["cov"], case["init"], max_chains=INC_B) as model:
        with ChainSampler(model, INC_CFG, INC_B, seed=INC_SEED, first_chain_id=5, trace_capacity=INC_SWEEPS[name],
                          disable=("hmc",), **form) as s:
            s.set_state(u, ev0)
            tr = s.sample(INC_SWEEPS[name])
    compared, worst = 0, (0.0, None)
    for i in range(INC_SWEEPS[name]):
        for b in range(INC_B):
            prev = float(tr.hmc["target_log_prob"][i, b])
            for key in INC_KEYS:
                cur = float(tr.moves[key]["target_log_prob"][i, b])
                acc = bool(tr.moves[key]["is_accepted"][i, b])
                assert acc == decisions[(i, b, key)], (i, b, key)
                if not acc:
                    assert cur == prev, (i, b, key)
                    assert (i, b, key) not in refs
                else:
                    inc, A = refs[(i, b, key)]
                    tol = 2e-15 * A + 4 * D.ulp(max(abs(cur), abs(prev)))
                    with mp.workdps(50):
                        err = float(abs((mp.mpf(cur) - mp.mpf(prev)) - inc))
                    compared += 1
                    if err / tol > worst[0]:
                        worst = (err / tol, (i, b, key, cur - prev, float(inc), A))
                    assert err <= tol, (i, b, key, cur - prev, float(inc), err, tol)
                prev = cur
    print(f"{name} {moves}: {compared} accepted updates {per_kind}, worst err / tol = {worst[0]:.3f} at {worst[1]}")
    assert compared == len(refs)

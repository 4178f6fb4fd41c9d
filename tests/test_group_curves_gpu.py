"""Group curves on the device (include/seir_hip.h, "Group curves on the device"; covid19uk_amd/csrc/group_curve_kernels.h):
R_t and the within / between pressures of every kept draw per group of locations.

A group sum of fp64 values has ONE order (the kernel file's header; `posterior.groups.weighted_sum_rows` restates it in
NumPy), so every comparison of a device sum is `np.array_equal`:

  - the kernel alone (`SeirModel.group_wsums`) against the NumPy definition on mixed-sign data of widely differing
    magnitudes, where another order gives other bits;
  - group R_t through the sampler against the definition applied to the stateless `SeirModel.reproduction_number` (k_rt) on
    the same run's recorded draws;
  - group within / between against the definition applied to wi, be restated cell by cell with an exact fma
    (tests/devmath_lib.py); the restatement itself is held, bit for bit, to the fractions of the stateless
    `SeirModel.within_between` (k_within_between) per (draw, day).

Two bounds are derived, not measured.  (1) The all-locations group with the national weights against samples/R_t for
M > 64: both are sums of the same non-negative terms r * w, each rounded once, in two different orders.  The group order
makes at most ceil(M / 64) adds per lane and 6 in the butterfly, the national order 6 in the butterfly and ceil(M / 64) - 1
over the column blocks: each is within (ceil(M / 64) + 6) 2^-53 (sum of terms) of the exact sum to first order, so they
are within 2 (ceil(M / 64) + 6) 2^-53 (sum of terms) of each other.  (2) none other: everything else is equality."""
import math
import os

import numpy as np
import pytest

from covid19uk_amd import _lib, synth
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.posterior import groups as G
from tests import devmath_lib as DM
from tests import helpers as H
from tests import test_wb_gpu as WB
from tests.test_groups_gpu import _csr, _groups_for, _set
from tests.test_recovery_gpu import _case, _same_bits
from tests.test_rt_device_gpu import _reference as _rit, _same_run as _same_rt_run, _weight
from tests.test_sampler_gpu import CFG_REF, CFG_SMALL, api  # noqa: F401  (fixture)
from tests.test_summary_gpu import _cli, _datasets, _sampler

pytestmark = pytest.mark.gpu

NDMAX = 1024                  # GRP_NDMAX: draws per launch (group_kernels.h)


def _table(groups):
    off, mem = _csr(groups)
    return G.GroupTable([str(i) for i in range(len(groups))], off, mem)


def _mixed(rng, shape):
    """Mixed signs, magnitudes over 16 decades: another order of the adds gives other bits."""
    return rng.standard_normal(shape) * 10.0 ** rng.integers(-8, 9, size=shape)


def _want(tab, v, w=None):
    """v [nd, L, M] -> [nd, G, L] by the NumPy definition."""
    return np.moveaxis(G.weighted_sum_rows(tab, v, w, axis=-1), -1, 1)


@pytest.fixture(scope="module")
def model(api):
    case = H.build_case("micro_3x1", 43)
    with api[0](case["cov"], case["init"], max_chains=1) as m:
        yield m


# ---------------------------------------------------------------------------------------------------------------------
# the kernel alone
# ---------------------------------------------------------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 129)


@pytest.mark.parametrize("L", [1, 63, 64, 65])
def test_group_wsums_equal_the_definition_at_every_group_size_and_day_extent(model, L):
    """Members per group 1, 63, 64, 65, 129 (one lane, one short of / exactly / one past a wave, a third round), groups that
    overlap, the last row alone; weighted and unweighted; L on both sides of the kernel's day tile and of 64."""
    M, nd = 200, 3
    rng = np.random.default_rng([L, 1])
    groups = [sorted(rng.choice(M, size=n, replace=False)) for n in SIZES] + [[M - 1], list(range(M))]
    tab = _table(groups)
    v = _mixed(rng, (nd, L, M))
    w = _mixed(rng, tab.members.shape)
    for weights in (None, w):
        got = model.group_wsums(v, tab.offsets, tab.members, weights)
        assert got.dtype == np.float64 and got.shape == (nd, len(groups), L)
        assert np.array_equal(got, _want(tab, v, weights))
    # the data does tell orders apart: a plain ascending sum of the same terms differs somewhere
    plain = np.stack([v[..., np.asarray(g)].sum(axis=-1) for g in groups], axis=1)
    assert not np.array_equal(plain, _want(tab, v))


@pytest.mark.parametrize("M", [1, 9, 65])
def test_singletons_return_the_input_bits_and_one_group_holds(model, M):
    rng = np.random.default_rng(M)
    v = _mixed(rng, (2, 5, M))
    v[0, 0, 0] = -0.0                                          # +0.0 + -0.0 = +0.0: the one value a singleton does not return
    tab = _table([[m] for m in range(M)])
    got = model.group_wsums(v, tab.offsets, tab.members, np.ones(M))
    want = np.moveaxis(v, -1, 1)
    assert np.array_equal(got, want) and np.array_equal(got, model.group_wsums(v, tab.offsets, tab.members))
    assert np.array_equal(np.signbit(got), np.signbit(want) & (want != 0.0))
    one = _table([list(range(M))])                             # G = 1
    assert np.array_equal(model.group_wsums(v, one.offsets, one.members), _want(one, v))


def test_256_groups(model):
    M = 300
    rng = np.random.default_rng(11)
    groups = [sorted(rng.choice(M, size=int(rng.integers(1, 140)), replace=False)) for _ in range(_lib.GROUPS_MAX)]
    tab = _table(groups)
    v, w = _mixed(rng, (2, 6, M)), _mixed(rng, tab.members.shape)
    assert np.array_equal(model.group_wsums(v, tab.offsets, tab.members, w), _want(tab, v, w))


def test_one_draw_and_one_past_a_launchs_draw_cut(model):
    rng = np.random.default_rng(13)
    tab = _table([[0, 2], [1], [0, 1, 2, 3]])
    for nd in (1, NDMAX + 1):
        v = _mixed(rng, (nd, 5, 4))
        assert np.array_equal(model.group_wsums(v, tab.offsets, tab.members), _want(tab, v)), nd


def test_group_wsums_do_not_depend_on_workgroup_timing(api):
    case = H.build_case("micro_3x1", 43)
    rng = np.random.default_rng(3)
    tab = _table([list(range(130)), list(range(0, 130, 2)), [129]])
    v, w = _mixed(rng, (5, 7, 130)), _mixed(rng, tab.members.shape)
    for skew in (1, 2, 3):
        with api[0](case["cov"], case["init"], max_chains=1) as m:
            m.set_option(debug_skew=skew)
            assert np.array_equal(m.group_wsums(v, tab.offsets, tab.members, w), _want(tab, v, w)), skew


def test_group_wsums_refusals(model):
    v = np.zeros((2, 3, 4))

    def refused(off, mem, word):
        with pytest.raises(_lib.SeirError) as e:
            model.group_wsums(v, np.asarray(off, np.int32), np.asarray(mem, np.int32))
        assert e.value.code == _lib.ERR_INVALID and word in str(e.value), str(e.value)

    refused([0, 0], [0], "empty")
    refused([0, 2, 1], [0, 1], "decrease")
    refused([0, 1], [4], "outside")
    refused([0, 2], [1, 0], "ascending")
    refused([1, 2], [0, 1], "starts at 0")
    refused(list(range(_lib.GROUPS_MAX + 2)), [0] * (_lib.GROUPS_MAX + 1), "G=")
    refused([0], [0], "G=")
    with pytest.raises(ValueError, match="aligned"):
        model.group_wsums(v, [0, 2], [0, 1], np.ones(3))
    with pytest.raises(ValueError, match="nd, L, M"):
        model.group_wsums(v[0], [0, 1], [0])
    assert model._lib.seir_group_wsums(model._ctx, None, 1, 3, 4, 1, None, None, None, None) == _lib.ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------------
# group R_t through the sampler
# ---------------------------------------------------------------------------------------------------------------------
def _rt_groups(M):
    """The all-locations group first, then every location alone (up to 40), then the overlapping groups of _groups_for."""
    return _groups_for(M)


def _rt_weights(case, groups):
    """(table, weights): the national weights on the all-locations group, 1.0 on the singletons, the population weights of
    `posterior.groups.rt_weights` on the rest."""
    tab = _table(groups)
    N = np.asarray(case["cov"].N, np.float64).reshape(-1)
    w = G.rt_weights(tab, N)
    w[:len(groups[0])] = _weight(case)
    k = min(len(N), 40)
    w[len(groups[0]):len(groups[0]) + k] = 1.0
    return tab, w


def _want_rg(tab, w, R):
    """R [n,B,D,M] -> [n,B,G,D] by the definition."""
    return np.moveaxis(G.weighted_sum_rows(tab, R, w, axis=-1), -1, 2)


RT_CASES = {
    # name, B, record, n, D
    "M=1,D=5,u16,B=3": ("micro_1x70", 3, "u16", 5, 5),
    "M=9,D=4,u16,B=3": ("micro_9x64", 3, "u16", 5, 4),
    "M=65,D=3,u16,B=1": ("micro_65x70", 1, "u16", 5, 3),
    "M=130,D=T=8,int32,B=1": ("micro_130x8", 1, True, 1, 8),
    "M=3,T=1,D=1,int32,B=3": ("micro_3x1", 3, True, 5, 1),
}


@pytest.mark.parametrize("case_id", list(RT_CASES))
def test_group_rt_equals_the_definition_on_the_stateless_kernels_r_it(api, case_id):
    name, B, record, n, D = RT_CASES[case_id]
    case, u, ev, cfg, eps = _case(name, B)
    if name == "micro_65x70":
        eps = 0.0001
    M = case["k"].M
    groups = _rt_groups(M)
    tab, w = _rt_weights(case, groups)
    wn = _weight(case)
    model, s = _sampler(api, case, cfg, u, ev, eps, n, record_events=record)
    with model, s:
        s.reset_rt(D, wn)
        tr0 = s.sample(n, rt=True)                             # the feature off: the parent's launches
        off = (s.rt_summary(), tr0.rt.copy())
        assert tr0.group_curves is None
    model, s = _sampler(api, case, cfg, u, ev, eps, n, record_events=record)
    with model, s:
        _set(s, groups)
        s.set_group_rt(w)
        s.reset_rt(D, wn)
        tr = s.sample(n, rt=True)                              # k_rt_trace_cells
        _same_bits(tr, tr0)
        assert tr.events.dtype == (np.uint16 if record == "u16" else np.int32)
        rg = tr.group_curves["rt_by_group"]
        assert set(tr.group_curves) == {"rt_by_group"} and rg.dtype == np.float64 and rg.shape == (n, B, len(groups), D)
        R = _rit(api, case, tr.theta, tr.events, D)
        assert np.all(np.isfinite(R)) and R.min() >= 0.0
        assert np.array_equal(rg, _want_rg(tab, w, R))
        k = min(M, 40)
        assert np.array_equal(rg[:, :, 1:1 + k], np.moveaxis(R[..., :k], -1, 2))     # singletons, weight 1.0: R_it's bits
        if M <= 64:
            assert np.array_equal(rg[:, :, 0], tr.rt)          # one wave: the national order is the group's
        else:
            terms = (R * wn).sum(-1)
            bound = 2 * (math.ceil(M / 64) + 6) * 2.0 ** -53 * terms
            assert np.all(np.abs(rg[:, :, 0] - tr.rt) <= bound)
        # everything k_rt_trace produced is what it was
        _same_rt_run((s.rt_summary(), tr.rt), off)
        assert np.array_equal(s.read_group_rt(2 if n > 1 else 1, first=n - (2 if n > 1 else 1)), rg[n - (2 if n > 1 else 1):])
        # the draw store on: k_rt_trace_keep plus the gather -- the same bits, and the order statistics are the store's
        s.reset_rt(D, wn)
        s.keep_rt_draws(n + 1)
        s.rt(0, n)
        assert np.array_equal(s.read_group_rt(n), rg)
        _same_rt_run((s.rt_summary(), s.read_rt_draws(n)), off)
        ranks = sorted({0, n - 1})
        assert np.array_equal(s.rt_order_stats(ranks), np.sort(R, axis=0)[ranks])
        s.keep_rt_draws(0)
        # another window sizes again
        D2 = 1 if D > 1 else case["k"].T
        if D2 != D:
            s.reset_rt(D2, wn)
            s.rt(0, n)
            assert np.array_equal(s.read_group_rt(n), _want_rg(tab, w, R[:, :, D - D2:]))
        assert not s.pair_timeouts().any()


# ---------------------------------------------------------------------------------------------------------------------
# group within / between through the sampler
# ---------------------------------------------------------------------------------------------------------------------
def _wb_cells(case, theta, I, draws, days, chains=None):
    """wi, be and the fractions of the (draw, chain, day) cells asked for, restated operation for operation (wb_kernels.h:
    wb_x, wb_row, wb_cell) with the exact fma of tests/devmath_lib.py.  I [n,B,D,M]; returns {(j, b, tw): (wi, be, fw, fb)},
    each [M]."""
    k = case["k"]
    M, T = k.M, k.T
    D = I.shape[2]
    Cs = np.asarray(k.Cstar, np.float64)
    invN = np.array([float(1.0 / v) for v in np.asarray(k.N, np.float64)])
    W = np.asarray(case["cov"].W, np.float64).reshape(-1)
    out = {}
    for j in draws:
        for b in (range(I.shape[1]) if chains is None else chains):
            for tw in days:
                pw = float(theta[j, b, 0]) * float(W[T - D + tw])
                x = [float(I[j, b, tw, i]) * float(invN[i]) for i in range(M)]
                wi, be, fw, fb = (np.empty(M) for _ in range(4))
                for m in range(M):
                    F = [0.0, 0.0, 0.0, 0.0]
                    for i in range(M):
                        F[i & 3] = DM.fma(0.0 if i == m else float(Cs[i, m]), x[i], F[i & 3])
                    self_ = float(Cs[m, m]) * x[m]
                    wi[m] = DM.fma(pw, self_, float(I[j, b, tw, m]))
                    Fs = (F[0] + F[1]) + (F[2] + F[3])
                    be[m] = pw * Fs
                    tot = DM.fma(pw, Fs, float(wi[m]))
                    with np.errstate(divide="ignore", invalid="ignore"):
                        fw[m], fb[m] = np.float64(wi[m]) / np.float64(tot), np.float64(be[m]) / np.float64(tot)
                out[(j, b, tw)] = (wi, be, fw, fb)
    return out


def _check_wb(api, case, tab, tr, gc, D, draws, days, chains=None):
    """The group pressures of the cells asked for against the definition on the restated wi, be; the restatement against the
    stateless kernel's fractions, every bit."""
    fw, fb, I = WB._reference(api, case, tr.theta, tr.events, D)
    cells = _wb_cells(case, tr.theta, I, draws, days, chains)
    for (j, b, tw), (wi, be, rw, rb) in cells.items():
        assert np.array_equal(rw, fw[j, b, tw], equal_nan=True) and np.array_equal(rb, fb[j, b, tw], equal_nan=True), (j, b, tw)
        assert np.array_equal(gc["within_by_group"][j, b, :, tw], G.weighted_sum_rows(tab, wi)), (j, b, tw)
        assert np.array_equal(gc["between_by_group"][j, b, :, tw], G.weighted_sum_rows(tab, be)), (j, b, tw)
    return fw, fb, I


WB_CASES = {
    # name, B, record, n, D, draws and days restated (None: all)
    "M=1,D=5,u16,B=3": ("micro_1x70", 3, "u16", 5, 5, None, None),
    "M=9,D=4,u16,B=3": ("micro_9x64", 3, "u16", 5, 4, None, None),
    "M=65,D=3,u16,B=1": ("micro_65x70", 1, "u16", 5, 3, (0, 4), (0, 2)),
    "M=130,D=T=8,int32,B=1": ("micro_130x8", 1, True, 1, 8, (0,), (0, 7)),
    "M=3,T=1,D=1,int32,B=3": ("micro_3x1", 3, True, 5, 1, None, None),
}


@pytest.mark.parametrize("case_id", list(WB_CASES))
def test_group_wb_equals_the_definition_on_the_restated_cells(api, case_id):
    name, B, record, n, D, draws, days = WB_CASES[case_id]
    case, u, ev, cfg, eps = _case(name, B)
    if name == "micro_65x70":
        eps = 0.0001
    M = case["k"].M
    groups = _groups_for(M)
    tab = _table(groups)
    model, s = _sampler(api, case, cfg, u, ev, eps, n, record_events=record)
    with model, s:
        s.reset_within_between(D)
        tr0 = s.sample(n, within_between=True)                 # the feature off: the parent's launches
        off = (s.within_between_summary(), {k: v.copy() for k, v in tr0.wb.items()})
        assert tr0.group_curves is None
    model, s = _sampler(api, case, cfg, u, ev, eps, n, record_events=record)
    with model, s:
        _set(s, groups)
        s.set_group_within_between(True)
        s.reset_within_between(D)
        tr = s.sample(n, within_between=True)
        _same_bits(tr, tr0)
        gc = tr.group_curves
        assert set(gc) == {"within_by_group", "between_by_group"}
        assert all(v.dtype == np.float64 and v.shape == (n, B, len(groups), D) for v in gc.values())
        _check_wb(api, case, tab, tr, gc, D, range(n) if draws is None else draws, range(D) if days is None else days)
        if M <= 64:                                            # one wave: the national order is the group's
            assert np.array_equal(gc["within_by_group"][:, :, 0], tr.wb["within_pressure"])
            assert np.array_equal(gc["between_by_group"][:, :, 0], tr.wb["between_pressure"])
        # everything k_wb_trace produced is what it was
        WB._same_run((s.within_between_summary(), tr.wb), off)
        back = s.read_group_wb(1, first=n - 1)
        assert all(np.array_equal(back[k], gc[k][n - 1:]) for k in gc)
        assert not s.pair_timeouts().any()


def test_group_wb_where_nobody_is_infectious(api):
    """WB._flicker_case: one location, nobody infectious on some days -- wi = be = 0, the shares are 0 / 0 and the draw is
    undefined for the cell; its zeros enter the group sums as they enter the national ones, and the host leaves
    Wg + Bg == 0 out of the share."""
    case = WB._flicker_case()
    B, n, D = 3, 8, case["k"].T
    u = synth.jitter_params(case["u"], B, scale=0.01, seed=3, T=case["k"].T)
    ev = np.stack([case["events"]] * B)
    tab = _table([[0]])
    model, s = _sampler(api, case, CFG_SMALL, u, ev, WB.FLICKER["eps"], n, seed=WB.FLICKER["seed"])
    with model, s:
        _set(s, [[0]])
        s.set_group_within_between(True)
        s.reset_within_between(D)
        tr = s.sample(n, within_between=True)
        ws = s.within_between_summary()
        gc = tr.group_curves
        assert np.array_equal(gc["within_by_group"][:, :, 0], tr.wb["within_pressure"])
        assert np.array_equal(gc["between_by_group"][:, :, 0], tr.wb["between_pressure"])
        tot = gc["within_by_group"] + gc["between_by_group"]
        assert (tot == 0.0).any() and (tot != 0.0).any()
        for b in range(B):                                     # M = 1: the group's defined draws are the cell's
            defined, share, _ = G.share_stats(gc["within_by_group"][:, b], gc["between_by_group"][:, b])
            assert np.array_equal(defined[0], ws.defined[b, :, 0])
            assert np.all(share[0][defined[0] > 0] == 1.0) and np.all(np.isnan(share[0][defined[0] == 0]))
        _check_wb(api, case, tab, tr, gc, D, range(n), range(D))


# ---------------------------------------------------------------------------------------------------------------------
# invariance and interplay
# ---------------------------------------------------------------------------------------------------------------------
def _both_on(s, case, groups, D, keep=0):
    tab, w = _rt_weights(case, groups)
    _set(s, groups)
    s.set_group_rt(w)
    s.set_group_within_between(True)
    s.reset_rt(D, _weight(case))
    if keep:
        s.keep_rt_draws(keep)
    s.reset_within_between(D)
    return tab, w


def _curves(s, n, first=0):
    return dict(rt_by_group=s.read_group_rt(n, first), **s.read_group_wb(n, first))


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("keep", [False, True])
def test_cutting_a_burst_into_calls_halves_or_batches_does_not_matter(api, keep):
    """Two bursts in the two halves of the buffer, then the same slots in ragged calls, then with a staging bound of 1 KiB
    (one slot per batch) and of 100 KiB (8 slots of the integer plane alone, 2 with the cell planes: the batch shrinks): the
    same bits."""
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    n, D = 11, 9
    groups = _groups_for(20)
    res = {}
    for kib in (0, 1, 100):
        model, s = _sampler(api, case, cfg, u, ev, eps, 2 * n)
        with model, s:
            if kib:
                model.set_option(rt_staging_kib=kib)
            tab, w = _both_on(s, case, groups, D, keep=2 * n if keep else 0)
            for first in (0, n):
                s.reset_trace(at=first)
                s.run(n)
                s.rt(first, n)
                s.within_between(first, n)
            tr = s.read_trace(2 * n)
            res[kib] = (_curves(s, 2 * n), s.rt_summary(), s.read_rt_draws(2 * n), tr)
            if not kib:
                assert np.array_equal(res[0][0]["rt_by_group"], _want_rg(tab, w, _rit(api, case, tr.theta, tr.events, D)))
                s.reset_rt(D, _weight(case))
                if keep:
                    s.keep_rt_draws(2 * n)
                s.reset_within_between(D)
                for first, count in ((0, 3), (3, 1), (4, 9), (13, 2 * n - 13)):
                    s.rt(first, count)
                    s.within_between(first, count)
                _same(_curves(s, 2 * n), res[0][0])
                _same_rt_run((s.rt_summary(), s.read_rt_draws(2 * n)), res[0][1:3])
    for kib in (1, 100):
        _same_bits(res[0][3], res[kib][3])
        _same(res[kib][0], res[0][0])
        _same_rt_run(res[kib][1:3], res[0][1:3])


@pytest.mark.parametrize("skew", [1, 2, 3])
def test_curves_do_not_depend_on_workgroup_timing_and_repeat(api, skew):
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    n, D = 6, 7
    groups = _groups_for(20)
    res = {}
    for tag, sk in (("a", 0), ("b", 0), ("skew", skew)):
        if tag == "b" and skew != 1:
            continue                                           # the repeat of the plain run is checked once
        model, s = _sampler(api, case, cfg, u, ev, eps, n, skew=sk, record_events="u16")
        with model, s:
            _both_on(s, case, groups, D)
            tr = s.sample(n, rt=True, within_between=True)
            res[tag] = (tr.group_curves, tr.events)
    assert res["a"][0]["rt_by_group"].any() and res["a"][0]["between_by_group"].any()
    for tag in res:
        assert np.array_equal(res["a"][1], res[tag][1])
        _same(res[tag][0], res["a"][0])


def test_chains_keep_their_curves_however_they_are_sharded_and_thinning_keeps_the_kept_draws(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 4)
    n, D, k = 6, 5, 3
    groups = _groups_for(20)
    got = []
    for sl, kw in ((slice(None), {}), (slice(2, None), dict(first_chain_id=2))):
        model, s = _sampler(api, case, cfg, u[sl], ev[sl], eps, n, **kw)
        with model, s:
            _both_on(s, case, groups, D)
            got.append(s.sample(n, rt=True, within_between=True).group_curves)
    _same({k_: v[:, 2:] for k_, v in got[0].items()}, got[1])
    model, s = _sampler(api, case, cfg, u, ev, eps, n, thin=k)
    with model, s:
        tab, w = _both_on(s, case, groups, D)
        kept = s.sample(n, rt=True, within_between=True)
    model, s = _sampler(api, case, cfg, u, ev, eps, n * k)
    with model, s:
        every = s.sample(n * k)
    assert np.array_equal(every.events[k - 1::k], kept.events)
    R = _rit(api, case, every.theta[k - 1::k], every.events[k - 1::k], D)
    assert np.array_equal(kept.group_curves["rt_by_group"], _want_rg(tab, w, R))


def test_a_burst_run_again_after_a_time_out_leaves_its_own_curves(api):
    """seir_sampler_debug_fail_handoff (the existing test hook, once) in the middle of overlapped bursts: the outputs are
    indexed by slot and rewritten by the re-run."""
    case, u, ev, cfg, eps = _case("micro_20x60", 8)
    B, nb, burst, D = 8, 6, 4, 5
    groups = _groups_for(20)
    model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
    with model, s:
        got = {}
        tab, w = _both_on(s, case, groups, D)

        def consume(tr, i):
            got[i] = (tr.events.copy(), tr.theta.copy(), {k: v.copy() for k, v in tr.group_curves.items()},
                      {k: v.copy() for k, v in tr.wb.items()})
            if i == 1 and not s.recoveries:                    # while burst 2 or 3 is in flight
                _lib.check(s._lib.seir_sampler_debug_fail_handoff(s._s, B - 1))
        s.sample_bursts(nb, burst, consume, rt=True, within_between=True)
        assert len(s.recoveries) == 1 and sorted(got) == list(range(nb))
        events = np.concatenate([got[i][0] for i in range(nb)])
        theta = np.concatenate([got[i][1] for i in range(nb)])
        gc = {k: np.concatenate([got[i][2][k] for i in range(nb)]) for k in got[0][2]}
        wb = {k: np.concatenate([got[i][3][k] for i in range(nb)]) for k in got[0][3]}
        assert np.array_equal(gc["rt_by_group"], _want_rg(tab, w, _rit(api, case, theta, events, D)))
        assert np.array_equal(gc["within_by_group"][:, :, 0], wb["within_pressure"])       # M = 20: one wave
        assert np.array_equal(gc["between_by_group"][:, :, 0], wb["between_pressure"])


def test_a_second_table_drops_the_weights_another_window_and_no_table(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 2)
    n, D = 4, 3
    wn = _weight(case)
    N = np.asarray(case["cov"].N, np.float64).reshape(-1)
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        def state(fn, *a):
            with pytest.raises(_lib.SeirError) as e:
                fn(*a)
            return e.value.code
        assert state(s.set_group_rt, np.ones(3)) == _lib.ERR_STATE                          # no table
        assert state(s.set_group_within_between, True) == _lib.ERR_STATE
        a = [[0, 1, 2], [19]]
        tab_a = _table(a)
        w_a = G.rt_weights(tab_a, N)
        _set(s, a)
        with pytest.raises(ValueError, match="aligned"):
            s.set_group_rt(np.ones(3))
        s.set_group_rt(w_a)
        s.set_group_within_between(True)
        assert state(s.read_group_rt, 1) == _lib.ERR_STATE                                  # rt is off
        assert state(s.read_group_wb, 1) == _lib.ERR_STATE
        s.reset_rt(D, wn)
        s.reset_within_between(D)
        tr = s.sample(n, rt=True, within_between=True)
        R = _rit(api, case, tr.theta, tr.events, D)
        assert np.array_equal(tr.group_curves["rt_by_group"], _want_rg(tab_a, w_a, R))
        wa = tr.group_curves["within_by_group"]
        # another table: group R_t goes off with the old weights, group within / between is sized for the new one
        b = [list(range(20)), [5], list(range(3, 17)), [0, 1, 2]]
        tab_b = _table(b)
        w_b = G.rt_weights(tab_b, N)
        _set(s, b)
        s.rt(0, n)
        s.within_between(0, n)
        assert state(s.read_group_rt, n) == _lib.ERR_STATE
        got = s.read_group_wb(n)
        assert got["within_by_group"].shape == (n, 2, 4, D) and np.array_equal(got["within_by_group"][:, :, 3], wa[:, :, 0])
        assert np.array_equal(got["within_by_group"][:, :, 0], tr.wb["within_pressure"])
        s.set_group_rt(w_b)                                                                 # on again: sized at the switch
        s.rt(0, n)
        assert np.array_equal(s.read_group_rt(n), _want_rg(tab_b, w_b, R))
        # another D
        s.reset_rt(D + 4, wn)
        s.rt(0, n)
        assert np.array_equal(s.read_group_rt(n), _want_rg(tab_b, w_b, _rit(api, case, tr.theta, tr.events, D + 4)))
        assert state(s.read_group_rt, n + 1) == _lib.ERR_INVALID
        assert state(s.set_group_rt, np.full(w_b.shape, np.inf)) == _lib.ERR_INVALID
        # switches off: nothing more is launched, the reads fail, rt is what it was
        s.set_group_rt(None)
        s.set_group_within_between(False)
        assert state(s.read_group_rt, 1) == _lib.ERR_STATE and state(s.read_group_wb, 1) == _lib.ERR_STATE
        s.set_group_within_between(True)
        s.set_groups(None, None)                                                            # G = 0: both off
        s.rt(0, n)
        s.within_between(0, n)
        assert state(s.read_group_wb, 1) == _lib.ERR_STATE
        again = s.sample(n, rt=True, within_between=True)
        assert again.group_curves is None


def test_outputs_above_half_of_the_free_memory_are_refused_and_the_next_calls_are_safe(api):
    """2^19 slots x 3 chains x 256 groups x 8 bytes: 3.2 GB per day and plane.  At D = 1 the outputs fit, at D = 70 they are
    225 GB (R_t) and 451 GB (within / between).  The refusal comes from the switch (which then stays off) or from the reset
    (the product is then on without group outputs)."""
    import torch
    case, u, ev, cfg, eps = _case("micro_1x70", 3)
    cap, n, Gn, D = 1 << 19, 4, _lib.GROUPS_MAX, 70
    need = cap * 3 * Gn * D * 8
    assert need > torch.cuda.mem_get_info()[0] / 2
    wn = _weight(case)
    model, s = _sampler(api, case, cfg, u, ev, eps, cap)
    with model, s:
        s.sample(n)                                            # the slots hold draws
        _set(s, [[0]] * Gn)
        s.reset_rt(1, wn)
        s.reset_within_between(1)
        s.set_group_rt(np.ones(Gn))
        s.set_group_within_between(True)
        s.rt(0, n)
        s.within_between(0, n)
        small = _curves(s, n)
        assert np.array_equal(small["rt_by_group"][:, :, 7], s.read_rt_draws(n))    # M = 1: the national weight is 1.0 too
        assert np.array_equal(small["within_by_group"][:, :, 5], s.read_wb_draws(n)["within_pressure"])
        # the refusal in a reset: the product is on with the new window, without group outputs
        with pytest.raises(_lib.SeirError, match=r"group curves need \d+ bytes .* more than half of the \d+ bytes free") as e:
            s.reset_rt(D, wn)
        assert e.value.code == _lib.ERR_INVALID
        st = s._state()
        assert (st.rt_D, st.rt_j, st.group_rt_on, st.group_rt_D) == (D, 0, 1, 0)
        with pytest.raises(_lib.SeirError, match="more than half of the") as e:
            s.reset_within_between(D)
        assert e.value.code == _lib.ERR_INVALID
        st = s._state()
        assert (st.wb_D, st.group_wb_on, st.group_wb_D) == (D, 1, 0)
        out = s.sample(n, rt=True, within_between=True)
        assert out.group_curves is None and out.rt.shape == (n, 3, D) and out.wb["within_pressure"].shape == (n, 3, D)
        for fn in (s.read_group_rt, s.read_group_wb):
            with pytest.raises(_lib.SeirError) as e:
                fn(n)
            assert e.value.code == _lib.ERR_STATE
        # the refusal at the switch: it stays off
        s.set_group_rt(None)
        s.set_group_within_between(False)
        for fn, arg in ((s.set_group_rt, np.ones(Gn)), (s.set_group_within_between, True)):
            with pytest.raises(_lib.SeirError, match="more than half of the") as e:
                fn(arg)
            assert e.value.code == _lib.ERR_INVALID
            st = s._state()
            assert (st.rt_D, st.wb_D, st.group_rt_on, st.group_rt_D, st.group_wb_on, st.group_wb_D) == (D, D, 0, 0, 0, 0)
        s.rt(0, n)
        s.within_between(0, n)
        assert np.array_equal(s.read_rt_draws(n), out.rt)
        # a smaller table fits again
        _set(s, [[0]])
        s.set_group_rt(np.ones(1))
        s.rt(0, n)
        assert np.array_equal(s.read_group_rt(n)[:, :, 0], _rit(api, case, out.theta, out.events, D)[..., 0])


def test_nothing_else_notices_the_curves(api):
    """A sampler with both curves on against one that never heard of them: chain, summaries, forecast, check, R_t with its
    order statistics, within / between and the group sums, bit for bit."""
    from tests import test_check_gpu as CG
    from tests import test_forecast_gpu as FG
    case, u, ev, cfg, eps = _case("micro_20x60", 3)
    nb, burst, Hn, K, D = 3, 4, 6, 5, 7
    groups = _groups_for(20)
    runs = {}
    for on in (False, True):
        model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
        with model, s:
            got = {}
            _set(s, groups)
            if on:
                s.set_group_rt(_rt_weights(case, groups)[1])
                s.set_group_within_between(True)
            FG._reset(s, case, Hn)
            CG._reset(s, case, K)
            s.reset_rt(D, _weight(case))
            s.keep_rt_draws(nb * burst)
            s.reset_within_between(D)

            def consume(tr, i, got=got):
                got[i] = dict(theta=tr.theta.copy(), events=tr.events.copy(), hmc={k: v.copy() for k, v in tr.hmc.items()},
                              moves={mk: {kk: v.copy() for kk, v in mv.items()} for mk, mv in tr.moves.items()},
                              rt=tr.rt.copy(), curves=tr.group_curves,
                              **{k: v.copy() for d in (tr.marginals, tr.forecast, tr.check, tr.wb, tr.groups) for k, v in d.items()})
            s.sample_bursts(nb, burst, consume, summarize=True, forecast=True, rt=True, check=True, within_between=True,
                            groups=True)
            cs, rs, ws = s.check_summary(), s.rt_summary(), s.within_between_summary()
            runs[on] = (got, s.get_state() + s.get_kernel(), [s.summary(), s.forecast_summary(), cs.moments],
                        [getattr(cs, k) for k in CG.COUNTS], [rs.count, rs.ref, rs.sum, rs.sumsq, rs.gt1],
                        [ws.count, ws.defined, ws.ref_w, ws.sum_w, ws.sumsq_w, ws.ref_b, ws.sum_b, ws.gt],
                        [s.rt_order_stats([0, 5, nb * burst - 1]), s.rt_order_stats([0, 17, 3 * nb * burst - 1], pooled=True)])
    from types import SimpleNamespace
    for i in range(nb):
        a, b = runs[False][0][i], runs[True][0][i]
        _same_bits(SimpleNamespace(**{k: a[k] for k in ("theta", "events", "hmc", "moves")}),
                   SimpleNamespace(**{k: b[k] for k in ("theta", "events", "hmc", "moves")}))
        assert a["curves"] is None and set(b["curves"]) == {"rt_by_group", "within_by_group", "between_by_group"}
        for k in a:
            if k not in ("theta", "events", "hmc", "moves", "curves"):
                assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
    for x, y in zip(runs[False][1], runs[True][1]):
        assert np.array_equal(x, y)
    for ma, mb in zip(runs[False][2], runs[True][2]):
        for k in ("count", "ref", "sum", "sumsq"):
            assert np.array_equal(getattr(ma, k), getattr(mb, k)), k
    for j in (3, 4, 5, 6):
        for x, y in zip(runs[False][j], runs[True][j]):
            assert np.array_equal(x, y, equal_nan=np.asarray(x).dtype.kind == "f")


# ---------------------------------------------------------------------------------------------------------------------
# the size users run, and the command line
# ---------------------------------------------------------------------------------------------------------------------
def test_uk380_nations(api):
    """UK-380 x 8 chains x 12 draws, `nations` (315, 32, 22 and 11 members), D = 14, uint16 trace."""
    case = H.build_case("uk380", 43, alpha_t_sd=0.005)
    B, n, D = 8, 12, 14
    u = synth.jitter_params(case["u"], B, scale=0.002, seed=3, T=case["k"].T)
    ev = np.stack([case["events"]] * B)
    codes = [str(x) for x in np.load(synth._DATA)["lad19cd"]]
    tab = G.parse_groups("nations", len(codes), codes)
    N = np.asarray(case["cov"].N, np.float64).reshape(-1)
    w = G.rt_weights(tab, N)
    model, s = _sampler(api, case, CFG_REF, u, ev, 1.2e-5, n, record_events="u16")
    with model, s:
        s.set_groups(tab.offsets, tab.members)
        s.set_group_rt(w)
        s.set_group_within_between(True)
        s.reset_rt(D, _weight(case))
        s.reset_within_between(D)
        tr = s.sample(n, rt=True, within_between=True)
        R = _rit(api, case, tr.theta, tr.events, D)
        rg = tr.group_curves["rt_by_group"]
        assert rg.shape == (n, B, 4, D) and np.array_equal(rg, _want_rg(tab, w, R))
        # the nations are a partition: their population-weighted curves recombine into the national one
        pop = tab.sum_rows(N)
        np.testing.assert_allclose((rg * (pop / pop.sum())[None, None, :, None]).sum(axis=2), tr.rt, rtol=1e-12)
        _check_wb(api, case, tab, tr, tr.group_curves, D, (n - 1,), (D - 1,), chains=(B - 1,))     # 380^2 exact fmas: one cell row
        for k, nat in (("within_by_group", "within_pressure"), ("between_by_group", "between_pressure")):
            np.testing.assert_allclose(tr.group_curves[k].sum(axis=2), tr.wb[nat], rtol=1e-12)


def test_cli_group_curves(api, tmp_path):
    """`--rt 7 --rt-quantiles 0.05,0.5,0.95 --within-between 7 --groups nations --summaries only` with and without
    `--groups-rt --groups-within-between` on an NI-11 data set whose locations carry codes of three nations."""
    tmp_path = str(tmp_path)
    cov = synth.make_covariates("ni11")
    events, init, _ = synth.simulate_epidemic(cov)
    M = events.shape[0]
    codes = ["E0%d" % m for m in range(5)] + ["S1%d" % m for m in range(4)] + ["W06", "W07"]
    data = os.path.join(tmp_path, "data.h5")
    inf.write_inference_data(data, cov, events[..., 2], locations=codes)
    base = ["--rt", "7", "--rt-quantiles", "0.05,0.5,0.95", "--within-between", "7", "--groups", "nations", "--summaries", "only"]
    plain_path, plain_log = _cli(tmp_path, "plain", data, base)
    plain = _datasets(plain_path)
    path, log = _cli(tmp_path, "curves", data, base + ["--groups-rt", "--groups-within-between"])
    got = _datasets(path)
    # without the two flags: exactly the keys of a run before the feature
    assert not any("by_group" in k and k != "samples/seir_by_group" for k in plain) and "groups/rt_weights" not in plain
    assert not any(k.startswith(("rt/group_", "rt/pooled_group_", "within_between/group_")) for k in plain)
    assert "by group, last day" not in plain_log
    new = sorted(set(got) - set(plain))
    assert not set(plain) - set(got)
    for k in plain:                                            # the same seed: the same run
        assert np.array_equal(plain[k], got[k], equal_nan=plain[k].dtype.kind == "f"), k
    assert new == sorted(["groups/rt_weights", "samples/R_t_by_group", "samples/within_pressure_by_group",
                          "samples/between_pressure_by_group", "rt/group_R_t_mean", "rt/group_R_t_var", "rt/group_prob_gt1",
                          "rt/group_R_t_quantiles", "rt/pooled_group_R_t_quantiles", "within_between/group_defined",
                          "within_between/group_within_share_mean", "within_between/group_p_within_gt_between"])
    tab = G.parse_groups("nations", M, codes)
    N = np.asarray(cov.N, np.float64).reshape(-1)
    assert np.array_equal(got["groups/rt_weights"], G.rt_weights(tab, N))
    rg, wg, bg = got["samples/R_t_by_group"], got["samples/within_pressure_by_group"], got["samples/between_pressure_by_group"]
    assert rg.shape == wg.shape == bg.shape == (12, 3, 7) and rg.dtype == np.float64
    pop = tab.sum_rows(N)
    np.testing.assert_allclose((rg * (pop / pop.sum())[None, :, None]).sum(axis=1), got["samples/R_t"], rtol=1e-12)
    np.testing.assert_allclose(wg.sum(axis=1), got["samples/within_pressure"], rtol=1e-12)
    np.testing.assert_allclose(bg.sum(axis=1), got["samples/between_pressure"], rtol=1e-12)
    mean, var, p1 = G.curve_moments(rg)
    assert np.array_equal(got["rt/group_R_t_mean"], mean) and np.array_equal(got["rt/group_R_t_var"], var)
    assert np.array_equal(got["rt/group_prob_gt1"], p1)
    want = np.quantile(rg, [0.05, 0.5, 0.95], axis=0)
    np.testing.assert_allclose(got["rt/group_R_t_quantiles"], want, rtol=1e-12)
    np.testing.assert_allclose(got["rt/pooled_group_R_t_quantiles"], want, rtol=1e-12)      # one chain
    d, sh, pg = G.share_stats(wg, bg)
    assert np.array_equal(got["within_between/group_defined"], d)
    assert np.array_equal(got["within_between/group_within_share_mean"], sh, equal_nan=True)
    assert np.array_equal(got["within_between/group_p_within_gt_between"], pg, equal_nan=True)
    assert log.count("R_t by group, last day") == 1 and log.count("Within share of the infection pressure") == 1

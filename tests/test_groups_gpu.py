"""Region totals on the device (include/seir_hip.h, "Region totals on the device"; covid19uk_amd/csrc/group_kernels.h):
for every kept draw, exact int64 sums of the event counts over groups of locations -- of the recorded epidemic, of the
forecast and of the in-sample check.

The kernel alone (`SeirModel.group_sums`) is held to `events[:, members].sum(1)` at the shapes that turn its branches.
Through the sampler the trace sums are held to NumPy on the same run's recorded events, and the forecast's and the check's
sums and state0 to `SeirModel.simulate` per chain, the way tests/test_forecast_gpu.py and tests/test_check_gpu.py form
their references.  Every comparison is `np.array_equal` on integers."""
import os

import numpy as np
import pytest

from covid19uk_amd import _lib, synth
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.posterior import groups as G
from tests import helpers as H
from tests import test_check_gpu as CG
from tests import test_forecast_gpu as FG
from tests.test_recovery_gpu import _case, _same_bits
from tests.test_sampler_gpu import CFG_REF, CFG_SMALL, api  # noqa: F401  (fixture)
from tests.test_summary_gpu import _cli, _datasets, _sampler

pytestmark = pytest.mark.gpu

WAVES, SEG, NDMAX = 8, 64, 1024      # GRP_WAVES, GRP_SEG, GRP_NDMAX of group_kernels.h


def _csr(groups):
    off = np.cumsum([0] + [len(g) for g in groups]).astype(np.int32)
    return off, np.concatenate([np.asarray(g, np.int32) for g in groups])


def _want(ev, groups):
    return np.stack([ev[:, np.asarray(g)].astype(np.int64).sum(axis=1) for g in groups], axis=1)


@pytest.fixture(scope="module")
def model(api):
    case = H.build_case("micro_3x1", 43)
    with api[0](case["cov"], case["init"], max_chains=1) as m:
        yield m


def _random(rng, n, M, L, hi=1000):
    return rng.integers(0, hi, size=(n, M, L, 3), dtype=np.int64).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 63, 64, 65, 365])
@pytest.mark.parametrize("M", [1, 9, 65, 520])
def test_group_sums_equal_numpy_at_the_chunk_and_segment_edges(model, M, L):
    """Days: one lane, one short of / exactly / one past a 64-day chunk, six chunks.  Rows: one, one past a workgroup's
    waves, one past a segment, nine segments.  Groups: all locations, a random overlapping pair, the last row alone."""
    rng = np.random.default_rng([M, L])
    n = 3
    ev = _random(rng, n, M, L)
    groups = [list(range(M)), sorted(rng.choice(M, size=max(1, M // 2), replace=False)),
              sorted(rng.choice(M, size=max(1, (2 * M) // 3), replace=False)), [M - 1]]
    got = model.group_sums(ev, *_csr(groups))
    assert got.dtype == np.int64 and got.shape == (n, len(groups), L, 3)
    assert np.array_equal(got, _want(ev, groups))
    assert np.array_equal(got[:, 0], ev.astype(np.int64).sum(axis=1))


@pytest.mark.parametrize("M", [1, 9, 65])
def test_singleton_groups_reproduce_the_input(model, M):
    ev = _random(np.random.default_rng(M), 2, M, 70)
    got = model.group_sums(ev, *_csr([[m] for m in range(M)]))
    assert np.array_equal(got, ev.astype(np.int64))


def test_a_group_of_more_members_than_waves_and_than_a_segment(model):
    """9 members: one wave takes two rows.  65 and 129: a second and a third segment meet in the output."""
    M = 200
    ev = _random(np.random.default_rng(7), 2, M, 65)
    groups = [list(range(3, 3 + WAVES + 1)), list(range(0, 2 * (SEG + 1), 2)), list(range(M - 2 * SEG - 1, M))]
    assert [len(g) for g in groups] == [WAVES + 1, SEG + 1, 2 * SEG + 1]
    assert np.array_equal(model.group_sums(ev, *_csr(groups)), _want(ev, groups))


def test_256_groups(model):
    M = 300
    rng = np.random.default_rng(11)
    ev = _random(rng, 2, M, 10)
    groups = [sorted(rng.choice(M, size=int(rng.integers(1, 80)), replace=False)) for _ in range(_lib.GROUPS_MAX)]
    assert np.array_equal(model.group_sums(ev, *_csr(groups)), _want(ev, groups))


def test_one_draw_and_more_draws_than_one_launch(model):
    rng = np.random.default_rng(13)
    groups = [[0, 2], [1], [0, 1, 2, 3]]
    for n in (1, NDMAX + 1):
        ev = _random(rng, n, 4, 5)
        assert np.array_equal(model.group_sums(ev, *_csr(groups)), _want(ev, groups)), n


def test_sums_beyond_32_bits(model):
    """520 members of 2^31 - 1 each: the sum needs 41 bits."""
    M, L = 520, 3
    ev = np.full((1, M, L, 3), 2 ** 31 - 1, np.int32)
    ev[0, 5, 1, 2] = 0
    groups = [list(range(M))]
    got = model.group_sums(ev, *_csr(groups))
    assert np.array_equal(got, _want(ev, groups))
    assert int(got[0, 0, 0, 0]) == M * (2 ** 31 - 1) and int(got[0, 0, 1, 2]) == (M - 1) * (2 ** 31 - 1)


def test_group_sums_do_not_depend_on_workgroup_timing(api):
    case = H.build_case("micro_3x1", 43)
    ev = _random(np.random.default_rng(3), 5, 130, 130)
    groups = [list(range(130)), list(range(0, 130, 3)), [129]]
    for skew in (1, 2, 3):
        with api[0](case["cov"], case["init"], max_chains=1) as m:
            m.set_option(debug_skew=skew)
            assert np.array_equal(m.group_sums(ev, *_csr(groups)), _want(ev, groups)), skew


def test_group_sums_refusals(model):
    ev = np.zeros((2, 4, 3, 3), np.int32)

    def refused(off, mem, word, ev=ev):
        with pytest.raises(_lib.SeirError) as e:
            model.group_sums(ev, np.asarray(off, np.int32), np.asarray(mem, np.int32))
        assert e.value.code == _lib.ERR_INVALID and word in str(e.value), str(e.value)

    refused([0, 0], [0], "empty")
    refused([0, 2, 1], [0, 1], "decrease")
    refused([0, 1], [4], "outside")
    refused([0, 1], [-1], "outside")
    refused([0, 2], [1, 0], "ascending")
    refused([0, 2], [1, 1], "ascending")
    refused([1, 2], [0, 1], "starts at 0")
    refused(list(range(_lib.GROUPS_MAX + 2)), [0] * (_lib.GROUPS_MAX + 1), "G=")
    refused([0], [0], "G=")
    rc = model._lib.seir_group_sums(model._ctx, None, 1, 4, 3, 1, None, None, None)
    assert rc == _lib.ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------------
# through the sampler
# ---------------------------------------------------------------------------------------------------------------------
def _groups_for(M, rng=None):
    """All locations, every location alone (up to 40 of them), two overlapping halves."""
    rng = np.random.default_rng(M) if rng is None else rng
    groups = [list(range(M))] + [[m] for m in range(min(M, 40))]
    if M > 1:
        groups += [sorted(rng.choice(M, size=(M + 1) // 2, replace=False)), list(range(M // 3, M))]
    return groups


def _set(s, groups):
    s.set_groups(*_csr(groups))


def _state0(init, events, t0, groups):
    """init [M,4], events [n,B,M,T,3] -> [n,B,G,3]: the members' sum of S, E, I at day t0."""
    st = np.stack([CG._state_at(init, events[:, b], t0) for b in range(events.shape[1])], axis=1)[..., :3]   # [n,B,M,3]
    return np.stack([st[:, :, np.asarray(g)].sum(axis=2) for g in groups], axis=2)


def _by_group(x, groups):
    """[n,B,M,L,3] -> [n,B,G,L,3]."""
    return np.stack([x[:, :, np.asarray(g)].astype(np.int64).sum(axis=2) for g in groups], axis=2)


TRACE_CASES = {
    # name, B, record, n
    "M=1,u16,B=3": ("micro_1x70", 3, "u16", 6),
    "T=1,B=1": ("micro_3x1", 1, True, 4),
    "T=64,M=9,u16,B=3": ("micro_9x64", 3, "u16", 5),
    "T=65,M=7,B=8": ("micro_7x65", 8, True, 4),
    "M=65,u16,B=1": ("micro_65x70", 1, "u16", 5),
}


@pytest.mark.parametrize("case_id", list(TRACE_CASES))
def test_trace_sums_equal_numpy_on_the_recorded_events(api, case_id):
    name, B, record, n = TRACE_CASES[case_id]
    case, u, ev, cfg, eps = _case(name, B)
    M, T = case["k"].M, case["k"].T
    groups = _groups_for(M)
    model, s = _sampler(api, case, cfg, u, ev, eps, n, record_events=record)
    with model, s:
        _set(s, groups)
        tr = s.sample(n, summarize=True, groups=True)
        got = tr.groups["seir_by_group"]
        assert set(tr.groups) == {"seir_by_group"} and got.dtype == np.int64 and got.shape == (n, B, len(groups), T, 3)
        assert np.array_equal(got, _by_group(tr.events, groups))
        assert np.array_equal(got[:, :, 0], tr.marginals["events_by_day"])                    # the all-locations group
        k = min(M, 40)
        assert np.array_equal(got[:, :, 1:1 + k], tr.events[:, :, :k].astype(np.int64))        # the singletons
        assert np.array_equal(s.read_group_marginals("trace", 2, first=n - 2)["seir_by_group"], got[n - 2:])


ROLL_CASES = {
    # name, B, record, n, H, K
    "M=1,H=7,K=7": ("micro_1x70", 3, "u16", 5, 7, 7),
    "T=1,H=1,K=1": ("micro_3x1", 2, True, 4, 1, 1),
    "M=9,H=64,K=64=T": ("micro_9x64", 3, "u16", 4, 64, 64),
    "M=7,H=65,K=64": ("micro_7x65", 2, True, 4, 65, 64),
    "M=65,H=128,K=65": ("micro_65x70", 1, "u16", 3, 128, 65),
    "T=800,H=128,K=128": ("slower_4x800", 3, True, 4, 128, 128),          # two full chunks on both sets of buffers
}


@pytest.mark.parametrize("case_id", list(ROLL_CASES))
def test_forecast_and_check_sums_equal_simulate_per_chain(api, case_id):
    name, B, record, n, Hn, K = ROLL_CASES[case_id]
    case, u, ev, cfg, eps = _case(name, B)
    if name.startswith("slower"):
        cfg, eps = CFG_REF, 3e-5                                # what tests/test_check_gpu.py runs this case with
    M, T = case["k"].M, case["k"].T
    groups = _groups_for(M)
    model, s = _sampler(api, case, cfg, u, ev, eps, n, record_events=record)
    with model, s:
        _set(s, groups)
        FG._reset(s, case, Hn)
        CG._reset(s, case, K)
        tr = s.sample(n, forecast=True, check=True, groups=True)
        assert set(tr.groups) == {"forecast_by_group", "forecast_group_state0", "check_by_group", "check_group_state0"}
        fw = FG._oracle(model, case, tr.theta, tr.events, Hn)
        cw = CG._oracle(model, case, tr.theta, tr.events, K)
        assert fw["sim"].any() or T == 1
        assert np.array_equal(tr.groups["forecast_by_group"], _by_group(fw["sim"], groups))
        assert np.array_equal(tr.groups["check_by_group"], _by_group(cw["sim"], groups))
        assert np.array_equal(tr.groups["forecast_group_state0"], _state0(case["init"], tr.events, T, groups))
        assert np.array_equal(tr.groups["check_group_state0"], _state0(case["init"], tr.events, T - K, groups))
        assert np.array_equal(tr.groups["forecast_by_group"][:, :, 0], tr.forecast["forecast_by_day"])
        assert np.array_equal(tr.groups["check_by_group"][:, :, 0], tr.check["check_by_day"])
        # the group's state from its sums is the per-location state summed: state_by_day of the all-locations group
        st = G.group_state(tr.groups["forecast_by_group"], tr.groups["forecast_group_state0"])
        assert np.array_equal(st[:, :, 0], tr.forecast["forecast_state_by_day"])


def _nations():
    codes = [str(x) for x in np.load(synth._DATA)["lad19cd"]]
    return G.parse_groups("nations", len(codes), codes)


def test_uk380_nations(api):
    """UK-380 x 8 chains x 12 draws, uint16 trace, H = 14, K = 14, the four nations."""
    case, u, ev, cfg, eps = _case("uk380", 8)
    n, Hn, K, T = 12, 14, 14, case["k"].T
    tab = _nations()
    groups = [list(tab.rows(g)) for g in range(tab.G)]
    assert [len(g) for g in groups] == [315, 32, 22, 11]
    model, s = _sampler(api, case, cfg, u, ev, eps, n, record_events="u16")
    with model, s:
        s.set_groups(tab.offsets, tab.members)
        FG._reset(s, case, Hn)
        CG._reset(s, case, K)
        tr = s.sample(n, summarize=True, forecast=True, check=True, groups=True)
        assert np.array_equal(tr.groups["seir_by_group"], _by_group(tr.events, groups))
        assert np.array_equal(tr.groups["seir_by_group"].sum(axis=2), tr.marginals["events_by_day"])    # a partition
        fw = FG._oracle(model, case, tr.theta, tr.events, Hn)
        cw = CG._oracle(model, case, tr.theta, tr.events, K)
        assert np.array_equal(tr.groups["forecast_by_group"], _by_group(fw["sim"], groups))
        assert np.array_equal(tr.groups["check_by_group"], _by_group(cw["sim"], groups))
        assert np.array_equal(tr.groups["forecast_group_state0"], _state0(case["init"], tr.events, T, groups))
        assert np.array_equal(tr.groups["check_group_state0"], _state0(case["init"], tr.events, T - K, groups))
        assert np.array_equal(tr.groups["forecast_by_group"].sum(axis=2), tr.forecast["forecast_by_day"])
        assert np.array_equal(tr.groups["check_by_group"].sum(axis=2), tr.check["check_by_day"])


def _all(s, n, first=0):
    out = {}
    for src in ("trace", "forecast", "check"):
        out.update(s.read_group_marginals(src, n, first=first))
    return out


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_cutting_a_burst_into_calls_halves_or_batches_does_not_matter(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    n, Hn, K = 11, 9, 6
    groups = _groups_for(20)
    model, s = _sampler(api, case, cfg, u, ev, eps, 2 * n)
    with model, s:
        _set(s, groups)
        s.reset_summary()
        FG._reset(s, case, Hn)
        CG._reset(s, case, K)
        for first in (0, n):                                   # two bursts in the two halves of the buffer
            s.reset_trace(at=first)
            s.run(n)
            s.summarize(first, n)
            s.forecast(first, n)
            s.check(first, n)
        tr = s.read_trace(2 * n)
        halves = _all(s, 2 * n)
        assert np.array_equal(halves["seir_by_group"], _by_group(tr.events, groups))
        assert np.array_equal(halves["forecast_by_group"], _by_group(FG._oracle(model, case, tr.theta, tr.events, Hn)["sim"], groups))
        assert np.array_equal(halves["check_by_group"], _by_group(CG._oracle(model, case, tr.theta, tr.events, K)["sim"], groups))
        s.reset_summary()
        FG._reset(s, case, Hn)
        CG._reset(s, case, K)
        for first, count in ((0, 3), (3, 1), (4, 9), (13, 2 * n - 13)):
            s.summarize(first, count)
            s.forecast(first, count)
            s.check(first, count)
        _same(_all(s, 2 * n), halves)


def test_a_call_longer_than_one_host_batch_holds(api):
    """130 slots: more than the 128 of a summary launch and of a forecast batch; 260 draws."""
    case, u, ev, cfg, eps = _case("micro_5x24", 2)
    n, Hn, K = 130, 3, 2
    groups = _groups_for(5)
    model, s = _sampler(api, case, cfg, u, ev, 0.002, n)
    with model, s:
        _set(s, groups)
        FG._reset(s, case, Hn)
        CG._reset(s, case, K)
        tr = s.sample(n, summarize=True, forecast=True, check=True, groups=True)
        assert np.array_equal(tr.groups["seir_by_group"], _by_group(tr.events, groups))
        assert np.array_equal(tr.groups["forecast_by_group"], _by_group(FG._oracle(model, case, tr.theta, tr.events, Hn)["sim"], groups))
        assert np.array_equal(tr.groups["check_by_group"], _by_group(CG._oracle(model, case, tr.theta, tr.events, K)["sim"], groups))
        assert np.array_equal(tr.groups["forecast_group_state0"], _state0(case["init"], tr.events, case["k"].T, groups))


@pytest.mark.parametrize("skew", [1, 2, 3])
def test_sums_do_not_depend_on_workgroup_timing_and_repeat(api, skew):
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    n, Hn, K = 6, 10, 5
    groups = _groups_for(20)
    res = {}
    for tag, sk in (("a", 0), ("b", 0), ("skew", skew)):
        if tag == "b" and skew != 1:
            continue                                           # the repeat of the plain run is checked once
        model, s = _sampler(api, case, cfg, u, ev, eps, n, skew=sk, record_events="u16")
        with model, s:
            _set(s, groups)
            FG._reset(s, case, Hn)
            CG._reset(s, case, K)
            tr = s.sample(n, summarize=True, forecast=True, check=True, groups=True)
            res[tag] = (tr.groups, tr.events)
    assert res["a"][0]["forecast_by_group"].any()
    for tag in res:
        assert np.array_equal(res["a"][1], res[tag][1])
        _same(res[tag][0], res["a"][0])


def test_chains_keep_their_sums_however_they_are_sharded(api):
    """Chains 2 and 3 of a 4-chain sampler against a 2-chain sampler created with first_chain_id = 2."""
    case, u, ev, cfg, eps = _case("micro_20x60", 4)
    n, Hn, K = 5, 8, 4
    groups = _groups_for(20)
    got = []
    for sl, kw in ((slice(None), {}), (slice(2, None), dict(first_chain_id=2))):
        model, s = _sampler(api, case, cfg, u[sl], ev[sl], eps, n, **kw)
        with model, s:
            _set(s, groups)
            FG._reset(s, case, Hn)
            CG._reset(s, case, K)
            got.append(s.sample(n, summarize=True, forecast=True, check=True, groups=True).groups)
    _same({k: v[:, 2:] for k, v in got[0].items()}, got[1])
    assert got[1]["forecast_by_group"].any()


def test_with_thinning_the_sums_are_those_of_the_kept_draws(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 4)
    n, k = 6, 3
    groups = _groups_for(20)
    model, s = _sampler(api, case, cfg, u, ev, eps, n, thin=k)
    with model, s:
        _set(s, groups)
        kept = s.sample(n, summarize=True, groups=True)
    model, s = _sampler(api, case, cfg, u, ev, eps, n * k)
    with model, s:
        every = s.sample(n * k)
    assert np.array_equal(every.events[k - 1::k], kept.events)
    assert np.array_equal(kept.groups["seir_by_group"], _by_group(every.events[k - 1::k], groups))


def test_a_burst_run_again_after_a_time_out_is_summed_once(api):
    """seir_sampler_debug_fail_handoff (the existing test hook, once) in the middle of overlapped bursts: the outputs are
    indexed by slot and rewritten by the re-run, so the disturbed run's sums are those of its own draws."""
    case, u, ev, cfg, eps = _case("micro_20x60", 8)
    B, nb, burst, Hn = 8, 6, 4, 5
    groups = _groups_for(20)
    model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
    with model, s:
        got = {}
        _set(s, groups)
        FG._reset(s, case, Hn)

        def consume(tr, i):
            got[i] = (tr.events.copy(), tr.theta.copy(), {k: v.copy() for k, v in tr.groups.items()})
            if i == 1 and not s.recoveries:                    # while burst 2 or 3 is in flight
                _lib.check(s._lib.seir_sampler_debug_fail_handoff(s._s, B - 1))
        s.sample_bursts(nb, burst, consume, summarize=True, forecast=True, groups=True)
        assert len(s.recoveries) == 1 and sorted(got) == list(range(nb))
        events = np.concatenate([got[i][0] for i in range(nb)])
        theta = np.concatenate([got[i][1] for i in range(nb)])
        grp = {k: np.concatenate([got[i][2][k] for i in range(nb)]) for k in got[0][2]}
        assert np.array_equal(grp["seir_by_group"], _by_group(events, groups))
        assert np.array_equal(grp["forecast_by_group"], _by_group(FG._oracle(model, case, theta, events, Hn)["sim"], groups))
        assert np.array_equal(grp["forecast_group_state0"], _state0(case["init"], events, case["k"].T, groups))


def test_another_table_then_none_and_the_refusals(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 2)
    n, Hn = 4, 3
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        def state(fn, *a):
            with pytest.raises(_lib.SeirError) as e:
                fn(*a)
            return e.value.code, str(e.value)
        assert state(s.read_group_marginals, "trace", 1)[0] == _lib.ERR_STATE              # no table
        a = [[0, 1, 2], [19]]
        _set(s, a)
        code, msg = state(s.read_group_marginals, "trace", 1)
        assert code == _lib.ERR_STATE and "summaries are not enabled" in msg                # the source is off
        assert state(s.read_group_marginals, "forecast", 1)[0] == _lib.ERR_STATE
        assert state(s.read_group_marginals, "check", 1)[0] == _lib.ERR_STATE
        FG._reset(s, case, Hn)                                                              # sizes the forecast's outputs
        tr = s.sample(n, summarize=True, forecast=True, groups=True)
        assert np.array_equal(tr.groups["seir_by_group"], _by_group(tr.events, a))
        fw = FG._oracle(model, case, tr.theta, tr.events, Hn)
        assert np.array_equal(tr.groups["forecast_by_group"], _by_group(fw["sim"], a))
        b = [list(range(20)), [5], list(range(3, 17))]                                      # another G: sized again
        _set(s, b)
        s.summarize(0, n, accumulate=False)
        assert np.array_equal(s.read_group_marginals("trace", n)["seir_by_group"], _by_group(tr.events, b))
        FG._reset(s, case, Hn + 70)                                                         # another H: sized again
        s.forecast(0, n)
        fw = FG._oracle(model, case, tr.theta, tr.events, Hn + 70)
        g = s.read_group_marginals("forecast", n)
        assert np.array_equal(g["forecast_by_group"], _by_group(fw["sim"], b))
        assert np.array_equal(g["forecast_group_state0"], _state0(case["init"], tr.events, case["k"].T, b))
        assert state(s.read_group_marginals, "trace", n + 1)[0] == _lib.ERR_INVALID
        for off, mem in (([0, 0], [0]), ([0, 1], [20]), ([0, 2], [3, 3]), ([0, 2], [4, 3]), ([0, 2, 1], [0, 1])):
            with pytest.raises(_lib.SeirError) as e:
                s.set_groups(np.asarray(off, np.int32), np.asarray(mem, np.int32))
            assert e.value.code == _lib.ERR_INVALID
        # a refused table leaves the one in force alone
        s.summarize(0, n, accumulate=False)
        assert np.array_equal(s.read_group_marginals("trace", n)["seir_by_group"], _by_group(tr.events, b))
        s.set_groups(None, None)                                                            # G = 0 frees everything
        assert state(s.read_group_marginals, "trace", 1)[0] == _lib.ERR_STATE
        s.summarize(0, n, accumulate=False)                                                 # and nothing more is launched
        assert np.array_equal(s.read_marginals(n)["events_by_day"], tr.marginals["events_by_day"])
    model, s = _sampler(api, case, cfg, u, ev, eps, n, record_events=False)
    with model, s:
        with pytest.raises(_lib.SeirError) as e:
            _set(s, [[0]])
        assert e.value.code == _lib.ERR_STATE


def test_outputs_above_half_of_the_free_memory_are_refused_and_the_next_call_is_safe(api):
    """2^19 slots x 256 groups: 6.4 GB at H = 1, 412 GB at H = 128, more than the device has.  The refusal comes from
    `groups_set` (which then leaves the table in force alone) or from the source's reset (whose source then has no group
    outputs); the calls that follow launch nothing for the groups and the forecast is what it was."""
    import torch
    case, u, ev, cfg, eps = _case("micro_1x70", 1)
    cap, n, G, Hn = 1 << 19, 4, _lib.GROUPS_MAX, 128
    big, small = [[0]] * G, [[0]]
    need = cap * G * (Hn + 1) * 24
    assert need > torch.cuda.mem_get_info()[0]                 # (between free / 2 and free another process may move the line)
    model, s = _sampler(api, case, cfg, u, ev, eps, cap)
    with model, s:
        tr = s.sample(n)
        # the refusal in a source's reset: the table fits at H = 1 and not at H = 128
        FG._reset(s, case, 1)
        _set(s, big)
        s.forecast(0, n)
        assert np.array_equal(s.read_group_marginals("forecast", n)["forecast_by_group"][:, :, 0],
                              s.read_forecast_marginals(n)["forecast_by_day"])
        with pytest.raises(_lib.SeirError, match=rf"need {need} bytes .* more than half of the \d+ bytes free") as e:
            FG._reset(s, case, Hn)
        assert e.value.code == _lib.ERR_INVALID
        st = s._state()
        assert (st.forecast_H, st.fc_j, st.groups_G, st.group_L) == (Hn, 0, G, (0, 0, 0))
        s.forecast(0, n)                                       # the forecast is on with H = 128 and has no group outputs
        with pytest.raises(_lib.SeirError) as e:
            s.read_group_marginals("forecast", n)
        assert e.value.code == _lib.ERR_STATE
        # the refusal in groups_set: the table in force stays
        s.set_groups(None, None)
        FG._reset(s, case, Hn)
        _set(s, small)
        with pytest.raises(_lib.SeirError, match="more than half of the") as e:
            _set(s, big)
        assert e.value.code == _lib.ERR_INVALID
        st = s._state()
        assert (st.forecast_H, st.groups_G, st.groups_nnz, st.group_L) == (Hn, 1, 1, (0, Hn, 0))
        s.forecast(0, n)
        fw = FG._oracle(model, case, tr.theta, tr.events, Hn)
        got = s.read_group_marginals("forecast", n)
        assert np.array_equal(got["forecast_by_group"], _by_group(fw["sim"], small))
        assert np.array_equal(got["forecast_group_state0"], _state0(case["init"], tr.events, case["k"].T, small))
        assert np.array_equal(s.read_forecast_marginals(n)["forecast_by_day"], fw["forecast_by_day"])


def test_nothing_else_notices_the_groups(api):
    """A sampler with a table against one without: chain, summaries, forecast, check, R_t and within/between bit for bit."""
    case, u, ev, cfg, eps = _case("micro_20x60", 3)
    nb, burst, Hn, K, D = 3, 4, 6, 5, 7
    N = np.asarray(case["cov"].N, np.float64)
    runs = {}
    for on in (False, True):
        model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
        with model, s:
            got = {}
            if on:
                _set(s, _groups_for(20))
            FG._reset(s, case, Hn)
            CG._reset(s, case, K)
            s.reset_rt(D, N / N.sum())
            s.reset_within_between(D)

            def consume(tr, i, got=got):
                got[i] = dict(theta=tr.theta.copy(), events=tr.events.copy(), hmc={k: v.copy() for k, v in tr.hmc.items()},
                              moves={mk: {kk: v.copy() for kk, v in mv.items()} for mk, mv in tr.moves.items()},
                              rt=tr.rt.copy(), groups=tr.groups,
                              **{k: v.copy() for d in (tr.marginals, tr.forecast, tr.check, tr.wb) for k, v in d.items()})
            s.sample_bursts(nb, burst, consume, summarize=True, forecast=True, rt=True, check=True, within_between=True,
                            **(dict(groups=True) if on else {}))
            cs, rs, ws = s.check_summary(), s.rt_summary(), s.within_between_summary()
            runs[on] = (got, s.get_state() + s.get_kernel(), [s.summary(), s.forecast_summary(), cs.moments],
                        [getattr(cs, k) for k in CG.COUNTS], [rs.count, rs.ref, rs.sum, rs.sumsq, rs.gt1],
                        [ws.count, ws.defined, ws.ref_w, ws.sum_w, ws.sumsq_w, ws.ref_b, ws.sum_b, ws.gt])
    from types import SimpleNamespace
    for i in range(nb):
        a, b = runs[False][0][i], runs[True][0][i]
        _same_bits(SimpleNamespace(**{k: a[k] for k in ("theta", "events", "hmc", "moves")}),
                   SimpleNamespace(**{k: b[k] for k in ("theta", "events", "hmc", "moves")}))
        assert a["groups"] is None and b["groups"] is not None
        for k in a:
            if k not in ("theta", "events", "hmc", "moves", "groups"):
                assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
    for x, y in zip(runs[False][1], runs[True][1]):
        assert np.array_equal(x, y)
    for ma, mb in zip(runs[False][2], runs[True][2]):
        for k in ("count", "ref", "sum", "sumsq"):
            assert np.array_equal(getattr(ma, k), getattr(mb, k)), k
    for j in (3, 4, 5):
        for x, y in zip(runs[False][j], runs[True][j]):
            assert np.array_equal(x, y, equal_nan=np.asarray(x).dtype.kind == "f")


# ---------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_groups(api, tmp_path):
    """`--summaries only --forecast 14 --forecast-quantiles 0.05,0.5,0.95 --check 7` with and without `--groups nations`
    on an NI-11 data set whose locations carry codes of three nations: without it exactly the datasets of a run that never
    heard of groups, with it those and the group datasets, which agree with the national ones and with posterior.groups."""
    tmp_path = str(tmp_path)
    cov = synth.make_covariates("ni11")
    events, init, _ = synth.simulate_epidemic(cov)
    M, T = events.shape[0], events.shape[1]
    codes = ["E0%d" % m for m in range(5)] + ["S1%d" % m for m in range(4)] + ["W06", "W07"]
    data = os.path.join(tmp_path, "data.h5")
    inf.write_inference_data(data, cov, events[..., 2], locations=codes)
    base = ["--summaries", "only", "--forecast", "14", "--forecast-quantiles", "0.05,0.5,0.95", "--check", "7"]
    plain = _datasets(_cli(tmp_path, "plain", data, base)[0])
    path, log = _cli(tmp_path, "grp", data, base + ["--groups", "nations"])
    grp = _datasets(path)
    new = sorted(set(grp) - set(plain))
    assert not set(plain) - set(grp)
    for k in plain:                                            # the same seed: the same run
        assert np.array_equal(plain[k], grp[k], equal_nan=plain[k].dtype.kind == "f"), k
    planes = [f"{p}group_{x}_quantiles" for p in ("", "pooled_") for x in G.PLANES]
    assert new == sorted(["groups/" + k for k in ("names", "offsets", "members", "population", "initial_state")] +
                         ["samples/" + k for k in ("seir_by_group", "forecast_by_group", "forecast_group_state0", "check_by_group",
                                                   "check_group_state0")] +
                         ["forecast/" + k for k in ["group_seir_mean", "group_state_mean"] + planes] +
                         ["check/group_" + k for k in ("observed", "lt", "eq", "window_lt", "window_eq", "pit", "window_pit")])
    assert "Groups: 3 group(s)" in log and "Groups:" not in _cli(tmp_path, "plain2", data, base)[1]
    assert [x.decode() for x in grp["groups/names"]] == ["E", "S", "W"]
    assert np.array_equal(grp["groups/offsets"], [0, 5, 9, 11]) and np.array_equal(grp["groups/members"], np.arange(11))
    tab = G.parse_groups("nations", M, codes)
    assert np.array_equal(grp["groups/population"], tab.sum_rows(np.asarray(cov.N, np.float64)))
    assert np.array_equal(grp["groups/initial_state"], tab.sum_rows(grp["initial_state"]))
    n, nf = grp["samples/seir_by_day"].shape[0], 12
    sg, fg, f0 = grp["samples/seir_by_group"], grp["samples/forecast_by_group"], grp["samples/forecast_group_state0"]
    assert sg.dtype == np.int64 and sg.shape == (n, 3, T, 3) and fg.shape == (nf, 3, 14, 3) and f0.shape == (nf, 3, 3)
    assert grp["samples/check_by_group"].shape == (nf, 3, 7, 3)
    assert np.array_equal(sg.sum(axis=1), grp["samples/seir_by_day"]) and sg[:inf.warmup_size()].any()     # a partition
    assert np.array_equal(fg.sum(axis=1), grp["samples/forecast_by_day"])
    assert np.array_equal(grp["samples/check_by_group"].sum(axis=1), grp["samples/check_by_day"])
    assert np.array_equal(G.group_state(fg, f0).sum(axis=1), grp["samples/forecast_state_by_day"])
    np.testing.assert_array_equal(grp["forecast/group_seir_mean"], fg.mean(axis=0))
    np.testing.assert_array_equal(grp["forecast/group_state_mean"], G.group_state(fg, f0).mean(axis=0))
    np.testing.assert_allclose(grp["forecast/group_seir_mean"].sum(axis=0), grp["forecast/seir_mean"].sum(axis=0), rtol=1e-12)
    pl = G.forecast_planes(fg, f0)
    for x, name in enumerate(G.PLANES):
        want = np.quantile(pl[x].astype(np.float64), [0.05, 0.5, 0.95], axis=0)
        np.testing.assert_allclose(grp[f"forecast/group_{name}_quantiles"], want, rtol=1e-12)
        np.testing.assert_allclose(grp[f"forecast/pooled_group_{name}_quantiles"], want, rtol=1e-12)    # one chain
    cc = G.check_counts(grp["samples/check_by_group"], tab.sum_rows(grp["check/observed"]))
    for k, v in cc.items():
        assert np.array_equal(grp["check/" + k], np.asarray(v, np.float64)), k
    assert np.array_equal(grp["check/group_observed"], tab.sum_rows(events[:, T - 7:, 2]))

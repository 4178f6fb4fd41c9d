"""The burst protocol of `ChainSampler` (covid19uk_amd/sampler.py, `BURST_PRODUCTS`; DESIGN.md, "The burst protocol") without
a GPU: a sampler whose library answers every call with "ok" has every product on at once, and `sample` / `sample_bursts`
must enqueue and read them in the order of the table.  The expectations are formed from the table, so a row added later is
covered as it stands -- and refused until this sampler switches it on."""
import numpy as np
import pytest

import covid19uk_amd.sampler as sm
from covid19uk_amd import _lib
from covid19uk_amd.sampler import BURST_PRODUCTS, PRODUCTS, ChainSampler, ProductState

BASE = ("snapshot", "restore", "reset_trace", "run", "mark", "read_trace", "read_trace_async", "trace_wait")
ENQUEUE = tuple(p.enqueue for p in BURST_PRODUCTS if p.enqueue)
READ = tuple(p.read for p in BURST_PRODUCTS)
READ_ASYNC = tuple(p.read_async for p in BURST_PRODUCTS)
B, M, T, BURST = 2, 3, 5, 4


class OkLib:
    """libseirhip's stand-in: every function returns SEIR_OK and touches nothing -- but the forecast's draw counter in the
    state of its sampler, which it keeps as the library does: a forecast advances it, a snapshot holds it, a restore brings
    it back."""

    def __init__(self, sampler):
        self.sampler, self.snap = sampler, {}

    def __getattr__(self, name):
        return lambda *a: 0

    def seir_sampler_forecast(self, s, first, count, steps):
        self.sampler.state = self.sampler.state._replace(fc_j=self.sampler.state.fc_j + count)
        return 0

    def seir_sampler_snapshot(self, s, slot):
        self.snap[slot] = self.sampler.state.fc_j
        return 0

    def seir_sampler_restore(self, s, slot):
        self.sampler.state = self.sampler.state._replace(fc_j=self.snap[slot])
        return 0


class AllOn(ChainSampler):
    """ChainSampler without a device and with every product on: the calls the loops make by name are recorded and then run
    as they are, down to the library's stand-in."""
    B, P, M, T, cap, mmax = B, 6 + T - 1 + M, M, T, 16, 2
    record_events, events_dtype, auto_recover = True, np.int32, True

    def __init__(self):
        self.calls, self.j0, self.time_outs = [], [], 0
        self._lib, self._s, self._log = OkLib(self), None, None
        self.state = ProductState(summary_on=1, forecast_H=2, rt_D=3, check_K=2, wb_D=3, groups_G=2, groups_nnz=4,
                                  group_L=(T, 2, 2), group_rt_on=1, group_wb_on=1, group_rt_D=3, group_wb_D=3)
        self._fallback_level, self._clean_bursts, self.recoveries, self.retry_after = 0, 0, [], 8

    def _state(self):
        return self.state

    def __getattribute__(self, name):
        real = object.__getattribute__(self, name)
        if name not in BASE + ENQUEUE + READ + READ_ASYNC:
            return real
        calls = object.__getattribute__(self, "calls")

        def recorded(*a, **kw):
            calls.append((name,) + a)
            return real(*a, **kw)
        return recorded

    def trace_wait(self):
        if self.time_outs:
            self.time_outs -= 1
            raise _lib.HandoffTimeout("libseirhip call failed (-4): chain 0: 1 in-launch hand-off(s) timed out", _lib.ERR_HANDOFF)

    def steps(self, j0, count):
        self.j0.append(j0)
        return np.zeros((count, self.B, self.state.forecast_H))

    def requests(self):
        """Every keyword a row of the table asks with; the forecast's as the callable."""
        return dict({p.request: True for p in BURST_PRODUCTS if p.request}, forecast=self.steps)


class NoPin:
    """PinnedTrace in ordinary memory, its products' arrays shaped by the table."""
    built = 0

    def __init__(self, sampler, count, events=True, **kw):
        NoPin.built += 1
        self.count, self.kw = count, kw
        self.theta = np.zeros((count, sampler.B, sampler.P))
        self.events = np.zeros((count, sampler.B, sampler.M, sampler.T, 3), np.int32) if events else None
        self.hmc, self.moves = np.zeros((count, sampler.B, 3)), np.zeros((count, sampler.B, 4, _lib.MOVE_TRACE))
        for p in BURST_PRODUCTS:
            setattr(self, p.field, sm._allocate(p.arrays(sampler, kw[p.field]), lambda sh, dt: np.zeros((count, sampler.B) + sh, dt))
                    if kw.get(p.field) else None)

    def close(self):
        pass


@pytest.fixture
def nopin(monkeypatch):
    monkeypatch.setattr(sm, "PinnedTrace", NoPin)
    NoPin.built = 0


def _names(calls, among):
    return [c[0] for c in calls if c[0] in among]


def test_sample_enqueues_and_reads_every_product_in_table_order():
    s = AllOn()
    tr = s.sample(BURST, **s.requests())
    assert [c[0] for c in s.calls] == ["snapshot", "reset_trace", "run", *ENQUEUE, "read_trace", *READ]
    assert [c[:3] for c in s.calls if c[0] in ENQUEUE] == [(name, 0, BURST) for name in ENQUEUE]
    assert s.j0 == [0] and s.state.fc_j == BURST                # the steps are drawn for the draws the forecast is about to make
    for p in BURST_PRODUCTS:                                    # every field is filled, with the shapes the table states
        got, want = getattr(tr, p.field), p.arrays(s, s._burst_products(s.requests())[p.field][1])
        if isinstance(want, tuple):
            got, want = {"": got}, {"": want}
        assert list(got) == list(want), p.field
        for k, (shape, dtype) in want.items():
            assert got[k].shape == (BURST, B) + shape and got[k].dtype == dtype, (p.field, k)
    # nothing on: nothing of the table is called
    s = AllOn()
    s.state = s.state._replace(group_rt_on=0, group_wb_on=0, group_rt_D=0, group_wb_D=0)
    tr = s.sample(BURST)
    assert [c[0] for c in s.calls] == ["snapshot", "reset_trace", "run", "read_trace"]
    assert all(getattr(tr, field) is None for field in PRODUCTS)


def test_each_half_of_sample_bursts_enqueues_and_reads_every_product_in_table_order(nopin):
    s = AllOn()
    got = []
    s.sample_bursts(2, BURST, lambda tr, i: got.append((i, {f: getattr(tr, f) is not None for f in PRODUCTS})), marks={0: 1},
                    **s.requests())
    assert [i for i, _ in got] == [0, 1] and all(all(on.values()) for _, on in got)
    bufs = s._pinned
    assert NoPin.built == 2 and list(bufs[0].kw) == [p.field for p in BURST_PRODUCTS]
    # each half: the products behind the sweeps in table order, the mark right behind the first row
    assert _names(s.calls, ("run", "mark") + ENQUEUE) == ["run", ENQUEUE[0], "mark", *ENQUEUE[1:], "run", *ENQUEUE]
    assert [c[:3] for c in s.calls if c[0] in ENQUEUE] == [(name, h * BURST, BURST) for h in (0, 1) for name in ENQUEUE]
    assert s.j0 == [0, BURST]
    # the reads on the copy stream follow the trace's copy in table order, into the half's own buffer
    assert _names(s.calls, ("read_trace_async",) + READ_ASYNC) == ["read_trace_async", *READ_ASYNC] * 2
    reads = [c for c in s.calls if c[0] in READ_ASYNC]
    assert [c[-3:-1] for c in reads] == [(BURST, h * BURST) for h in (0, 1) for _ in READ_ASYNC]
    assert all(c[-1] is bufs[h] for h in (0, 1) for c in reads[h * len(READ_ASYNC):(h + 1) * len(READ_ASYNC)])
    # burst 1 is enqueued before burst 0 is waited for
    names = [c[0] for c in s.calls]
    assert names.index("trace_wait") > [i for i, n in enumerate(names) if n == "run"][1]


# what the library does to its state at a reset with another extent, at another table, at a switch that goes off
TWEAKS = ((dict(forecast_H=3, group_L=(T, 3, 2)), dict(rt_D=2, group_rt_D=2), dict(check_K=1, group_L=(T, 3, 1)),
           dict(wb_D=2, group_wb_D=2), dict(groups_G=3), dict(group_wb_on=0, group_wb_D=0), dict(group_rt_on=0, group_rt_D=0)))


def test_the_pinned_buffers_are_kept_until_a_size_changes(nopin):
    s = AllOn()

    def call(burst=BURST, **kw):
        s.sample_bursts(2, burst, lambda tr, i: None, **dict(s.requests(), **kw))
        return dict(s._pinned[0].kw)
    sizes = call()
    assert NoPin.built == 2 and call() == sizes and NoPin.built == 2        # two equal calls: built once
    built, moved = 2, set()
    for tweak in TWEAKS:
        s.state = s.state._replace(**tweak)
        now = call()
        built += 2
        assert NoPin.built == built and call() == now and NoPin.built == built, tweak
        moved |= {f for f in PRODUCTS if now.get(f) != sizes.get(f)}
        sizes = now
    now = call(summarize=False, groups=("forecast", "check"))
    moved |= {f for f in PRODUCTS if now.get(f) != sizes.get(f)}
    assert NoPin.built == built + 2 and "marginals" not in now               # a product that is off adds no keyword
    assert moved == set(PRODUCTS), "a row of the table whose size this test never changes"
    call(summarize=False, groups=("forecast", "check"), events=False)
    assert NoPin.built == built + 4
    call(burst=2, summarize=False, groups=("forecast", "check"), events=False)
    assert NoPin.built == built + 6
    # nothing on at all: the class is called without keywords
    s = AllOn()
    s.state = s.state._replace(group_rt_on=0, group_wb_on=0, group_rt_D=0, group_wb_D=0)
    s.sample_bursts(2, BURST, lambda tr, i: None)
    assert s._pinned[0].kw == {}


def test_a_burst_that_is_run_again_gets_the_same_steps(nopin):
    s = AllOn()
    s.time_outs = 1                                             # burst 0 times out: seen at its wait, when burst 1 is enqueued
    got = []
    s.sample_bursts(2, BURST, lambda tr, i: got.append(i), **s.requests())
    assert got == [0, 1] and len(s.recoveries) == 1
    assert s.j0 == [0, BURST, 0, BURST] and s.state.fc_j == 2 * BURST
    assert [c[:3] for c in s.calls if c[0] in ENQUEUE] == [(name, h * BURST, BURST) for h in (0, 1, 0, 1) for name in ENQUEUE]
    s = AllOn()
    real_read, failed = s.read_trace, []

    def read_trace(n, **kw):
        if not failed:
            failed.append(1)
            raise _lib.HandoffTimeout("libseirhip call failed (-4): chain 0: 1 in-launch hand-off(s) timed out", _lib.ERR_HANDOFF)
        return real_read(n, **kw)
    s.read_trace = read_trace
    s.sample(BURST, **s.requests())
    assert s.j0 == [0, 0] and s.state.fc_j == BURST and len(s.recoveries) == 1

"""The seams between the two windowed trace products (the reproduction number, the within/between pressure shares) and the
host code they share with every other reader ("The shape of a product on the host"), held to what the library did
before the two were given one shape: a window that changes and comes back starts from zero, bit for bit; the within/between
accumulators travel with a snapshot and are dropped from it by a reset; the blocking and the asynchronous reader of a pair
deliver the same bytes, and refuse with the same code and the same words."""
import dataclasses

import numpy as np
import pytest

from covid19uk_amd import _lib
from covid19uk_amd.sampler import PinnedTrace
from tests.test_groups_gpu import _set
from tests.test_recovery_gpu import _case
from tests.test_rt_device_gpu import _weight
from tests.test_sampler_gpu import api  # noqa: F401  (fixture)
from tests.test_summary_gpu import _sampler

pytestmark = pytest.mark.gpu

NAME, B, CAP, N, T = "micro_20x60", 3, 8, 4, 60
GROUPS = [[0, 1, 2], [19]]
NNZ = 4


def _started(api):
    """The sampler of tests/test_product_state_gpu.py with trace slots [0, N) filled, and the national weights."""
    case, u, ev, cfg, eps = _case(NAME, B)
    model, s = _sampler(api, case, cfg, u, ev, eps, CAP)
    s.sample(N)
    return model, s, _weight(case)


def _fields(summary):
    return {f.name: getattr(summary, f.name) for f in dataclasses.fields(summary)}


def _same(got, want):
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


# product -> (reset at a window, fold slots, everything it leaves: the summary, the per-draw curves, the group curves)
def _rt_read(s):
    return dict(_fields(s.rt_summary()), draws=s.read_rt_draws(N), rt_by_group=s.read_group_rt(N))


def _wb_read(s):
    return dict(_fields(s.within_between_summary()), **s.read_wb_draws(N), **s.read_group_wb(N))


WINDOWS = {
    "rt": (lambda s, w, D: s.reset_rt(D, w), lambda s: s.rt(0, N), _rt_read, lambda s: s.set_group_rt(np.ones(NNZ)),
           ("rt_D", "group_rt_D")),
    "wb": (lambda s, w, D: s.reset_within_between(D), lambda s: s.within_between(0, N), _wb_read,
           lambda s: s.set_group_within_between(True), ("wb_D", "group_wb_D")),
}


@pytest.mark.parametrize("product", WINDOWS)
def test_a_window_comes_back_from_zero(api, product):
    reset, fold, read, group_on, (d_key, gd_key) = WINDOWS[product]
    model, s, w = _started(api)
    with model, s:
        _set(s, GROUPS)
        group_on(s)
        reset(s, w, 6)
        if product == "rt":                                    # the stores sized by the window
            s.keep_rt_draws(CAP)
            s.set_group_ngm(np.ones(NNZ), CAP)
        fold(s)
        A = read(s)
        assert all(int(c) == N for c in A["count"]) and any(np.any(v != 0) for k, v in A.items() if k != "count")
        reset(s, w, 2)
        st = s._state()
        assert (getattr(st, d_key), getattr(st, gd_key)) == (2, 2)
        if product == "rt":                                    # the stores went with the window they were sized by
            assert (st.rt_keep_cap, st.ngm_cap, st.ngm_D, st.rt_j) == (0, 0, 0, 0)
            with pytest.raises(_lib.SeirError, match="the draw store is not enabled: call seir_sampler_rt_keep first") as e:
                s.rt_order_stats([0])
            assert e.value.code == _lib.ERR_STATE
            with pytest.raises(_lib.SeirError, match="the group next-generation matrix is not enabled: call "
                                                     "seir_sampler_group_ngm behind seir_sampler_rt_reset") as e:
                s.read_group_ngm(1)
            assert e.value.code == _lib.ERR_STATE
        fold(s)
        assert all(int(c) == N for c in read(s)["count"])
        reset(s, w, 6)
        st = s._state()
        assert (getattr(st, d_key), getattr(st, gd_key)) == (6, 6)
        fold(s)
        _same(read(s), A)


def test_within_between_travels_with_a_snapshot_and_a_reset_drops_it(api):
    model, s, _ = _started(api)
    with model, s:
        s.reset_within_between(6)
        s.within_between(0, 2)
        s.snapshot(0)
        before = _fields(s.within_between_summary())
        s.within_between(2, 2)
        folded = _fields(s.within_between_summary())
        assert all(int(c) == 4 for c in folded["count"])
        s.restore(0)
        _same(_fields(s.within_between_summary()), before)
        assert all(int(c) == 2 for c in before["count"])
        # a reset behind the snapshot drops what the snapshot held of the product: the restore leaves the accumulators alone
        s.reset_within_between(6)
        s.within_between(1, 3)
        after = _fields(s.within_between_summary())
        assert all(int(c) == 3 for c in after["count"])
        s.restore(0)
        _same(_fields(s.within_between_summary()), after)


def _flat(tr):
    out = dict(theta=tr.theta, events=tr.events, **{"hmc." + k: v for k, v in tr.hmc.items()})
    for mk, mv in tr.moves.items():
        out.update({f"{mk}.{k}": v for k, v in mv.items()})
    return out


def test_blocking_and_asynchronous_readers_deliver_the_same_bytes(api):
    model, s, w = _started(api)
    with model, s:
        D, G, first, n = 3, len(GROUPS), 2, 2
        s.reset_summary()
        s.reset_rt(D, w)
        s.reset_within_between(D)
        _set(s, GROUPS)
        s.set_group_rt(np.ones(NNZ))
        s.set_group_within_between(True)
        s.summarize(0, N)
        s.rt(0, N)
        s.within_between(0, N)
        curves = (G, {"rt_by_group": D, "within_by_group": D, "between_by_group": D})
        buf = PinnedTrace(s, n, events=True, marginals=True, rt=D, wb=D, groups=(G, {"trace": T}), group_curves=curves)

        def poison(arrays):                                    # what is read afterwards was delivered, not left over
            for a in arrays:
                a.view(np.uint8)[...] = 0xA5

        # the trace
        poison([buf.theta, buf.events, buf.hmc, buf.moves])
        s.read_trace_async(n, first, buf)
        s.trace_wait()
        _same(_flat(s.trace_view(buf, n)), _flat(s.read_trace(n, first)))
        # the marginals, the national curves of the two windows, the group sums, the group curves
        pairs = [
            ("marginals", lambda: s.read_marginals_async(n, first, buf), lambda: s.read_marginals(n, first)),
            ("rt", lambda: s.read_rt_draws_async(n, first, buf), lambda: {"rt": s.read_rt_draws(n, first)}),
            ("wb", lambda: s.read_wb_draws_async(n, first, buf), lambda: s.read_wb_draws(n, first)),
            ("groups", lambda: s.read_group_marginals_async("trace", n, first, buf),
             lambda: s.read_group_marginals("trace", n, first)),
            ("group_curves", lambda: s._read_group_curves(curves, n, first, buf), lambda: s._read_group_curves(curves, n, first)),
        ]
        for field, read_async, read in pairs:
            got = getattr(buf, field)
            got = got if isinstance(got, dict) else {field: got}
            poison(got.values())
            read_async()
            s.trace_wait()
            want = read()
            assert any(np.any(v != 0) for v in want.values()), field
            _same({k: got[k] for k in want}, want)
        buf.close()


# pair -> (the blocking entry point; the asynchronous one has _async behind it), what it takes behind (first, count)
READERS = {
    "trace": ("seir_sampler_read_trace", (), (None,) * 4),
    "marginals": ("seir_sampler_read_marginals", (), (None,) * 3),
    "rt_draws": ("seir_sampler_read_rt_draws", (), (None,)),
    "wb_draws": ("seir_sampler_read_wb_draws", (), (None,) * 2),
    "group_marginals": ("seir_sampler_read_group_marginals", (0,), (None,) * 2),
    "group_rt": ("seir_sampler_read_group_rt", (), (None,)),
    "group_wb": ("seir_sampler_read_group_wb", (), (None,) * 2),
}
NO_SUMMARY = "summaries are not enabled: call seir_sampler_summary_reset first"
NO_RT = "the reproduction number is not enabled: call seir_sampler_rt_reset first"
NO_WB = "the within/between pressure shares are not enabled: call seir_sampler_wb_reset first"
NO_TABLE = "no group table is set: call seir_sampler_groups_set first"
NO_GROUP_RT = "group R_t is not enabled: call seir_sampler_group_rt first"
NO_GROUP_WB = "group within/between is not enabled: call seir_sampler_group_wb first"
BEYOND = "trace range [7,9) outside capacity 8"


def test_both_readers_of_a_pair_refuse_alike(api):
    lib = _lib.load()
    model, s, w = _started(api)

    def both(pair, first, count, want):
        name, head, pointers = READERS[pair]
        answers = []
        for fn in (getattr(lib, name), getattr(lib, name + "_async")):
            rc = fn(s._s, *head, first, count, *pointers)
            answers.append((rc, lib.seir_last_error().decode() if rc else ""))
            if rc == 0:
                s.trace_wait()
        assert answers[0] == answers[1] == want, (pair, answers)

    with model, s:
        INV, STATE = _lib.ERR_INVALID, _lib.ERR_STATE
        # nothing is on
        for pair, text in dict(marginals=NO_SUMMARY, rt_draws=NO_RT, wb_draws=NO_WB, group_marginals=NO_TABLE, group_rt=NO_RT,
                               group_wb=NO_WB).items():
            both(pair, 2, 2, (STATE, text))
        # a table, and the source of the group sums is off
        _set(s, GROUPS)
        both("group_marginals", 2, 2, (STATE, NO_SUMMARY))
        # the products are on and no table is set
        s.set_groups(None, None)
        s.reset_summary()
        s.reset_rt(3, w)
        s.reset_within_between(3)
        for pair, text in dict(group_marginals=NO_TABLE, group_rt=NO_GROUP_RT, group_wb=NO_GROUP_WB).items():
            both(pair, 2, 2, (STATE, text))
        # everything is on: a range beyond the capacity
        _set(s, GROUPS)
        s.set_group_rt(np.ones(NNZ))
        s.set_group_within_between(True)
        for pair in READERS:
            both(pair, CAP - 1, 2, (INV, BEYOND))
        # a null destination, behind the range check: refused where there is one plane, nothing to copy where there are two
        for pair in ("rt_draws", "group_rt"):
            both(pair, 2, 2, (INV, "null pointer"))
        for pair in ("trace", "marginals", "wb_draws", "group_marginals", "group_wb"):
            both(pair, 2, 2, (0, ""))

"""The state of the products has one owner, the library (`seir_sampler_product_state`, include/seir_hip.h; DESIGN.md, "Who owns
the product state"): `ChainSampler._state()` is walked through every call that changes it and held to literal values, and
after a reset whose group outputs the library refuses -- done, and answered with an error -- the binding sizes its arrays
for the extent the library has, not for the one before."""
import numpy as np
import pytest

from covid19uk_amd import _lib
from covid19uk_amd.sampler import ProductState
from tests import test_check_gpu as CG
from tests import test_forecast_gpu as FG
from tests.test_groups_gpu import _set
from tests.test_recovery_gpu import _case
from tests.test_rt_device_gpu import _weight
from tests.test_sampler_gpu import api  # noqa: F401  (fixture)
from tests.test_summary_gpu import _sampler

pytestmark = pytest.mark.gpu


def test_the_record_follows_every_call_that_changes_the_state(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 3)
    T, cap, n = 60, 8, 4
    w = _weight(case)
    model, s = _sampler(api, case, cfg, u, ev, eps, cap)
    with model, s:
        want = ProductState()
        assert s._state() == want == ProductState(*([0] * 8 + [(0, 0, 0)] + [0] * 11))         # 1. nothing is on

        def step(call, **changed):
            nonlocal want
            call()
            want = want._replace(**changed)
            assert s._state() == want, (changed, s._state())
        # 2. the resets, the stores, the table and the switches
        step(s.reset_summary, summary_on=1)
        step(lambda: s.reset_diagnostics(2), diag_batch_len=2)
        step(lambda: FG._reset(s, case, 5), forecast_H=5)
        step(lambda: CG._reset(s, case, 4), check_K=4)
        step(lambda: s.reset_rt(3, w), rt_D=3)
        step(lambda: s.reset_within_between(6), wb_D=6)
        step(lambda: s.keep_forecast_draws(cap), fc_keep_cap=8)
        step(lambda: s.keep_rt_draws(cap), rt_keep_cap=8)
        step(lambda: _set(s, [[0, 1, 2], [19]]), groups_G=2, groups_nnz=4, group_L=(T, 5, 4))
        step(lambda: s.set_group_rt(np.ones(4)), group_rt_on=1, group_rt_D=3)
        step(lambda: s.set_group_within_between(True), group_wb_on=1, group_wb_D=6)
        step(lambda: s.set_group_ngm(np.ones(4), cap), ngm_cap=8, ngm_D=3)
        # 3. one kept burst: the counters advance with the calls that fold it
        step(lambda: s.sample(n))
        step(lambda: s.forecast(0, n), fc_j=4)
        step(lambda: s.check(0, n), ck_j=4)
        step(lambda: s.rt(0, n), rt_j=4)
        # 4. a snapshot holds the counters and a restore brings them back
        step(lambda: s.snapshot(0))
        step(lambda: (s.forecast(0, 2), s.check(0, 2), s.rt(0, 2)), fc_j=6, ck_j=6, rt_j=6)
        step(lambda: s.restore(0), fc_j=4, ck_j=4, rt_j=4)
        # 5. a reset behind the snapshot drops what the snapshot holds of the product: the restore leaves its counter alone
        step(lambda: (FG._reset(s, case, 5), CG._reset(s, case, 4), s.reset_rt(3, w)), fc_j=0, ck_j=0, rt_j=0)
        step(lambda: (s.forecast(0, 2), s.check(0, 2), s.rt(0, 2)), fc_j=2, ck_j=2, rt_j=2)
        step(lambda: s.restore(0))
        # 6. another window: the stores sized by it are gone, group R_t is sized again
        step(lambda: s.reset_rt(5, w), rt_D=5, rt_j=0, rt_keep_cap=0, ngm_cap=0, ngm_D=0, group_rt_D=5)
        # 7. another table: group R_t went with the old table's weights, group within / between is sized again
        step(lambda: _set(s, [[0], [1], [2, 3]]), groups_G=3, groups_nnz=4, group_rt_on=0, group_rt_D=0)
        # 8. no table
        step(lambda: s.set_groups(None, None), groups_G=0, groups_nnz=0, group_L=(0, 0, 0), group_wb_on=0, group_wb_D=0)
        assert want == ProductState(summary_on=1, diag_batch_len=2, forecast_H=5, check_K=4, rt_D=5, wb_D=6, fc_j=2, ck_j=2,
                                    fc_keep_cap=8)


# source, also its keyword of sample -> (reset at an extent, enqueue, read, the record's (extent, counter), which, the extent refused)
REFUSED = {
    "forecast": (FG._reset, "forecast", "read_forecast_marginals", ("forecast_H", "fc_j"), 1, 128),
    "check": (CG._reset, "check", "read_check_marginals", ("check_K", "ck_j"), 2, 70),
}


@pytest.mark.parametrize("source", REFUSED)
def test_a_reset_whose_group_outputs_are_refused_leaves_python_and_the_library_agreeing(api, source):
    """2^19 slots x 256 groups, as tests/test_groups_gpu.py: the group outputs fit at an extent of 1 day and are refused at
    128 (forecast) / 70 (check) -- after the source itself was reset to that extent."""
    reset, enqueue, read, (extent_key, j_key), which, L = REFUSED[source]
    case, u, ev, cfg, eps = _case("micro_1x70", 1)
    cap, n = 1 << 19, 4
    model, s = _sampler(api, case, cfg, u, ev, eps, cap)       # the same draws and seed, no table
    with model, s:
        s.sample(n)
        reset(s, case, L)
        getattr(s, enqueue)(0, n)
        want = getattr(s, read)(n)
    model, s = _sampler(api, case, cfg, u, ev, eps, cap)
    with model, s:
        s.sample(n)
        reset(s, case, 1)
        _set(s, [[0]] * _lib.GROUPS_MAX)
        assert s._state().group_L[which] == 1
        with pytest.raises(_lib.SeirError, match="more than half of the") as e:
            reset(s, case, L)
        assert e.value.code == _lib.ERR_INVALID
        st = s._state()
        assert (getattr(st, extent_key), getattr(st, j_key), st.group_L) == (L, 0, (0, 0, 0))
        getattr(s, enqueue)(0, n)
        got = getattr(s, read)(n)
        assert [a.shape for a in got.values()] == [(n, 1, L, 3), (n, 1, 1, 3), (n, 1, L, 3)]
        assert list(got) == list(want) and all(np.array_equal(got[k], want[k]) for k in want)
        assert getattr(s._state(), j_key) == n
        with pytest.raises(ValueError, match="groups needs one of summarize, forecast, check"):
            s.sample(n, groups=True, **{source: True})


def test_a_summary_reset_whose_group_outputs_are_refused_leaves_the_summaries_on(api):
    """The table is set while nothing is on (it needs nothing then); the trace's group outputs, T = 70 days of them, are
    refused by the reset that enables the summaries."""
    case, u, ev, cfg, eps = _case("micro_1x70", 1)
    cap, n = 1 << 19, 4
    model, s = _sampler(api, case, cfg, u, ev, eps, cap)       # the same draws and seed, no table
    with model, s:
        want = s.sample(n, summarize=True)
    model, s = _sampler(api, case, cfg, u, ev, eps, cap)
    with model, s:
        s.sample(n)
        _set(s, [[0]] * _lib.GROUPS_MAX)
        with pytest.raises(_lib.SeirError, match="more than half of the") as e:
            s.reset_summary()
        assert e.value.code == _lib.ERR_INVALID
        st = s._state()
        assert (st.summary_on, st.groups_G, st.group_L) == (1, _lib.GROUPS_MAX, (0, 0, 0))
        s.summarize(0, n)
        got = s.read_marginals(n)
        assert [a.shape for a in got.values()] == [(n, 1, 70, 3), (n, 1, 1, 3), (n, 1, 70, 3)]
        assert all(np.array_equal(got[k], want.marginals[k]) for k in want.marginals)
        with pytest.raises(ValueError, match="groups needs one of summarize, forecast, check"):
            s.sample(n, summarize=True, groups=True)
        tr = s.sample(n, summarize=True)                       # on, and not reset again: nothing is refused
        assert np.array_equal(tr.marginals["events_by_day"], tr.events.astype(np.int64).sum(axis=2))

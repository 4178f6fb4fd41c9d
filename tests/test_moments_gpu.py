"""The three users of the device's moment accumulators at once (covid19uk_amd/csrc/seir_hip.hip, MomentAcc): the summaries,
the convergence diagnostics and the forecast all enabled, their three shadows alive in ONE snapshot slot, and a burst that
is run a second time from that snapshot.

After the second run every accumulator, mark, count and marginal is the first run's (a burst that is run again is counted
once: the forecast's count is n, not 2n), and the moments are the NumPy restatement on the recorded events with the oracles
of tests/test_summary_gpu.py, tests/test_diagnostics_gpu.py and tests/test_forecast_gpu.py.  Integer arithmetic on both
sides: every comparison is `np.array_equal`.

The shapes are the smallest at which each branch of the fold turns: one day chunk exactly with one row past the 8-row block
(uint16 trace), one day past a chunk with one row short of the block (int32 trace); a horizon of one day and one of 65, which
takes the forecast's fold and finish through a second 64-day chunk.  n = 8 draws in batches of L = 3 leave one batch open."""
import numpy as np
import pytest

from covid19uk_amd import synth
from tests import helpers as H
from tests import test_forecast_gpu as tf
from tests.test_diagnostics_gpu import _equals_numpy
from tests.test_diagnostics_host import same_accumulators
from tests.test_sampler_gpu import CFG_SMALL, api  # noqa: F401  (fixture)
from tests.test_summary_gpu import CASES, MARG, _oracle, _same_marginals, _same_moments, _sampler

pytestmark = pytest.mark.gpu

N, L = 8, 3
# name, B, record: the step sizes are the ones tests/test_summary_gpu.py's CASES pairs with these shapes
SHAPES = {"T=64,M=rowblock+1,u16": ("micro_9x64", 3, "u16"), "T=65,M=rowblock-1,int32": ("micro_7x65", 2, True)}
EPS = {name: eps for name, _, eps, *_ in CASES.values()}


def _burst(s):
    """One burst with all three users, mark 0 behind it, and everything they hold."""
    tr = s.sample(N, summarize=True, forecast=True)
    s.mark(0)
    return tr, s.diagnostics(), s.forecast_summary()


@pytest.mark.parametrize("Hn", [1, 65])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_burst_run_again_from_a_snapshot_with_all_three_users_is_counted_once(api, shape, Hn):
    name, B, record = SHAPES[shape]
    case = H.build_case(name, 43, alpha_t_sd=0.005)
    u = synth.jitter_params(case["u"], B, scale=0.01, seed=3, T=case["k"].T)
    ev = np.stack([case["events"]] * B)
    # auto_recover=False: the only snapshots are the ones taken here
    model, s = _sampler(api, case, CFG_SMALL, u, ev, EPS[name], N, record_events=record, auto_recover=False)
    with model, s:
        for slot in (0, 1):
            s.reset_diagnostics(L)
            tf._reset(s, case, Hn)
            s.snapshot(slot)
            tr, dg, fc = _burst(s)
            s.restore(slot)
            tr2, dg2, fc2 = _burst(s)

            assert tr.events.dtype == (np.uint16 if record == "u16" else np.int32)
            assert (tr.events != tr.events[:1]).any(), "no event update was accepted: all draws equal"
            assert np.array_equal(tr2.events, tr.events) and np.array_equal(tr2.theta, tr.theta)
            # the second run left what the first did
            same_accumulators(dg2, dg)
            tf._same_forecast((fc2, tr2.forecast), (fc, tr.forecast))
            for k in MARG:
                assert np.array_equal(tr2.marginals[k], tr.marginals[k]), k
            assert np.array_equal(fc2.count, np.full(B, N)) and np.array_equal(dg2.count, np.full(B, N))
            assert np.array_equal(dg2.mark_count, [[N] * B, [0] * B]) and np.array_equal(dg2.nbatch, np.full(B, N // L))
            # and that is the restatement on the recorded events
            want = _oracle(tr2.events, case["init"])
            _same_moments(s.summary(), want)
            _same_marginals(tr2.marginals, want)
            _equals_numpy(dg2, tr2.events, case["init"], L, {N: 0})
            assert dg2.bsum.any(), "the open batch holds nothing"
            fwant = tf._oracle(model, case, tr2.theta, tr2.events, Hn)
            tf._moved(fwant, fc2)
            tf._same_moments(fc2, fwant)
            tf._same_marginals(tr2.forecast, fwant)
        assert not s.pair_timeouts().any()

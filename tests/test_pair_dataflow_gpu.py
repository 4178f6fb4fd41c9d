"""Steps of k_move_pairs that overtake each other.  The band workgroups of the persistent pair launch take no part in the
roles' step barrier: what they leave for the next step (their partial sums, and F with the step's band applied) travels as
hand-off words, and a band workgroup goes on to its next step on its own.  `debug_skew` delays workgroups only at the
start of a launch, which says nothing about step 3 against step 2 inside one; the hooks used here (further bits of
seir_sampler_desc::debug_pair, delays only) sleep ~30 us at the entry of EVERY step in the band workgroups (16), role 0 (32),
roles 1 and 2 (64) or a third of all workgroups drawn again per step (128).  A stale L1 line, a torn word or an overtaken
buffer shows as a difference in the bits: 100 sweeps under each hook must reproduce the undisturbed run exactly, with no
wait timed out (a fatal time-out makes the read of the trace fail; the benign ones are counted) -- and both accept
branches of every update kind must have been taken, so that the test cannot pass on chains that never accept."""
import hashlib

import numpy as np
import pytest

from covid19uk_amd import synth
from tests import helpers as H

pytestmark = pytest.mark.gpu

CFG_NI = dict(dmax=10, nmax=5, m=2, occult_nmax=5, num_event_time_updates=3)
CFG_UK = dict(dmax=84, nmax=25, m=2, occult_nmax=15, num_event_time_updates=5)
HOOKS = (16, 32, 64, 128)
N, BURST = 100, 25


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as entry
    entry.build()
    from covid19uk_amd.seir import SeirModel
    from covid19uk_amd.sampler import ChainSampler
    return SeirModel, ChainSampler


def _run(api, case, cfg, B, eps, u, ev, dbg):
    """100 sweeps in bursts of 25: the small trace columns whole, the event trace as a digest per burst (UK-380 x 16
    records 0.67 GB per burst), the final state whole."""
    SeirModel, ChainSampler = api
    cols, digests = [], []
    with SeirModel(case["cov"], case["init"], max_chains=B) as model:
        with ChainSampler(model, cfg, B, seed=91, trace_capacity=BURST, moves="paired", debug_pair=dbg) as s:
            if not s.xcd_local():
                pytest.skip("this GPU does not place block ids congruent mod 8 on one XCD: the fused form is not used")
            assert s.launch_form()[1] == "paired", s.launch_form()
            s.set_state(u, ev)
            s.set_kernel(step_size=eps)
            for _ in range(N // BURST):
                s.reset_trace()
                s.run(BURST)
                tr = s.read_trace(BURST)               # raises if a wait that cannot be recovered from timed out
                digests.append(hashlib.sha256(np.ascontiguousarray(tr.events).tobytes()).hexdigest())
                cols.append((tr.theta, tr.hmc, tr.moves))
            late = s.pair_timeouts()
            state = s.get_state()
    return cols, digests, state, late


@pytest.mark.parametrize("name,B,cfg,eps", [("uk380", 8, CFG_UK, 1.2e-5), ("uk380", 16, CFG_UK, 1.2e-5),
                                            ("uk380", 3, CFG_UK, 1.2e-5), ("ni11", 5, CFG_NI, 0.02)])
def test_delayed_steps_of_the_pair_launch_give_the_same_bits(api, name, B, cfg, eps):
    case = H.build_case(name, 41)
    u = synth.jitter_params(case["u"], B, scale=0.01 if name == "ni11" else 0.002, seed=5, T=case["k"].T)
    ev = np.stack([case["events"]] * B)
    base_cols, base_dig, base_state, base_late = _run(api, case, cfg, B, eps, u, ev, 0)
    assert not base_late.any()
    # both branches of every update kind, or the comparison below proves little
    for mk in base_cols[0][2]:
        acc = np.concatenate([c[2][mk]["is_accepted"] for c in base_cols])
        print(f"{name} x {B} {mk}: accepted {int(acc.sum())} of {acc.size}")
        assert acc.any() and not acc.all(), (mk, int(acc.sum()), acc.size)
    for hook in HOOKS:
        cols, dig, state, late = _run(api, case, cfg, B, eps, u, ev, hook)
        assert not late.any(), (hook, late)
        assert dig == base_dig, (hook, "event trace")
        for (theta, hmc, moves), (theta0, hmc0, moves0) in zip(cols, base_cols):
            assert np.array_equal(theta, theta0), (hook, "theta")
            for k in hmc0:
                assert np.array_equal(hmc[k], hmc0[k]), (hook, "hmc", k)
            for mk in moves0:
                for k in moves0[mk]:
                    assert np.array_equal(moves[mk][k], moves0[mk][k]), (hook, mk, k)
        for a, a0 in zip(state, base_state):
            assert np.array_equal(np.asarray(a), np.asarray(a0)), (hook, "state")

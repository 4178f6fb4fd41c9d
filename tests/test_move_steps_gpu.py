"""The three launch forms of the event updates on the same chains -- "paired" (k_move_pairs: every pair of a sweep in one
persistent launch), "paired-launch" (k_move_pair: one launch per pair) and "split" (k_move_pa2 + k_move_delta per update) --
after per-step work left the pair launches: no prefetch iterations for rows beyond M, the row of an own-rows cell by
compares instead of a division, the band's rows per workgroup from the host.  None of it may move a bit: move trace,
events, theta and the final state of 30 sweeps must be equal in all three forms (the split form shares neither pair_step nor the band workgroups with the other two), at

  * 17 and 33 rows x 65 days, m = 1 and 2: M <= 512, one prefetched row per thread; one band workgroup, and two plus a rest;
  * 520 rows x 130 days, m = 2: M > 512, the prefetch iterations k >= 1 run; band workgroups of four rows per wave;
  * 17 rows, m = 3 and 4: the `_m4` instances.

Every case's own trace must show each update kind accepted and rejected and, where m >= 2, an E->I-type event-time update
with two windows (with m = 1 there is one window and no row to find: tests/test_move_steps_host.py, where the seeds are
held to the C oracle).  A persistent launch after a restore of the sampler starts from nothing an earlier launch left in
the workgroups: the sweeps run a second time from a snapshot give the bits of the first time."""
import numpy as np
import pytest

from covid19uk_amd import _lib
from tests import move_steps_lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as entry
    entry.build()
    from covid19uk_amd.seir import SeirModel
    from covid19uk_amd.sampler import ChainSampler
    return SeirModel, ChainSampler


def _bits(s, n):
    tr = s.read_trace(n)
    return dict(theta=tr.theta.tobytes(), events=np.ascontiguousarray(tr.events).tobytes(),
                hmc=b"".join(np.ascontiguousarray(tr.hmc[k]).tobytes() for k in sorted(tr.hmc)),
                columns=s.read_move_columns(n).tobytes(), state=b"".join(np.ascontiguousarray(a).tobytes() for a in s.get_state())), tr


def _run(api, case_id, moves, again=False):
    SeirModel, ChainSampler = api
    name, m, B, eps, seed = L.CASES[case_id]
    case, u, ev = L.start(case_id)
    n = L.N_SWEEPS
    with SeirModel(case["cov"], case["init"], max_chains=B) as model:
        with ChainSampler(model, L.config(case_id), B, seed=seed, first_chain_id=L.FIRST_CHAIN, trace_capacity=n, moves=moves,
                          log=None, auto_recover=False) as s:
            if moves == "paired" and not s.xcd_local():
                pytest.skip("this GPU does not place block ids congruent mod 8 on one XCD: no persistent pair launch")
            assert s.move_instance() == (_lib.MM_SMALL if m <= 2 else _lib.MMAX)
            plan = s.sweep_plan()
            s.set_state(u, ev)
            s.set_kernel(step_size=eps)
            s.snapshot(0)
            s.reset_trace()
            s.run(n)
            bits, tr = _bits(s, n)
            assert s.launch_form()[1] == moves, "the run fell back to another launch form"
            bits2 = None
            if again:                                        # the same sweeps once more, from the snapshot
                s.restore(0)
                s.reset_trace()
                s.run(n)
                bits2, _ = _bits(s, n)
            assert not s.pair_timeouts().any()
    return bits, tr, plan, bits2


@pytest.mark.parametrize("case_id", sorted(L.CASES))
def test_the_three_launch_forms_give_the_same_bits(api, case_id):
    name, m, B, eps, seed = L.CASES[case_id]
    M, T = (int(v) for v in name.split("_")[1].split("x"))
    paired, tr, plan, paired2 = _run(api, case_id, "paired", again=True)
    # the case runs what it is there for: the persistent launch with band workgroups, of the shape the size asks for
    nband = (M + 15) // 16 if M <= 512 else (M + 31) // 32
    assert (plan["moves"], plan["fpend"], plan["nband"]) == ("pairs", "k_move_pairs", nband), plan
    acc = np.stack([tr.moves[k]["is_accepted"] for k in L.MOVE_KEYS], axis=-1)
    prop = np.stack([tr.moves[k]["proposed_delta"] for k in L.MOVE_KEYS], axis=2)
    two = L.two_windows(prop, T)
    print(case_id, "accepted of", L.N_SWEEPS * B, ":", dict(zip(L.MOVE_KEYS, acc.reshape(-1, 4).sum(axis=0))),
          "E->I-type proposals with two windows:", two, "HMC accepted:", int(tr.hmc["is_accepted"].sum()))
    assert L.both_ways(acc), "an update kind was never accepted, or never rejected"
    assert (two > 0) == (m >= 2)
    assert tr.hmc["is_accepted"].any()
    for k in paired:
        assert paired2[k] == paired[k], ("after a restore", k)
    for moves in ("paired-launch", "split"):
        other, _, oplan, _ = _run(api, case_id, moves)
        assert oplan["moves"] == ("pair" if moves == "paired-launch" else "split"), oplan
        for k in paired:
            assert other[k] == paired[k], (moves, k)

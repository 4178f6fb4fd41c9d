"""The event-update instances for m <= 2 (the kernels' plain names) against the ones for every m (`_m4`, forced by
SEIR_OPT_GENERIC_MOVES) on the same chains: the same code with its sub-move loops cut at 2 instead of 4 must give the
same bits -- theta, the events, and every column of the move trace, the columns of the sub-moves that do not exist
included.  30 sweeps per case (tests/move_instances_lib.py: the sizes, and seeds chosen on the C oracle so that every
update kind is accepted and rejected along the way)."""
import numpy as np
import pytest

from covid19uk_amd import _lib
from tests import move_instances_lib as L

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


def _run(api, case_id, generic):
    SeirModel, ChainSampler = api
    name, cfg, B, moves, eps, seed = L.CASES[case_id]
    case, u, ev = L.start(case_id)
    n = L.N_SWEEPS
    with SeirModel(case["cov"], case["init"], max_chains=B) as model:
        model.set_option(generic_moves=generic)
        with ChainSampler(model, cfg, B, seed=seed, first_chain_id=L.FIRST_CHAIN, trace_capacity=n, moves=moves, log=None) as s:
            assert s.move_instance() == (_lib.MMAX if generic else _lib.MM_SMALL)
            plan = s.sweep_plan()
            s.set_state(u, ev)
            s.set_kernel(step_size=eps)
            tr = s.sample(n)
            cols = s.read_move_columns(n)
            assert s.launch_form()[1] == moves, "the run fell back to another launch form"
    return tr, cols, plan


@pytest.mark.parametrize("case_id", sorted(L.CASES))
def test_small_and_generic_instances_give_the_same_bits(api, case_id):
    name, cfg, B, moves, eps, seed = L.CASES[case_id]
    small, cols_s, plan_s = _run(api, case_id, generic=False)
    generic, cols_g, plan_g = _run(api, case_id, generic=True)
    assert plan_s == plan_g                                   # the instance is no part of the plan: the same launches
    if B == 8:
        # the eight-chain cases are there for the persistent pair launch with its band workgroups, and for the same chains
        # by one launch per pair
        want = dict(moves="pairs", fpend="k_move_pairs") if moves == "paired" else dict(moves="pair")
        assert {k: plan_s[k] for k in want} == want and plan_s["nband"] > 0, plan_s
    assert small.theta.tobytes() == generic.theta.tobytes()
    assert np.array_equal(small.events, generic.events)
    for k in ("is_accepted", "target_log_prob", "step_size"):
        assert small.hmc[k].tobytes() == generic.hmc[k].tobytes(), k
    assert cols_s.shape == (L.N_SWEEPS, B, 4, _lib.MOVE_TRACE)
    assert cols_s.tobytes() == cols_g.tobytes()
    for i, key in enumerate(L.MOVE_KEYS):
        assert np.array_equal(small.moves[key]["proposed_delta"], generic.moves[key]["proposed_delta"]), key
        # the columns of the sub-moves beyond m: zeros, +0.0 bit for bit, from either set of instances
        beyond = cols_s[:, :, i, 2:].reshape(L.N_SWEEPS, B, 4, _lib.MMAX)[..., cfg["m"]:]
        assert beyond.size > 0 and not beyond.view(np.uint64).any(), key
    acc = np.stack([small.moves[k]["is_accepted"] for k in L.MOVE_KEYS], axis=-1)
    print(case_id, "accepted of", L.N_SWEEPS * B, ":", dict(zip(L.MOVE_KEYS, acc.reshape(-1, 4).sum(axis=0))))
    assert L.both_ways(acc), "an update kind was never accepted, or never rejected"
    assert small.hmc["is_accepted"].any()


@pytest.mark.parametrize("m", [3, 4])
def test_more_than_two_sub_moves_run_the_generic_instances(api, m):
    """m = 3, 4 have no instances of their own (tests/test_sampler_gpu.py and tests/test_mcmc_oracle.py hold them to the
    oracle): the sampler says so, with or without the option."""
    SeirModel, ChainSampler = api
    case, u, ev = L.start("micro_5x24-m2")
    with SeirModel(case["cov"], case["init"], max_chains=1) as model:
        with ChainSampler(model, dict(L.CFG_SMALL, m=m), 1, seed=1, trace_capacity=2, log=None) as s:
            assert s.move_instance() == _lib.MMAX
            model.set_option(generic_moves=True)
            assert s.move_instance() == _lib.MMAX
            model.set_option(generic_moves=False)
            s.set_state(u, ev)
            s.set_kernel(step_size=0.002)
            tr = s.sample(2)
            assert tr.moves["move/S->E"]["proposed_delta"].shape[-1] == m

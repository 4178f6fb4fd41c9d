"""An E->I-type update's log-ratio inside the pair launches at the shapes where its two parts can go wrong -- tests/move_eval_lib.py
lists them -- in the three launch forms of the event updates on the same chains: "paired" (k_move_pairs, every pair of a sweep in
one launch), "paired-launch" (k_move_pair, one launch per pair) and "split" (k_move_pa2 / k_move_delta<true>).  The roles of the
pair launches evaluate the updated rows' part with the proposal's target fixed at compile time and a thread's second item
loaded ahead of its first item's arithmetic (own_rows_delta<NT, MM, TGT>, covid19uk_amd/csrc/sampler_kernels.h); the split form
reads the target from the descriptor.  The band workgroups (pair_band_block) walk the hull in 64-day pieces; k_move_delta walks
it day by day.  The move trace rows, the events and the chains' state after 40 sweeps, bit for bit; and each case's own trace
must show what the case is there for (a window of exactly 64, 65, 128 or 129 days; two windows in pieces 0 and 2 of a
three-piece hull; a hull that ends in the one day of a second 64-day chunk)."""
import numpy as np
import pytest

from tests import move_eval_lib as L

pytestmark = pytest.mark.gpu

FORMS = ("paired", "paired-launch", "split")


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as entry
    entry.build()
    from covid19uk_amd.seir import SeirModel
    from covid19uk_amd.sampler import ChainSampler
    return SeirModel, ChainSampler


def _run(api, case_id, moves):
    SeirModel, ChainSampler = api
    name, cfg, B, eps, seed, want = L.CASES[case_id]
    case, u, ev = L.start(case_id)
    n = L.N_SWEEPS
    with SeirModel(case["cov"], case["init"], max_chains=B) as model:
        with ChainSampler(model, cfg, B, seed=seed, first_chain_id=L.FIRST_CHAIN, trace_capacity=n, moves=moves, log=None) as s:
            if moves != "split" and not s.xcd_local():
                pytest.skip("this GPU does not place block ids congruent mod 8 on one XCD: no band workgroups in the pair launch")
            plan = s.sweep_plan()
            s.set_state(u, ev)
            s.set_kernel(step_size=eps)
            tr = s.sample(n)
            cols = s.read_move_columns(n)
            state = s.get_state()
            assert not s.pair_timeouts().any()
            assert s.launch_form()[1] == moves, "the run fell back to another launch form"
    return tr, cols, state, plan, case["k"].T


def _bits_differ(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    return int((a.view(np.uint8) != b.view(np.uint8)).reshape(a.size, -1).any(axis=1).sum()) if a.size else 0


@pytest.mark.parametrize("case_id", sorted(L.CASES))
def test_the_three_launch_forms_give_the_same_bits(api, case_id):
    name, cfg, B, eps, seed, want = L.CASES[case_id]
    out = {f: _run(api, case_id, f) for f in FORMS}
    tr, cols, state, plan, T = out["paired"]
    # the forms that were asked for are the ones that ran, with band workgroups inside the pair launches
    M = tr.events.shape[2]
    assert plan["moves"] == "pairs" and plan["fpend"] == "k_move_pairs" and plan["nband"] == (M + 15) // 16, plan
    assert out["paired-launch"][3]["moves"] == "pair" and out["paired-launch"][3]["nband"] == plan["nband"]
    assert out["split"][3]["moves"] == "split" and out["split"][3]["nband"] == 0
    # what the recorded E->I-type updates were: the case's reason to exist, shown by the run's own trace
    ups = L.recorded_updates(L.move_columns_as_delta(cols, cfg["m"]), T, cfg["m"])
    seen = L.shows(want, ups)
    acc = np.stack([tr.moves[k]["is_accepted"] for k in L.MOVE_KEYS], axis=-1).reshape(-1, 4)
    print(case_id, "recorded E->I-type updates with a band:", len(ups), "showing", want, ":", seen, "| hull pieces:",
          np.bincount([u[4] for u in ups], minlength=4), "| accepted of", len(acc), ":", acc.sum(axis=0))
    # every figure before any assertion: elements whose bits differ from the "paired" run's
    diffs = {}
    for f in FORMS[1:]:
        t2, c2, s2 = out[f][:3]
        diffs[f] = dict(events=_bits_differ(tr.events, t2.events), rows=_bits_differ(cols, c2), theta=_bits_differ(tr.theta, t2.theta),
                        hmc_lp=_bits_differ(tr.hmc["target_log_prob"], t2.hmc["target_log_prob"]),
                        state_u=_bits_differ(state[0], s2[0]), state_events=_bits_differ(state[1], s2[1]), state_lp=_bits_differ(state[2], s2[2]))
        worst = max((float(np.max(np.abs(tr.moves[k]["target_log_prob"] - t2.moves[k]["target_log_prob"]) /
                                  np.abs(tr.moves[k]["target_log_prob"]))) for k in L.MOVE_KEYS))
        print("  ", f, "against paired, elements with other bits:", diffs[f], "| largest relative difference of a move's target_log_prob:", worst)
        for at in np.argwhere(cols.view(np.uint64) != c2.view(np.uint64))[:8]:      # (sweep, chain, update kind, column)
            print("     row element", tuple(int(v) for v in at), ":", float(cols[tuple(at)]).hex(), "|", float(c2[tuple(at)]).hex())
    assert seen > 0, (want, len(ups))
    assert acc[:, 1].any() and not acc[:, 1].all(), "the E->I-type event-time update was never accepted, or never rejected"
    for f in FORMS[1:]:
        assert not any(diffs[f].values()), (f, diffs[f])

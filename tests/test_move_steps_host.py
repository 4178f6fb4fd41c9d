"""The seeds of tests/test_move_steps_gpu.py do what they were chosen for, on the C oracle and without a GPU
(tests/move_steps_lib.py): in the 30 sweeps of every case each of the four update kinds is accepted and rejected, HMC is
accepted at least once (psi, a constant of a k_move_pairs launch, differs from launch to launch), and where m >= 2
E->I-type event-time updates with two windows are proposed -- the only ones whose own-rows cells have a row to find (with
m = 1 there is one window, and cell_row's compares are all false by n = 1)."""
import pytest

from tests import move_steps_lib as L


@pytest.mark.parametrize("case_id", sorted(L.CASES))
def test_the_gpu_cases_seeds_take_every_branch_on_the_oracle(case_id):
    name, m, B, eps, seed = L.CASES[case_id]
    T = int(name.split("x")[1])
    acc, prop, hmc = L.oracle_run(case_id)
    two = L.two_windows(prop, T)
    print(case_id, "accepted of", acc.shape[0] * acc.shape[1], ":", dict(zip(L.MOVE_KEYS, acc.reshape(-1, 4).sum(axis=0))),
          "E->I-type proposals with two windows:", two, "HMC accepted:", int(hmc.sum()))
    assert L.both_ways(acc)
    assert hmc.any()
    assert (two > 0) == (m >= 2)

"""What tests/test_move_instances_gpu.py and tests/test_move_instances_host.py share: the cases at which the event-update
instances for m <= 2 (the kernels' plain names) are held to the ones for every m (`_m4`), and the C oracle's account of
which update kinds such a run accepts and rejects -- the seeds below were chosen on it (CPU), so that in every case each of
the four kinds is both accepted and rejected at least once in the sweeps the trace keeps."""
import numpy as np

from covid19uk_amd import synth
from oracle import c_binding
from tests import helpers as H

N_SWEEPS = 30
MOVE_KEYS = ("move/S->E", "move/E->I", "occult/S->E", "occult/E->I")
CFG_SMALL = dict(dmax=8, nmax=6, m=2, occult_nmax=5, num_event_time_updates=3)
CFG_NI = dict(dmax=10, nmax=5, m=2, occult_nmax=5, num_event_time_updates=3)

# id -> (workload, Mcmc configuration, chains, launch form of the event updates, step size, sampler seed)
CASES = {
    "micro_5x24-m1": ("micro_5x24", dict(CFG_SMALL, m=1), 1, "paired", 0.002, 1),
    "micro_5x24-m2": ("micro_5x24", CFG_SMALL, 1, "paired", 0.002, 1),
    # more updates per row than rows
    "micro_3x70-m2": ("micro_3x70", dict(dmax=84, nmax=25, m=2, occult_nmax=15, num_event_time_updates=4), 1, "paired", 0.001, 1),
    # eight chains: the persistent pair launch with band workgroups, and the same chains one launch per pair
    "ni11x8-paired": ("ni11", CFG_NI, 8, "paired", 0.002, 1),
    "ni11x8-paired-launch": ("ni11", CFG_NI, 8, "paired-launch", 0.002, 1),
}
CASE_SEED = 23          # the workload's epidemic and the chains' starting points
FIRST_CHAIN = 3


def start(case_id):
    name, cfg, B, moves, eps, seed = CASES[case_id]
    case = H.build_case(name, CASE_SEED, alpha_t_sd=0.005)
    u = synth.jitter_params(case["u"], B, scale=0.05, seed=CASE_SEED, T=case["k"].T)
    ev = np.stack([case["events"]] * B)
    return case, u, ev


def oracle_decisions(case_id, seed=None):
    """[N_SWEEPS, B, 4] accept flags of the updates the trace keeps (the last scan's), from the C oracle."""
    name, cfg, B, moves, eps, seed0 = CASES[case_id]
    case, u, ev = start(case_id)
    acc = np.zeros((N_SWEEPS, B, 4), dtype=bool)
    for b in range(B):
        ch = c_binding.COracleChain(case["k"], cfg, u[b], ev[b], seed=seed0 if seed is None else seed, chain_id=FIRST_CHAIN + b)
        ch.eps = eps
        for i in range(N_SWEEPS):
            o = ch.sweep_once()
            acc[i, b] = [o[k]["is_accepted"] for k in MOVE_KEYS]
    return acc


def both_ways(acc):
    """Every update kind accepted at least once and rejected at least once."""
    flat = acc.reshape(-1, 4)
    return bool(flat.any(axis=0).all() and (~flat).any(axis=0).all())

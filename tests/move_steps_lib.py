"""What tests/test_move_steps_gpu.py and tests/test_move_steps_host.py share: the cases at which the three launch forms of
the event updates are held to each other after per-step work left the pair launches (row prefetch beyond M, the row of an
own-rows cell, the band's shape), and the C oracle's account of what such a run proposes,
accepts and rejects -- the seeds below were chosen on it (CPU), so that in every case each of the four update kinds is both
accepted and rejected, HMC moves theta (and psi with it) between launches, and (m >= 2) an E->I-type event-time update with two windows is
evaluated: the only proposals whose cells have a row to find."""
import numpy as np

from covid19uk_amd import synth
from oracle import c_binding
from tests import helpers as H

N_SWEEPS = 30
MOVE_KEYS = ("move/S->E", "move/E->I", "occult/S->E", "occult/E->I")
FORMS = ("paired", "paired-launch", "split")
CFG = dict(dmax=8, nmax=6, m=2, occult_nmax=5, num_event_time_updates=3)

# id -> (workload, m, chains, step size, sampler seed)
#   17 and 33 rows x 65 days: M <= 512 -- one prefetched row per thread; one band workgroup of 16 rows, two of them plus a rest
#   520 rows x 130 days: M > 512 -- the prefetch iterations k >= 1 run; 17 band workgroups of 31 rows, four rows per wave
#   m = 3, 4: the `_m4` instances (cell_row<MMAX>)
CASES = {
    "17x65-m1": ("micro_17x65", 1, 2, 0.0005, 1),
    "17x65-m2": ("micro_17x65", 2, 2, 0.0005, 1),
    "33x65-m1": ("micro_33x65", 1, 2, 0.0001, 1),
    "33x65-m2": ("micro_33x65", 2, 2, 0.0001, 1),
    "520x130-m2": ("slow_520x130", 2, 1, 0.0002, 1),
    "17x65-m3": ("micro_17x65", 3, 2, 0.0005, 1),
    "17x65-m4": ("micro_17x65", 4, 2, 0.0005, 1),
}
CASE_SEED = 23          # the workload's epidemic and the chains' starting points
FIRST_CHAIN = 3


def config(case_id):
    return dict(CFG, m=CASES[case_id][1])


def start(case_id):
    name, m, B, eps, seed = CASES[case_id]
    case = H.build_case(name, CASE_SEED, alpha_t_sd=0.005)
    u = synth.jitter_params(case["u"], B, scale=0.05, seed=CASE_SEED, T=case["k"].T)
    ev = np.stack([case["events"]] * B)
    return case, u, ev


def oracle_run(case_id, seed=None):
    """From the C oracle: [N_SWEEPS, B, 4] accept flags, [N_SWEEPS, B, 4, 4, m] proposals (m, t, delta_t, x per sub-move)
    and [N_SWEEPS, B] HMC accept flags of the updates the trace keeps (the last scan's)."""
    name, m, B, eps, seed0 = CASES[case_id]
    case, u, ev = start(case_id)
    acc = np.zeros((N_SWEEPS, B, 4), dtype=bool)
    prop = np.zeros((N_SWEEPS, B, 4, 4, m), dtype=np.int64)
    hmc = np.zeros((N_SWEEPS, B), dtype=bool)
    for b in range(B):
        ch = c_binding.COracleChain(case["k"], config(case_id), u[b], ev[b], seed=seed0 if seed is None else seed,
                                    chain_id=FIRST_CHAIN + b)
        ch.eps = eps
        for i in range(N_SWEEPS):
            o = ch.sweep_once()
            acc[i, b] = [o[k]["is_accepted"] for k in MOVE_KEYS]
            prop[i, b] = [o[k]["proposed_delta"] for k in MOVE_KEYS]
            hmc[i, b] = o["hmc"]["is_accepted"]
    return acc, prop, hmc


def both_ways(acc):
    """Every update kind accepted at least once and rejected at least once."""
    flat = acc.reshape(-1, 4)
    return bool(flat.any(axis=0).all() and (~flat).any(axis=0).all())


def two_windows(prop, T):
    """E->I-type event-time updates whose first two sub-moves were both drawn and both land inside the series: n >= 2
    windows, the proposals own_rows_delta enumerates row by row.  prop: [..., 4 kinds, 4 columns, m] (a sub-move that was
    not drawn has delta_t == 0; a drawn one never has)."""
    if prop.shape[-1] < 2:
        return 0
    t, dt = prop[..., 1, 1, :2], prop[..., 1, 2, :2]
    inside = (dt != 0) & (t + dt >= 0) & (t + dt < T)
    return int(inside.all(axis=-1).sum())

"""What tests/test_move_eval_gpu.py runs: the shapes at which the two parts of an E->I-type update's log-ratio can go wrong --
the band workgroups' walk over the proposal's hull in 64-day pieces (pair_band_block, covid19uk_amd/csrc/moves_kernel.h) and the
updated rows' part, whose cells are spread over the threads as one or two items each (own_rows_delta, sampler_kernels.h) -- and
the account, from a run's own move trace, of the windows and pieces its recorded E->I-type updates had.  The seeds were chosen on
the C oracle (CPU), so that the recorded updates of each case show what the case is there for."""
import numpy as np

from covid19uk_amd import _lib, synth
from tests import helpers as H

PIECE = 64
N_SWEEPS = 40
CASE_SEED = 29
FIRST_CHAIN = 2
MOVE_KEYS = ("move/S->E", "move/E->I", "occult/S->E", "occult/E->I")

# id -> (workload, Mcmc configuration, chains, step size, sampler seed, what the recorded updates must show)
#   ("window", d): an E->I-type event-time sub-move that moves events by exactly d days -- a window of d days
#   ("skip",): two sub-moves whose windows lie in pieces 0 and 2 of a three-piece hull: no day of piece 1 changes
#   ("pieces", k): a hull of k pieces
#   ("reach", t): a hull that ends on day t (T = 65: the one day of the series' second 64-day chunk)
# T = 130: three pieces, a pair and an odd one; T = 64 / 65: one piece / a second piece of one day.  M = 17 / 33: the last band
# workgroup (16 rows each) holds one row -- a part-filled wave -- and with so few rows the proposal's own rows are among a
# band workgroup's in every step.  3 and 5 chains: the 8-chain layout with chains that do not exist.  Windows of 64 days and more
# with m = 2: more than 170 cells of the updated rows, so that a thread of the pair launch holds two items (3 x cells > 512);
# 128 and 129 days: more than 341 cells, every thread takes whole cells in passes.
CASES = {
    "T130-M17-m2-b8-d64": ("slow_17x130", dict(dmax=64, nmax=25, m=2, occult_nmax=15, num_event_time_updates=3), 8, 2e-4, 12, ("window", 64)),
    "T130-M33-m2-b8-d65": ("slow_33x130", dict(dmax=65, nmax=25, m=2, occult_nmax=15, num_event_time_updates=3), 8, 2e-4, 23, ("window", 65)),
    "T192-M17-m2-b5-d128": ("slow_17x192", dict(dmax=128, nmax=25, m=2, occult_nmax=15, num_event_time_updates=3), 5, 2e-4, 2, ("window", 128)),
    "T192-M33-m2-b8-d129": ("slow_33x192", dict(dmax=129, nmax=25, m=2, occult_nmax=15, num_event_time_updates=3), 8, 2e-4, 16, ("window", 129)),
    "T130-M33-m1-b3": ("slow_33x130", dict(dmax=100, nmax=25, m=1, occult_nmax=15, num_event_time_updates=3), 3, 2e-4, 4, ("pieces", 2)),
    "T64-M17-m1-b5": ("micro_17x64", dict(dmax=10, nmax=25, m=1, occult_nmax=15, num_event_time_updates=3), 5, 1e-4, 1, ("pieces", 1)),
    "T65-M33-m2-b3": ("micro_33x65", dict(dmax=10, nmax=25, m=2, occult_nmax=15, num_event_time_updates=3), 3, 1e-4, 8, ("reach", 64)),
    "T192-M17-m2-b3-skip": ("slow_17x192", dict(dmax=12, nmax=25, m=2, occult_nmax=15, num_event_time_updates=3), 3, 2e-4, 1, ("skip",)),
}


def start(case_id):
    name, cfg, B, eps, seed, want = CASES[case_id]
    case = H.build_case(name, CASE_SEED, alpha_t_sd=0.005)
    u = synth.jitter_params(case["u"], B, scale=0.02, seed=CASE_SEED, T=case["k"].T)
    ev = np.stack([case["events"]] * B)
    return case, u, ev


def kept_pieces(lo, hi):
    """The pieces of the hull [min lo, max hi] that hold a day of a window (lo[i], hi[i]] -- per day, as the definition
    reads -- and the number of pieces of the hull."""
    LO, HI = min(lo), max(hi)
    days = sorted({t for a, b in zip(lo, hi) for t in range(a + 1, b + 1)})
    return sorted({(t - LO) // PIECE for t in days}), (HI - LO) // PIECE + 1


def recorded_updates(delta, T, m):
    """delta: [..., 4, m] of one recorded move/E->I update each (rows m, t, delta_t, x_star) -> a list of
    (windows' lo, hi, largest |delta_t| of a sub-move that moves events, kept pieces, pieces of the hull) for the updates the
    band workgroups evaluated: every sub-move in range, one of them moving events."""
    out = []
    for d in np.asarray(delta).reshape(-1, 4, m):
        t, dt, x = d[1], d[2], d[3]
        t2 = t + dt
        if ((t2 < 0) | (t2 >= T)).any() or not (x > 0).any():
            continue
        lo, hi = np.minimum(t, t2), np.maximum(t, t2)
        kept, npieces = kept_pieces([int(v) for v in lo], [int(v) for v in hi])
        out.append((lo, hi, int(np.abs(dt[x > 0]).max()), kept, npieces))
    return out


def shows(want, updates):
    if want[0] == "window":
        return sum(1 for u in updates if u[2] == want[1])
    if want[0] == "skip":
        return sum(1 for u in updates if u[3] == [0, 2] and u[4] == 3)
    if want[0] == "reach":
        return sum(1 for u in updates if int(max(u[1])) == want[1])
    return sum(1 for u in updates if u[4] == want[1])


def move_columns_as_delta(cols, m):
    """read_move_columns' rows of move/E->I -> [n, B, 4, m] (m, t, delta_t, x_star)."""
    n, B = cols.shape[:2]
    return cols[:, :, 1, 2:].reshape(n, B, 4, _lib.MMAX)[..., :m].astype(np.int64)

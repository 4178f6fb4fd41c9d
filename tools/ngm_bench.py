#!/usr/bin/env python3
"""What the group next-generation matrix on the device costs and buys (GPU box, UK-380 x 8 chains, a 100-draw burst, uint16
trace, the four nations of `groups: nations`, D = 14), in ONE call on one box:

  * the `rt` call of a burst that lies in the trace with the matrix on against off (group R_t on in both), the two
    interleaved, median of --reps, HIP events (seir_timer_*) around the call.  The yardstick is the call without it, which
    is k_rt_trace's time: for a partition k_ngm_rows evaluates the same nnz x M x D = M^2 D cells per draw;
  * the same values by way of the trace: read the burst, form the rows with the stateless `SeirModel.group_ngm_rows` and
    sum on the host (`posterior.groups.group_ngm`) -- compared with the store before anything is recorded -- and by way of
    the oracle's NumPy (`oracle.rt_oracle.next_generation_matrix`, a full M x M matrix per draw and day), timed on
    --oracle-draws draws and scaled to the burst.

With --parent DIR (a checkout of the parent commit with its library built) the tool also runs `bench.py` of DIR and of this
tree in turns -- parent, parent2 (DIR again: the A/A pair), product; the order rotated from round to round -- and writes
the runs to --ab (profiles/r21_ab.txt), to be read against the parent's own run-to-run span.

    python tools/ngm_bench.py [--out profiles/r21_ngm.json] [--parent DIR --ab profiles/r21_ab.txt]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def ab(parent, path, rounds):
    import groups_bench as GB
    trees = {"parent": parent, "parent2": parent, "product": ROOT}
    names = list(trees)
    runs = {k: [] for k in names}
    order_log = []
    for r in range(rounds):
        order = names[r % 3:] + names[:r % 3]
        order_log.append(" ".join(order))
        for k in order:
            runs[k].append(GB.bench_value(trees[k]))
            print(f"[ab] round {r} {k}: {runs[k][-1]:.1f}", file=sys.stderr, flush=True)
    med = {k: float(np.median(v)) for k, v in runs.items()}
    spread = abs(med["parent"] - med["parent2"])
    mean_p = 0.5 * (med["parent"] + med["parent2"])
    diff = med["product"] - mean_p
    single = runs["parent"] + runs["parent2"]
    inside = sum(min(single) <= v <= max(single) for v in runs["product"])
    with open(path, "w") as f:
        f.write(f"Round 21 (group next-generation matrix on the device, the key ABSENT): alternating A/B inside ONE call, one MI355X.\n"
                f"parent / parent2: the parent commit's tree and library, run twice per round (the A/A pair); product: this change.  "
                f"{rounds} rounds of\n  bench.py {' '.join(GB.BENCH)}\nin the orders: {' | '.join(order_log)}.\n\n"
                "bench.py posterior samples/sec (higher is better)\n"
                "   runs    " + " | ".join(f"{k} " + " ".join(f"{v:.1f}" for v in runs[k]) for k in names) + "\n"
                "   medians " + "  ".join(f"{k} {med[k]:.1f}" for k in names) +
                f"   A/A spread {spread:.1f}   product {'AHEAD of' if diff >= 0 else 'BEHIND'} mean(parent, parent2) by "
                f"{abs(diff):.1f} ({100.0 * abs(diff) / mean_p:.2f} %)\n"
                f"   (the parents' single runs span {min(single):.1f} .. {max(single):.1f}; {inside} of the product's "
                f"{len(runs['product'])} lie inside that span)\n")
    return {"runs": runs, "medians": med, "aa_spread": spread, "product_minus_mean_parent": diff,
            "parents_single_run_span": [min(single), max(single)], "product_runs_inside_span": inside}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="uk380")
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--draws", type=int, default=100, help="kept draws per burst")
    ap.add_argument("--days", type=int, default=14)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--oracle-draws", type=int, default=2, help="(draw, chain) pairs the oracle's NumPy route is timed on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_ngm.json"))
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: run the A/B of bench.py")
    ap.add_argument("--ab", default=os.path.join(ROOT, "profiles", "r21_ab.txt"))
    ap.add_argument("--ab-rounds", type=int, default=3)
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import torch
    from covid19uk_amd import synth
    from covid19uk_amd.posterior import groups as G
    from covid19uk_amd.sampler import ChainSampler
    from covid19uk_amd.seir import SeirModel
    from oracle import rt_oracle as ro
    from oracle import seir_oracle as so
    cfg = dict(dmax=84, nmax=25, m=2, occult_nmax=15, num_event_time_updates=5)       # example_config.yaml:26-30
    cov = synth.make_covariates(a.workload)
    events, init, truth = synth.simulate_epidemic(cov)
    u0 = synth.unconstrain(synth.pack_params(truth, cov.M, cov.T))
    M, T, B, n, D = cov.M, cov.T, a.chains, a.draws, a.days
    codes = [str(x) for x in np.load(synth._DATA)["lad19cd"]] if a.workload == "uk380" else None
    tab = G.parse_groups("nations", M, codes) if codes else G.parse_groups({"low": list(range(M // 2)), "high": list(range(M // 2, M))}, M)
    N = np.asarray(cov.N, np.float64).reshape(-1)
    w = G.rt_weights(tab, N)
    u = synth.jitter_params(u0, B, scale=0.002, seed=7, T=T)
    ev = np.stack([events] * B)
    Mp = (M + 63) // 64 * 64
    kr = json.load(open(entry.RESOURCES))
    res = {"workload": a.workload, "M": M, "T": T, "chains": B, "draws": n, "days": D, "groups": tab.names,
           "group_sizes": [int(x) for x in np.diff(tab.offsets)], "device": torch.cuda.get_device_name(0),
           "command": " ".join(sys.argv), "rows_plane_bytes_per_slot": B * tab.G * D * Mp * 8, "store_bytes": n * B * tab.G * tab.G * D * 8,
           "cells_per_draw": int(tab.offsets[-1]) * M * D, "k_rt_trace_cells_per_draw": M * M * D,
           "k_ngm_rows": kr["k_ngm_rows<4>"], "k_rt_trace": kr["k_rt_trace<4>"]}

    with SeirModel(cov, init, max_chains=B) as model:
        with ChainSampler(model, cfg, B, seed=1, trace_capacity=2 * n, record_events="u16") as s:
            s.set_state(u, ev)
            s.set_kernel(step_size=1.2e-5)
            s.reset_trace()
            s.run(n)
            s.set_groups(tab.offsets, tab.members)
            s.set_group_rt(w)

            def rt_call(on):
                s.reset_rt(D, N / N.sum())
                s.set_group_ngm(w if on else None, n if on else 0)
                model.sync()
                model.timer_start()
                s.rt(0, n)
                return float(model.timer_stop())

            times = {False: [], True: []}
            for rep in range(a.reps + 1):                                              # the first pass is untimed: first launches
                for on in (False, True):
                    ms = rt_call(on)
                    if rep:
                        times[on].append(ms)
            off, on = float(np.median(times[False])), float(np.median(times[True]))
            res["rt"] = {"ms_without": off, "ms_with": on, "ratio": on / off, "added_ms": on - off,
                         "ms_all_without": times[False], "ms_all_with": times[True]}
            print(f"rt of {n} x {B} draws: off {off:.3f} ms, on {on:.3f} ms (+{on - off:.3f})", file=sys.stderr, flush=True)
            # ---- the same values by way of the trace, the stateless kernel and NumPy ---------------------------------------
            dev = s.read_group_ngm(n)
            t0 = time.perf_counter()
            tr = s.read_trace(n)
            t_read = time.perf_counter() - t0
            rows = model.group_ngm_rows(tr.theta.reshape(n * B, -1), tr.events.reshape((n * B,) + tr.events.shape[2:]).astype(np.int32),
                                        tab.offsets, tab.members, D)
            t_rows = time.perf_counter() - t0
            host = G.group_ngm(rows, tab, w).reshape(n, B, tab.G, tab.G, D)
            t_host = time.perf_counter() - t0
            res["by_way_of_the_trace"] = {"seconds_per_burst": t_host, "of_which_reading_the_trace": t_read,
                                          "of_which_the_stateless_kernel": t_rows - t_read,
                                          "same_bits": bool(np.array_equal(host.view(np.uint64), dev.view(np.uint64))),
                                          "trace_bytes": int(tr.events.nbytes)}
            print(f"by way of the trace: {t_host:.2f} s, same bits: {res['by_way_of_the_trace']['same_bits']}", file=sys.stderr,
                  flush=True)
            # ---- by way of the oracle's NumPy: a full M x M matrix of 1 - exp(-x) per draw and day --------------------------
            k = so.make_constants(cov.C, cov.N, cov.W, cov.weekday, cov.area, cov.adjacency, init)
            pairs = [(j, b) for j in range(n) for b in range(B)][:max(a.oracle_draws, 1)]
            worst = 0.0
            t0 = time.perf_counter()
            for j, b in pairs:
                par = so.unpack(tr.theta[j, b], M, T)
                state = so.compute_state(k.initial_state, tr.events[j, b].astype(np.float64))
                for tw in range(D):
                    t = T - D + tw
                    ngm = ro.next_generation_matrix(t, state[:, t, :], par, k, stable=True)
                    P = np.stack([ngm[tab.rows(g)].sum(axis=0) for g in range(tab.G)])              # [G, M]
                    K = np.stack([[float((w[tab.offsets[h]:tab.offsets[h + 1]] * P[g, tab.rows(h)]).sum()) for h in range(tab.G)]
                                  for g in range(tab.G)])
                    worst = max(worst, float(np.max(np.abs(K - dev[j, b, :, :, tw]) / np.maximum(np.abs(K), 1e-300))))
            t_or = time.perf_counter() - t0
            res["by_way_of_the_oracle"] = {"draws_timed": len(pairs), "seconds_timed": t_or,
                                           "seconds_per_burst_scaled": t_or * n * B / len(pairs), "max_relative_difference": worst}
            print(f"by way of the oracle: {t_or:.2f} s for {len(pairs)} draw(s), {res['by_way_of_the_oracle']['seconds_per_burst_scaled']:.1f} s "
                  f"per burst scaled; max relative difference {worst:.2e}", file=sys.stderr, flush=True)
    if a.parent:
        res["bench_ab"] = ab(os.path.abspath(a.parent), a.ab, a.ab_rounds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

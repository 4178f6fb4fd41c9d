#!/usr/bin/env python3
"""What the group curves on the device cost and buy (GPU box, UK-380 x 8 chains, a 100-draw burst, uint16 trace, the four
nations of `groups: nations`, D = 14), in ONE call on one box:

  * the `rt` call of a burst that lies in the trace with group R_t on against off, the two interleaved, median of --reps,
    HIP events (seir_timer_*) around the call: once with the draw store off (k_rt_trace_cells in place of k_rt_trace) and
    once with it on (k_rt_trace_keep, then the gather k_rt_cells_from_keep);
  * the `within_between` call with group within / between on against off likewise;
  * k_group_wsums by itself: `SeirModel.group_wsums` is timed on the host around the whole call (copies included), so the
    kernel's own time is reported as the on / off difference above and the host call only as an upper bound;
  * the same bits by way of the trace: read the burst, form R_it with the stateless `SeirModel.reproduction_number` and
    sum on the host (`posterior.groups.weighted_sum_rows`).  The two routes are compared before anything is recorded.

The expectation the numbers are read against: a cell plane is n x B x D x Mp x 8 bytes (34 MB here), written once by the
trace kernel and read once per group that a location lies in by k_group_wsums.

With --parent DIR (a checkout of the parent commit with its library built) the tool also runs `bench.py` of DIR and of this
tree in turns -- parent, parent2 (DIR again: the A/A pair), product; the order rotated from round to round -- and writes
the runs to --ab (profiles/r18_ab.txt), to be read against the parent's own run-to-run span.

    python tools/group_curves_bench.py [--out profiles/r18_group_curves.json] [--parent DIR --ab profiles/r18_ab.txt]"""
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
        f.write(f"Round 18 (group curves on the device, both keys ABSENT): alternating A/B inside ONE call, one MI355X.\n"
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_group_curves.json"))
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: run the A/B of bench.py")
    ap.add_argument("--ab", default=os.path.join(ROOT, "profiles", "r18_ab.txt"))
    ap.add_argument("--ab-rounds", type=int, default=3)
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import torch
    from covid19uk_amd import synth
    from covid19uk_amd.posterior import groups as G
    from covid19uk_amd.sampler import ChainSampler
    from covid19uk_amd.seir import SeirModel
    cfg = dict(dmax=84, nmax=25, m=2, occult_nmax=15, num_event_time_updates=5)       # example_config.yaml:26-30
    cov = synth.make_covariates(a.workload)
    events, init, truth = synth.simulate_epidemic(cov)
    u0 = synth.unconstrain(synth.pack_params(truth, cov.M, cov.T))
    M, T, B, n, D = cov.M, cov.T, a.chains, a.draws, a.days
    codes = [str(x) for x in np.load(synth._DATA)["lad19cd"]] if a.workload == "uk380" else None
    tab = G.parse_groups("nations", M, codes) if codes else G.parse_groups({"all": list(range(M)), "half": list(range(M // 2))}, M)
    N = np.asarray(cov.N, np.float64).reshape(-1)
    w = G.rt_weights(tab, N)
    u = synth.jitter_params(u0, B, scale=0.002, seed=7, T=T)
    ev = np.stack([events] * B)
    Mp = (M + 63) // 64 * 64
    kr = json.load(open(entry.RESOURCES))
    res = {"workload": a.workload, "M": M, "T": T, "chains": B, "draws": n, "days": D, "groups": tab.names,
           "group_sizes": [int(x) for x in np.diff(tab.offsets)], "device": torch.cuda.get_device_name(0),
           "command": " ".join(sys.argv), "cell_plane_bytes": n * B * D * Mp * 8, "group_output_bytes": n * B * tab.G * D * 8,
           "k_rt_trace_cells": kr["k_rt_trace_cells<4>"], "k_rt_trace": kr["k_rt_trace<4>"]}

    with SeirModel(cov, init, max_chains=B) as model:
        with ChainSampler(model, cfg, B, seed=1, trace_capacity=2 * n, record_events="u16") as s:
            s.set_state(u, ev)
            s.set_kernel(step_size=1.2e-5)
            s.reset_trace()
            s.run(n)
            s.set_groups(tab.offsets, tab.members)

            def timed(fn):
                model.sync()
                model.timer_start()
                fn()
                return float(model.timer_stop())

            def rt_call(keep, on):
                s.set_group_rt(w if on else None)
                s.reset_rt(D, N / N.sum())
                s.keep_rt_draws(n if keep else 0)
                return timed(lambda: s.rt(0, n))

            def wb_call(on):
                s.set_group_within_between(on)
                s.reset_within_between(D)
                return timed(lambda: s.within_between(0, n))

            calls = {"rt_store_off": lambda on: rt_call(False, on), "rt_store_on": lambda on: rt_call(True, on),
                     "within_between": wb_call}
            times = {(k, on): [] for k in calls for on in (False, True)}
            for rep in range(a.reps + 1):                                              # the first pass is untimed: first launches
                for on in (False, True):
                    for k, fn in calls.items():
                        ms = fn(on)
                        if rep:
                            times[(k, on)].append(ms)
            s.keep_rt_draws(0)
            for k in calls:
                off, on = float(np.median(times[(k, False)])), float(np.median(times[(k, True)]))
                planes = 2 if k == "within_between" else 1
                res[k] = {"ms_without": off, "ms_with": on, "ratio": on / off, "added_ms": on - off,
                          "cell_plane_GBps_by_difference": (2 * planes * res["cell_plane_bytes"] / (on - off) / 1e6
                                                            if on > off else None),
                          "ms_all_without": times[(k, False)], "ms_all_with": times[(k, True)]}
                print(f"{k} of {n} x {B} draws: off {off:.3f} ms, on {on:.3f} ms (+{on - off:.3f})", file=sys.stderr, flush=True)
            # ---- the same bits by way of the trace, the stateless kernel and NumPy -----------------------------------------
            s.set_group_rt(w)
            s.reset_rt(D, N / N.sum())
            s.rt(0, n)
            dev = s.read_group_rt(n)
            t0 = time.perf_counter()
            tr = s.read_trace(n)
            t_read = time.perf_counter() - t0
            with SeirModel(cov, init, max_chains=16) as m2:
                R = m2.reproduction_number(tr.theta.reshape(n * B, -1),
                                           tr.events.reshape((n * B,) + tr.events.shape[2:]).astype(np.float64))
            R = R.reshape(n, B, T, -1)[:, :, T - D:]
            t_rit = time.perf_counter() - t0
            host = np.moveaxis(G.weighted_sum_rows(tab, R, w), -1, 2)
            t_host = time.perf_counter() - t0
            res["by_way_of_the_trace"] = {"seconds_per_burst": t_host, "of_which_reading_the_trace": t_read,
                                          "of_which_the_stateless_kernel": t_rit - t_read,
                                          "same_bits": bool(np.array_equal(host, dev)), "trace_bytes": int(tr.events.nbytes)}
            print(f"by way of the trace: {t_host:.2f} s, same bits: {res['by_way_of_the_trace']['same_bits']}", file=sys.stderr,
                  flush=True)
            # ---- k_group_wsums by itself on host arrays (an upper bound: the copies are inside) ---------------------------
            plane = np.ascontiguousarray(R.reshape(n * B, D, -1))
            model.group_wsums(plane, tab.offsets, tab.members, w)
            t0 = time.perf_counter()
            alone = model.group_wsums(plane, tab.offsets, tab.members, w)
            res["group_wsums_host_call_ms"] = 1e3 * (time.perf_counter() - t0)
            res["group_wsums_same_bits"] = bool(np.array_equal(alone.reshape(n, B, tab.G, D), dev))
    if a.parent:
        res["bench_ab"] = ab(os.path.abspath(a.parent), a.ab, a.ab_rounds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

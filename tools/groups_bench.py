#!/usr/bin/env python3
"""What the region totals on the device cost and buy (GPU box, UK-380 x 8 chains, a 100-draw burst, uint16 trace, the four
nations of `groups: nations`), in ONE call on one box:

  * `summarize`, `forecast` (H = 56) and `check` (K = 14) of a burst that lies in the trace, each with the table set
    against the same call without it, the two interleaved, median of --reps: HIP events (seir_timer_*) around the call.
    The difference of the medians is what the group launch (and the memset of its outputs) adds;
  * `summarize` alone is the yardstick: k_summarize and k_group_sums both read the burst buffer once (DESIGN.md section
    3e's bytes; a location that lies in several groups is read once per group);
  * the same integers by way of the trace and NumPy: read the burst, sum over the members on the host.  The two routes
    are compared before anything is recorded.

With --parent DIR (a checkout of the parent commit with its library built) the tool also runs `bench.py` of DIR and of this
tree in turns -- parent, parent2 (DIR again: the A/A pair), product; the order rotated from round to round -- and writes
the runs to --ab (profiles/r17_ab.txt), to be read against the parent's own run-to-run span.

    python tools/groups_bench.py [--out profiles/r17_groups.json] [--parent DIR --ab profiles/r17_ab.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
BENCH = ["--gpus", "1", "--steps", "200", "--warmup", "20"]


def bench_value(tree):
    r = subprocess.run([sys.executable, "bench.py"] + BENCH, cwd=tree, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py in {tree} failed:\n{r.stderr[-2000:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["value"])


def ab(parent, path, rounds):
    trees = {"parent": parent, "parent2": parent, "product": ROOT}
    names = list(trees)
    runs = {k: [] for k in names}
    order_log = []
    for r in range(rounds):
        order = names[r % 3:] + names[:r % 3]
        order_log.append(" ".join(order))
        for k in order:
            runs[k].append(bench_value(trees[k]))
            print(f"[ab] round {r} {k}: {runs[k][-1]:.1f}", file=sys.stderr, flush=True)
    med = {k: float(np.median(v)) for k, v in runs.items()}
    spread = abs(med["parent"] - med["parent2"])
    mean_p = 0.5 * (med["parent"] + med["parent2"])
    diff = med["product"] - mean_p
    single = runs["parent"] + runs["parent2"]
    inside = sum(min(single) <= v <= max(single) for v in runs["product"])
    with open(path, "w") as f:
        f.write(f"Round 17 (region totals on the device, key ABSENT): alternating A/B inside ONE call, one MI355X.\n"
                f"parent / parent2: the parent commit's tree and library, run twice per round (the A/A pair); product: this change.  "
                f"{rounds} rounds of\n  bench.py {' '.join(BENCH)}\nin the orders: {' | '.join(order_log)}.\n\n"
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
    ap.add_argument("--horizon", type=int, default=56)
    ap.add_argument("--check", type=int, default=14)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_groups.json"))
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: run the A/B of bench.py")
    ap.add_argument("--ab", default=os.path.join(ROOT, "profiles", "r17_ab.txt"))
    ap.add_argument("--ab-rounds", type=int, default=3)
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import torch
    from covid19uk_amd import synth
    from covid19uk_amd.posterior import groups as G
    from covid19uk_amd.posterior import predict
    from covid19uk_amd.sampler import ChainSampler
    from covid19uk_amd.seir import SeirModel
    cfg = dict(dmax=84, nmax=25, m=2, occult_nmax=15, num_event_time_updates=5)       # example_config.yaml:26-30
    cov = synth.make_covariates(a.workload)
    events, init, truth = synth.simulate_epidemic(cov)
    u0 = synth.unconstrain(synth.pack_params(truth, cov.M, cov.T))
    M, T, B, n, Hn, K = cov.M, cov.T, a.chains, a.draws, a.horizon, a.check
    codes = [str(x) for x in np.load(synth._DATA)["lad19cd"]] if a.workload == "uk380" else None
    tab = G.parse_groups("nations", M, codes) if codes else G.parse_groups({"all": list(range(M)), "half": list(range(M // 2))}, M)
    u = synth.jitter_params(u0, B, scale=0.002, seed=7, T=T)
    ev = np.stack([events] * B)
    sizes = [int(x) for x in np.diff(tab.offsets)]
    res = {"workload": a.workload, "M": M, "T": T, "chains": B, "draws": n, "horizon": Hn, "check_days": K, "groups": tab.names,
           "group_sizes": sizes, "device": torch.cuda.get_device_name(0), "command": " ".join(sys.argv),
           "burst_buffer_bytes": n * B * M * T * 3 * 2, "trace_group_output_bytes": n * B * tab.G * T * 3 * 8}

    with SeirModel(cov, init, max_chains=B) as model:
        with ChainSampler(model, cfg, B, seed=1, trace_capacity=2 * n, record_events="u16") as s:
            s.set_state(u, ev)
            s.set_kernel(step_size=1.2e-5)
            s.reset_trace()
            s.run(n)
            s.reset_summary()
            s.reset_forecast(Hn, *predict.forecast_calendar(cov, None, T, Hn), 3)
            s.reset_check(K, *predict.check_calendar(cov, None, T, K), 4)
            calls = {"summarize": lambda: s.summarize(0, n, accumulate=False), "forecast": lambda: s.forecast(0, n),
                     "check": lambda: s.check(0, n)}
            times = {(k, on): [] for k in calls for on in (False, True)}
            for rep in range(a.reps + 1):                                              # the first pass is untimed: first launches
                for on in (False, True):
                    s.set_groups(*((tab.offsets, tab.members) if on else (None, None)))
                    for k, fn in calls.items():
                        model.sync()
                        model.timer_start()
                        fn()
                        ms = model.timer_stop()
                        if rep:
                            times[(k, on)].append(float(ms))
            for k in calls:
                off, on = float(np.median(times[(k, False)])), float(np.median(times[(k, True)]))
                res[k] = {"ms_without": off, "ms_with": on, "ratio": on / off, "group_launch_ms_by_difference": on - off,
                          "ms_all_without": times[(k, False)], "ms_all_with": times[(k, True)]}
                print(f"{k} of {n} x {B} draws: without {off:.3f} ms, with the table {on:.3f} ms (+{on - off:.3f})",
                      file=sys.stderr, flush=True)
            d = res["summarize"]["group_launch_ms_by_difference"]
            res["summarize"]["burst_buffer_GBps_by_difference"] = res["burst_buffer_bytes"] / max(d, 1e-6) / 1e6
            res["summarize"]["k_summarize_GBps"] = res["burst_buffer_bytes"] / res["summarize"]["ms_without"] / 1e6
            # ---- the same integers by way of the trace and NumPy -------------------------------------------------------
            dev = s.read_group_marginals("trace", n)["seir_by_group"]
            t0 = time.perf_counter()
            tr = s.read_trace(n)
            t_read = time.perf_counter() - t0
            host = np.stack([tr.events[:, :, tab.rows(g)].sum(axis=2, dtype=np.int64) for g in range(tab.G)], axis=2)
            t_host = time.perf_counter() - t0
            res["by_way_of_the_trace"] = {"seconds_per_burst": t_host, "of_which_reading_the_trace": t_read,
                                          "same_integers": bool(np.array_equal(host, dev)), "trace_bytes": int(tr.events.nbytes)}
            print(f"by way of the trace: {t_host:.2f} s ({t_read:.2f} s reading it), same integers: "
                  f"{res['by_way_of_the_trace']['same_integers']}", file=sys.stderr, flush=True)
    if a.parent:
        res["bench_ab"] = ab(os.path.abspath(a.parent), a.ab, a.ab_rounds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

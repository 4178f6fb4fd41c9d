#!/usr/bin/env python3
"""What scenarios riding on the forecast cost (GPU box, UK-380 x 8 chains, a 100-draw burst, uint16 trace, H = 56 by
default), in ONE call on one box:

  * the forecast call with K = 0, 1, 2, 4 scenarios: HIP events (seir_timer_*) around `forecast(0, n)` of a burst that lies
    in the trace; --reps rounds (default 7), the four K in turn within every round, the median per K; K = 0 is the yardstick.
    The design's claim to check: the scenario axis lies in the columns of one contraction and one day launch per forecast
    day, so the increment of K = 4 should stay well under 4 x the increment of K = 1;
  * the same integers by the route without the feature, as the point of comparison: read the burst's trace, host sums over
    T for the state at day T, `seir_simulate` per chain for the baseline and for every scenario, the NumPy fold of the
    paired differences.  The integers of the two routes are compared before anything is recorded.

With --local: what the local entry point and the scenarios' region totals cost against the global set, in ONE call,
interleaved, medians of --reps: the forecast call with K = 1 and K = 4 set globally, the same numbers set through
`seir_sampler_scenarios_set_local` (tensors constant over the locations), and the local set with the `nations` group sums of
the scenarios on (the table is in force in all three, so the forecast's own group sums are in every figure).  The integers
of the global and the local route are compared before anything is recorded.

With --trigger: what a rule costs against the targeted set, in ONE call, interleaved, medians of --reps, K = 1 and K = 4: the
forecast call with the targeted set (tensors that vary over the locations), the same numbers through
`seir_sampler_scenarios_set_triggered` with a rule that never fires, a rule that fires in roughly half of the (draw, location)
cells (a 7-day window against the median over the draws of the row's recorded window sum; then: transmission x 0.7), and the
two reads of the record.  The integers of the never-firing set are compared with the targeted set's before anything is recorded.

    python tools/scenario_bench.py [--out profiles/r29_scenarios.json]
    python tools/scenario_bench.py --local [--out profiles/r32_scenarios_local.json]
    python tools/scenario_bench.py --trigger [--out profiles/r36_scenario_triggers.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="uk380")
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--draws", type=int, default=100, help="kept draws per burst")
    ap.add_argument("--horizon", type=int, default=56)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--local", action="store_true", help="time the local entry point and the region totals against the global set")
    ap.add_argument("--trigger", action="store_true", help="time a triggered set against the targeted set with the same numbers")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "r36_scenario_triggers.json" if a.trigger else
                             "r32_scenarios_local.json" if a.local else "r29_scenarios.json")
    import __graft_entry__ as entry
    entry.build()
    import torch
    from covid19uk_amd import synth
    from covid19uk_amd.posterior import predict
    from covid19uk_amd.posterior import scenarios as SC
    from covid19uk_amd.sampler import ChainSampler, forecast_draw_id
    from covid19uk_amd.seir import SeirModel
    cfg = dict(dmax=84, nmax=25, m=2, occult_nmax=15, num_event_time_updates=5)       # example_config.yaml:26-30
    cov = synth.make_covariates(a.workload)
    events, init, truth = synth.simulate_epidemic(cov)
    u0 = synth.unconstrain(synth.pack_params(truth, cov.M, cov.T))
    M, T, B, n, Hn = cov.M, cov.T, a.chains, a.draws, a.horizon
    W, wd = predict.forecast_calendar(cov, None, T, Hn)
    u = synth.jitter_params(u0, B, scale=0.002, seed=7, T=T)
    ev = np.stack([events] * B)
    spec = {"transmission_down_a_fifth": dict(transmission=0.8, from_day=7), "commuting_halved": dict(commute=0.5),
            "both": dict(transmission=0.8, commute=0.5, from_day=7), "no_commuting": dict(commute=0.0)}
    sets = {0: SC.Scenarios(), **{K: SC.parse_scenarios(dict(list(spec.items())[:K]), Hn) for K in (1, 2, 4)}}
    res = {"workload": a.workload, "M": M, "T": T, "chains": B, "draws": n, "horizon": Hn, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "command": " ".join(sys.argv)}

    with SeirModel(cov, init, max_chains=B) as model:
        with ChainSampler(model, cfg, B, seed=1, trace_capacity=2 * n, record_events="u16") as s:
            s.set_state(u, ev)
            s.set_kernel(step_size=1.2e-5)
            s.reset_trace()
            s.run(n)
            model.sync()
            if a.local:
                local_against_global(a, res, model, s, sets, cov, W, wd)
                return write(a, res)
            if a.trigger:
                triggered_against_targeted(a, res, model, s, cov, W, wd)
                return write(a, res)

            def call(K, timed):
                s.reset_forecast(Hn, W, wd, 5)
                s.set_scenarios(sets[K].log_shift if K else None, sets[K].commute if K else None, n if K else 0)
                model.sync()
                if timed:
                    model.timer_start()
                s.forecast(0, n)
                return model.timer_stop() if timed else model.sync()
            for K in sets:                                                             # untimed: first launches, allocations
                call(K, False)
            times = {K: [] for K in sets}
            for _ in range(a.reps):
                for K in sets:                                                         # interleaved: a round holds every K once
                    times[K].append(call(K, True))
            med = {K: float(np.median(v)) for K, v in times.items()}
            res["forecast_call"] = {str(K): {"ms_median": med[K], "ms_min": float(min(times[K])), "ms_all": [float(t) for t in times[K]],
                                             "launches": 2 * Hn + 3 + (2 * Hn + 1 + 3 * K if K else 0), "device_to_device_copies": 2 * K,
                                             "increment_ms": med[K] - med[0]} for K in sets}
            res["increment_K4_over_K1"] = (med[4] - med[0]) / (med[1] - med[0])
            print("forecast call, ms (median of %d): " % a.reps + ", ".join(f"K={K}: {med[K]:.2f}" for K in sets) +
                  f"; increment K=4 / K=1: {res['increment_K4_over_K1']:.2f}", file=sys.stderr, flush=True)

            # ---- K = 4 by the route without the feature: trace over PCIe, seir_simulate per chain and scenario, NumPy ----
            call(4, False)
            device = (s.scenario_diffs(), s.read_scenario_draws())
            t0 = time.perf_counter()
            tr = s.read_trace(n)
            t_read = time.perf_counter() - t0
            sims = {k: [] for k in (None, 0, 1, 2, 3)}
            for b in range(B):
                th, e = tr.theta[:, b], tr.events[:, b]
                tot = e.sum(axis=2, dtype=np.int64)
                i0 = init.astype(np.int64)
                st0 = np.stack([i0[:, 0] - tot[..., 0], i0[:, 1] + tot[..., 0] - tot[..., 1], i0[:, 2] + tot[..., 1] - tot[..., 2],
                                i0[:, 3] + tot[..., 2]], axis=-1)
                a_path = predict.log_baseline_path(th[:, 5], th[:, 6:6 + T - 1], T, Hn)
                for k in sims:
                    a_k, W_k = (a_path, W) if k is None else SC.scenario_inputs(a_path, W, sets[4], k)
                    sims[k].append(model.simulate(th[:, :5], a_k, th[:, 6 + T - 1:], W_k, wd, st0.astype(np.float64), seed=5,
                                                  first_draw_id=forecast_draw_id(b, 0)).astype(np.int64))
            base = np.stack(sims[None], axis=1)
            same = True
            for k in range(4):
                sim = np.stack(sims[k], axis=1)
                fold = SC.fold_differences(base, sim)
                same = same and all(np.array_equal(fold[key], device[0][key][k]) for key in ("ref", "sum", "sumsq", "lt", "eq"))
                same = same and np.array_equal(sim.sum(axis=2), device[1]["by_day"][k])
            t_host = time.perf_counter() - t0
            if not same:
                raise SystemExit("the two routes give different integers: nothing recorded")
            res["route_without_the_feature"] = {"K": 4, "seconds": t_host, "of_which_reading_the_trace": t_read, "same_integers": True,
                                                "device_increment_ms": med[4] - med[0],
                                                "ratio_to_the_device_increment": t_host * 1e3 / (med[4] - med[0])}
            print(f"without the feature, K = 4: {t_host:.2f} s ({t_read:.2f} s reading the trace), same integers: {same}",
                  file=sys.stderr, flush=True)
    write(a, res)


def write(a, res):
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def local_against_global(a, res, model, s, sets, cov, W, wd):
    """--local: the forecast call with K = 1 and K = 4 set globally, set locally, and set locally with the scenarios' region
    totals over the nations; a round holds every variant once."""
    from covid19uk_amd.posterior import groups as G
    M, n, Hn = cov.M, a.draws, a.horizon
    codes = [str(x) for x in np.load(os.path.join(ROOT, "covid19uk_amd", "data", "uk_lad2019.npz"))["lad19cd"]]
    if len(codes) != M:
        raise SystemExit(f"--local needs the bundled codes: {len(codes)} of them, the workload has M={M}")
    tab = G.parse_groups("nations", M, codes)
    s.set_groups(tab.offsets, tab.members)
    over = lambda x: np.ascontiguousarray(np.repeat(x[:, None, :], M, axis=1))          # noqa: E731  [K,H] -> [K,M,H]
    variants = [(kind, K) for K in (1, 4) for kind in ("global", "local", "local_groups")]

    def call(kind, K, timed):
        s.reset_forecast(Hn, W, wd, 5)
        s.set_scenario_groups(False)
        ls, cm = sets[K].log_shift, sets[K].commute
        s.set_scenarios(ls if kind == "global" else over(ls), cm if kind == "global" else over(cm), n)
        if kind == "local_groups":
            s.set_scenario_groups(True)
        model.sync()
        if timed:
            model.timer_start()
        s.forecast(0, n)
        return model.timer_stop() if timed else model.sync()
    ints = {}
    for kind, K in variants:                                                              # untimed: first launches, allocations
        call(kind, K, False)
        d, dr = s.scenario_diffs(), s.read_scenario_draws()
        ints[kind, K] = [d[key] for key in ("ref", "sum", "sumsq", "lt", "eq")] + [dr["by_day"], dr["state_by_day"]]
        if kind == "local_groups":
            tot = s.read_scenario_group_draws()
            if not np.array_equal(tot.sum(axis=3), dr["by_day"]):                         # the nations are a partition
                raise SystemExit("the nations' totals do not add up to the national curve: nothing recorded")
    for K in (1, 4):
        for kind in ("local", "local_groups"):
            if not all(np.array_equal(x, y) for x, y in zip(ints[kind, K], ints["global", K])):
                raise SystemExit(f"{kind}, K = {K}: not the global set's integers: nothing recorded")
    times = {v: [] for v in variants}
    for _ in range(a.reps):
        for v in variants:
            times[v].append(call(*v, True))
    med = {v: float(np.median(t)) for v, t in times.items()}
    res["groups"] = dict(table="nations", G=int(tab.G))
    res["same_integers"] = True
    res["forecast_call"] = {f"{kind},K={K}": {"ms_median": med[kind, K], "ms_min": float(min(times[kind, K])),
                                             "ms_max": float(max(times[kind, K])), "ms_all": [float(t) for t in times[kind, K]]}
                            for kind, K in variants}
    res["local_minus_global_ms"] = {f"K={K}": med["local", K] - med["global", K] for K in (1, 4)}
    res["global_spread_ms"] = {f"K={K}": float(max(times["global", K]) - min(times["global", K])) for K in (1, 4)}
    res["region_totals_ms"] = {f"K={K}": med["local_groups", K] - med["local", K] for K in (1, 4)}
    print("forecast call, ms (median of %d): " % a.reps + ", ".join(f"{kind} K={K}: {med[kind, K]:.2f}" for kind, K in variants),
          file=sys.stderr, flush=True)


def triggered_against_targeted(a, res, model, s, cov, W, wd):
    """--trigger: the forecast call with K = 1 and K = 4 targeted scenarios, the same through the triggered entry with a rule that
    never fires, with a rule that fires in about half of the cells, and the two reads; a round holds every variant once."""
    M, B, n, Hn, w = cov.M, a.chains, a.draws, a.horizon, 7
    rng = np.random.default_rng(36)
    ls, cm = rng.normal(-0.1, 0.1, size=(4, M, Hn)), rng.uniform(0.5, 1.5, size=(4, M, Hn))
    ls_on, cm_on = ls + np.log(0.7), cm
    c0 = s.read_trace(n).events[..., -w:, 2].astype(np.int64).sum(axis=-1)            # [n, B, M]: the window at day 0
    half = np.median(c0.reshape(n * B, M), axis=0).astype(np.int64)
    never = np.full(M, 2 ** 31 - 1, np.int64)
    variants = [(kind, K) for K in (1, 4) for kind in ("targeted", "never", "half")]

    def rule(K, on):
        return dict(log_shift_on=ls_on[:K], commute_on=cm_on[:K], on=np.tile(on, (K, 1)), off=np.tile(on // 2 if on is half else 0 * on, (K, 1)),
                    window=np.full(K, w), from_day=np.zeros(K, int), min_days=np.full(K, 3), review_every=np.ones(K, int))

    def call(kind, K, timed):
        s.reset_forecast(Hn, W, wd, 5)
        s.set_scenarios(ls[:K], cm[:K], n, **({} if kind == "targeted" else dict(triggers=rule(K, never if kind == "never" else half))))
        model.sync()
        if timed:
            model.timer_start()
        s.forecast(0, n)
        return model.timer_stop() if timed else model.sync()
    ints, share = {}, {}
    for kind, K in variants:                                                              # untimed: first launches, allocations
        call(kind, K, False)
        d, dr = s.scenario_diffs(), s.read_scenario_draws()
        ints[kind, K] = [d[key] for key in ("ref", "sum", "sumsq", "lt", "eq")] + [dr["by_day"], dr["state_by_day"]]
        if kind != "targeted":
            share[kind, K] = float(s.scenario_triggers()["active_count"].mean() / n)
    for K in (1, 4):
        if not all(np.array_equal(x, y) for x, y in zip(ints["never", K], ints["targeted", K])) or share["never", K] != 0.0:
            raise SystemExit(f"never-firing rule, K = {K}: not the targeted set's integers: nothing recorded")
        if all(np.array_equal(x, y) for x, y in zip(ints["half", K], ints["targeted", K])):
            raise SystemExit(f"half-firing rule, K = {K}: the targeted set's integers -- the rule did nothing: nothing recorded")
    times, reads = {v: [] for v in variants}, {K: [] for K in (1, 4)}
    for _ in range(a.reps):
        for v in variants:
            times[v].append(call(*v, True))
            if v[0] == "half":
                model.sync()
                t0 = time.perf_counter()
                s.scenario_triggers()
                s.read_scenario_trigger_draws()
                reads[v[1]].append((time.perf_counter() - t0) * 1e3)
    med = {v: float(np.median(t)) for v, t in times.items()}
    res["same_integers"] = True
    res["share_of_cell_days_under_the_measure"] = {f"{kind},K={K}": v for (kind, K), v in share.items()}
    res["forecast_call"] = {f"{kind},K={K}": {"ms_median": med[kind, K], "ms_min": float(min(times[kind, K])),
                                             "ms_max": float(max(times[kind, K])), "ms_all": [float(t) for t in times[kind, K]]}
                            for kind, K in variants}
    res["never_minus_targeted_ms"] = {f"K={K}": med["never", K] - med["targeted", K] for K in (1, 4)}
    res["half_minus_targeted_ms"] = {f"K={K}": med["half", K] - med["targeted", K] for K in (1, 4)}
    res["targeted_spread_ms"] = {f"K={K}": float(max(times["targeted", K]) - min(times["targeted", K])) for K in (1, 4)}
    res["two_reads_ms"] = {f"K={K}": {"median": float(np.median(reads[K])), "all": [float(t) for t in reads[K]]} for K in (1, 4)}
    print("forecast call, ms (median of %d): " % a.reps + ", ".join(f"{kind} K={K}: {med[kind, K]:.2f}" for kind, K in variants),
          file=sys.stderr, flush=True)


if __name__ == "__main__":
    main()

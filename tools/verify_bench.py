#!/usr/bin/env python3
"""What scoring the forecast against later data costs (GPU box, UK-380 x 8 chains, a 100-draw burst, uint16 trace, H = 56 by
default), in ONE call on one box:

  * the forecast call with the truth set against without: HIP events (seir_timer_*) around `forecast(0, n)` of a burst that
    lies in the trace; --reps rounds (default 7), the two variants in turn within every round, the median of each;
  * `forecast_pair_sums` per chain and pooled over a store of --store draws per chain (default 5000: the burst forecast
    fifty times behind one reset), against `forecast_order_stats` for three ranks over the same store, in turn, the
    median of --reps; host clock around the blocking calls.  The pair sums sort every cell where the select only counts
    digits: they do strictly more work, and no ratio is asked of them;
  * the same integers by the route without the feature, for the burst: read its trace, host sums over T for the state at
    day T, `seir_simulate` per chain, the NumPy fold against the truth and `np.sort` per cell for the pair sums.  The integers
    of the two routes are compared before anything is recorded.

    python tools/verify_bench.py [--out profiles/r30_verify.json]"""
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
    ap.add_argument("--store", type=int, default=5000, help="draws per chain in the store the pair sums run over")
    ap.add_argument("--horizon", type=int, default=56)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_verify.json"))
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import torch
    from covid19uk_amd import synth
    from covid19uk_amd.posterior import predict
    from covid19uk_amd.posterior import verify as V
    from covid19uk_amd.sampler import ChainSampler, forecast_draw_id
    from covid19uk_amd.seir import SeirModel
    cfg = dict(dmax=84, nmax=25, m=2, occult_nmax=15, num_event_time_updates=5)       # example_config.yaml:26-30
    cov = synth.make_covariates(a.workload)
    events, init, truth_par = synth.simulate_epidemic(cov)
    u0 = synth.unconstrain(synth.pack_params(truth_par, cov.M, cov.T))
    M, T, B, n, Hn = cov.M, cov.T, a.chains, a.draws, a.horizon
    W, wd = predict.forecast_calendar(cov, None, T, Hn)
    u = synth.jitter_params(u0, B, scale=0.002, seed=7, T=T)
    ev = np.stack([events] * B)
    res = {"workload": a.workload, "M": M, "T": T, "chains": B, "draws": n, "horizon": Hn, "reps": a.reps, "store_draws": a.store,
           "device": torch.cuda.get_device_name(0), "command": " ".join(sys.argv)}

    with SeirModel(cov, init, max_chains=B) as model:
        with ChainSampler(model, cfg, B, seed=1, trace_capacity=2 * n, record_events="u16") as s:
            s.set_state(u, ev)
            s.set_kernel(step_size=1.2e-5)
            s.reset_trace()
            s.run(n)
            model.sync()

            # ---- the burst by the route without the feature: its simulated planes give the truth as well ----
            t0 = time.perf_counter()
            tr = s.read_trace(n)
            t_read = time.perf_counter() - t0
            sims = []
            for b in range(B):
                th, e = tr.theta[:, b], tr.events[:, b]
                tot = e.sum(axis=2, dtype=np.int64)
                i0 = init.astype(np.int64)
                st0 = np.stack([i0[:, 0] - tot[..., 0], i0[:, 1] + tot[..., 0] - tot[..., 1], i0[:, 2] + tot[..., 1] - tot[..., 2],
                                i0[:, 3] + tot[..., 2]], axis=-1)
                a_path = predict.log_baseline_path(th[:, 5], th[:, 6:6 + T - 1], T, Hn)
                sims.append(model.simulate(th[:, :5], a_path, th[:, 6 + T - 1:], W, wd, st0.astype(np.float64), seed=5,
                                           first_draw_id=forecast_draw_id(b, 0)).astype(np.int64))
            x = V.targets(np.stack(sims, axis=1))                                      # [n,B,M,H,2]
            t_sim = time.perf_counter() - t0
            truth = x[n // 2, 0, :, :, 0].astype(np.int32)                             # one draw's cases as the later data
            truth[::7, Hn - 3:] = -1
            y, valid = V.truth_targets(truth)
            t1 = time.perf_counter()
            host_fold = [V.fold(x[:, b], y, valid) for b in range(B)]
            host_pair = np.moveaxis(V.pair_sum(np.moveaxis(x, 0, -1)), -1, 1)           # np.sort per cell
            host_pooled = np.moveaxis(V.pair_sum(np.moveaxis(x.reshape((n * B,) + x.shape[2:]), 0, -1)), -1, 0)
            t_numpy = time.perf_counter() - t1

            def call(on, timed):
                s.reset_forecast(Hn, W, wd, 5)
                s.set_verify(truth if on else None)
                model.sync()
                if timed:
                    model.timer_start()
                s.forecast(0, n)
                return model.timer_stop() if timed else model.sync()
            for on in (False, True):                                                   # untimed: first launches, allocations
                call(on, False)
            times = {False: [], True: []}
            for _ in range(a.reps):
                for on in (False, True):                                               # interleaved: a round holds both once
                    times[on].append(call(on, True))
            med = {on: float(np.median(v)) for on, v in times.items()}
            res["forecast_call"] = {("verify_on" if on else "verify_off"): {"ms_median": med[on], "ms_min": float(min(times[on])),
                                                                            "ms_all": [float(t) for t in times[on]]} for on in times}
            res["forecast_call"]["increment_ms"] = med[True] - med[False]
            print(f"forecast call, ms (median of {a.reps}): off {med[False]:.3f}, on {med[True]:.3f}", file=sys.stderr, flush=True)

            # ---- the same integers from the device, for the burst ----
            s.reset_forecast(Hn, W, wd, 5)
            s.keep_forecast_draws(n)
            s.set_verify(truth)
            s.forecast(0, n)
            acc = s.verify_summary()
            same = all(np.array_equal(acc[k][b], host_fold[b][k]) for b in range(B) for k in ("lt", "eq", "abs_sum"))
            same = same and np.array_equal(s.forecast_pair_sums(), host_pair)
            same = same and np.array_equal(s.forecast_pair_sums(pooled=True), host_pooled)
            if not same:
                raise SystemExit("the two routes give different integers: nothing recorded")
            res["route_without_the_feature"] = {"draws": n, "seconds": t_sim + t_numpy, "of_which_reading_the_trace": t_read,
                                                "of_which_numpy_fold_and_sort": t_numpy, "same_integers": True}
            print(f"without the feature, {n} draws: {t_sim + t_numpy:.2f} s ({t_read:.2f} s reading the trace, {t_numpy:.2f} s NumPy), "
                  f"same integers: {same}", file=sys.stderr, flush=True)

            # ---- the pair sums over a store of a.store draws per chain, against a three-rank select ----
            times_n = a.store // n
            s.reset_forecast(Hn, W, wd, 5)
            s.keep_forecast_draws(times_n * n)
            s.set_verify(None)
            for _ in range(times_n):
                s.forecast(0, n)
            model.sync()
            N = times_n * n
            ranks = {False: [int(0.05 * (N - 1)), (N - 1) // 2, int(0.95 * (N - 1))],
                     True: [int(0.05 * (N * B - 1)), (N * B - 1) // 2, int(0.95 * (N * B - 1))]}
            variants = {"pair_sums_per_chain": lambda: s.forecast_pair_sums(), "pair_sums_pooled": lambda: s.forecast_pair_sums(pooled=True),
                        "order_stats_3_ranks_per_chain": lambda: s.forecast_order_stats(ranks[False]),
                        "order_stats_3_ranks_pooled": lambda: s.forecast_order_stats(ranks[True], pooled=True)}
            for f in variants.values():
                f()
            tv = {k: [] for k in variants}
            for _ in range(a.reps):
                for k, f in variants.items():
                    t0 = time.perf_counter()
                    f()
                    tv[k].append((time.perf_counter() - t0) * 1e3)
            res["store"] = {k: {"ms_median": float(np.median(v)), "ms_min": float(min(v)), "ms_all": [float(t) for t in v]}
                            for k, v in tv.items()}
            res["store"]["draws_per_chain"] = N
            res["store"]["cells_per_chain_pair_sums"] = 2 * M * Hn
            res["store"]["cells_per_chain_order_stats"] = 3 * M * Hn
            res["store"]["fifty_forecast_calls_ms"] = 50 * med[False]
            print("store of %d draws per chain, ms (median of %d): " % (N, a.reps) +
                  ", ".join(f"{k}: {res['store'][k]['ms_median']:.1f}" for k in variants), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

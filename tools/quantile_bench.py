#!/usr/bin/env python3
"""What the forecast intervals on the device cost and buy (GPU box, UK-380 x 8 chains, a 100-draw burst, H = 56, uint16 trace,
a store of 5000 draws per chain by default), in ONE call on one box:

  * the forecast call with the draw store off and on: HIP events (seir_timer_*) around `forecast(0, n)` of a burst that lies
    in the trace, the two interleaved, median of --reps each.  A 100-draw burst is one host batch, so the difference of
    the medians is what the one k_forecast_keep launch adds; it is set against the bytes the kernel moves
    (DESIGN.md section 3j);
  * k_order_stats for the ranks of K = 3 probabilities over the full store, per chain and pooled over the chains: HIP
    events around the blocking call (selection and the copy of the [R, cells] result) and the wall clock of the Python
    call with the interpolation;
  * the parent's route to the same integers, for the burst: read the trace, host sums for the state at day T,
    `seir_simulate` per chain ([n, M, H, 3] fp64 over PCIe), the three planes and np.sort.  The order statistics of the
    two routes are compared before anything is recorded.

    python tools/quantile_bench.py [--out profiles/r13_quantiles.json]"""
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
    ap.add_argument("--store", type=int, default=5000, help="draws per chain the store is sized and filled for")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--probs", default="0.05,0.5,0.95")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_quantiles.json"))
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import torch
    from covid19uk_amd import synth
    from covid19uk_amd.posterior import predict
    from covid19uk_amd.posterior import quantiles as Q
    from covid19uk_amd.sampler import ChainSampler, forecast_draw_id
    from covid19uk_amd.seir import SeirModel
    cfg = dict(dmax=84, nmax=25, m=2, occult_nmax=15, num_event_time_updates=5)       # example_config.yaml:26-30
    cov = synth.make_covariates(a.workload)
    events, init, truth = synth.simulate_epidemic(cov)
    u0 = synth.unconstrain(synth.pack_params(truth, cov.M, cov.T))
    M, T, B, n, Hn, cap = cov.M, cov.T, a.chains, a.draws, a.horizon, a.store
    probs = Q.parse_probs(a.probs)
    W, wd = predict.forecast_calendar(cov, None, T, Hn)
    u = synth.jitter_params(u0, B, scale=0.002, seed=7, T=T)
    ev = np.stack([events] * B)
    res = {"workload": a.workload, "M": M, "T": T, "chains": B, "draws": n, "horizon": Hn, "store_draws": cap,
           "probs": list(probs), "device": torch.cuda.get_device_name(0), "command": " ".join(sys.argv),
           "store_bytes": B * 3 * M * Hn * cap * 4}

    with SeirModel(cov, init, max_chains=B) as model:
        with ChainSampler(model, cfg, B, seed=1, trace_capacity=2 * n, record_events="u16") as s:
            s.set_state(u, ev)
            s.set_kernel(step_size=1.2e-5)
            s.reset_trace()
            s.run(n)
            # ---- the forecast call, store off / on, interleaved -------------------------------------------------------
            times = {False: [], True: []}
            for rep in range(a.reps + 1):                                              # the first pair is untimed: first launches
                for keep in (False, True):
                    s.reset_forecast(Hn, W, wd, 5)
                    s.keep_forecast_draws(cap if keep else 0)
                    model.sync()
                    model.timer_start()
                    s.forecast(0, n)
                    ms = model.timer_stop()
                    if rep:
                        times[keep].append(float(ms))
            off, on = float(np.median(times[False])), float(np.median(times[True]))
            moved = B * M * Hn * n * (12 + 12) + B * M * n * 4                         # fev in, three planes out, the I plane in
            res["forecast_call"] = {"ms_store_off": off, "ms_store_on": on, "ratio_on_to_off": on / off, "ms_all_off": times[False],
                                    "ms_all_on": times[True], "keep_ms_per_batch_by_difference": on - off,
                                    "keep_bytes_per_batch": moved,
                                    "keep_GBps_by_difference": moved / max(on - off, 1e-6) / 1e6}
            print(f"forecast of {n} x {B} draws, H = {Hn}: store off {off:.3f} ms, on {on:.3f} ms ({on / off:.4f}); "
                  f"k_forecast_keep ~ {on - off:.3f} ms for {moved / 1e6:.0f} MB", file=sys.stderr, flush=True)

            # ---- the burst by both routes: the same integers ----------------------------------------------------------
            ranks = Q.quantile_ranks(n, probs)
            dev_own = s.forecast_order_stats(ranks)                                    # the store holds the last timed call's n draws
            rp = Q.quantile_ranks(n * B, probs)
            dev_pool = s.forecast_order_stats(rp, pooled=True)
            t0 = time.perf_counter()
            tr = s.read_trace(n)
            t_read = time.perf_counter() - t0
            planes = []
            for b in range(B):
                th, e = tr.theta[:, b], tr.events[:, b]
                tot = e.sum(axis=2, dtype=np.int64)
                i0 = init.astype(np.int64)
                st0 = np.stack([i0[:, 0] - tot[..., 0], i0[:, 1] + tot[..., 0] - tot[..., 1], i0[:, 2] + tot[..., 1] - tot[..., 2],
                                i0[:, 3] + tot[..., 2]], axis=-1)
                a_path = predict.log_baseline_path(th[:, 5], th[:, 6:6 + T - 1], T, Hn)
                sim = model.simulate(th[:, :5], a_path, th[:, 6 + T - 1:], W, wd, st0.astype(np.float64), seed=5,
                                     first_draw_id=forecast_draw_id(b, 0)).astype(np.int64)
                ex = np.cumsum(sim, axis=2) - sim
                planes.append(np.stack([sim[..., 2], np.cumsum(sim[..., 2], axis=2),
                                        st0[:, :, None, 2] + ex[..., 1] - ex[..., 2]], axis=1))
            planes = np.stack(planes, axis=1)                                          # [n, B, 3, M, H]
            host_own = np.sort(planes, axis=0)[ranks]
            host_pool = np.sort(planes.reshape((-1,) + planes.shape[2:]), axis=0)[rp]
            t_host = time.perf_counter() - t0
            same = bool(np.array_equal(host_own, dev_own) and np.array_equal(host_pool, dev_pool))
            res["parents_route"] = {"seconds_per_burst": t_host, "of_which_reading_the_trace": t_read, "same_integers": same,
                                    "trace_bytes": int(tr.events.nbytes + tr.theta.nbytes),
                                    "simulated_bytes_over_pcie": int(n * B * M * Hn * 3 * 8),
                                    "seconds_for_the_store_extrapolated": t_host * cap / n}
            print(f"parent's route for the burst: {t_host:.2f} s ({t_read:.2f} s reading the trace), same integers: {same}",
                  file=sys.stderr, flush=True)

            # ---- the full store: fill it with the burst forecast again and again (j goes on), then select --------------
            for _ in range(cap // n - 1):
                s.forecast(0, n)
            model.sync()
            full = cap // n * n
            sel = {}
            for pooled in (False, True):
                nn = full * (B if pooled else 1)
                r = Q.quantile_ranks(nn, probs)
                ms_all, wall_all = [], []
                for rep in range(a.reps + 1):
                    t0 = time.perf_counter()
                    model.timer_start()
                    st = s.forecast_order_stats(r, pooled=pooled)
                    ms = model.timer_stop()
                    q = Q.interpolate(st, r, nn, probs)
                    wall = time.perf_counter() - t0
                    if rep:
                        ms_all.append(float(ms)); wall_all.append(wall)
                cells = int(np.prod(st.shape[1:]))
                sel["pooled" if pooled else "per_chain"] = {
                    "values_per_cell": nn, "cells": cells, "ranks": len(r), "ms_median": float(np.median(ms_all)), "ms_all": ms_all,
                    "python_call_seconds_median": float(np.median(wall_all)), "result_bytes": int(st.nbytes),
                    "store_bytes_read_once": cells * nn * 4, "quantiles_shape": list(q.shape),
                    "GBps_of_one_read_of_the_store": cells * nn * 4 / float(np.median(ms_all)) / 1e6}
                print(f"order statistics, {'pooled' if pooled else 'per chain'}: {len(r)} ranks of {cells} cells of {nn} values: "
                      f"{np.median(ms_all):.1f} ms", file=sys.stderr, flush=True)
            res["order_stats_full_store"] = sel
            res["device_route_seconds_for_the_store"] = (on - off) * 1e-3 * cap / n + \
                (sel["per_chain"]["ms_median"] + sel["pooled"]["ms_median"]) * 1e-3
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

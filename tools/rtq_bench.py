#!/usr/bin/env python3
"""What the R_t intervals on the device cost and buy (GPU box, UK-380 x 8 chains, a 100-draw burst, D = 14, uint16 trace, a
store of 5000 draws per chain by default), in ONE call on one box:

  * `seir_sampler_rt` with the draw store off and on: HIP events (seir_timer_*) around `rt(0, n)` of a burst that lies in
    the trace, the two interleaved, median of --reps each.  With the store on k_rt_trace_keep runs in place of k_rt_trace,
    so the difference of the medians is what the staged writes add; it is set against the bytes written,
    B x D x M x n x 8;
  * k_order_stats_f64 for the ranks of K = 3 probabilities over the full store, per chain and pooled over the chains: HIP
    events around the blocking call (selection and the copy of the [R, cells] result) and the wall clock of the Python
    call with the interpolation;
  * the parent's route to the same bits, for the burst: read the trace, `seir_reproduction_number` on its draws
    ([n, T, M] fp64 over PCIe) and np.sort.  The order statistics of the two routes are compared before anything is
    recorded.

    python tools/rtq_bench.py [--out profiles/r16_rtq.json]"""
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
    ap.add_argument("--days", type=int, default=14)
    ap.add_argument("--store", type=int, default=5000, help="draws per chain the store is sized and filled for")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--probs", default="0.05,0.5,0.95")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_rtq.json"))
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import torch
    from covid19uk_amd import synth
    from covid19uk_amd.posterior import quantiles as Q
    from covid19uk_amd.sampler import ChainSampler
    from covid19uk_amd.seir import SeirModel
    cfg = dict(dmax=84, nmax=25, m=2, occult_nmax=15, num_event_time_updates=5)       # example_config.yaml:26-30
    cov = synth.make_covariates(a.workload)
    events, init, truth = synth.simulate_epidemic(cov)
    u0 = synth.unconstrain(synth.pack_params(truth, cov.M, cov.T))
    M, T, B, n, D, cap = cov.M, cov.T, a.chains, a.draws, a.days, a.store
    probs = Q.parse_probs(a.probs, name="probs")
    N = np.asarray(cov.N, dtype=np.float64).reshape(-1)
    w = N / N.sum()
    u = synth.jitter_params(u0, B, scale=0.002, seed=7, T=T)
    ev = np.stack([events] * B)
    res = {"workload": a.workload, "M": M, "T": T, "chains": B, "draws": n, "days": D, "store_draws": cap,
           "probs": list(probs), "device": torch.cuda.get_device_name(0), "command": " ".join(sys.argv),
           "store_bytes": B * D * M * cap * 8}

    with SeirModel(cov, init, max_chains=B) as model:
        with ChainSampler(model, cfg, B, seed=1, trace_capacity=2 * n, record_events="u16") as s:
            s.set_state(u, ev)
            s.set_kernel(step_size=1.2e-5)
            s.reset_trace()
            s.run(n)
            # ---- the rt call, store off / on, interleaved ---------------------------------------------------------------
            times = {False: [], True: []}
            for rep in range(a.reps + 1):                                              # the first pair is untimed: first launches
                for keep in (False, True):
                    s.reset_rt(D, w)
                    s.keep_rt_draws(cap if keep else 0)
                    model.sync()
                    model.timer_start()
                    s.rt(0, n)
                    ms = model.timer_stop()
                    if rep:
                        times[keep].append(float(ms))
            off, on = float(np.median(times[False])), float(np.median(times[True]))
            written = B * D * M * n * 8
            res["rt_call"] = {"ms_store_off": off, "ms_store_on": on, "ratio_on_to_off": on / off, "ms_all_off": times[False],
                              "ms_all_on": times[True], "keep_ms_per_call_by_difference": on - off,
                              "keep_bytes_written_per_call": written, "store_bytes_of_the_call": B * D * M * n * 8,
                              "keep_GBps_by_difference": written / max(on - off, 1e-6) / 1e6}
            print(f"rt of {n} x {B} draws, D = {D}: store off {off:.3f} ms, on {on:.3f} ms ({on / off:.4f}); "
                  f"the staged writes ~ {on - off:.3f} ms for {written / 1e6:.1f} MB", file=sys.stderr, flush=True)

            # ---- the burst by both routes: the same bits --------------------------------------------------------------
            ranks = Q.quantile_ranks(n, probs)
            dev_own = s.rt_order_stats(ranks)                                          # the store holds the last timed call's n draws
            rp = Q.quantile_ranks(n * B, probs)
            dev_pool = s.rt_order_stats(rp, pooled=True)
            t0 = time.perf_counter()
            tr = s.read_trace(n)
            t_read = time.perf_counter() - t0
            with SeirModel(cov, init, max_chains=16) as ref:                           # a context of its own, as the tests use
                R = ref.reproduction_number(tr.theta.reshape(n * B, -1),
                                            tr.events.reshape((n * B,) + tr.events.shape[2:]).astype(np.float64))
            R = R.reshape(n, B, T, M)[:, :, T - D:]
            host_own = np.sort(R, axis=0)[ranks]
            host_pool = np.sort(R.reshape((-1,) + R.shape[2:]), axis=0)[rp]
            t_host = time.perf_counter() - t0
            same = bool(np.array_equal(host_own.view(np.uint64), dev_own.view(np.uint64)) and
                        np.array_equal(host_pool.view(np.uint64), dev_pool.view(np.uint64)))
            res["parents_route"] = {"seconds_per_burst": t_host, "of_which_reading_the_trace": t_read, "same_bits": same,
                                    "trace_bytes": int(tr.events.nbytes + tr.theta.nbytes),
                                    "R_it_bytes_over_pcie": int(n * B * T * M * 8),
                                    "seconds_for_the_store_extrapolated": t_host * cap / n}
            print(f"parent's route for the burst: {t_host:.2f} s ({t_read:.2f} s reading the trace), same bits: {same}",
                  file=sys.stderr, flush=True)

            # ---- the full store: fill it with the burst folded again and again (count goes on), then select ------------
            for _ in range(cap // n - 1):
                s.rt(0, n)
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
                    st = s.rt_order_stats(r, pooled=pooled)
                    ms = model.timer_stop()
                    q = Q.interpolate(st, r, nn, probs)
                    wall = time.perf_counter() - t0
                    if rep:
                        ms_all.append(float(ms)); wall_all.append(wall)
                cells = int(np.prod(st.shape[1:]))
                sel["pooled" if pooled else "per_chain"] = {
                    "values_per_cell": nn, "cells": cells, "ranks": len(r), "ms_median": float(np.median(ms_all)), "ms_all": ms_all,
                    "python_call_seconds_median": float(np.median(wall_all)), "result_bytes": int(st.nbytes),
                    "store_bytes_read_once": cells * nn * 8, "quantiles_shape": list(q.shape),
                    "GBps_of_one_read_of_the_store": cells * nn * 8 / float(np.median(ms_all)) / 1e6}
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

#!/usr/bin/env python3
"""What the in-sample check on the device costs and buys (GPU box, UK-380 x 8 chains, a 100-draw burst, K = 14 and 56 by
default), in ONE call on one box:

  * the check call alone: HIP events (seir_timer_*) around `check(0, n)` of a burst that lies in the trace, median of
    --reps, next to the time of the burst's own sweeps measured in the same call;
  * the sampling phase with the check off / on: `sample_bursts` with the summaries on and the event tensors kept on the
    device (what `summaries: only` runs), a consumer that does nothing, against the device-only rate (`run` between two
    HIP events, nothing read back) of the same call;
  * the parent's way to the same integers, as the point of comparison: read the burst's trace, NumPy sums for the state
    at day T - K, `seir_simulate` per chain (which returns [n, M, K, 3] fp64 over PCIe), NumPy moments and comparisons.
    The integers of the two routes are compared before the ratio is recorded.

    python tools/check_bench.py [--out profiles/r12_check.json]"""
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
    ap.add_argument("--days", type=int, nargs="+", default=[14, 56])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bursts", type=int, default=4)
    ap.add_argument("--device-sweeps", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_check.json"))
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import torch
    from covid19uk_amd import synth
    from covid19uk_amd.posterior import predict
    from covid19uk_amd.sampler import ChainSampler, forecast_draw_id
    from covid19uk_amd.seir import SeirModel
    cfg = dict(dmax=84, nmax=25, m=2, occult_nmax=15, num_event_time_updates=5)       # example_config.yaml:26-30
    cov = synth.make_covariates(a.workload)
    events, init, truth = synth.simulate_epidemic(cov)
    u0 = synth.unconstrain(synth.pack_params(truth, cov.M, cov.T))
    M, T, B, n, nb = cov.M, cov.T, a.chains, a.draws, a.bursts
    u = synth.jitter_params(u0, B, scale=0.002, seed=7, T=T)
    ev = np.stack([events] * B)
    res = {"workload": a.workload, "M": M, "T": T, "chains": B, "draws": n, "device": torch.cuda.get_device_name(0),
           "command": " ".join(sys.argv), "check_call": [], "parents_route": []}

    with SeirModel(cov, init, max_chains=B) as model:
        with ChainSampler(model, cfg, B, seed=1, trace_capacity=2 * n, record_events="u16") as s:
            s.set_state(u, ev)
            s.set_kernel(step_size=1.2e-5)
            s.reset_trace()
            model.timer_start()
            s.run(n)
            burst_ms = model.timer_stop()
            tr = None
            for K in a.days:
                W, wd = predict.check_calendar(cov, None, T, K)
                s.reset_check(K, W, wd, 5)
                s.check(0, n)                                                          # untimed: first launches
                model.sync()
                times = []
                for _ in range(a.reps):
                    s.reset_check(K, W, wd, 5)
                    model.timer_start()
                    s.check(0, n)
                    times.append(model.timer_stop())
                ms = float(np.median(times))
                res["check_call"].append({"days": K, "ms_median": ms, "ms_min": float(min(times)), "ms_all": [float(t) for t in times],
                                          "launches": 2 * K + 5, "us_per_draw_day": ms * 1e3 / (n * B * K),
                                          "burst_sweeps_ms": burst_ms, "share_of_the_bursts_sweeps": ms / burst_ms})
                print(f"check of {n} x {B} draws, K = {K}: {ms:.2f} ms; the burst's sweeps {burst_ms:.1f} ms ({ms / burst_ms:.3f})",
                      file=sys.stderr, flush=True)
                cs, marg = s.check_summary(), s.read_check_marginals(n)

                # ---- the parent's way: trace over PCIe, NumPy state, seir_simulate per chain, NumPy comparisons -------------
                t0 = time.perf_counter()
                tr = s.read_trace(n)
                t_read = time.perf_counter() - t0
                same = True
                for b in range(B):
                    th, e = tr.theta[:, b], tr.events[:, b]
                    tot = e[:, :, :T - K].sum(axis=2, dtype=np.int64)
                    i0 = init.astype(np.int64)
                    st0 = np.stack([i0[:, 0] - tot[..., 0], i0[:, 1] + tot[..., 0] - tot[..., 1], i0[:, 2] + tot[..., 1] - tot[..., 2],
                                    i0[:, 3] + tot[..., 2]], axis=-1)
                    a_path = predict.log_baseline_path(th[:, 5], th[:, 6:6 + T - 1], T - K, K)
                    sim = model.simulate(th[:, :5], a_path, th[:, 6 + T - 1:], W, wd, st0.astype(np.float64), seed=5,
                                         first_draw_id=forecast_draw_id(b, 0)).astype(np.int64)
                    ex = np.cumsum(sim, axis=2) - sim
                    x = np.concatenate([sim, np.stack([st0[:, :, None, 0] - ex[..., 0], st0[:, :, None, 1] + ex[..., 0] - ex[..., 1],
                                                       st0[:, :, None, 2] + ex[..., 1] - ex[..., 2]], axis=-1)], axis=-1)
                    d = x - x[0]
                    obs = e[:, :, T - K:, 2].astype(np.int64)
                    y = sim[..., 2]
                    same = (same and np.array_equal(x[0], cs.moments.ref[b]) and np.array_equal(d.sum(axis=0), cs.moments.sum[b])
                            and np.array_equal((d * d).sum(axis=0).astype(np.uint64), cs.moments.sumsq[b])
                            and np.array_equal(sim.sum(axis=1), marg["check_by_day"][:, b])
                            and np.array_equal((y < obs).sum(axis=0), cs.lt[b]) and np.array_equal((y == obs).sum(axis=0), cs.eq[b])
                            and np.array_equal((y.sum(axis=2) < obs.sum(axis=2)).sum(axis=0), cs.location_lt[b])
                            and np.array_equal((y.sum(axis=1) == obs.sum(axis=1)).sum(axis=0), cs.day_eq[b])
                            and int((y.sum(axis=(1, 2)) < obs.sum(axis=(1, 2))).sum()) == int(cs.total_lt[b]))
                t_host = time.perf_counter() - t0
                res["parents_route"].append({"days": K, "seconds": t_host, "of_which_reading_the_trace": t_read,
                                             "same_integers": bool(same), "trace_bytes": int(tr.events.nbytes + tr.theta.nbytes),
                                             "simulated_bytes_over_pcie": int(n * B * M * K * 3 * 8), "device_call_ms": ms,
                                             "ratio_to_the_device_call": t_host * 1e3 / ms})
                print(f"parent's route, K = {K}: {t_host:.2f} s ({t_read:.2f} s reading the trace), same integers: {same}; "
                      f"{t_host * 1e3 / ms:.0f} x the device call", file=sys.stderr, flush=True)

            # ---- the sampling phase, check off / on, against the device-only rate ------------------------------------------
            K = a.days[0]
            W, wd = predict.check_calendar(cov, None, T, K)
            s.reset_trace()
            model.timer_start()
            s.run(a.device_sweeps)
            dms = model.timer_stop()
            dev_rate = B * a.device_sweeps / (dms * 1e-3)
            res["device_only"] = {"sweeps": a.device_sweeps, "ms_per_sweep": dms / a.device_sweeps, "sweeps_per_s": dev_rate}
            res["sampling_phase"] = []
            for ck in (False, True, False, True):
                kw = dict(events=False, summarize=True, **(dict(check=True) if ck else {}))
                s.reset_check(K, W, wd, 5)
                s.sample_bursts(2, n, lambda tr, i: None, **kw)                        # untimed: page-locks the host buffers
                s.reset_summary()
                s.reset_check(K, W, wd, 5)
                t0 = time.perf_counter()
                s.sample_bursts(nb, n, lambda tr, i: None, **kw)
                model.sync()
                dt = time.perf_counter() - t0
                rate = nb * n * B / dt
                res["sampling_phase"].append({"check": ck, "days": K, "sweeps": nb * n, "seconds": dt, "sweeps_per_s": rate,
                                              "of_device_only": rate / dev_rate, "recoveries": len(s.recoveries)})
                print(f"sampling phase, check {ck}: {rate:.0f} sweeps/s, {rate / dev_rate:.3f} of device-only {dev_rate:.0f}",
                      file=sys.stderr, flush=True)
            on = np.mean([r["sweeps_per_s"] for r in res["sampling_phase"] if r["check"]])
            off = np.mean([r["sweeps_per_s"] for r in res["sampling_phase"] if not r["check"]])
            res["sampling_phase_on_over_off"] = float(on / off)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the forecast on the device costs and buys (GPU box, UK-380 x 8 chains, a 100-draw burst, H = 56 by default), in ONE
call on one box:

  * the forecast call alone: HIP events (seir_timer_*) around `forecast(0, n)` of a burst that lies in the trace, next to
    the time of the burst's own sweeps.  Per-kernel shares come from a run of their own,
        rocprofv3 --kernel-trace --stats -d DIR -- python tools/forecast_bench.py --kernels-only
    (no counters in that run); `--kernel-stats DIR/.../*_kernel_stats.csv` folds that table into the JSON;
  * the sampling phase with the forecast off / on: `sample_bursts` with the summaries on and the event tensors kept on
    the device (what `summaries: only` runs), a consumer that does nothing, against the device-only rate (`run` between
    two HIP events, nothing read back) of the same call;
  * the parent's way to the same numbers, as the point of comparison: read the burst's trace, host sums over T for the
    state at day T, `seir_simulate` per chain (which returns [n, M, H, 3] fp64 over PCIe), NumPy moments and marginals.
    The integers of the two routes are compared before the ratio is recorded.

    python tools/forecast_bench.py [--out profiles/r09_forecast.json]"""
import argparse
import csv
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bursts", type=int, default=4)
    ap.add_argument("--device-sweeps", type=int, default=300)
    ap.add_argument("--kernels-only", action="store_true", help="one burst and --reps forecast calls, nothing else (for rocprofv3)")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv of a --kernels-only run")
    ap.add_argument("--lib", default=None, help="load this libseirhip.so in place of the tree's: another build of the same ABI, "
                    "for an A/B in one call (profiles/r10_ab.txt)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_forecast.json"))
    a = ap.parse_args()
    if a.lib:
        from covid19uk_amd import _lib
        _lib.LIB_PATH = os.path.abspath(a.lib)
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
    M, T, B, n, Hn, nb = cov.M, cov.T, a.chains, a.draws, a.horizon, a.bursts
    W, wd = predict.forecast_calendar(cov, None, T, Hn)
    u = synth.jitter_params(u0, B, scale=0.002, seed=7, T=T)
    ev = np.stack([events] * B)
    res = {"workload": a.workload, "M": M, "T": T, "chains": B, "draws": n, "horizon": Hn,
           "device": torch.cuda.get_device_name(0), "command": " ".join(sys.argv)}

    with SeirModel(cov, init, max_chains=B) as model:
        with ChainSampler(model, cfg, B, seed=1, trace_capacity=2 * n, record_events="u16") as s:
            s.set_state(u, ev)
            s.set_kernel(step_size=1.2e-5)
            s.reset_forecast(Hn, W, wd, 5)
            s.reset_trace()
            model.timer_start()
            s.run(n)
            burst_ms = model.timer_stop()
            s.forecast(0, n)                                                           # untimed: first launches
            model.sync()
            times = []
            for _ in range(a.reps):
                s.reset_forecast(Hn, W, wd, 5)
                model.timer_start()
                s.forecast(0, n)
                times.append(model.timer_stop())
            ms = float(np.median(times))
            res["forecast_call"] = {"ms_median": ms, "ms_min": float(min(times)), "ms_all": [float(t) for t in times],
                                    "launches": 2 * Hn + 3, "us_per_draw_day": ms * 1e3 / (n * B * Hn),
                                    "burst_sweeps_ms": burst_ms, "share_of_the_bursts_sweeps": ms / burst_ms}
            print(f"forecast of {n} x {B} draws, H = {Hn}: {ms:.2f} ms; the burst's sweeps {burst_ms:.1f} ms "
                  f"({ms / burst_ms:.3f})", file=sys.stderr, flush=True)
            if a.kernels_only:
                print(json.dumps(res))
                return
            if a.kernel_stats:
                rows = list(csv.DictReader(open(a.kernel_stats)))
                name = next(k for k in rows[0] if k.lower() in ("name", "kernelname", "kernel_name"))
                tot = next(k for k in rows[0] if k.lower() in ("totaldurationns", "total_duration_ns", "totalduration"))
                mine = [r for r in rows if "forecast" in r[name] or "k_gemm" in r[name]]
                total = sum(float(r[tot]) for r in mine)
                res["forecast_call"]["kernel_shares"] = {r[name].split("(")[0]: float(r[tot]) / total for r in mine}
            device = (s.forecast_summary(), s.read_forecast_marginals(n))

            # ---- the parent's way: trace over PCIe, host sums, seir_simulate per chain, NumPy ------------------------------
            t0 = time.perf_counter()
            tr = s.read_trace(n)
            t_read = time.perf_counter() - t0
            sums = {k: [] for k in ("ref", "sum", "sumsq", "by_day")}
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
                x = np.concatenate([sim, np.stack([st0[:, :, None, 0] - ex[..., 0], st0[:, :, None, 1] + ex[..., 0] - ex[..., 1],
                                                   st0[:, :, None, 2] + ex[..., 1] - ex[..., 2]], axis=-1)], axis=-1)
                d = x - x[0]
                sums["ref"].append(x[0]); sums["sum"].append(d.sum(axis=0)); sums["sumsq"].append((d * d).sum(axis=0))
                sums["by_day"].append(sim.sum(axis=1))
            t_host = time.perf_counter() - t0
            same = (np.array_equal(np.stack(sums["ref"]), device[0].ref) and np.array_equal(np.stack(sums["sum"]), device[0].sum)
                    and np.array_equal(np.stack(sums["sumsq"]).astype(np.uint64), device[0].sumsq)
                    and np.array_equal(np.stack(sums["by_day"], axis=1), device[1]["forecast_by_day"]))
            res["parents_route"] = {"seconds": t_host, "of_which_reading_the_trace": t_read, "same_integers": bool(same),
                                    "trace_bytes": int(tr.events.nbytes + tr.theta.nbytes),
                                    "simulated_bytes_over_pcie": int(n * B * M * Hn * 3 * 8),
                                    "device_call_ms": ms, "ratio_to_the_device_call": t_host * 1e3 / ms}
            print(f"parent's route: {t_host:.2f} s ({t_read:.2f} s reading the trace), same integers: {same}; "
                  f"{t_host * 1e3 / ms:.0f} x the device call", file=sys.stderr, flush=True)

            # ---- the sampling phase, forecast off / on, against the device-only rate ---------------------------------------
            s.reset_trace()
            model.timer_start()
            s.run(a.device_sweeps)
            dms = model.timer_stop()
            dev_rate = B * a.device_sweeps / (dms * 1e-3)
            res["device_only"] = {"sweeps": a.device_sweeps, "ms_per_sweep": dms / a.device_sweeps, "sweeps_per_s": dev_rate}
            res["sampling_phase"] = []
            for fc in (False, True):
                kw = dict(events=False, summarize=True, **(dict(forecast=True) if fc else {}))
                s.sample_bursts(2, n, lambda tr, i: None, **kw)                        # untimed: page-locks the host buffers
                s.reset_summary()
                s.reset_forecast(Hn, W, wd, 5)
                t0 = time.perf_counter()
                s.sample_bursts(nb, n, lambda tr, i: None, **kw)
                model.sync()
                dt = time.perf_counter() - t0
                rate = nb * n * B / dt
                res["sampling_phase"].append({"forecast": fc, "sweeps": nb * n, "seconds": dt, "sweeps_per_s": rate,
                                              "of_device_only": rate / dev_rate, "recoveries": len(s.recoveries)})
                print(f"sampling phase, forecast {fc}: {rate:.0f} sweeps/s, {rate / dev_rate:.3f} of device-only {dev_rate:.0f}",
                      file=sys.stderr, flush=True)
            res["sampling_phase"][1]["of_off"] = res["sampling_phase"][1]["sweeps_per_s"] / res["sampling_phase"][0]["sweeps_per_s"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

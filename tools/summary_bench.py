#!/usr/bin/env python3
"""What the device-side summaries cost and buy (GPU box, UK-380 by default), in ONE call on one box:

  * k_summarize alone: HIP events (seir_timer_*) around `summarize` of a 100-draw burst, for 8 chains and for 1, uint16 and
    int32 trace, marginals only and with the moments folded.  The bytes are computed from the shapes (trace read once,
    accumulators in and out at 20 B per cell and quantity, marginals written); achieved bytes/s and the share of the
    8 TB/s peak are stated as such, next to the floor the same bytes give at the peak;
  * end to end: the sampling phase of `run_mcmc` at thin 1 -- ChainSampler.sample_bursts into one posterior.hd5 per chain,
    device -> host -> HDF5 included -- with summaries off, on and only, for 1 and for 8 chains, and the device-only rate
    (`run` between two HIP events, nothing read back) measured in the same call.

    python tools/summary_bench.py [--out profiles/r07_summary.json]
    python tools/summary_bench.py --diagnostics --out profiles/r08_diag.json

With --diagnostics every folding row of the kernel table is followed by the same call with the convergence diagnostics on
(the DIAG instance of k_summarize: 16 B more per cell and quantity, read and written): the same burst in a second sampler,
the two timed in turns, launch by launch, with `of_the_same_call_without` the ratio of the medians and
`bytes_of_the_same_call_without` that of the derived bytes.  The end-to-end table gains `off+diag` and `only+diag`: the
sampling phase as `run_mcmc` runs it with `diagnostics: on` (marks, the parameters' accumulators on the host, diagnostics()
and the group diagnostics/ at the end).

Every timed folding launch is the second of two after a reset (the first untimed): what a run's second burst costs, with
nothing piling up from one repetition to the next.

Rates are sweeps per second summed over the chains; `of_device_only` is the ratio to the device-only rate of the same
number of chains, `of_off` the ratio to the `off` row of the same call."""
import argparse
import contextlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
PEAK = 8.0e12          # bytes/s, the MI355X's HBM3E peak


def kernel_bytes(B, M, T, n, width, fold, diag=False):
    trace = n * B * M * T * 3 * width
    acc = 2 * B * M * T * 6 * (36 if diag else 20) if fold else 0 # ref + sum + sumsq (+ bsum + bsumsq), read and written once per call
    marg = n * B * (2 * T * 3 + M * 3) * 8
    return trace + acc + marg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="uk380")
    ap.add_argument("--chains", default="8,1")
    ap.add_argument("--draws", type=int, default=100, help="draws per burst for the kernel timing")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bursts", type=int, default=4)
    ap.add_argument("--kept-per-burst", default="20,50", help="kept draws per burst end to end, per entry of --chains")
    ap.add_argument("--device-sweeps", type=int, default=400)
    ap.add_argument("--diagnostics", action="store_true", help="add the diagnostics rows (see above)")
    ap.add_argument("--kernels-only", action="store_true", help="the kernel table alone, not the sampling phase through the file")
    ap.add_argument("--lib", default=None, help="load this libseirhip.so in place of the tree's: another build of the same ABI, "
                    "for an A/B in one call (profiles/r10_ab.txt)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_summary.json"))
    a = ap.parse_args()
    if a.lib:
        from covid19uk_amd import _lib
        _lib.LIB_PATH = os.path.abspath(a.lib)
    import __graft_entry__ as entry
    entry.build()
    import torch
    from covid19uk_amd import synth
    from covid19uk_amd.inference import inference as inf
    from covid19uk_amd.posterior import diagnostics as dm
    from covid19uk_amd.sampler import ChainSampler
    from covid19uk_amd.seir import SeirModel
    cfg = dict(dmax=84, nmax=25, m=2, occult_nmax=15, num_event_time_updates=5)       # example_config.yaml:26-30
    cov = synth.make_covariates(a.workload)
    events, init, truth = synth.simulate_epidemic(cov)
    u0 = synth.unconstrain(synth.pack_params(truth, cov.M, cov.T))
    M, T = cov.M, cov.T
    chains = [int(x) for x in a.chains.split(",")]
    kept = [int(x) for x in a.kept_per_burst.split(",")]
    n, nb = a.draws, a.bursts
    res = {"workload": a.workload, "M": M, "T": T, "device": torch.cuda.get_device_name(0), "command": " ".join(sys.argv),
           "peak_bytes_per_s": PEAK, "kernel": [], "end_to_end": []}

    # ---- k_summarize alone ------------------------------------------------------------------------------------------------
    def kernel_row(B, width, fold, diag, times, burst_ms):
        ms = float(np.median(times))
        nbytes = kernel_bytes(B, M, T, n, width, fold, diag)
        row = {"chains": B, "draws": n, "trace": "uint16" if width == 2 else "int32", "accumulate": fold, "diagnostics": diag,
               "ms_median": ms, "ms_min": float(min(times)), "ms_all": [float(t) for t in times],
               "bytes": nbytes, "floor_ms_at_peak": nbytes / PEAK * 1e3, "achieved_bytes_per_s": nbytes / (ms * 1e-3),
               "share_of_peak": nbytes / (ms * 1e-3) / PEAK, "burst_sweeps_ms": burst_ms,
               "share_of_the_bursts_sweeps": ms / burst_ms}
        res["kernel"].append(row)
        print(f"k_summarize chains {B} {row['trace']} fold {fold} diag {diag}: {ms:.3f} ms ({row['share_of_peak']:.3f} of peak, "
              f"floor {row['floor_ms_at_peak']:.3f} ms; the burst's sweeps {burst_ms:.1f} ms)", file=sys.stderr, flush=True)
        return row

    def burst_in_the_trace(stack, B, record, u, ev):
        """A sampler of its own context with one burst of n draws in its trace: (model, sampler, ms of the burst's sweeps)."""
        model = stack.enter_context(SeirModel(cov, init, max_chains=B))
        s = stack.enter_context(ChainSampler(model, cfg, B, seed=1, trace_capacity=n, record_events=record))
        s.set_state(u, ev)
        s.set_kernel(step_size=1.2e-5)
        s.reset_summary()
        s.reset_trace()
        model.timer_start()
        s.run(n)
        return model, s, model.timer_stop()

    def time_fold(model, s, reset):
        """One timed folding launch of the burst as a run's second burst sees it: accumulators started again and one burst
        folded (untimed) before it, so that no repetition piles up on the one before and ref is read, not set."""
        reset()
        s.summarize(0, n, True)
        model.sync()
        model.timer_start()
        s.summarize(0, n, True)
        return model.timer_stop()

    for B in chains:
        u = synth.jitter_params(u0, B, scale=0.002, seed=7, T=T)
        ev = np.stack([events] * B)
        for record, width in (("u16", 2), (True, 4)):
            with contextlib.ExitStack() as stack:
                model, s, burst_ms = burst_in_the_trace(stack, B, record, u, ev)
                s.summarize(0, n, False)                                               # untimed: first launch
                model.sync()
                times = []
                for _ in range(a.reps):
                    model.timer_start()
                    s.summarize(0, n, False)
                    times.append(model.timer_stop())
                kernel_row(B, width, False, False, times, burst_ms)
                if not a.diagnostics:
                    kernel_row(B, width, True, False, [time_fold(model, s, s.reset_summary) for _ in range(a.reps)], burst_ms)
                    continue
                # the same burst (same seed, same start) in a second sampler that has the diagnostics on; the two folding
                # instances are then timed in turns, one launch each, so that a drift of the box meets both alike
                model_d, s_d, _ = burst_in_the_trace(stack, B, record, u, ev)
                plain, diag = [], []
                for _ in range(a.reps):
                    plain.append(time_fold(model, s, s.reset_summary))
                    diag.append(time_fold(model_d, s_d, lambda: s_d.reset_diagnostics(n)))
                without = kernel_row(B, width, True, False, plain, burst_ms)
                row = kernel_row(B, width, True, True, diag, burst_ms)
                row["of_the_same_call_without"] = row["ms_median"] / without["ms_median"]
                row["bytes_of_the_same_call_without"] = row["bytes"] / without["bytes"]

    # ---- end to end: the sampling phase through the file --------------------------------------------------------------------
    for B, ns in [] if a.kernels_only else zip(chains, kept):
        u = synth.jitter_params(u0, B, scale=0.002, seed=7, T=T)
        ev = np.stack([events] * B)
        with SeirModel(cov, init, max_chains=B) as model:
            with ChainSampler(model, cfg, B, seed=1, trace_capacity=2 * ns, record_events="u16") as s:
                s.set_state(u, ev)
                s.set_kernel(step_size=1.2e-5)
                s.reset_trace()
                s.run(50)
                model.sync()
                s.reset_trace()
                model.timer_start()
                s.run(a.device_sweeps)
                ms = model.timer_stop()
                dev_rate = B * a.device_sweeps / (ms * 1e-3)
                row = {"chains": B, "kept_draws_per_burst": ns, "thin": 1,
                       "device_only": {"sweeps": a.device_sweeps, "ms_per_sweep": ms / a.device_sweeps, "sweeps_per_s": dev_rate},
                       "through_the_file": []}
                for mode in ("off", "on", "only") + (("off+diag", "only+diag") if a.diagnostics else ()):
                    diag = mode.endswith("+diag")
                    mode = mode.split("+")[0]
                    kw = {} if mode == "off" and not diag else dict(events=mode != "only", summarize=True)
                    marks = inf.diagnostics_marks(nb) if diag else {}
                    s.sample_bursts(2, ns, lambda tr, i: None, **kw)                   # untimed: page-locks the host buffers
                    with tempfile.TemporaryDirectory() as tmp:
                        pk = {} if mode == "off" else dict(summaries=mode)
                        posts = [inf.Posterior(os.path.join(tmp, f"posterior_chain{c}.hd5"), M, T, cfg["m"], nb * ns, burst=ns, **pk)
                                 for c in range(B)]
                        off = [0]

                        acc = dm.DrawAccumulator(ns) if diag else None

                        def flush(tr, i):                                              # run_mcmc's flush
                            if acc is not None:
                                acc.fold(tr.theta)
                                if i in marks:
                                    acc.mark(marks[i])
                            for c, post in enumerate(posts):
                                mk = {} if mode == "off" else dict(marginals=tr.marginals)
                                post.write_samples(inf.draws_to_dict(tr.theta, tr.events, c, **mk), first_dim_offset=off[0])
                                post.write_results(inf.trace_to_dict(tr, c), first_dim_offset=off[0])
                            off[0] += tr.theta.shape[0]
                        if diag:
                            s.reset_diagnostics(ns)
                        elif mode != "off":
                            s.reset_summary()
                        t0 = time.perf_counter()
                        s.sample_bursts(nb, ns, flush, **kw, **(dict(marks=marks) if diag else {}))
                        if diag:
                            ev = dm.evaluate(s.diagnostics(), acc.result())
                            for c, post in enumerate(posts):
                                post.write_diagnostics(dm.chain_datasets(ev, c))
                        if mode != "off":
                            sm = s.summary()
                            mean, var = sm.mean, sm.var
                            for c, post in enumerate(posts):
                                post.write_summary(sm.count[c], mean[c], var[c])
                        for post in posts:
                            post.close()
                        dt = time.perf_counter() - t0
                        fmt = "hdf5" if posts[0].use_h5 else "npz (no libhdf5 on this host)"
                        size = sum(os.path.getsize(p.filename) for p in posts)
                    rate = nb * ns * B / dt
                    row["through_the_file"].append({"summaries": mode, "diagnostics": "on" if diag else "off", "sweeps": nb * ns, "seconds": dt, "format": fmt,
                                                    "sweeps_per_s": rate, "of_device_only": rate / dev_rate, "file_gb": size / 1e9,
                                                    "recoveries": len(s.recoveries)})
                    print(f"chains {B} summaries {mode} diagnostics {diag}: {rate:.0f} sweeps/s, {rate / dev_rate:.3f} of device-only {dev_rate:.0f}",
                          file=sys.stderr, flush=True)
                base = row["through_the_file"][0]["sweeps_per_s"]
                for r in row["through_the_file"]:
                    r["of_off"] = r["sweeps_per_s"] / base
                res["end_to_end"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What thinning on the device buys end to end (GPU box, UK-380 by default), in ONE call on one box:

  * the device-only rate: `run` of 400 sweeps between two HIP events, nothing read back (bench.py's steady state);
  * the sampling phase of `run_mcmc` -- ChainSampler.sample_bursts into one posterior.hd5 per chain, the reference's schema
    (samples/seir float64 [n, M, T, 3]: 3.33 MB per kept draw at UK-380), warm-up excluded, device -> host -> HDF5 included
    -- at thin 1, 5 and 20, for 1 and for 8 chains.

    python tools/thin_bench.py [--out profiles/r06_thin.json]

Rates are in sweeps per second summed over the chains (kept draws per second = that / thin); `of_device_only` is the
ratio to the device-only rate of the same number of chains."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="uk380")
    ap.add_argument("--chains", default="1,8")
    ap.add_argument("--thin", default="1,5,20")
    ap.add_argument("--bursts", type=int, default=4)
    ap.add_argument("--kept-per-burst", default="50,20", help="kept draws per burst, per entry of --chains")
    ap.add_argument("--device-sweeps", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_thin.json"))
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import torch
    from covid19uk_amd import synth
    from covid19uk_amd.inference import inference as inf
    from covid19uk_amd.sampler import ChainSampler
    from covid19uk_amd.seir import SeirModel
    cfg = dict(dmax=84, nmax=25, m=2, occult_nmax=15, num_event_time_updates=5)       # example_config.yaml:26-30
    cov = synth.make_covariates(a.workload)
    events, init, truth = synth.simulate_epidemic(cov)
    u0 = synth.unconstrain(synth.pack_params(truth, cov.M, cov.T))
    M, T = cov.M, cov.T
    chains = [int(x) for x in a.chains.split(",")]
    kept = [int(x) for x in a.kept_per_burst.split(",")]
    thins = [int(x) for x in a.thin.split(",")]
    nb = a.bursts
    res = {"workload": a.workload, "M": M, "T": T, "device": torch.cuda.get_device_name(0), "command": " ".join(sys.argv),
           "bytes_per_kept_draw_in_file": 8 * 3 * M * T, "bursts": nb, "configs": []}
    for B, ns in zip(chains, kept):
        u = synth.jitter_params(u0, B, scale=0.002, seed=7, T=T)
        ev = np.stack([events] * B)
        with SeirModel(cov, init, max_chains=B) as model:
            with ChainSampler(model, cfg, B, seed=1, trace_capacity=2 * ns, record_events="u16") as s:
                s.set_state(u, ev)
                s.set_kernel(step_size=1.2e-5)
                s.reset_trace(); s.run(50); model.sync()
                s.reset_trace()
                model.timer_start()
                s.run(a.device_sweeps)
                ms = model.timer_stop()
                dev_rate = B * a.device_sweeps / (ms * 1e-3)
                row = {"chains": B, "kept_draws_per_burst": ns, "device_only": {"sweeps": a.device_sweeps, "ms_per_sweep": ms / a.device_sweeps,
                                                                             "sweeps_per_s": dev_rate}, "through_the_file": []}
                for k in thins:
                    s.set_thin(k)
                    s.sample_bursts(2, ns, lambda tr, i: None)                         # untimed: page-locks the host buffers
                    with tempfile.TemporaryDirectory() as tmp:
                        posts = [inf.Posterior(os.path.join(tmp, f"posterior_chain{c}.hd5"), M, T, cfg["m"], nb * ns, burst=ns)
                                 for c in range(B)]
                        off = [0]

                        def flush(tr, i):                                              # run_mcmc's flush
                            for c, post in enumerate(posts):
                                post.write_samples(inf.draws_to_dict(tr.theta, tr.events, c), first_dim_offset=off[0])
                                post.write_results(inf.trace_to_dict(tr, c), first_dim_offset=off[0])
                            off[0] += tr.theta.shape[0]
                        t0 = time.perf_counter()
                        s.sample_bursts(nb, ns, flush)
                        for post in posts:
                            post.close()
                        dt = time.perf_counter() - t0
                        fmt = "hdf5" if posts[0].use_h5 else "npz (no libhdf5 on this host)"
                    rate = nb * ns * k * B / dt
                    row["through_the_file"].append({"thin": k, "sweeps": nb * ns * k, "kept_draws": nb * ns, "seconds": dt, "format": fmt,
                                                    "sweeps_per_s": rate, "kept_draws_per_s": rate / k, "of_device_only": rate / dev_rate,
                                                    "file_gb": B * nb * ns * 8 * 3 * M * T / 1e9, "recoveries": len(s.recoveries)})
                    print(f"chains {B} thin {k}: {rate:.0f} sweeps/s, {rate / k:.0f} kept/s, {rate / dev_rate:.3f} of device-only "
                          f"{dev_rate:.0f}", file=sys.stderr, flush=True)
                res["configs"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

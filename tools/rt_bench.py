#!/usr/bin/env python3
"""What the reproduction number on the device costs and buys (GPU box, UK-380 x 8 chains, a 100-draw burst, uint16 trace),
in ONE call on one box:

  * the `rt` call alone at D = 14 and at D = T: HIP events (seir_timer_*) around `rt(0, n)` of a burst that lies in the
    trace, median of --reps, next to the time of the burst's own sweeps in the same call;
  * the sampling phase with the feature off / on (D = 14): `sample_bursts` with the summaries on and the event tensors kept
    on the device (what `summaries: only` runs), a consumer that does nothing, against the device-only rate;
  * the parent's way to the same numbers, as the point of comparison: read the burst's trace, `seir_reproduction_number`
    chain by chain (fp64 events up over PCIe, R_it [n, T, M] back), the NumPy fold in draw order.  The accumulators of the
    two routes are compared bit for bit before the ratio is recorded;
  * what bounds k_rt_trace: the cell evaluations per second it reaches against the chip's fp64 vector rate, with the
    compiler's account of the kernel (registers, occupancy, LDS).  That figure is derived from the timing, not read from
    counters, and is marked so.

    python tools/rt_bench.py [--out profiles/r11_rt.json] [--lib other/libseirhip.so]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

FLOP_PER_CELL = 25            # fp64 vector operations of one rt_cell (the series branch of prob_of_rate), FMA = 1
PEAK_FP64_VALU = 78.6e12      # MI355X fp64 vector peak, FMA counted as two: flop / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="uk380")
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--draws", type=int, default=100, help="kept draws per burst")
    ap.add_argument("--days", type=int, nargs="*", default=None, help="windows to time (default: 14 and T)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bursts", type=int, default=4)
    ap.add_argument("--device-sweeps", type=int, default=300)
    ap.add_argument("--no-parent", action="store_true", help="skip the parent's route")
    ap.add_argument("--lib", default=None, help="load this libseirhip.so in place of the tree's: another build of the same ABI")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_rt.json"))
    a = ap.parse_args()
    if a.lib:
        from covid19uk_amd import _lib
        _lib.LIB_PATH = os.path.abspath(a.lib)
    import __graft_entry__ as entry
    entry.build()
    import torch
    from covid19uk_amd import synth
    from covid19uk_amd.sampler import ChainSampler
    from covid19uk_amd.seir import SeirModel
    cfg = dict(dmax=84, nmax=25, m=2, occult_nmax=15, num_event_time_updates=5)       # example_config.yaml:26-30
    cov = synth.make_covariates(a.workload)
    events, init, truth = synth.simulate_epidemic(cov)
    u0 = synth.unconstrain(synth.pack_params(truth, cov.M, cov.T))
    M, T, B, n, nb = cov.M, cov.T, a.chains, a.draws, a.bursts
    days = a.days or [min(14, T), T]
    N = np.asarray(cov.N, dtype=np.float64).reshape(-1)
    w = N / N.sum()
    u = synth.jitter_params(u0, B, scale=0.002, seed=7, T=T)
    ev = np.stack([events] * B)
    res = {"workload": a.workload, "M": M, "T": T, "chains": B, "draws": n, "device": torch.cuda.get_device_name(0),
           "command": " ".join(sys.argv), "rt_call": []}
    try:
        kr = json.load(open(entry.RESOURCES))["k_rt_trace<4>"]
    except (OSError, KeyError):
        kr = None

    with SeirModel(cov, init, max_chains=B) as model:
        with ChainSampler(model, cfg, B, seed=1, trace_capacity=2 * n, record_events="u16") as s:
            s.set_state(u, ev)
            s.set_kernel(step_size=1.2e-5)
            s.reset_trace()
            model.timer_start()
            s.run(n)
            burst_ms = model.timer_stop()
            device = {}
            for D in days:
                s.reset_rt(D, w)
                s.rt(0, n)                                                             # untimed: first launches
                model.sync()
                times = []
                for _ in range(a.reps):
                    s.reset_rt(D, w)
                    model.timer_start()
                    s.rt(0, n)
                    times.append(model.timer_stop())
                ms = float(np.median(times))
                cells = float(n) * B * D * M * M
                rate = cells / (ms * 1e-3)
                share = rate * FLOP_PER_CELL * 2 / PEAK_FP64_VALU
                res["rt_call"].append({
                    "days": D, "ms_median": ms, "ms_min": float(min(times)), "ms_all": [float(t) for t in times],
                    "cell_evaluations": cells, "cell_evaluations_per_s": rate, "burst_sweeps_ms": burst_ms,
                    "share_of_the_bursts_sweeps": ms / burst_ms,
                    "derived_share_of_fp64_valu_peak": share,
                    "limited_by": ("fp64 VALU" if share > 0.5 else "occupancy / latency (fewer workgroups than the chip holds, or "
                                   "waiting on LDS and the draw loop's barriers)") + " -- derived from the timing, not from counters",
                    "k_rt_trace_resources": kr})
                print(f"rt of {n} x {B} draws, D = {D}: {ms:.2f} ms ({rate:.3g} cells/s, {share:.2f} of the fp64 vector peak by "
                      f"{FLOP_PER_CELL} operations a cell); the burst's sweeps {burst_ms:.1f} ms ({ms / burst_ms:.3f})",
                      file=sys.stderr, flush=True)
                device[D] = (s.rt_summary(), s.read_rt_draws(n))

            # ---- the parent's way: trace over PCIe, seir_reproduction_number chain by chain, NumPy fold ------------------
            if not a.no_parent:
                t0 = time.perf_counter()
                tr = s.read_trace(n)
                t_read = time.perf_counter() - t0
                acc = {D: {k: [] for k in ("ref", "sum", "sumsq", "gt1")} for D in days}
                with SeirModel(cov, init, max_chains=50) as ref_model:                 # CHUNKSIZE of posterior.reproduction_number
                    t1 = time.perf_counter()
                    for b in range(B):
                        R = ref_model.reproduction_number(tr.theta[:, b], tr.events[:, b].astype(np.float64))
                        for D in days:
                            Rw = R[:, T - D:]
                            ref = Rw[0].copy()
                            sm, sq = np.zeros_like(ref), np.zeros_like(ref)
                            for r in Rw:
                                d = r - ref
                                sm = sm + d
                                sq = sq + d * d
                            acc[D]["ref"].append(ref); acc[D]["sum"].append(sm); acc[D]["sumsq"].append(sq)
                            acc[D]["gt1"].append((Rw > 1.0).sum(axis=0).astype(np.uint32))
                    t_host = time.perf_counter() - t1 + t_read
                same = all(np.array_equal(np.stack(acc[D][k]), getattr(device[D][0], k)) for D in days for k in acc[D])
                res["parents_route"] = {"seconds": t_host, "of_which_reading_the_trace": t_read, "same_bits": bool(same),
                                        "trace_bytes": int(tr.events.nbytes + tr.theta.nbytes),
                                        "events_up_over_pcie_bytes": int(n * B * M * T * 3 * 8),
                                        "R_it_down_over_pcie_bytes": int(n * B * T * M * 8),
                                        "ratio_to_the_device_calls": t_host * 1e3 / sum(c["ms_median"] for c in res["rt_call"])}
                print(f"parent's route: {t_host:.2f} s ({t_read:.2f} s reading the trace), same bits: {same}", file=sys.stderr, flush=True)

            # ---- the sampling phase, feature off / on, against the device-only rate ----------------------------------------
            D = days[0]
            s.reset_trace()
            model.timer_start()
            s.run(a.device_sweeps)
            dms = model.timer_stop()
            dev_rate = B * a.device_sweeps / (dms * 1e-3)
            res["device_only"] = {"sweeps": a.device_sweeps, "ms_per_sweep": dms / a.device_sweeps, "sweeps_per_s": dev_rate}
            res["sampling_phase"] = []
            for on in (False, True):
                kw = dict(events=False, summarize=True, **(dict(rt=True) if on else {}))
                s.reset_rt(D, w)
                s.sample_bursts(2, n, lambda tr, i: None, **kw)                        # untimed: page-locks the host buffers
                s.reset_summary()
                s.reset_rt(D, w)
                t0 = time.perf_counter()
                s.sample_bursts(nb, n, lambda tr, i: None, **kw)
                model.sync()
                dt = time.perf_counter() - t0
                rate = nb * n * B / dt
                res["sampling_phase"].append({"rt": on, "days": D, "sweeps": nb * n, "seconds": dt, "sweeps_per_s": rate,
                                              "of_device_only": rate / dev_rate, "recoveries": len(s.recoveries)})
                print(f"sampling phase, rt {on}: {rate:.0f} sweeps/s, {rate / dev_rate:.3f} of device-only {dev_rate:.0f}",
                      file=sys.stderr, flush=True)
            res["sampling_phase"][1]["of_off"] = res["sampling_phase"][1]["sweeps_per_s"] / res["sampling_phase"][0]["sweeps_per_s"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

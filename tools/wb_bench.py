#!/usr/bin/env python3
"""What the within/between pressure shares on the device cost and buy (GPU box, UK-380 x 8 chains, a 100-draw burst,
uint16 trace), in ONE call on one box:

  * the `within_between` call alone at D = 1 and at D = 14: HIP events (seir_timer_*) around `within_between(0, n)` of a
    burst that lies in the trace, median of --reps, next to the time of the burst's own sweeps in the same call;
  * the same bits by way of the trace, as the point of comparison: read the burst's trace, form I_t in NumPy,
    `seir_within_between` per window day (psi and I up over PCIe, the shares back), the NumPy fold in draw order.  The
    accumulators of the two routes are compared bit for bit before the ratio is recorded;
  * the sampling phase with the feature off / on (D = 14): `sample_bursts` with the summaries on and the event tensors kept
    on the device (what `summaries: only` runs), a consumer that does nothing, against the device-only rate;
  * what bounds k_wb_trace: the fused multiply-adds per second it reaches against the chip's fp64 vector rate, with the
    compiler's account of the kernel.  That figure is derived from the timing, not read from counters, and is marked so.

    python tools/wb_bench.py [--out profiles/r15_wb.json] [--lib other/libseirhip.so]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

PEAK_FP64_VALU = 78.6e12      # MI355X fp64 vector peak, FMA counted as two: flop / s


def fold(fw, fb):
    """Shares [n, D, M] of one chain -> the accumulators, by the loop csrc/wb_kernels.h states."""
    shape = fw.shape[1:]
    n, gt = np.zeros(shape, np.uint32), np.zeros(shape, np.uint32)
    ref_w, sum_w, sumsq_w, ref_b, sum_b = (np.zeros(shape) for _ in range(5))
    with np.errstate(invalid="ignore"):
        for w, b in zip(fw, fb):
            d = np.isfinite(w) & np.isfinite(b)
            first = d & (n == 0)
            ref_w, ref_b = np.where(first, w, ref_w), np.where(first, b, ref_b)
            dw, db = w - ref_w, b - ref_b
            sum_w = np.where(d, sum_w + dw, sum_w)
            sumsq_w = np.where(d, sumsq_w + dw * dw, sumsq_w)
            sum_b = np.where(d, sum_b + db, sum_b)
            gt = gt + (d & (w > b)).astype(np.uint32)
            n = n + d.astype(np.uint32)
    return dict(defined=n, ref_w=ref_w, sum_w=sum_w, sumsq_w=sumsq_w, ref_b=ref_b, sum_b=sum_b, gt=gt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="uk380")
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--draws", type=int, default=100, help="kept draws per burst")
    ap.add_argument("--days", type=int, nargs="*", default=None, help="windows to time (default: 1 and 14)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bursts", type=int, default=4)
    ap.add_argument("--device-sweeps", type=int, default=300)
    ap.add_argument("--no-trace-route", action="store_true", help="skip the route by way of the trace")
    ap.add_argument("--lib", default=None, help="load this libseirhip.so in place of the tree's: another build of the same ABI")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_wb.json"))
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
    days = a.days or [1, min(14, T)]
    W = np.asarray(cov.W, dtype=np.float64).reshape(-1)
    u = synth.jitter_params(u0, B, scale=0.002, seed=7, T=T)
    ev = np.stack([events] * B)
    res = {"workload": a.workload, "M": M, "T": T, "chains": B, "draws": n, "device": torch.cuda.get_device_name(0),
           "command": " ".join(sys.argv), "wb_call": []}
    try:
        kr = json.load(open(entry.RESOURCES))["k_wb_trace<4>"]
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
                s.reset_within_between(D)
                s.within_between(0, n)                                                 # untimed: first launches
                model.sync()
                times = []
                for _ in range(a.reps):
                    s.reset_within_between(D)
                    model.timer_start()
                    s.within_between(0, n)
                    times.append(model.timer_stop())
                ms = float(np.median(times))
                fmas = float(n) * B * D * M * M
                rate = fmas / (ms * 1e-3)
                share = rate * 2 / PEAK_FP64_VALU
                res["wb_call"].append({
                    "days": D, "ms_median": ms, "ms_min": float(min(times)), "ms_all": [float(t) for t in times],
                    "fused_multiply_adds": fmas, "fused_multiply_adds_per_s": rate, "burst_sweeps_ms": burst_ms,
                    "share_of_the_bursts_sweeps": ms / burst_ms,
                    "events_read_bytes": int(n * B * M * T * 3 * 2), "events_read_bytes_per_s": n * B * M * T * 6 / (ms * 1e-3),
                    "derived_share_of_fp64_valu_peak": share,
                    "limited_by": ("fp64 VALU" if share > 0.5 else "not the arithmetic: the prefix over the recorded events (memory) and, "
                                   "in k_wb_trace, occupancy / latency (fewer workgroups than the chip holds, the draw loop's barriers)")
                    + " -- derived from the timing, not from counters",
                    "k_wb_trace_resources": kr})
                print(f"within_between of {n} x {B} draws, D = {D}: {ms:.2f} ms ({rate:.3g} fma/s, {share:.3f} of the fp64 vector "
                      f"peak); the burst's sweeps {burst_ms:.1f} ms ({ms / burst_ms:.4f})", file=sys.stderr, flush=True)
                device[D] = s.within_between_summary()

            # ---- by way of the trace: the trace over PCIe, seir_within_between per day, NumPy fold -------------------------
            if not a.no_trace_route:
                res["trace_route"] = []
                for D in days:
                    t0 = time.perf_counter()
                    tr = s.read_trace(n)
                    t_read = time.perf_counter() - t0
                    t1 = time.perf_counter()
                    d = tr.events[..., 1].astype(np.int64) - tr.events[..., 2].astype(np.int64)          # [n,B,M,T]
                    I = np.asarray(init)[:, 2].astype(np.int64)[None, None, :, None] + np.cumsum(d, axis=-1) - d
                    I = np.moveaxis(I[..., T - D:], -1, 2).astype(np.float64)                            # [n,B,D,M]
                    psi = np.ascontiguousarray(tr.theta[:, :, 0]).reshape(-1)
                    fw, fb = np.empty((n, B, D, M)), np.empty((n, B, D, M))
                    for tw in range(D):
                        w_, b_ = model.within_between(psi, I[:, :, tw].reshape(n * B, M), W[T - D + tw])
                        fw[:, :, tw], fb[:, :, tw] = w_.reshape(n, B, M), b_.reshape(n, B, M)
                    acc = [fold(fw[:, b], fb[:, b]) for b in range(B)]
                    t_host = time.perf_counter() - t1 + t_read
                    same = all(np.array_equal(np.stack([acc[b][k] for b in range(B)]), getattr(device[D], k)) for k in acc[0])
                    call_ms = [c["ms_median"] for c in res["wb_call"] if c["days"] == D][0]
                    res["trace_route"].append({"days": D, "seconds": t_host, "of_which_reading_the_trace": t_read,
                                               "same_bits": bool(same), "trace_bytes": int(tr.events.nbytes + tr.theta.nbytes),
                                               "ratio_to_the_device_call": t_host * 1e3 / call_ms})
                    print(f"by way of the trace, D = {D}: {t_host:.2f} s ({t_read:.2f} s reading the trace), same bits: {same}",
                          file=sys.stderr, flush=True)

            # ---- the sampling phase, feature off / on, against the device-only rate ----------------------------------------
            D = days[-1]
            s.reset_trace()
            model.timer_start()
            s.run(a.device_sweeps)
            dms = model.timer_stop()
            dev_rate = B * a.device_sweeps / (dms * 1e-3)
            res["device_only"] = {"sweeps": a.device_sweeps, "ms_per_sweep": dms / a.device_sweeps, "sweeps_per_s": dev_rate}
            res["sampling_phase"] = []
            for on in (False, True):
                kw = dict(events=False, summarize=True, **(dict(within_between=True) if on else {}))
                s.reset_within_between(D)
                s.sample_bursts(2, n, lambda tr, i: None, **kw)                        # untimed: page-locks the host buffers
                s.reset_summary()
                s.reset_within_between(D)
                t0 = time.perf_counter()
                s.sample_bursts(nb, n, lambda tr, i: None, **kw)
                model.sync()
                dt = time.perf_counter() - t0
                rate = nb * n * B / dt
                res["sampling_phase"].append({"within_between": on, "days": D, "sweeps": nb * n, "seconds": dt, "sweeps_per_s": rate,
                                              "of_device_only": rate / dev_rate, "recoveries": len(s.recoveries)})
                print(f"sampling phase, within_between {on}: {rate:.0f} sweeps/s, {rate / dev_rate:.3f} of device-only {dev_rate:.0f}",
                      file=sys.stderr, flush=True)
            res["sampling_phase"][1]["of_off"] = res["sampling_phase"][1]["sweeps_per_s"] / res["sampling_phase"][0]["sweeps_per_s"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What a replay of stored draws costs (GPU box, UK-380 x 8 chains, a 100-draw burst, uint16 trace), in ONE call on one box:

  * `seir_sampler_load_trace` of one chain's burst (HIP events around the call: its copies and its kernels), the
    host-to-device copies of the same rows alone (`seir_memcpy_h2d` into a device buffer), and the kernels by difference --
    k_trace_load and k_trace_load_theta, in ms and GB/s of bytes read plus bytes written.  The yardstick is k_summarize on
    the same burst, which reads the same slots (`seir_sampler_summarize`, per chain).  Interleaved, median of --reps;
  * `replay` of the burst with every product on against `sample` of the same burst with every product on: the difference
    is the sweeps minus the load;
  * end to end through the files (--files chains): `posterior.replay.replay_files` with a 56-day forecast against reading
    the same rows with `read_rows` and discarding them -- whether the replay is bound by the file and the link or by the
    device;
  * one product by the old route: the rows read from the file, `SeirModel.simulate` for H = 56 per chain and the moments in
    NumPy -- compared with the replay's forecast accumulators before anything is recorded.

With --parent DIR (a checkout of the parent commit with its library built) the tool also runs `bench.py` of DIR and of this
tree in turns -- parent, parent2 (DIR again: the A/A pair), product; the order rotated from round to round -- and writes the
runs to --ab (profiles/r22_ab.txt), to be read against the parent's own run-to-run span.

    python tools/replay_bench.py [--out profiles/r22_replay.json] [--parent DIR --ab profiles/r22_ab.txt]"""
import argparse
import ctypes
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def ab(parent, path, rounds):
    import groups_bench as GB
    trees = {"parent": parent, "parent2": parent, "product": ROOT}
    names = list(trees)
    runs = {k: [] for k in names}
    order_log = []
    for r in range(rounds):
        order = names[r % 3:] + names[:r % 3]
        order_log.append(" ".join(order))
        for k in order:
            runs[k].append(GB.bench_value(trees[k]))
            print(f"[ab] round {r} {k}: {runs[k][-1]:.1f}", file=sys.stderr, flush=True)
    med = {k: float(np.median(v)) for k, v in runs.items()}
    spread = abs(med["parent"] - med["parent2"])
    mean_p = 0.5 * (med["parent"] + med["parent2"])
    diff = med["product"] - mean_p
    single = runs["parent"] + runs["parent2"]
    inside = sum(min(single) <= v <= max(single) for v in runs["product"])
    with open(path, "w") as f:
        f.write("Round 22 (stored draws into trace slots, nothing loaded): alternating A/B inside ONE call, one MI355X.\n"
                "parent / parent2: the parent commit's tree and library, run twice per round (the A/A pair); product: this change.  "
                f"{rounds} rounds of\n  bench.py {' '.join(GB.BENCH)}\nin the orders: {' | '.join(order_log)}.\n\n"
                "bench.py posterior samples/sec (higher is better)\n"
                "   runs    " + " | ".join(f"{k} " + " ".join(f"{v:.1f}" for v in runs[k]) for k in names) + "\n"
                "   medians " + "  ".join(f"{k} {med[k]:.1f}" for k in names) +
                f"   A/A spread {spread:.1f}   product {'AHEAD of' if diff >= 0 else 'BEHIND'} mean(parent, parent2) by "
                f"{abs(diff):.1f} ({100.0 * abs(diff) / mean_p:.2f} %)\n"
                f"   (the parents' single runs span {min(single):.1f} .. {max(single):.1f}; {inside} of the product's "
                f"{len(runs['product'])} lie inside that span)\n")
    return {"runs": runs, "medians": med, "aa_spread": spread, "product_minus_mean_parent": diff,
            "parents_single_run_span": [min(single), max(single)], "product_runs_inside_span": inside}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="uk380")
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--draws", type=int, default=100, help="kept draws per burst")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--horizon", type=int, default=56)
    ap.add_argument("--files", type=int, default=2, help="chains written to files for the end-to-end figures")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_replay.json"))
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: run the A/B of bench.py")
    ap.add_argument("--ab", default=os.path.join(ROOT, "profiles", "r22_ab.txt"))
    ap.add_argument("--ab-rounds", type=int, default=3)
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import torch
    from covid19uk_amd import _lib, hdf5io, kernel_resources, synth
    from covid19uk_amd.inference import inference as inf
    from covid19uk_amd.posterior import groups as G
    from covid19uk_amd.posterior import predict
    from covid19uk_amd.posterior import replay as R
    from covid19uk_amd.sampler import ChainSampler, forecast_draw_id
    from covid19uk_amd.seir import SeirModel, _dptr
    cfg = dict(dmax=84, nmax=25, m=2, occult_nmax=15, num_event_time_updates=5)       # example_config.yaml:26-30
    cov = synth.make_covariates(a.workload)
    events, init, truth = synth.simulate_epidemic(cov)
    u0 = synth.unconstrain(synth.pack_params(truth, cov.M, cov.T))
    M, T, B, n, Hn = cov.M, cov.T, a.chains, a.draws, a.horizon
    P = 6 + T - 1 + M
    codes = [str(x) for x in np.load(synth._DATA)["lad19cd"]] if a.workload == "uk380" else None
    tab = G.parse_groups("nations", M, codes) if codes else G.parse_groups({"low": list(range(M // 2)), "high": list(range(M // 2, M))}, M)
    N = np.asarray(cov.N, np.float64).reshape(-1)
    w = G.rt_weights(tab, N)
    u = synth.jitter_params(u0, B, scale=0.002, seed=7, T=T)
    ev = np.stack([events] * B)
    W, wd = predict.forecast_calendar(cov, None, T, Hn)
    Wc, wdc = predict.check_calendar(cov, None, T, 14)
    on = dict(summarize=True, forecast=True, rt=True, check=True, within_between=True, groups=True)
    kr = json.load(open(entry.RESOURCES))
    res = {"workload": a.workload, "M": M, "T": T, "chains": B, "draws": n, "device": torch.cuda.get_device_name(0),
           "command": " ".join(sys.argv), "kernels": kernel_resources.owned(kr, "replay"),
           "k_summarize": kr["k_summarize<1,0>"]}
    ev_bytes_in, ev_bytes_out = n * M * T * 3 * 8, n * M * T * 3 * 2
    res["bytes_per_chain_burst"] = {"read_fp64": ev_bytes_in + n * P * 8, "written": ev_bytes_out + n * P * 8 + n * (3 + 4 * _lib.MOVE_TRACE) * 8}

    def everything(s, cap):
        s.set_groups(tab.offsets, tab.members)
        s.set_group_rt(w)
        s.set_group_within_between(True)
        s.reset_summary()
        s.reset_forecast(Hn, W, wd, 5)
        s.reset_rt(14, N / N.sum())
        s.set_group_ngm(w, cap)
        s.reset_check(14, Wc, wdc, 6)
        s.reset_within_between(14)

    with SeirModel(cov, init, max_chains=B) as model:
        with ChainSampler(model, cfg, B, seed=1, trace_capacity=n, record_events="u16") as s:
            s.set_state(u, ev)
            s.set_kernel(step_size=1.2e-5)
            # ---- sample with every product on: the burst whose draws are replayed below ----------------------------------
            everything(s, n)
            s.sample(n, **on)                                                         # first launches, untimed
            t_sample = []
            for _ in range(3):
                everything(s, n)
                t0 = time.perf_counter()
                tr = s.sample(n, **on)
                t_sample.append(time.perf_counter() - t0)
            theta = [np.ascontiguousarray(tr.theta[:, b]) for b in range(B)]
            evs = [np.ascontiguousarray(tr.events[:, b], dtype=np.float64) for b in range(B)]
            # ---- the load of one chain's burst, its copies alone, k_summarize of the same slots -----------------------------
            lib = s._lib
            dbuf = ctypes.c_void_p()
            nbytes = evs[0].nbytes + theta[0].nbytes
            _lib.check(lib.seir_malloc(ctypes.byref(dbuf), nbytes))
            times = {"load": [], "h2d": [], "summarize": []}
            for rep in range(a.reps + 1):                                             # the first pass is untimed
                model.sync()
                model.timer_start()
                _lib.check(lib.seir_sampler_load_trace(s._s, 0, 0, n, _dptr(theta[0]), _dptr(evs[0])))
                t_load = float(model.timer_stop())
                model.sync()
                model.timer_start()
                _lib.check(lib.seir_memcpy_h2d(dbuf, evs[0].ctypes.data_as(ctypes.c_void_p), evs[0].nbytes))
                _lib.check(lib.seir_memcpy_h2d(ctypes.c_void_p(dbuf.value + evs[0].nbytes), theta[0].ctypes.data_as(ctypes.c_void_p),
                                               theta[0].nbytes))
                t_h2d = float(model.timer_stop())
                model.sync()
                model.timer_start()
                s.summarize(0, n, accumulate=False)
                t_sum = float(model.timer_stop())
                if rep:
                    times["load"].append(t_load), times["h2d"].append(t_h2d), times["summarize"].append(t_sum / B)
            _lib.check(lib.seir_free(dbuf))
            assert not s.load_status(clear=True).any()
            med = {k: float(np.median(v)) for k, v in times.items()}
            kern = med["load"] - med["h2d"]
            moved = res["bytes_per_chain_burst"]["read_fp64"] + res["bytes_per_chain_burst"]["written"]
            res["load_one_chain_burst"] = {"ms_call": med["load"], "ms_h2d_alone": med["h2d"], "ms_kernels_by_difference": kern,
                                           "kernels_gb_per_s": moved / (kern * 1e-3) / 1e9 if kern > 0 else None,
                                           "h2d_gb_per_s": res["bytes_per_chain_burst"]["read_fp64"] / (med["h2d"] * 1e-3) / 1e9,
                                           "ms_k_summarize_per_chain": med["summarize"], "ms_all": times}
            print(f"load of {n} draws of one chain: {med['load']:.2f} ms, its copies alone {med['h2d']:.2f} ms, k_summarize per chain "
                  f"{med['summarize']:.3f} ms", file=sys.stderr, flush=True)
            # ---- replay with every product on against sample ---------------------------------------------------------------
            t_replay = []
            for rep in range(3):
                everything(s, n)
                t0 = time.perf_counter()
                rp = s.replay(theta, evs, **on)
                t_replay.append(time.perf_counter() - t0)
            same = all(np.array_equal(getattr(rp, f)[k] if k else getattr(rp, f), getattr(tr, f)[k] if k else getattr(tr, f))
                       for f, k in (("rt", None), ("forecast", "forecast_by_day"), ("check", "check_by_day"), ("marginals", "events_by_day")))
            res["replay_against_sample"] = {"seconds_sample": float(np.median(t_sample)), "seconds_replay": float(np.median(t_replay)),
                                            "same_products": bool(same), "seconds_sample_all": t_sample, "seconds_replay_all": t_replay}
            print(f"every product on: sample {np.median(t_sample):.3f} s, replay {np.median(t_replay):.3f} s, same products: {same}",
                  file=sys.stderr, flush=True)
    # ---- end to end through the files --------------------------------------------------------------------------------------
    nf = min(a.files, B)
    with tempfile.TemporaryDirectory() as d:
        data = os.path.join(d, "data.h5")
        inf.write_inference_data(data, cov, events[..., 2], locations=codes)
        files = []
        for c in range(nf):
            name = os.path.join(d, f"posterior_chain{c}.hd5")
            post = inf.Posterior(name, M, T, cfg["m"], n)
            post.write_samples(inf.draws_to_dict(tr.theta, tr.events, c), 0)
            post.create_dataset("initial_state", init)
            post.close()
            files.append(name)
        t0 = time.perf_counter()
        for name in files:
            with hdf5io.File(name, "r") as f:
                for j0 in range(0, n, 50):
                    f.read_rows("/samples/seir", j0, 50, 1)
        t_read = time.perf_counter() - t0
        log = io.StringIO()
        mcmc = dict(cfg, num_bursts=2, num_burst_samples=50)
        t0 = time.perf_counter()
        outs = R.replay_files(data, files, os.path.join(d, "products.hd5"), mcmc, seed=5, first=0, events_dtype="u16", forecast=Hn, log=log)
        t_e2e = time.perf_counter() - t0
        line = [ln for ln in log.getvalue().splitlines() if ln.startswith("Replay:")][0]
        got = {}
        for c, name in enumerate(outs):
            with hdf5io.File(name, "r") as f:
                got[c] = (f.read("/forecast/seir_mean"), f.read("/samples/forecast_by_day"))
        res["through_the_files"] = {"files": nf, "rows": n, "seconds_replay_files": t_e2e, "draws_per_s": n * nf / t_e2e,
                                    "seconds_reading_the_same_rows": t_read, "log_line": line,
                                    "file_bytes_read": nf * ev_bytes_in}
        print(f"through the files: {t_e2e:.2f} s for {n} x {nf} draws ({n * nf / t_e2e:.0f} draws/s); reading the same rows alone "
              f"{t_read:.2f} s; {line}", file=sys.stderr, flush=True)
        # ---- one product by the old route: the file's rows, seir_simulate per chain, the moments in NumPy ----------------------
        t0 = time.perf_counter()
        same = True
        with SeirModel(cov, init, max_chains=1) as model:
            for c, name in enumerate(files):
                src = R.Source(name)
                th, e = src.draws(np.arange(n))
                src.close()
                tot = e.sum(axis=2).astype(np.int64)
                i0 = init.astype(np.int64)
                st0 = np.stack([i0[:, 0] - tot[..., 0], i0[:, 1] + tot[..., 0] - tot[..., 1], i0[:, 2] + tot[..., 1] - tot[..., 2],
                                i0[:, 3] + tot[..., 2]], axis=-1)
                a_path = predict.log_baseline_path(th[:, 5], th[:, 6:6 + T - 1], T, Hn)
                sim = model.simulate(th[:, :5], a_path, th[:, 6 + T - 1:], W, wd, st0.astype(np.float64), seed=5,
                                     first_draw_id=forecast_draw_id(c, 0)).astype(np.int64)
                same = same and np.array_equal(sim.sum(axis=1), got[c][1]) and np.allclose(sim.mean(axis=0), got[c][0], rtol=1e-12, atol=1e-12)
        t_old = time.perf_counter() - t0
        res["forecast_by_the_old_route"] = {"seconds": t_old, "seconds_per_chain_burst": t_old / nf, "same_draws_and_means": bool(same),
                                            "horizon": Hn}
        print(f"the forecast by way of the file, seir_simulate and NumPy: {t_old:.2f} s, same draws: {same}", file=sys.stderr, flush=True)
    if a.parent:
        res["bench_ab"] = ab(os.path.abspath(a.parent), a.ab, a.ab_rounds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

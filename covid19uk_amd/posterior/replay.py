"""Replay stored draws on the device: every product from a posterior file.

The reference samples once and derives its products afterwards (covid19uk/posterior/thin.py, then predict.py,
reproduction_number.py, within_between.py).  Here the rows of finished `posterior_chain*.hd5` files go back into trace slots
of a sampler (`ChainSampler.load_trace`, include/seir_hip.h "Stored draws into trace slots") and `run_mcmc`'s product
records run over them: another horizon, other probabilities, another table of regions, a product that was not switched on --
and, because the files of all ranks of a job go into one sampler, quantiles pooled over every chain of the job.

This module holds the NumPy definitions the device is held to (`classify`, `check_draws`), the inverse of
`inference.draws_to_dict` (`theta_from_samples`), the row selection, and the driver with its command line:

    python -m covid19uk_amd.posterior.replay -c config.yaml -o products.hd5 data.nc posterior_chain*.hd5
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

# csrc/trace_load.h: the codes of a loaded item
LOAD_OK, LOAD_NOT_INTEGER, LOAD_NEGATIVE, LOAD_OVER_WIDTH, LOAD_NEG_STATE, LOAD_BAD_THETA = range(6)
THETA_SCALARS = ("psi", "sigma_space", "beta_area", "gamma0", "gamma1", "alpha_0")   # inference.py:541-552


def classify(x, width):
    """`load_classify` of csrc/trace_load.h over an array: (value int64, code) -- the first that applies of NOT_INTEGER (NaN,
    +-inf, a fractional part, a magnitude at or above 2^53), NEGATIVE, OVER_WIDTH (above 65535 for width 16, above 2^31 - 1
    for width 32); -0.0 is 0.  The value of a cell that is not OK is 0."""
    if width not in (16, 32):
        raise ValueError(f"width={width}: 16 or 32")
    x = np.asarray(x, np.float64)
    top = 65535 if width == 16 else 2 ** 31 - 1
    inside = (x > -2.0 ** 53) & (x < 2.0 ** 53)                # NaN fails both
    xi = np.where(inside, x, 0.0)
    integer = inside & (np.trunc(xi) == xi)
    code = np.where(~integer, LOAD_NOT_INTEGER, np.where(xi < 0, LOAD_NEGATIVE, np.where(xi > top, LOAD_OVER_WIDTH, LOAD_OK)))
    return np.where(code == LOAD_OK, xi, 0.0).astype(np.int64), code.astype(np.int64)


def check_draws(theta, events, initial_state, width):
    """THE NumPy definition of `seir_sampler_load_status` for one call: theta [n,P], events [n,M,T,3] (fp64, as the file has
    them), initial_state [M, >= 3] -> uint64 [6]: the cells that are not an integer / negative / over the width, the
    (draw, location, boundary, compartment) states below zero -- S, E, I behind every day from the initial state and the
    stored counts (a bad cell counts 0), in int64 --, the theta entries that are not finite, and the smallest key
    flat_index * 8 + code of a bad item (0: none)."""
    theta, events = np.asarray(theta, np.float64), np.asarray(events, np.float64)
    value, code = classify(events, width)
    cum = np.cumsum(value, axis=2, dtype=np.int64)             # [n,M,T,3]: the inclusive sums, boundary t + 1
    s0 = np.asarray(initial_state)[:, :3].astype(np.int64)[None, :, None, :]
    state = np.stack([s0[..., 0] - cum[..., 0], s0[..., 1] + cum[..., 0] - cum[..., 1], s0[..., 2] + cum[..., 1] - cum[..., 2]], axis=-1)
    neg = state < 0
    bad_theta = ~np.isfinite(theta)
    out = np.zeros(6, np.uint64)
    for c in (LOAD_NOT_INTEGER, LOAD_NEGATIVE, LOAD_OVER_WIDTH):
        out[c - 1] = np.count_nonzero(code == c)
    out[LOAD_NEG_STATE - 1] = np.count_nonzero(neg)
    out[LOAD_BAD_THETA - 1] = np.count_nonzero(bad_theta)
    keys = []
    flat = np.flatnonzero(code.reshape(-1))
    if flat.size:
        keys.append(int((flat * 8 + code.reshape(-1)[flat]).min()))
    for mask, c in ((neg, LOAD_NEG_STATE), (bad_theta, LOAD_BAD_THETA)):
        flat = np.flatnonzero(mask.reshape(-1))
        if flat.size:
            keys.append(int(flat[0]) * 8 + c)
    out[5] = min(keys) if keys else 0
    return out


def theta_from_samples(samples, M, T):
    """The inverse of `inference.draws_to_dict`: {psi, sigma_space, beta_area, gamma0, gamma1, alpha_0 [n], alpha_t [n,T-1],
    spatial_effect [n,M]} -> theta [n,P] in the order of inference.py:541-552, the values as they are."""
    n = np.asarray(samples["psi"]).shape[0]
    theta = np.empty((n, 6 + (T - 1) + M))
    for i, k in enumerate(THETA_SCALARS):
        theta[:, i] = np.asarray(samples[k], np.float64).reshape(n)
    theta[:, 6:6 + T - 1] = np.asarray(samples["alpha_t"], np.float64).reshape(n, T - 1)
    theta[:, 6 + T - 1:] = np.asarray(samples["spatial_effect"], np.float64).reshape(n, M)
    return theta


def select_rows(n, first, stop=None, every=1):
    """The rows range(first, stop, every) of a file of n draws (stop: default n).  Refuses first >= n, a stop outside
    (first, n], every < 1 -- an empty range."""
    first, every = int(first), int(every)
    stop = int(n) if stop is None else int(stop)
    if every < 1:
        raise ValueError(f"every={every}: the stride is >= 1")
    if first < 0 or first >= n:
        raise ValueError(f"first={first}: the file holds {n} draw(s), rows [0, {n})")
    if stop > n:
        raise ValueError(f"stop={stop}: the file holds {n} draw(s)")
    rows = np.arange(first, stop, every, dtype=np.int64)
    if rows.size == 0:
        raise ValueError(f"rows range({first}, {stop}, {every}) of {n} draw(s): nothing to replay")
    return rows


# ---------------------------------------------------------------------------------------------------------------------
# the files
# ---------------------------------------------------------------------------------------------------------------------
PARAMETER_KEYS = THETA_SCALARS + ("alpha_t", "spatial_effect")


class Source:
    """One chain's posterior file, read by rows: the HDF5 file `inference.Posterior` writes, or its `.npz` fallback (keys
    samples__psi ...)."""

    def __init__(self, path):
        from .. import hdf5io
        self.path = str(path)
        self.npz = self.path.endswith(".npz") or not hdf5io.available()
        if self.npz:
            z = np.load(self.path)
            self._z = {k: z[k] for k in z.files if k == "initial_state" or k.startswith("samples__")}   # an archive has no rows to seek
            names = {k.replace("__", "/") for k in self._z}
            self._shape = lambda name: self._z[name.replace("/", "__")].shape
        else:
            self._f = hdf5io.File(self.path, "r")
            names = {n for n in ["samples/seir", "initial_state"] + [f"samples/{k}" for k in PARAMETER_KEYS] if self._f.exists("/" + n)}
            self._shape = lambda name: tuple(self._f.shape("/" + name))
        missing = [k for k in PARAMETER_KEYS if f"samples/{k}" not in names]
        if missing:
            raise ValueError(f"{self.path}: no samples/{missing[0]}: not a posterior file of the inference")
        if "samples/seir" not in names:
            raise ValueError(f"{self.path}: no samples/seir -- an output of `summaries: only`, whose event tensors never left the "
                             "device: the draws of the latent epidemic are not in the file and there is nothing to replay")
        self.has_initial_state = "initial_state" in names
        shape = self._shape("samples/seir")
        self.n, self.M, self.T = int(shape[0]), int(shape[1]), int(shape[2])

    def rows(self, name, rows):
        """ds[rows] for an arithmetic progression of rows: one strided hyperslab of the file."""
        rows = np.asarray(rows, np.int64)
        step = int(rows[1] - rows[0]) if rows.size > 1 else 1
        if self.npz:
            return np.asarray(self._z[name.replace("/", "__")][rows[0]:rows[-1] + 1:step], np.float64)
        return self._f.read_rows("/" + name, int(rows[0]), int(rows.size), step)

    def draws(self, rows):
        """(theta [n,P], events [n,M,T,3]) of `rows`, float64, as the file has them."""
        samples = {k: self.rows(f"samples/{k}", rows) for k in PARAMETER_KEYS}
        return theta_from_samples(samples, self.M, self.T), np.ascontiguousarray(self.rows("samples/seir", rows), dtype=np.float64)

    def initial_state(self):
        if not self.has_initial_state:
            return None
        return np.asarray(self._z["initial_state"] if self.npz else self._f.read("/initial_state"), np.float64)

    def close(self):
        if not self.npz:
            self._f.close()


def open_sources(files, M, T, first=None, stop=None, every=1):
    """The input files as `Source`s and the rows to replay of every one of them -- or the refusal: a file without
    samples/seir, a file of another M or T than the data, files of different length, first >= n, an empty row range."""
    from ..inference import inference as inf
    if not files:
        raise ValueError("no posterior file given")
    sources = []
    try:
        for path in files:
            src = Source(path)
            sources.append(src)
            if (src.M, src.T) != (int(M), int(T)):
                raise ValueError(f"{src.path}: samples/seir is for M = {src.M}, T = {src.T}, the data for M = {M}, T = {T}")
            if src.n != sources[0].n:
                raise ValueError(f"{src.path} holds {src.n} draw(s), {sources[0].path} {sources[0].n}: files of one job have one length")
        rows = select_rows(sources[0].n, inf.warmup_size() if first is None else first, stop, every)
    except Exception:
        for src in sources:
            src.close()
        raise
    return sources, rows


# ---------------------------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------------------------
def replay_bursts(sampler, sources, rows, burst, records, log=sys.stderr):
    """`run_mcmc`'s sampling phase over stored draws: begin() of every record once; per burst of `burst` rows one
    `sampler.replay` with the sampling phase's keywords, the diagnostics' mark where `diagnostics_marks` puts it, and the
    flush; then every finish().  While a burst is on the device and being written, a worker thread reads the next one from
    the files -- the file library is entered by one thread at a time, so what overlaps the reading is the device's work and
    the reads of its products, not the writing.  Returns (draws replayed per chain, seconds in all, seconds the loop waited
    for the files)."""
    import threading
    from concurrent.futures import ThreadPoolExecutor
    io = threading.Lock()
    pr = records
    kw = {k: v for k, v in pr.burst_kw.items() if k != "events"}   # a replay returns no event tensor: they are the input's
    cuts = [rows[i:i + burst] for i in range(0, len(rows), burst)]

    def read(i):
        with io:
            draws = [src.draws(cuts[i]) for src in sources]
        return [d[0] for d in draws], [d[1] for d in draws]

    t0 = time.perf_counter()
    waited = 0.0
    for record in pr.records:
        record.begin()
    with ThreadPoolExecutor(max_workers=1) as pool:
        nxt = pool.submit(read, 0)
        for i in range(len(cuts)):
            t1 = time.perf_counter()
            theta, events = nxt.result()
            waited += time.perf_counter() - t1
            if i + 1 < len(cuts):
                nxt = pool.submit(read, i + 1)
            tr = sampler.replay(theta, events, **kw)
            if i in pr.marks:
                sampler.mark(pr.marks[i])
            with io:
                pr.flush(tr, i)
            print(f"  burst {i + 1}/{len(cuts)}", file=log, flush=True)
    for record in pr.records:
        record.finish()
    return len(rows), time.perf_counter() - t0, waited


def replay_files(data_file, files, output_file, config, seed=0, device=None, first=None, stop=None, every=1, burst=None,
                 first_chain_id=0, events_dtype="auto", log=sys.stderr, **overrides):
    """Every product of the inference command line from finished posterior files: one chain of one sampler per file, in the
    order given, with global chain ids first_chain_id + c (the forecast's and the check's Philox streams); rows
    range(first, stop, every) of every file (`first`: default the warm-up's length); `burst`: rows per replay (default
    Mcmc.num_burst_samples).  `overrides`: the product keywords of `inference.mcmc` (summaries, forecast, rt, ...).  One
    output per input, named as `inference.chain_file_name` names them, with the datasets a live run with the same options
    writes for its sampling phase, no results/* and no samples/seir, and a group replay/ (source, rows, first_chain_id); the
    pooled_* datasets are pooled over every file given.  Returns the output names."""
    from ..inference import inference as inf
    from ..inference.mcmc_kernel_factory import event_kernel_config, hmc_kernel_kwargs_default
    from ..sampler import ChainSampler
    from ..seir import SeirModel
    from .. import model_spec
    cov, cases, dates = inf.read_inference_data(data_file)
    M, T = int(cases.shape[0]), int(cases.shape[1])
    sources, rows = open_sources(files, M, T, first, stop, every)        # refused here: before any GPU call
    try:
        B, n = len(sources), len(rows)
        ns = int(config["num_burst_samples"] if burst is None else burst)
        if ns < 1:
            raise ValueError(f"burst={ns}: at least one row per replay")
        config = dict(config, num_burst_samples=ns, num_bursts=-(-n // ns), thin=1)
        if overrides.get("scenarios") is not None:                       # the mapping of --scenarios: in the place of Mcmc.scenarios
            config = dict(config, scenarios=overrides["scenarios"])
        if overrides.get("verify") is not None:                          # the path of --verify: in the place of Mcmc.verify
            config = dict(config, verify=overrides["verify"])
        if overrides.get("groups_scenarios") is not None:                # --groups-scenarios: in the place of Mcmc.groups_scenarios
            config = dict(config, groups_scenarios=overrides["groups_scenarios"])
        overrides = {k: v for k, v in overrides.items() if k not in ("scenarios", "verify", "groups_scenarios")}
        config, opt = inf.resolve_products(config, **overrides)          # every product refusal: before any GPU call
        pending = inf.resolve_scenarios(config, opt.horizon)             # ... the scenarios' too
        inf.resolve_scenario_groups(config, pending, opt.group_spec)
        truth = None
        if inf.resolve_verify(config, opt.horizon) is not None:          # ... and the truth's, held to the fitted file
            from .verify import load_truth
            truth = load_truth(inf.resolve_verify(config, opt.horizon), data_file, opt.horizon, log=log)
        if config.get("diagnostics") == "on" and n % ns:
            raise ValueError(f"diagnostics: {n} row(s) in bursts of {ns} -- the split R-hat compares half-chains of one length, "
                             "which takes whole bursts (choose --stop or --burst accordingly)")
        group_table = opt.bind(M, T, lambda: inf.read_location_names(data_file))   # the table, the windows against the series
        # the members of a targeted scenario against the same codes (read once, and only when a member is a code or a pattern)
        import functools
        from .scenarios import PendingScenarios
        codes = functools.lru_cache(maxsize=None)(lambda: inf.read_location_names(data_file)) if isinstance(pending, PendingScenarios) else None
        inf.bind_scenarios(pending, M, codes, cov.N)                     # ... and a trigger's per-100k thresholds
        # the initial state the draws were recorded from: the files' own, else the imputation of `seed` as `mcmc` forms it
        states = [src.initial_state() for src in sources]
        if states[0] is not None:
            if any(st is None or not np.array_equal(st, states[0]) for st in states):
                raise ValueError("the files do not hold the same initial_state: they are not chains of one job")
            initial_state = states[0]
        else:
            initial_state, _ = model_spec.initial_conditions(cases, cov.N, np.random.default_rng(seed))
        record = inf.trace_events_dtype(cases, events_dtype)
        # the sampler's state: the first replayed draw of each file -- checked here, on the host, before it reaches a kernel
        start = [src.draws(rows[:1]) for src in sources]
        for c, (th, ev) in enumerate(start):
            bad = check_draws(th, ev, initial_state, 16 if record == "u16" else 32)
            if bad.any():
                raise ValueError(f"{sources[c].path}: row {int(rows[0])} is not a draw of this model and data ({bad[:5].tolist()} "
                                 "cells not an integer / negative / over the trace's width, states below zero, theta entries not finite)")
        cfg = event_kernel_config(config)
        model = SeirModel(cov, initial_state, max_chains=B, device=0 if device is None else int(device))
        sampler = ChainSampler(model, cfg, B, seed=seed, t_range=(max(T - 21, 0), T),
                               num_leapfrog_steps=hmc_kernel_kwargs_default()["num_leapfrog_steps"], trace_capacity=max(ns, 1),
                               record_events=record, first_chain_id=int(first_chain_id), auto_recover=False)
        sampler.set_state(inf.unconstrain_theta(np.stack([th[0] for th, _ in start])), np.stack([ev[0] for _, ev in start]))
        names = [inf.chain_file_name(output_file, int(first_chain_id) + c, B) for c in range(B)]
        posteriors = [inf.Posterior(name, M, T, cfg["m"], n, burst=ns, results=False, **inf.posterior_kwargs(config, opt, group_table, n))
                      for name in names]
        kw = inf.product_inputs(cov, dates, T, opt, seed, group_table)
        from .scenarios import is_triggered
        if is_triggered(pending):
            kw.setdefault("population", np.asarray(cov.N, dtype=np.float64).reshape(-1))
        if group_table is not None:
            for post in posteriors:
                post.write_groups(group_table, cov.N, initial_state)
        pr = inf.product_records(sampler, config, posteriors, log=log, total=n, results=False, **kw,
                                 **({} if truth is None else dict(verify=truth)),
                                 **({} if codes is None else dict(location_names=codes)))
        n, dt, waited = replay_bursts(sampler, sources, rows, ns, pr, log=log)
        print(f"Replay: rows {int(rows[0])}..{int(rows[-1])} step {int(every)} ({n} draw(s)) of {B} file(s), "
              f"{n * B / dt:.1f} draws/s, {100.0 * waited / dt:.0f} % of the time waiting for the files", file=log, flush=True)
        for c, post in enumerate(posteriors):
            post.create_dataset("initial_state", initial_state)
            width = max(len(s) for s in dates)
            post.create_dataset("time", np.array(dates, dtype=f"S{width}"))
            src = os.path.basename(sources[c].path).encode()
            post.create_dataset("replay/source", np.array([src], dtype=f"S{max(len(src), 1)}"))
            post.create_dataset("replay/rows", rows, dtype=np.int64)
            post.create_dataset("replay/first_chain_id", np.array([int(first_chain_id)]), dtype=np.int64)
            post.close()
        sampler.close()
        model.close()
    finally:
        for src in sources:
            src.close()
    return names


def main(argv=None):
    from argparse import ArgumentParser

    import yaml
    from ..inference.options import (add_product_arguments, add_scenarios_argument, add_verify_argument, product_overrides,
                                     scenarios_override, verify_override)
    parser = ArgumentParser(description="Replay stored draws on the device: every product of the inference from posterior files")
    parser.add_argument("-c", "--config", type=str, required=True, help="Config file (its Mcmc section)")
    parser.add_argument("-o", "--output", type=str, required=True, help="Output file (one per input: _chain<id> is added)")
    parser.add_argument("data_file", type=str, help="Data NetCDF file")
    parser.add_argument("posteriors", type=str, nargs="+", help="posterior files, one chain each, in the order of their chain ids")
    parser.add_argument("--first", type=int, default=None, metavar="N", help="first row to replay (default: the warm-up's length)")
    parser.add_argument("--stop", type=int, default=None, metavar="N", help="one past the last row (default: the file's length)")
    parser.add_argument("--every", type=int, default=1, metavar="K", help="replay every K-th row")
    parser.add_argument("--burst", type=int, default=None, metavar="NS", help="rows per replay (default: Mcmc.num_burst_samples)")
    parser.add_argument("--first-chain-id", type=int, default=0, metavar="C",
                        help="global chain id of the first file: the forecast's and the check's random streams are keyed by it")
    parser.add_argument("--seed", type=int, default=0, help="the seed of the run that wrote the files")
    parser.add_argument("--device", type=int, default=None, help="HIP device (default 0)")
    parser.add_argument("--events-dtype", choices=["auto", "u16", "int32"], default="auto",
                        help="width of the event counts in the device-side burst buffer")
    add_product_arguments(parser)
    add_scenarios_argument(parser)
    add_verify_argument(parser)
    args = parser.parse_args(argv)
    with open(args.config, "r") as f:
        config = yaml.load(f, Loader=yaml.FullLoader)
    replay_files(args.data_file, args.posteriors, args.output, config["Mcmc"], seed=args.seed, device=args.device, first=args.first,
                 stop=args.stop, every=args.every, burst=args.burst, first_chain_id=args.first_chain_id,
                 events_dtype=args.events_dtype, **product_overrides(args), **scenarios_override(args), **verify_override(args))


if __name__ == "__main__":
    main()

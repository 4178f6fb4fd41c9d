"""MCMC driver for the COVID-19 UK spatial SEIR model on MI355X.

Host-side mirror of the reference's `covid19uk/inference/inference.py`: the same
CLI (`python -m covid19uk_amd.inference.inference -c config.yaml -o posterior.hd5
data.nc`; `python -m covid19uk.inference.inference` forwards here), the same
`config["Mcmc"]` keys, the same windowed warm-up schedule and the same
`posterior.hd5` layout.  Everything numerical -- the joint log-probability, HMC,
the event-time and occult Metropolis-Hastings kernels -- runs in libseirhip's HIP
kernels through `covid19uk_amd.sampler.ChainSampler`; this file only sequences
windows and moves draws from the device burst buffer to disk.
"""
from __future__ import annotations

import collections
import functools
import os
import sys
import time
import types

import numpy as np

from .. import hdf5io
from .. import model_spec
from ..posterior import diagnostics as diag_mod
from ..posterior import groups as G_mod
from ..sampler import MOVE_KEYS, ChainSampler, Summary, mid_p
from ..seir import SeirModel
from .mcmc_kernel_factory import event_kernel_config, hmc_kernel_kwargs_default
from .options import (CHECK_SEED_SALT, DIAGNOSTICS, SUMMARIES, Products, add_product_arguments, add_scenarios_argument, add_verify_argument, scenarios_override, verify_override, bind_scenarios, resolve_scenario_groups, check_mode, check_seed,  # noqa: F401
                      diagnostics_mode, forecast_mode, forecast_quantiles_mode, posterior_kwargs, product_inputs, product_overrides,
                      resolve_products, resolve_scenarios, resolve_verify, rt_mode, rt_quantiles_mode, summaries_mode, thin_interval, within_between_mode)

DTYPE = model_spec.DTYPE


# ---------------------------------------------------------------------------
# inference data (the reference's NetCDF4 `constant_data` / `observations` groups)
# ---------------------------------------------------------------------------
def read_inference_data(path):
    """(Covariates, cases [M,T], dates [T] of str) from the file `assemble_data` writes
    (covid19uk/data/assemble.py:8-16; variables of model_spec.py:88-105).  `.npz` files with
    the same variable names are accepted too."""
    if str(path).endswith(".npz"):
        d = np.load(path, allow_pickle=False)
        cov = model_spec.Covariates(C=d["C"], W=d["W"], N=d["N"], adjacency=d["adjacency"],
                                    weekday=d["weekday"], area=d["area"])
        dates = [str(x) for x in d["time"]] if "time" in d.files else [str(i) for i in range(cov.T)]
        return cov, np.asarray(d["cases"], DTYPE), dates
    with hdf5io.File(path, "r") as f:
        g = {k: f.read(f"/constant_data/{k}") for k in ("C", "W", "N", "adjacency", "weekday", "area")}
        cases = np.asarray(f.read("/observations/cases"), DTYPE)
        dates = None
        if f.exists("/observations/time"):
            t = f.read("/observations/time")
            if t.dtype.kind == "S":
                dates = [x.decode() for x in t]
            else:
                units = f.read_str_attr("/observations/time", "units") or ""
                if units.startswith("days since "):
                    t0 = np.datetime64(units[len("days since "):].split()[0])
                    dates = [str(t0 + np.timedelta64(int(x), "D")) for x in t]
                else:
                    dates = [str(int(x)) for x in t]
    cov = model_spec.Covariates(**{k: np.asarray(v, DTYPE) for k, v in g.items()})
    if cases.shape == (cov.T, cov.M) and cov.T != cov.M:
        cases = cases.T
    if dates is None:
        dates = [str(i) for i in range(cases.shape[1])]
    return cov, cases, dates


def write_inference_data(path, cov: model_spec.Covariates, cases, dates=None, locations=None):
    """Write an input file with the layout `read_inference_data` expects (tests, synthetic runs).  `locations` [M] of str
    (an .hd5 file only): the `location` coordinate that `read_location_names` returns."""
    cases = np.asarray(cases, DTYPE)
    dates = [str(i) for i in range(cases.shape[1])] if dates is None else list(dates)
    if str(path).endswith(".npz"):
        np.savez(path, C=cov.C, W=cov.W, N=cov.N, adjacency=cov.adjacency, weekday=cov.weekday, area=cov.area,
                 cases=cases, time=np.array(dates))
        return
    with hdf5io.File(path, "w") as f:
        for k in ("C", "W", "N", "adjacency", "weekday", "area"):
            a = np.asarray(getattr(cov, k), DTYPE)
            f.create_dataset(f"/constant_data/{k}", a.shape, np.float64)
            f.write(f"/constant_data/{k}", a)
        f.create_dataset("/observations/cases", cases.shape, np.float64)
        f.write("/observations/cases", cases)
        n = max(len(s) for s in dates)
        f.create_dataset("/observations/time", (len(dates),), f"S{n}")
        f.write("/observations/time", np.array(dates, dtype=f"S{n}"))
        if locations is not None:
            n = max(len(str(x)) for x in locations)
            f.create_dataset("/constant_data/location", (len(locations),), f"S{n}")
            f.write("/constant_data/location", np.array([str(x) for x in locations], dtype=f"S{n}"))


def read_location_names(path):
    """The `location` coordinate of the input file (LAD codes; covid19uk/data/assemble.py writes it with the
    `constant_data` group), or None when the file carries none."""
    if str(path).endswith(".npz"):
        return None
    with hdf5io.File(path, "r") as f:
        for name in ("/constant_data/location", "/observations/location"):
            if f.exists(name):
                v = f.read(name)
                if v.dtype.kind in "SO":
                    return [x.decode() if isinstance(x, bytes) else str(x) for x in v.reshape(-1)]
                return [str(int(x)) for x in v.reshape(-1)]
    return None


# ---------------------------------------------------------------------------
# posterior.hd5 (gemlib `Posterior`: samples/<key>, results/<nested/keys>)
# ---------------------------------------------------------------------------
class Posterior:
    """HDF5 sink with the dataset layout of inference.py:285-300 / :245-282 / :588-592.
    `is_accepted` is a bool dataset the way h5py stores one (gemlib's Posterior writes numpy bools through h5py):
    the int8 enum {FALSE = 0, TRUE = 1}."""

    def __init__(self, filename, M, T, mmax, num_samples, burst=100, summaries="off", forecast=None, rt=None, check=None,
                 within_between=None, groups=None, group_curves=None, results=True):
        """`summaries` ("off" | "on" | "only", Mcmc.summaries / --summaries): with "on" and "only" the per-draw marginals
        samples/seir_by_day [n,T,3], samples/seir_by_location [n,M,3], samples/state_by_day [n,T,3] (int64) are written
        with every burst and `write_summary` adds summaries/* at the end of the run; with "only" samples/seir is not
        created.  "off" creates exactly the datasets of a run without the option.

        `forecast` ((H, n) or None, Mcmc.forecast / --forecast): samples/forecast_by_day [n,H,3], forecast_by_location
        [n,M,3], forecast_state_by_day [n,H,3] (int64), one row per kept draw of the sampling phase -- n of them, not
        num_samples: the warm-up is not forecast -- and `write_forecast` adds the group forecast/ at the end of the run.

        `rt` ((D, n) or None, Mcmc.rt / --rt): samples/R_t [n,D] (float64), the national reproduction number of the last
        D days, one row per kept draw of the sampling phase, and `write_rt` adds the group rt/ at the end of the run.

        `check` ((K, n) or None, Mcmc.check / --check): samples/check_by_day [n,K,3], check_by_location [n,M,3],
        check_state_by_day [n,K,3] (int64), one row per kept draw of the sampling phase, and `write_check` adds the group
        check/ at the end of the run.

        `within_between` ((D, n) or None, Mcmc.within_between / --within-between): samples/within_pressure and
        samples/between_pressure [n,D] (float64), the national within- and between-location infection pressure of the last
        D days, one row per kept draw of the sampling phase, and `write_within_between` adds the group within_between/ at the
        end of the run.

        `groups` (G or None, Mcmc.groups / --groups): the per-draw sums over G groups of locations (int64) of whichever
        sources are on -- samples/seir_by_group [n,G,T,3] with `summaries` on / only (warm-up rows included, like
        seir_by_day); samples/forecast_by_group [nf,G,H,3] and forecast_group_state0 [nf,G,3] with `forecast`;
        samples/check_by_group [nf,G,K,3] and check_group_state0 [nf,G,3] with `check` -- and `write_groups`,
        `write_group_forecast`, `write_group_check` add groups/* and the group_* datasets of forecast/ and check/.

        `group_curves` ({"rt": (D, n)} and / or {"within_between": (D, n)} or None; Mcmc.groups_rt,
        Mcmc.groups_within_between; needs `groups`): samples/R_t_by_group [n,G,D], samples/within_pressure_by_group and
        samples/between_pressure_by_group [n,G,D] (float64), one row per kept draw of the sampling phase, and
        `write_group_rt`, `write_group_within_between` add the group_* datasets of rt/ and within_between/.

        `results` (False: the output of `posterior.replay`): no results/* and no samples/seir -- a replay has no kernel
        results and its event tensors are the input's."""
        self.filename = filename
        self.use_h5 = not str(filename).endswith(".npz") and hdf5io.available()
        self.shapes = {
            "samples/psi": (), "samples/sigma_space": (), "samples/beta_area": (), "samples/gamma0": (),
            "samples/gamma1": (), "samples/alpha_0": (), "samples/alpha_t": (T - 1,),
            "samples/spatial_effect": (M,), "samples/seir": (M, T, 3),
            "results/hmc/is_accepted": (), "results/hmc/target_log_prob": (), "results/hmc/step_size": (),
        }
        self.dtypes = {"results/hmc/is_accepted": np.bool_}
        if summaries != "off":
            self.shapes.update({"samples/seir_by_day": (T, 3), "samples/seir_by_location": (M, 3),
                                "samples/state_by_day": (T, 3)})
            self.dtypes.update({k: np.int64 for k in ("samples/seir_by_day", "samples/seir_by_location",
                                                      "samples/state_by_day")})
        if summaries == "only":
            del self.shapes["samples/seir"]
        for key in MOVE_KEYS:
            self.shapes[f"results/{key}/is_accepted"] = ()
            self.shapes[f"results/{key}/target_log_prob"] = ()
            self.shapes[f"results/{key}/proposed_delta"] = (4, mmax)
            self.dtypes[f"results/{key}/is_accepted"] = np.bool_
        if not results:
            for key in [k for k in self.shapes if k.startswith("results/") or k == "samples/seir"]:
                del self.shapes[key]
            self.dtypes = {k: v for k, v in self.dtypes.items() if k in self.shapes}
        self.num_samples = int(num_samples)
        self.rows = {}                                     # datasets with another number of rows than num_samples
        if forecast is not None:
            H, n_fc = int(forecast[0]), int(forecast[1])
            for k, shp in (("samples/forecast_by_day", (H, 3)), ("samples/forecast_by_location", (M, 3)),
                           ("samples/forecast_state_by_day", (H, 3))):
                self.shapes[k], self.dtypes[k], self.rows[k] = shp, np.int64, n_fc
        if rt is not None:
            self.shapes["samples/R_t"], self.rows["samples/R_t"] = (int(rt[0]),), int(rt[1])
        if check is not None:
            K, n_ck = int(check[0]), int(check[1])
            for k, shp in (("samples/check_by_day", (K, 3)), ("samples/check_by_location", (M, 3)),
                           ("samples/check_state_by_day", (K, 3))):
                self.shapes[k], self.dtypes[k], self.rows[k] = shp, np.int64, n_ck
        if within_between is not None:
            for k in ("samples/within_pressure", "samples/between_pressure"):
                self.shapes[k], self.rows[k] = (int(within_between[0]),), int(within_between[1])
        if groups:
            G = int(groups)
            if summaries != "off":
                self.shapes["samples/seir_by_group"], self.dtypes["samples/seir_by_group"] = (G, T, 3), np.int64
            for src, spec in (("forecast", forecast), ("check", check)):
                if spec is not None:
                    for k, shp in ((f"samples/{src}_by_group", (G, int(spec[0]), 3)), (f"samples/{src}_group_state0", (G, 3))):
                        self.shapes[k], self.dtypes[k], self.rows[k] = shp, np.int64, int(spec[1])
        for key, names in (("rt", ("R_t_by_group",)), ("within_between", ("within_pressure_by_group", "between_pressure_by_group"))):
            if group_curves and groups and key in group_curves:
                for k in names:
                    self.shapes[f"samples/{k}"] = (int(groups), int(group_curves[key][0]))
                    self.rows[f"samples/{k}"] = int(group_curves[key][1])
        self._scratch = {}
        if self.use_h5:
            self._file = hdf5io.File(filename, "w")
            for name, shp in self.shapes.items():
                self._file.create_dataset("/" + name, (self.rows.get(name, self.num_samples),) + shp, self.dtypes.get(name, np.float64),
                                          raw=name == "samples/seir")
        else:
            self._file = None
            self._mem = {name: np.zeros((self.rows.get(name, self.num_samples),) + shp, self.dtypes.get(name, np.float64))
                         for name, shp in self.shapes.items()}
            self._extra = {}

    def write(self, name, value, first_dim_offset):
        if self.use_h5:
            v = np.asarray(value)
            if name == "samples/seir":
                # the event tensor arrives as the device's integer counts (a strided view of the burst): converted to
                # the file's float64 and written at its file address by a few threads (hdf5io.write_rows_parallel)
                self._file.write_rows_parallel("/" + name, v, offset=first_dim_offset)
                return
            if v.dtype != np.float64 and v.dtype.kind in "iu" and v.nbytes > (1 << 20) and name not in self.dtypes:
                # the event tensor arrives as the device's integer counts (a strided view of the burst); it is
                # converted to the file's float64 in ONE pass into a buffer kept between bursts -- a fresh
                # 165 MB array per burst costs more in page faults than the conversion itself
                buf = self._scratch.get(v.shape)
                if buf is None:
                    buf = self._scratch[v.shape] = np.empty(v.shape, np.float64)
                np.copyto(buf, v, casting="unsafe")
                v = buf
            self._file.write("/" + name, v, offset=first_dim_offset)
        else:
            v = np.asarray(value)
            self._mem[name][first_dim_offset:first_dim_offset + v.shape[0]] = v

    def write_samples(self, samples: dict, first_dim_offset):
        for k, v in samples.items():
            self.write(f"samples/{k}", v, first_dim_offset)

    def write_results(self, results: dict, first_dim_offset):
        for k, v in results.items():
            for kk, vv in v.items():
                self.write(f"results/{k}/{kk}", vv, first_dim_offset)

    def create_dataset(self, name, data, dtype=None):
        """A dataset of its own, float64 unless `dtype` says otherwise (fixed-length strings keep their type)."""
        data = np.asarray(data) if dtype is None else np.asarray(data, dtype)
        if self.use_h5:
            self._file.create_dataset("/" + name, data.shape, data.dtype if data.dtype.kind == "S" or dtype is not None else np.float64)
            self._file.write("/" + name, data)
        else:
            self._extra[name] = data

    def _write_moments(self, group, mean, var):
        """<group>/seir_mean, seir_var (k_se, k_ei, k_ir) and state_mean, state_var (S, E, I) from [M,days,6] rows."""
        self.create_dataset(f"{group}/seir_mean", np.ascontiguousarray(mean[..., :3]))
        self.create_dataset(f"{group}/seir_var", np.ascontiguousarray(var[..., :3]))
        self.create_dataset(f"{group}/state_mean", np.ascontiguousarray(mean[..., 3:]))
        self.create_dataset(f"{group}/state_var", np.ascontiguousarray(var[..., 3:]))

    def write_summary(self, count, mean, var):
        """The moments of one chain over the sampling phase (`Summary.mean` / `.var` rows, [M,T,6] float64):
        summaries/count [1], summaries/seir_mean, seir_var (k_se, k_ei, k_ir) and state_mean, state_var (S, E, I),
        each [M,T,3]."""
        self.create_dataset("summaries/count", np.array([float(count)]))
        self._write_moments("summaries", mean, var)

    def write_forecast(self, horizon, first_day, count, mean, var):
        """The group forecast/ of one chain: horizon [1], first_day [1] (= T, the absolute day of forecast day 0),
        count [1] and the moments of the simulated events and of the state at the start of each forecast day over the
        draws forecast (`Summary.mean` / `.var` rows, [M,H,6]): seir_mean, seir_var, state_mean, state_var, each [M,H,3]."""
        self.create_dataset("forecast/horizon", np.array([float(horizon)]))
        self.create_dataset("forecast/first_day", np.array([float(first_day)]))
        self.create_dataset("forecast/count", np.array([float(count)]))
        self._write_moments("forecast", mean, var)

    def write_forecast_quantiles(self, probs, chain, pooled, pooled_chains):
        """forecast/quantile_probs [K]; forecast/cases_quantiles, cum_cases_quantiles, prevalence_quantiles, each [K,M,H]
        float64 over this chain's draws (`chain` [K,3,M,H]); forecast/pooled_* likewise over the draws of all chains of the
        process (`pooled` [K,3,M,H], the same in every chain's file) with forecast/pooled_chains, their global ids."""
        from ..sampler import FORECAST_QUANTILE_PLANES
        self.create_dataset("forecast/quantile_probs", np.asarray(probs, np.float64))
        self.create_dataset("forecast/pooled_chains", np.asarray(pooled_chains, np.float64))
        for x, name in enumerate(FORECAST_QUANTILE_PLANES):
            self.create_dataset(f"forecast/{name}_quantiles", np.ascontiguousarray(chain[:, x], dtype=np.float64))
            self.create_dataset(f"forecast/pooled_{name}_quantiles", np.ascontiguousarray(pooled[:, x], dtype=np.float64))

    def write_rt(self, days, first_day, count, mean, var, prob_gt1):
        """The group rt/ of one chain: days [1], first_day [1] (= T - D, the absolute day of the window's first day),
        count [1] and R_it_mean, R_it_var, R_it_prob_gt1 over the draws folded (`RtSummary` rows), each [D,M]."""
        self.create_dataset("rt/days", np.array([float(days)]))
        self.create_dataset("rt/first_day", np.array([float(first_day)]))
        self.create_dataset("rt/count", np.array([float(count)]))
        self.create_dataset("rt/R_it_mean", np.ascontiguousarray(mean, dtype=np.float64))
        self.create_dataset("rt/R_it_var", np.ascontiguousarray(var, dtype=np.float64))
        self.create_dataset("rt/R_it_prob_gt1", np.ascontiguousarray(prob_gt1, dtype=np.float64))

    def write_rt_quantiles(self, probs, chain, pooled, pooled_chains, national, pooled_national):
        """rt/quantile_probs [K]; rt/R_it_quantiles [K,D,M] float64 over this chain's draws; rt/pooled_R_it_quantiles
        likewise over the draws of all chains of the process (the same in every chain's file) with rt/pooled_chains, their
        global ids; rt/R_t_quantiles and rt/pooled_R_t_quantiles [K,D], the national curve's."""
        self.create_dataset("rt/quantile_probs", np.asarray(probs, np.float64))
        self.create_dataset("rt/pooled_chains", np.asarray(pooled_chains, np.float64))
        self.create_dataset("rt/R_it_quantiles", np.ascontiguousarray(chain, dtype=np.float64))
        self.create_dataset("rt/pooled_R_it_quantiles", np.ascontiguousarray(pooled, dtype=np.float64))
        self.create_dataset("rt/R_t_quantiles", np.ascontiguousarray(national, dtype=np.float64))
        self.create_dataset("rt/pooled_R_t_quantiles", np.ascontiguousarray(pooled_national, dtype=np.float64))

    def write_check(self, days, first_day, count, mean, var, counts: dict):
        """The group check/ of one chain: days [1], first_day [1] (= T - K, the absolute day of check day 0), count [1],
        the moments of the re-simulated events and state ([M,K,6] rows: seir_mean, seir_var, state_mean, state_var, each
        [M,K,3]) and `counts` (`check_chain_datasets`): observed, lt, eq [M,K], location_lt, location_eq [M], day_lt,
        day_eq [K], total_lt, total_eq [1] -- the raw counts, so that pooling over chains and ranks is a sum -- and the
        mid-p values pit, location_pit, day_pit, total_pit."""
        self.create_dataset("check/days", np.array([float(days)]))
        self.create_dataset("check/first_day", np.array([float(first_day)]))
        self.create_dataset("check/count", np.array([float(count)]))
        self._write_moments("check", mean, var)
        for k, v in counts.items():
            self.create_dataset(f"check/{k}", np.atleast_1d(np.asarray(v, np.float64)))

    def write_within_between(self, days, first_day, count, defined, within_mean, within_var, between_mean, p_within_gt_between):
        """The group within_between/ of one chain: days [1], first_day [1] (= T - D, the absolute day of the window's first
        day), count [1] (draws folded) and defined (draws with finite shares; the weight when files are pooled),
        within_mean, within_var, between_mean, p_within_gt_between over them (`WbSummary` rows), each [D,M]."""
        self.create_dataset("within_between/days", np.array([float(days)]))
        self.create_dataset("within_between/first_day", np.array([float(first_day)]))
        self.create_dataset("within_between/count", np.array([float(count)]))
        for k, v in (("defined", defined), ("within_mean", within_mean), ("within_var", within_var),
                     ("between_mean", between_mean), ("p_within_gt_between", p_within_gt_between)):
            self.create_dataset(f"within_between/{k}", np.ascontiguousarray(v, dtype=np.float64))

    def write_groups(self, table, population, initial_state):
        """The group groups/: names [G] (bytes), offsets [G+1] and members [nnz] (the CSR pair of `posterior.groups`),
        population [G] and initial_state [G,4], the members' sums of N and of the run's initial state."""
        n = max(len(x) for x in table.names)
        self.create_dataset("groups/names", np.array([x.encode() for x in table.names], dtype=f"S{max(n, 1)}"))
        self.create_dataset("groups/offsets", np.asarray(table.offsets, np.float64))
        self.create_dataset("groups/members", np.asarray(table.members, np.float64))
        self.create_dataset("groups/population", table.sum_rows(np.asarray(population, np.float64).reshape(-1)))
        self.create_dataset("groups/initial_state", table.sum_rows(np.asarray(initial_state, np.float64)))

    def write_group_forecast(self, seir_mean, state_mean, quantiles=None):
        """forecast/group_seir_mean, group_state_mean [G,H,3] over this chain's draws; `quantiles` (or None): {plane:
        (chain [K,G,H], pooled [K,G,H])} -> forecast/group_<plane>_quantiles and forecast/pooled_group_<plane>_quantiles."""
        self.create_dataset("forecast/group_seir_mean", np.ascontiguousarray(seir_mean, dtype=np.float64))
        self.create_dataset("forecast/group_state_mean", np.ascontiguousarray(state_mean, dtype=np.float64))
        for name, (own, pooled) in (quantiles or {}).items():
            self.create_dataset(f"forecast/group_{name}_quantiles", np.ascontiguousarray(own, dtype=np.float64))
            self.create_dataset(f"forecast/pooled_group_{name}_quantiles", np.ascontiguousarray(pooled, dtype=np.float64))

    def write_group_rt(self, mean, var, prob_gt1, quantiles=None):
        """rt/group_R_t_mean, group_R_t_var, group_prob_gt1 [G,D] over this chain's per-draw group curves; `quantiles` (or
        None): (chain [K,G,D], pooled [K,G,D]) -> rt/group_R_t_quantiles and rt/pooled_group_R_t_quantiles."""
        for k, v in (("group_R_t_mean", mean), ("group_R_t_var", var), ("group_prob_gt1", prob_gt1)):
            self.create_dataset(f"rt/{k}", np.ascontiguousarray(v, dtype=np.float64))
        if quantiles is not None:
            self.create_dataset("rt/group_R_t_quantiles", np.ascontiguousarray(quantiles[0], dtype=np.float64))
            self.create_dataset("rt/pooled_group_R_t_quantiles", np.ascontiguousarray(quantiles[1], dtype=np.float64))

    def write_group_ngm(self, days, first_day, K, stats, pooled=None, radius=None):
        """samples/ngm_by_group [n,G,G,D] (destination, source, day: this chain's draws of the group next-generation matrix)
        and the group ngm/: days [1], first_day [1] (= T - D), count [1], K_mean, K_var [G,G,D], local_share_mean [G,D]
        (`posterior.groups.ngm_stats`) and, where `stats` has them, K_quantiles [k,G,G,D] and local_share_quantiles [k,G,D];
        `pooled` (or None): (K_quantiles, local_share_quantiles, chain ids) over the draws of all chains of the process ->
        ngm/pooled_K_quantiles, pooled_local_share_quantiles, pooled_chains; `radius` (or None: the table is no partition):
        samples/ngm_spectral_radius [n,D] (`posterior.groups.spectral_radius`)."""
        K = np.ascontiguousarray(K, dtype=np.float64)
        self.create_dataset("samples/ngm_by_group", K)
        self.create_dataset("ngm/days", np.array([float(days)]))
        self.create_dataset("ngm/first_day", np.array([float(first_day)]))
        self.create_dataset("ngm/count", np.array([float(K.shape[0])]))
        for k in ("K_mean", "K_var", "local_share_mean", "K_quantiles", "local_share_quantiles"):
            if k in stats:
                self.create_dataset(f"ngm/{k}", np.ascontiguousarray(stats[k], dtype=np.float64))
        if pooled is not None:
            self.create_dataset("ngm/pooled_K_quantiles", np.ascontiguousarray(pooled[0], dtype=np.float64))
            self.create_dataset("ngm/pooled_local_share_quantiles", np.ascontiguousarray(pooled[1], dtype=np.float64))
            self.create_dataset("ngm/pooled_chains", np.asarray(pooled[2], np.float64))
        if radius is not None:
            self.create_dataset("samples/ngm_spectral_radius", np.ascontiguousarray(radius, dtype=np.float64))

    def write_group_within_between(self, defined, within_share_mean, p_within_gt_between):
        """within_between/group_defined, group_within_share_mean, group_p_within_gt_between [G,D] over this chain's draws:
        the share is Wg / (Wg + Bg) of the members' summed pressures ("between": from outside each member location, as in
        the national figure, not from outside the group); a draw with Wg + Bg == 0 is undefined and left out."""
        for k, v in (("group_defined", defined), ("group_within_share_mean", within_share_mean),
                     ("group_p_within_gt_between", p_within_gt_between)):
            self.create_dataset(f"within_between/{k}", np.ascontiguousarray(v, dtype=np.float64))

    def write_group_check(self, counts: dict):
        """check/group_* of one chain (`posterior.groups.check_counts`): the raw counts and the mid-p values."""
        for k, v in counts.items():
            self.create_dataset(f"check/{k}", np.atleast_1d(np.asarray(v, np.float64)))

    def write_diagnostics(self, datasets: dict):
        """The group diagnostics/ of one chain (`posterior.diagnostics.chain_datasets`), float64."""
        for k, v in datasets.items():
            self.create_dataset(f"diagnostics/{k}", np.asarray(v, np.float64))

    def __getitem__(self, name):
        if self.use_h5:
            self._file.flush()
            return self._file.read("/" + name)
        return self._mem[name]

    def close(self):
        if self.use_h5:
            self._file.close()
        else:
            out = {k.replace("/", "__"): v for k, v in {**self._mem, **self._extra}.items()}
            np.savez(self.filename, **out)


def get_weighted_running_variance(u_draws):
    """inference.py:36-47: mean/variance of the second half of a window's (unconstrained)
    draws, with pseudo-count n/2.  u_draws [n,B,P] -> (count [B], mean [B,P], var [B,P])."""
    n = u_draws.shape[0]
    half = u_draws[(-n) // 2:]      # as the reference's `draws[-draws.shape[0] // 2:]`: floor of the NEGATIVE -> 13 of 25
    mean, var = half.mean(axis=0), half.var(axis=0)
    return np.full(u_draws.shape[1], n / 2.0), mean, np.maximum(var, 1e-300)


def unconstrain_theta(theta):
    u = np.array(theta, dtype=DTYPE, copy=True)
    y = u[..., :2] - np.finfo(DTYPE).eps
    u[..., :2] = y + np.log(-np.expm1(-y))
    return u


def draws_to_dict(theta, events, chain, marginals=None):
    """inference.py:285-300 for one chain: theta [n,B,P] constrained, events [n,B,M,T,3] -- None when the event tensors
    stay on the device (summaries "only"); then, and with summaries "on", `marginals` (Trace.marginals) gives the shapes
    and the three per-draw marginal datasets."""
    if events is not None:
        M, T = events.shape[2], events.shape[3]
    else:
        M, T = marginals["events_by_location"].shape[2], marginals["events_by_day"].shape[2]
    th = theta[:, chain]
    out = {
        "psi": th[:, 0], "sigma_space": th[:, 1], "beta_area": th[:, 2], "gamma0": th[:, 3],
        "gamma1": th[:, 4], "alpha_0": th[:, 5], "alpha_t": th[:, 6:6 + T - 1],
        "spatial_effect": th[:, 6 + T - 1:6 + T - 1 + M],
    }
    if events is not None:
        out["seir"] = events[:, chain] if events.dtype.kind in "iu" else events[:, chain].astype(DTYPE)   # Posterior.write converts
    if marginals is not None:
        out["seir_by_day"] = marginals["events_by_day"][:, chain]
        out["seir_by_location"] = marginals["events_by_location"][:, chain]
        out["state_by_day"] = marginals["state_by_day"][:, chain]
    return out


def theta_to_dict(th, M, T, marginals=None, chain=0):
    """The parameters' datasets of `draws_to_dict` from one chain's theta [n,P], and the three marginal datasets of `chain`
    when `marginals` (Trace.marginals) is given: what a replay writes per burst."""
    out = {
        "psi": th[:, 0], "sigma_space": th[:, 1], "beta_area": th[:, 2], "gamma0": th[:, 3],
        "gamma1": th[:, 4], "alpha_0": th[:, 5], "alpha_t": th[:, 6:6 + T - 1],
        "spatial_effect": th[:, 6 + T - 1:6 + T - 1 + M],
    }
    if marginals is not None:
        out["seir_by_day"] = marginals["events_by_day"][:, chain]
        out["seir_by_location"] = marginals["events_by_location"][:, chain]
        out["state_by_day"] = marginals["state_by_day"][:, chain]
    return out


def trace_to_dict(tr, chain):
    """trace_results_fn (inference.py:245-282) for one chain."""
    out = {"hmc": {k: v[:, chain] for k, v in tr.hmc.items()}}
    for key in MOVE_KEYS:
        out[key] = {k: v[:, chain] for k, v in tr.moves[key].items()}
    return out


def draw_quantiles(x, probs):
    """Quantiles `probs` over the first axis of x [n, ...] by the one rank rule (`posterior.quantiles`): float64 [K, ...]."""
    from ..posterior import quantiles as Q
    x = np.asarray(x, np.float64)
    ranks = Q.quantile_ranks(x.shape[0], probs)
    return Q.interpolate(np.sort(x, axis=0)[ranks], ranks, x.shape[0], probs)


def rt_quantiles_run_line(probs, days, T, n, B, own):
    """One log line for rt_quantiles: of the last day, the widest and narrowest band between the outermost probabilities
    over chains and locations, and the share of (chain, location) cells whose band excludes 1.  own [K,B,D,M]."""
    lo, hi = own[0, :, -1], own[-1, :, -1]
    width = hi - lo
    out = float(np.mean((lo > 1.0) | (hi < 1.0))) if width.size else float("nan")
    return (f"R_t quantiles: {', '.join(f'{p:g}' for p in probs)} of R_it per day and location over days [{T - days}, {T}), exact "
            f"over {n} kept draw(s) per chain and pooled over the {B} chain(s) of this process, selected on the device; on day "
            f"{T - 1} the {probs[0]:g}-{probs[-1]:g} band is {float(width.min()):.3g} to {float(width.max()):.3g} wide and excludes 1 "
            f"in {100.0 * out:.1f} % of the locations; rt/*_quantiles written")


def check_chain_datasets(cs, c):
    """check/* of chain c beyond the moments, from a `CheckSummary`: the raw counts and the mid-p values."""
    return {"observed": cs.observed[c], "lt": cs.lt[c], "eq": cs.eq[c],
            "location_lt": cs.location_lt[c], "location_eq": cs.location_eq[c],
            "day_lt": cs.day_lt[c], "day_eq": cs.day_eq[c], "total_lt": cs.total_lt[c], "total_eq": cs.total_eq[c],
            "pit": cs.pit[c], "location_pit": cs.location_pit[c], "day_pit": cs.day_pit[c], "total_pit": cs.total_pit[c]}


def check_run_line(days, T, cs):
    """The run's one line about the check: the mid-p value of the national total over the window, pooled over the
    process's chains (the counts add), and the share of locations whose `location_pit`, pooled likewise, lies in
    [0.05, 0.95]."""
    n = np.asarray(cs.count, np.uint64).sum()
    if n == 0:
        return f"Check: window of {days} day(s) from day {T - days}, no kept draw"
    total = float(mid_p(n, cs.total_lt.astype(np.uint64).sum(), cs.total_eq.astype(np.uint64).sum()))
    loc = mid_p(n, cs.location_lt.astype(np.uint64).sum(axis=0), cs.location_eq.astype(np.uint64).sum(axis=0))
    share = float(np.mean((loc >= 0.05) & (loc <= 0.95)))
    return (f"Check: last {days} day(s) from day {T - days} simulated again from {int(n)} kept draw(s): national total mid-p "
            f"{total:.3f}; location totals with mid-p in [0.05, 0.95]: {100.0 * share:.1f} %; formed on the device; check/* "
            "and samples/check_* written")


def rt_run_line(days, T, r_t, prob_gt1):
    """The run's one line about R_t: the national value on the last day (mean and 0.05 / 0.95 quantiles over the per-draw
    curves `r_t` [n, chains, D]) and the share of locations whose P(R_it > 1) on that day exceeds 0.5 (`prob_gt1`
    [chains, D, M])."""
    last = np.asarray(r_t, np.float64)[..., -1].reshape(-1)
    if last.size == 0:
        return f"R_t: window of {days} day(s) from day {T - days}, no kept draw"
    lo, hi = np.quantile(last, [0.05, 0.95])
    share = float(np.mean(np.asarray(prob_gt1)[:, -1, :] > 0.5))
    return (f"R_t: day {T - 1} national mean {last.mean():.3f} (0.05 / 0.95 quantiles {lo:.3f} / {hi:.3f}) over {last.size} "
            f"kept draw(s); P(R_it > 1) > 0.5 in {100.0 * share:.1f} % of locations; window of {days} day(s) from day "
            f"{T - days}, formed on the device; rt/* and samples/R_t written")


def within_between_run_line(days, T, within_pressure, between_pressure, p_gt):
    """The run's one line about the within/between shares: the national within share Wn / (Wn + Bn) on the last day (mean
    and 0.05 / 0.95 quantiles over the per-draw pressures [n, chains, D]; draws without any pressure left out) and the share
    of locations whose P(within > between) on that day (`p_gt` [chains, D, M], pooled by the mean over the chains that
    define it) exceeds 0.5."""
    wn = np.asarray(within_pressure, np.float64)[..., -1].reshape(-1)
    bn = np.asarray(between_pressure, np.float64)[..., -1].reshape(-1)
    tot = wn + bn
    ok = np.isfinite(tot) & (tot != 0.0)
    if not ok.any():
        return f"Within/between: window of {days} day(s) from day {T - days}, no kept draw with infection pressure"
    share = wn[ok] / tot[ok]
    lo, hi = np.quantile(share, [0.05, 0.95])
    p = np.asarray(p_gt, np.float64)[:, -1, :]
    seen = np.isfinite(p)
    pm = np.where(seen, p, 0.0).sum(axis=0) / np.maximum(seen.sum(axis=0), 1)
    locs = float(np.mean(pm[seen.any(axis=0)] > 0.5)) if seen.any() else float("nan")
    return (f"Within/between: day {T - 1} national within share mean {share.mean():.3f} (0.05 / 0.95 quantiles {lo:.3f} / "
            f"{hi:.3f}) over {share.size} kept draw(s); P(within > between) > 0.5 in {100.0 * locs:.1f} % of locations; window "
            f"of {days} day(s) from day {T - days}, formed on the device; within_between/* and samples/within_pressure, "
            "between_pressure written")


def forecast_steps_fn(seed, chain_ids, horizon):
    """The random-walk steps of the forecast baseline (`forecast_walk`): for the j-th forecast draw of global chain c,
    H normals N(0, ALPHA_T_SCALE = 0.005) from np.random.default_rng([seed, c, j]) -- keyed like the device's draw id, so
    they do not depend on how the run is cut into bursts or sharded.  Returns the callable `ChainSampler.sample(...,
    forecast=)` takes: (j0, count) -> [count, B, H]."""
    from ..posterior.predict import ALPHA_T_SCALE

    def steps(j0, count):
        out = np.empty((int(count), len(chain_ids), int(horizon)))
        for jj in range(int(count)):
            for b, c in enumerate(chain_ids):
                out[jj, b] = np.random.default_rng([int(seed), int(c), int(j0) + jj]).normal(0.0, ALPHA_T_SCALE, int(horizon))
        return out
    return steps


def diagnostics_marks(nb):
    """{burst index: mark}: mark 0 behind burst nb // 2 - 1 and, with nb odd, mark 1 behind burst nb - nb // 2 - 1, so that
    the middle burst belongs to neither half."""
    marks = {nb // 2 - 1: 0}
    if nb % 2:
        marks[nb - nb // 2 - 1] = 1
    return marks


def _stack(bursts, *shape):
    """The bursts' kept arrays as one [n, ...]; [0, *shape] when there was no burst."""
    return np.concatenate(bursts) if bursts else np.empty((0,) + shape)


# A product's three parts side by side and what it adds to the keywords of the warm-up's and the sampling phase's draws: begin() --
# the reset behind the warm-up, the draw store where quantiles are on; flush(tr, burst) -- what must outlive the pinned view copied, its
# datasets written at its row offset, what the end needs kept (burst is None in the warm-up); finish() -- the blocking summary read,
# the write_* calls and the log line
Record = collections.namedtuple("Record", "begin flush finish warm_kw burst_kw")


def write_rows(ctx, arrays, row):
    """Every chain's slice of per-draw arrays [n,B,...] into its file, from row `row` on."""
    for c, post in enumerate(ctx.posteriors):
        post.write_samples({k: v[:, c] for k, v in arrays.items()}, first_dim_offset=row)


def _writes(ctx, field):
    """The flush of a product whose arrays go to the files as they are."""
    def flush(tr, burst):
        if getattr(tr, field, None) is not None:
            write_rows(ctx, getattr(tr, field), ctx.rows["kept"])
    return flush


def summaries_record(ctx):
    """Mcmc.summaries and Mcmc.diagnostics.  Summaries "off": sample / sample_bursts are called exactly as before the option
    existed.  Otherwise every written draw gets its marginals (the warm-up without folding), the moments cover the sampling
    phase, and with "only" no event tensor is read.  Diagnostics "on" folds the sampling phase's draws whatever `summaries`
    says (which then only decides what is written)."""
    s, posteriors, log, summaries, batch_len = ctx.s, ctx.posteriors, ctx.log, ctx.opt.summaries, ctx.opt.batch_len
    if summaries == "off" and ctx.opt.diagnostics != "on":
        return None
    theta_acc = diag_mod.DrawAccumulator(batch_len) if ctx.opt.diagnostics == "on" else None

    def begin():
        if theta_acc is not None:
            s.reset_diagnostics(batch_len)                  # the moments too: all of it is over the sampling phase
        else:
            s.reset_summary()                               # the moments are over the sampling phase
        if summaries == "only":
            print("summaries only: the event tensors stay on the device and samples/seir is not created -- what reads it "
                  "(thin_posterior, predict, reproduction_number) cannot run on this output", file=log, flush=True)

    def flush(tr, burst):
        if theta_acc is not None and burst is not None:     # the parameters' accumulators, marked where the device's are
            theta_acc.fold(tr.theta)
            if burst in ctx.marks:
                theta_acc.mark(ctx.marks[burst])

    def finish():
        dg = None
        if theta_acc is not None:
            dg = s.diagnostics()
            ev = diag_mod.evaluate(dg, theta_acc.result())
            for c, post in enumerate(posteriors):
                post.write_diagnostics(diag_mod.chain_datasets(ev, c))
            print(diag_mod.run_line(ev, diag_mod.theta_names(s.P, s.M, s.T))
                  + f" ({s.B} chain(s) of this process, batches of {batch_len})", file=log, flush=True)
        if summaries != "off":
            sm = s.summary() if dg is None else Summary(count=dg.count, ref=dg.ref, sum=dg.sum, sumsq=dg.sumsq)
            mean, var = sm.mean, sm.var
            for c, post in enumerate(posteriors):
                post.write_summary(sm.count[c], mean[c], var[c])
    return Record(begin, flush, finish, {} if summaries == "off" else dict(events=summaries != "only", summarize="marginals"),
                  dict(events=summaries != "only", summarize=True))


def forecast_record(ctx):
    """With Mcmc.forecast = H (`forecast_mode`) every kept draw of the sampling phase is forecast H days on the device
    behind its burst; `forecast_calendar` = (W [H], weekday_c [H]) (`posterior.predict.forecast_calendar`) and `seed`
    (the forecast's Philox stream and, with forecast_walk, the steps) are then needed.  The warm-up is not forecast.
    With Mcmc.forecast_quantiles (`forecast_quantiles_mode`; needs Mcmc.forecast) the device keeps cases, cumulative cases
    and prevalence of every forecast draw: the store is sized once, right behind the forecast's reset, for num_bursts x
    num_burst_samples draws per chain, and at the end of the run exact quantiles per location and forecast day are selected
    on the device, per chain and pooled over the chains of this process.  Without the key nothing of it is called.
    With Mcmc.scenarios the set goes right behind the reset and the draw store -- [K, H] arrays, or [K, M, H] for a specification with
    a targeted scenario -- and with Mcmc.groups_scenarios the switch of the scenarios' region totals right behind the set; their store
    is read once, at the end (`scenarios_write_up`)."""
    s, posteriors, log, total, horizon, walk, fq_probs = (ctx.s, ctx.posteriors, ctx.log, ctx.total, ctx.opt.horizon, ctx.opt.walk,
                                                          ctx.opt.fq_probs)
    if not horizon:
        return None
    from ..posterior import scenarios as SC_mod
    sc, base_by_day, grp_by_day, writes = ctx.scenarios, [], [], _writes(ctx, "forecast")
    vf = getattr(ctx, "verify", None)                       # the later data the forecast is scored against, or None
    grp_sc = bool(sc) and getattr(ctx, "grp_sc_on", False)   # the scenarios' region totals (Mcmc.groups_scenarios)

    def begin():
        s.reset_forecast(horizon, ctx.forecast_calendar[0], ctx.forecast_calendar[1], ctx.seed)   # once: the sampling phase
        if fq_probs:
            s.keep_forecast_draws(total)                    # the draw store of the quantiles: every kept draw of the phase
        if sc and SC_mod.is_triggered(sc):                  # a specification with a trigger: the whole set through the triggered entry
            s.set_scenarios(sc.log_shift, sc.commute, total, triggers=sc.trigger_args())
        elif sc:
            s.set_scenarios(sc.log_shift, sc.commute, total)   # once, behind the reset and the draw store: they ride from now on
        if sc:
            if grp_sc:
                s.set_scenario_groups(True)                 # right behind the set: the table is in force since groups_record was built
        if vf is not None:
            s.set_verify(vf.truth)                          # once, behind the reset, the draw store and the scenarios

    def flush(tr, burst):
        if (sc or vf is not None) and getattr(tr, "forecast", None) is not None:   # the baseline's curves: paired differences, national scores
            base_by_day.append(np.array(tr.forecast["forecast_by_day"]))
        if (vf is not None or grp_sc) and ctx.groups is not None and "forecast_by_group" in (getattr(tr, "groups", None) or {}):
            grp_by_day.append(np.array(tr.groups["forecast_by_group"]))   # the groups' curves, for the per-group scores
        writes(tr, burst)

    def finish():
        fs = s.forecast_summary()
        mean, var = fs.mean, fs.var
        for c, post in enumerate(posteriors):
            post.write_forecast(horizon, s.T, fs.count[c], mean[c], var[c])
        print(f"Forecast: {horizon} day(s) from day {s.T} for {int(fs.count.min()) if len(fs.count) else 0} kept draw(s) per "
              f"chain, formed on the device ({'random-walk' if walk else 'held'} baseline); forecast/* and "
              "samples/forecast_* written", file=log, flush=True)
        own = pooled = None
        if fq_probs and total:
            own = s.forecast_quantiles(fq_probs)                        # [K,B,3,M,H]
            pooled = s.forecast_quantiles(fq_probs, pooled=True)        # [K,3,M,H]
            for c, post in enumerate(posteriors):
                post.write_forecast_quantiles(fq_probs, own[:, c], pooled, ctx.chain_ids)
            print(f"Forecast quantiles: {', '.join(f'{p:g}' for p in fq_probs)} of cases, cumulative cases and prevalence per "
                  f"location and forecast day, exact over {total} kept draw(s) per chain and pooled over the {s.B} "
                  "chain(s) of this process, selected on the device; forecast/*_quantiles written", file=log, flush=True)
        if sc:
            scenarios_write_up(ctx, sc, _stack(base_by_day, s.B, horizon, 3),
                               **(dict(base_by_group=_stack(grp_by_day, s.B, ctx.groups.G, horizon, 3)) if grp_sc else {}))
        if vf is not None:
            verify_write_up(ctx, vf, _stack(base_by_day, s.B, horizon, 3), own, pooled,
                            _stack(grp_by_day, s.B, ctx.groups.G, horizon, 3) if ctx.groups is not None else None)
    return Record(begin, flush, finish, {},
                  dict(forecast=forecast_steps_fn(ctx.seed, ctx.chain_ids, horizon) if walk else True))


def verify_write_up(ctx, vf, by_day, own_q, pooled_q, by_group=None):
    """The one read of each kind at the end of the run (`posterior.verify`; Mcmc.verify rides on Mcmc.forecast) and what every
    chain's file gains: the group verify/ -- truth [M,H], valid [M,H,2] (cases, cum_cases), horizon, first_day, count; the raw lt,
    eq, abs_sum [M,H,2], so that pooling over files is a sum; pit, mae; with the draw store (forecast_quantiles) pair_sum, crps and
    pooled_pair_sum, pooled_crps (over the chains of this process: pooled_chains); national_truth, national_valid and the
    national_* scores [H,2] from the per-draw curves samples/forecast_by_day (`by_day` [n,B,H,3]); with forecast_quantiles
    coverage_probs and coverage, pooled_coverage [P,H,2], the share of valid cells inside every central interval the
    probabilities contain; with `groups` group_truth [G,H], group_valid and the group_* scores [G,H,2] from the per-draw curves
    samples/forecast_by_group (`by_group` [n,B,G,H,3]): a group's truth is the sum over its members, valid where every member
    is.  The pooled pair sum covers B x n values per cell: above `_lib.PAIR_ABS_MAX_N` (`ctx.verify_pooled` False, decided and
    logged before the first GPU call) pooled_pair_sum and pooled_crps are not written.  One log line."""
    from ..posterior import verify as V
    s, horizon, probs = ctx.s, ctx.opt.horizon, ctx.opt.fq_probs
    y, valid = V.truth_targets(vf.truth)
    acc = s.verify_summary()                                # one read of the accumulators ...
    n = int(acc["count"].min()) if len(acc["count"]) else 0
    store = own_q is not None and n > 0
    per = s.forecast_pair_sums() if store else None         # ... and one of each kind of the pair sums: [B,2,M,H], [2,M,H]
    pooled_pair = s.forecast_pair_sums(pooled=True) if store and getattr(ctx, "verify_pooled", True) else None
    if store:                                               # a cell without truth has all four zero
        per = np.where(np.moveaxis(valid, -1, 0), per, 0)
    if pooled_pair is not None:
        pooled_pair = np.where(np.moveaxis(valid, -1, 0), pooled_pair, 0)
    pooled = V.pool([dict(count=n, **{k: acc[k][c] for k in ("lt", "eq", "abs_sum")}) for c in range(s.B)])
    pooled_sc = V.scores(pooled["count"], pooled["lt"], pooled["eq"], pooled["abs_sum"], valid,
                         None if pooled_pair is None else np.moveaxis(pooled_pair, 0, -1))
    tnat = np.where((vf.truth >= 0).all(axis=0), np.where(vf.truth >= 0, vf.truth, 0).astype(np.int64).sum(axis=0), -1)[None]
    ynat, vnat = V.truth_targets(tnat)
    ygrp = vgrp = None
    if by_group is not None:
        ok = ctx.groups.sum_rows((vf.truth < 0).astype(np.int64)) == 0            # [G,H]: every member observed
        ygrp, vgrp = V.truth_targets(np.where(ok, ctx.groups.sum_rows(np.where(vf.truth >= 0, vf.truth, 0).astype(np.int64)), -1))
    pairs = V.interval_pairs(probs) if store else []
    yq = np.moveaxis(y, -1, 0)                              # [2,M,H], as the quantiles' planes 0 and 1

    def cover(q):                                           # q [K,2,M,H] -> [P,H,2]
        return np.stack([V.coverage(np.moveaxis(q[lo], 0, -1), np.moveaxis(q[hi], 0, -1), np.moveaxis(yq, 0, -1), valid)
                         for lo, hi, _ in pairs])
    own_crps = []
    for c, post in enumerate(ctx.posteriors):
        sc = V.scores(n, acc["lt"][c], acc["eq"][c], acc["abs_sum"][c], valid, None if per is None else np.moveaxis(per[c], 0, -1))
        own_crps.append(sc.get("crps"))
        post.create_dataset("verify/truth", vf.truth, dtype=np.int64)
        post.create_dataset("verify/valid", valid, dtype=np.int64)
        for key, v in (("horizon", horizon), ("first_day", s.T), ("count", n)):
            post.create_dataset(f"verify/{key}", np.array([float(v)]))
        for key in ("lt", "eq", "abs_sum"):
            post.create_dataset(f"verify/{key}", acc[key][c], dtype=np.int64)
        for key in ("pit", "mae"):
            post.create_dataset(f"verify/{key}", sc[key])
        if store:
            post.create_dataset("verify/pair_sum", np.moveaxis(per[c], 0, -1), dtype=np.int64)
            post.create_dataset("verify/crps", sc["crps"])
            if pooled_pair is not None:
                post.create_dataset("verify/pooled_pair_sum", np.moveaxis(pooled_pair, 0, -1), dtype=np.int64)
                post.create_dataset("verify/pooled_crps", pooled_sc["crps"])
            post.create_dataset("verify/pooled_chains", np.asarray(ctx.chain_ids), dtype=np.int64)
        nat = V.score_draws(V.targets(by_day[:, c][:, None]), ynat, vnat)
        post.create_dataset("verify/national_truth", ynat[0], dtype=np.int64)
        post.create_dataset("verify/national_valid", vnat[0], dtype=np.int64)
        for key in ("lt", "eq", "abs_sum", "pair_sum"):
            post.create_dataset(f"verify/national_{key}", nat[key][0], dtype=np.int64)
        for key in ("pit", "mae", "crps"):
            post.create_dataset(f"verify/national_{key}", nat[key][0])
        if ygrp is not None:
            grp = V.score_draws(V.targets(by_group[:, c]), ygrp, vgrp)
            post.create_dataset("verify/group_truth", ygrp[..., 0], dtype=np.int64)
            post.create_dataset("verify/group_valid", vgrp, dtype=np.int64)
            for key in ("lt", "eq", "abs_sum", "pair_sum"):
                post.create_dataset(f"verify/group_{key}", grp[key], dtype=np.int64)
            for key in ("pit", "mae", "crps"):
                post.create_dataset(f"verify/group_{key}", grp[key])
        if pairs:
            post.create_dataset("verify/coverage_probs", np.array([p for _, _, p in pairs]))
            post.create_dataset("verify/coverage", cover(own_q[:, c, :2]))
            post.create_dataset("verify/pooled_coverage", cover(pooled_q[:, :2]))
    crps = pooled_sc.get("crps") if pooled_pair is not None else (np.stack(own_crps) if store else None)   # else the chains' own
    print(V.run_line(vf.truth, by_day, pooled_sc["pit"], crps, valid), file=ctx.log, flush=True)


def scenarios_write_up(ctx, sc, base_by_day, base_by_group=None):
    """The one read of the scenarios at the end of the run (`posterior.scenarios`; Mcmc.scenarios rides on Mcmc.forecast) and what
    every chain's file gains: the group scenarios/ -- names, log_shift, commute [K,H], horizon, first_day, count; the moments
    seir_mean, seir_var, state_mean, state_var [K,M,H,3]; of the paired differences to the forecast diff_mean, diff_var, p_below,
    p_equal [K,M,H,4] (cases, cum_cases, prevalence, cum_infections) with the raw counts diff_lt, diff_eq, so that pooling over
    files is a sum -- and per kept draw samples/scenario_by_day, scenario_state_by_day and scenario_diff_by_day [n,K,H,3], the last
    one the scenario's curve minus samples/forecast_by_day (`base_by_day` [n,B,H,3]), formed here; with forecast_quantiles also
    scenarios/national_diff_quantiles [Kq,K,H,3] of those differences.  One log line per scenario.
    A specification with a targeted scenario (`posterior.scenarios.LocalScenarios`) writes scenarios/log_shift_by_location and
    commute_by_location [K,M,H] in the place of log_shift and commute, and scenarios/locations [K,M] uint8, 1 where any multiplier of
    the row differs from the identity.  With Mcmc.groups_scenarios (`base_by_group` [n,B,G,H,3], the forecast's samples/forecast_by_group)
    one read of the scenarios' group store: samples/scenario_by_group [n,K,G,H,3] and scenario_diff_by_group, the scenario's totals
    minus the forecast's, formed here; with forecast_quantiles scenarios/group_diff_quantiles [Kq,K,G,H,3]; one log line per scenario
    and group.
    A specification with a trigger (`posterior.scenarios.TriggeredScenarios`) makes two more reads, the record of the rule, and
    writes the rule -- scenarios/trigger_on, trigger_off [K,M] int32, trigger_window, _from_day, _min_days, _review_every [K], the
    on pair log_shift_on_by_location, commute_on_by_location [K,M,H] -- scenarios/active_count [K,M,H] uint32 (the draws in which
    the location is under the measure on the day: pooling over files is a sum), p_active = active_count / count,
    samples/scenario_active_by_day [n,K,H] int32 (the locations under the measure) and, with forecast_quantiles,
    scenarios/active_by_day_quantiles [Kq,K,H]; one more log line per triggered scenario."""
    from ..posterior import scenarios as SC
    s, horizon = ctx.s, ctx.opt.horizon
    sums, diffs, draws = s.scenario_summary(), s.scenario_diffs(), s.read_scenario_draws()
    n = int(diffs["count"])
    st = SC.statistics(n, diffs["ref"], diffs["sum"], diffs["sumsq"], diffs["lt"], diffs["eq"]) if n else None
    by_day = np.moveaxis(draws["by_day"], 0, 2)             # [n,B,K,H,3]
    state = np.moveaxis(draws["state_by_day"], 0, 2)
    diff = by_day - np.asarray(base_by_day, np.int64)[:, :, None]
    local = SC.is_local(sc)
    triggered = SC.is_triggered(sc)
    if triggered:
        active_count = s.scenario_triggers()["active_count"]                   # [K,B,M,H]
        active_by_day = np.moveaxis(s.read_scenario_trigger_draws(), 0, 2)     # [n,B,K,H]
    by_group = diff_group = None
    if base_by_group is not None:
        by_group = np.moveaxis(s.read_scenario_group_draws(), 0, 2)            # [n,B,K,G,H,3]
        diff_group = by_group - np.asarray(base_by_group, np.int64)[:, :, None]
    width = max(len(name.encode()) for name in sc.names)
    for c, post in enumerate(ctx.posteriors):
        post.create_dataset("scenarios/names", np.array([name.encode() for name in sc.names], dtype=f"S{width}"))
        if local:
            post.create_dataset("scenarios/log_shift_by_location", sc.log_shift)
            post.create_dataset("scenarios/commute_by_location", sc.commute)
            post.create_dataset("scenarios/locations", sc.locations, dtype=np.uint8)
        else:
            post.create_dataset("scenarios/log_shift", sc.log_shift)
            post.create_dataset("scenarios/commute", sc.commute)
        for key, v in (("horizon", horizon), ("first_day", s.T), ("count", n)):
            post.create_dataset(f"scenarios/{key}", np.array([float(v)]))
        mean, var = np.stack([m.mean[c] for m in sums]), np.stack([m.var[c] for m in sums])
        post._write_moments("scenarios", mean, var)
        if st is not None:
            for key in ("mean", "var"):
                post.create_dataset(f"scenarios/diff_{key}", st[key][:, c])
            for key in ("p_below", "p_equal"):
                post.create_dataset(f"scenarios/{key}", st[key][:, c])
        for key in ("lt", "eq"):
            post.create_dataset(f"scenarios/diff_{key}", diffs[key][:, c], dtype=np.int64)
        for key, v in (("scenario_by_day", by_day), ("scenario_state_by_day", state), ("scenario_diff_by_day", diff)):
            post.create_dataset(f"samples/{key}", np.ascontiguousarray(v[:, c]), dtype=np.int64)
        if ctx.opt.fq_probs and n:
            post.create_dataset("scenarios/national_diff_quantiles", draw_quantiles(diff[:, c], ctx.opt.fq_probs))
        if by_group is not None:
            for key, v in (("scenario_by_group", by_group), ("scenario_diff_by_group", diff_group)):
                post.create_dataset(f"samples/{key}", np.ascontiguousarray(v[:, c]), dtype=np.int64)
            if ctx.opt.fq_probs and n:
                post.create_dataset("scenarios/group_diff_quantiles", draw_quantiles(diff_group[:, c], ctx.opt.fq_probs))
        if triggered:
            for key, v in (("trigger_on", sc.trigger_on), ("trigger_off", sc.trigger_off), ("trigger_window", sc.window),
                           ("trigger_from_day", sc.from_day), ("trigger_min_days", sc.min_days), ("trigger_review_every", sc.review_every)):
                post.create_dataset(f"scenarios/{key}", v, dtype=np.int32)
            post.create_dataset("scenarios/log_shift_on_by_location", sc.log_shift_on)
            post.create_dataset("scenarios/commute_on_by_location", sc.commute_on)
            post.create_dataset("scenarios/active_count", active_count[:, c], dtype=np.uint32)
            if n:
                post.create_dataset("scenarios/p_active", active_count[:, c] / n)
            post.create_dataset("samples/scenario_active_by_day", np.ascontiguousarray(active_by_day[:, c]), dtype=np.int32)
            if ctx.opt.fq_probs and n:
                post.create_dataset("scenarios/active_by_day_quantiles", draw_quantiles(active_by_day[:, c], ctx.opt.fq_probs))
    for k, name in enumerate(sc.names):
        if n:
            print(SC.run_line(name, diff[:, :, k].reshape(-1, horizon, 3)), file=ctx.log, flush=True)
        if n and triggered and sc.triggered[k]:
            print(SC.trigger_run_line(name, active_by_day[:, :, k].reshape(-1, horizon)), file=ctx.log, flush=True)
        for g in range(ctx.groups.G if by_group is not None and n else 0):
            print(SC.group_run_line(name, ctx.groups.names[g], diff_group[:, :, k, g].reshape(-1, horizon, 3)), file=ctx.log, flush=True)


def rt_record(ctx):
    """With Mcmc.rt = D (`rt_mode`) R_it of every kept draw of the sampling phase over the last D days is formed and folded
    on the device behind its burst (and behind the burst's summary and forecast); `rt_weight` [M] = N / N.sum() is then
    needed.  The warm-up is not folded; without the key nothing of it is called.
    With Mcmc.rt_quantiles (`rt_quantiles_mode`; needs Mcmc.rt) the device keeps R_it of every folded draw: the store is
    sized once, right behind the rt reset, for num_bursts x num_burst_samples draws per chain, and at the end of the run
    exact quantiles per day and location are selected on the device, per chain and pooled over the chains of this process;
    the national curve's quantiles are formed here from the draws of R_t.  Without the key nothing of it is called."""
    s, posteriors, log, total, rt_days, rq_probs = ctx.s, ctx.posteriors, ctx.log, ctx.total, ctx.opt.rt_days, ctx.opt.rq_probs
    if not rt_days:
        return None
    rt_draws = []                                           # the national curve of every burst: flush keeps, finish reads

    def begin():
        s.reset_rt(rt_days, ctx.rt_weight)                  # once: the sampling phase
        if rq_probs:
            s.keep_rt_draws(total)                          # the draw store of the quantiles: every kept draw of the phase

    def flush(tr, burst):
        if getattr(tr, "rt", None) is not None:
            rt_draws.append(np.array(tr.rt))                # the pinned buffer is used again two bursts later
            write_rows(ctx, {"R_t": rt_draws[-1]}, ctx.rows["kept"])

    def finish():
        rs = s.rt_summary()
        mean, var, prob = rs.mean, rs.var, rs.prob_gt1
        for c, post in enumerate(posteriors):
            post.write_rt(rt_days, s.T - rt_days, rs.count[c], mean[c], var[c], prob[c])
        r_t = _stack(rt_draws, s.B, rt_days)
        print(rt_run_line(rt_days, s.T, r_t, prob), file=log, flush=True)
        if rq_probs and total:
            own = s.rt_quantiles(rq_probs)                              # [K,B,D,M]
            pooled = s.rt_quantiles(rq_probs, pooled=True)              # [K,D,M]
            nat = draw_quantiles(r_t, rq_probs)                         # [K,B,D]: costs nothing here
            pnat = draw_quantiles(r_t.reshape(-1, rt_days), rq_probs)   # [K,D]
            for c, post in enumerate(posteriors):
                post.write_rt_quantiles(rq_probs, own[:, c], pooled, ctx.chain_ids, nat[:, c], pnat)
            print(rt_quantiles_run_line(rq_probs, rt_days, s.T, total, s.B, own), file=log, flush=True)
    return Record(begin, flush, finish, {}, dict(rt=True))


def check_record(ctx):
    """With Mcmc.check = K (`check_mode`) the last K days are simulated again from every kept draw of the sampling phase and
    set against the observed removals on the device, behind the burst's summary, forecast and R_t; `check_calendar` =
    (W [K], weekday_c [K]) (`posterior.predict.check_calendar`) is then needed, and the check's stream is keyed by
    `check_seed(seed)`.  The warm-up is not checked; without the key nothing of it is called."""
    s, check_days = ctx.s, ctx.opt.check_days
    if not check_days:
        return None

    def begin():
        s.reset_check(check_days, ctx.check_calendar[0], ctx.check_calendar[1], check_seed(ctx.seed))   # once

    def finish():
        ctx.rows["check"] = cs = s.check_summary()          # read by the groups' finish, which runs behind this one
        mean, var = cs.moments.mean, cs.moments.var
        for c, post in enumerate(ctx.posteriors):
            post.write_check(check_days, s.T - check_days, cs.count[c], mean[c], var[c], check_chain_datasets(cs, c))
        print(check_run_line(check_days, s.T, cs), file=ctx.log, flush=True)
    return Record(begin, _writes(ctx, "check"), finish, {}, dict(check=True))


def groups_record(ctx):
    """With `groups` (a `posterior.groups.GroupTable`, Mcmc.groups bound by `Products.bind`; needs one of summaries on / only, forecast,
    check) the table is set on the sampler once, before the first draw: from then on the summary, the forecast and the check of every
    burst also form the draw's sums over each group's members on the device, and these cross with the trace.  In the warm-up that rides
    on the summary which `summaries` already asks for there, and on nothing else. The statistics are formed here (`posterior.groups`).
    Without it nothing of it is called. With Mcmc.groups_rt (needs `groups`, Mcmc.rt and `population` = N [M]) and
    Mcmc.groups_within_between (needs `groups` and Mcmc.within_between) the switches are set on the sampler once, behind the table: R_t,
    population-weighted, and the within / between pressures of every kept draw of the sampling phase are then also formed per group on
    the device and cross with the trace (`trace.group_curves`).  Without the keys nothing of it is called. With Mcmc.groups_ngm (needs
    `groups`, Mcmc.rt and Mcmc.groups_rt) the group next-generation matrix of every kept draw of the sampling phase is kept on the
    device: the switch is set once, behind set_group_rt and the rt reset, with a store of num_bursts x num_burst_samples draws per
    chain, and read once at the end of sampling.  It is no burst product: the draws' keywords are what they were.  Without the key
    nothing of it is called."""
    s, opt, posteriors, log, rows, groups, total = ctx.s, ctx.opt, ctx.posteriors, ctx.log, ctx.rows, ctx.groups, ctx.total
    if groups is None:
        return None
    summaries, horizon, check_days, rt_days, wb_days, fq_probs, rq_probs = (opt.summaries, opt.horizon, opt.check_days, opt.rt_days,
                                                                            opt.wb_days, opt.fq_probs, opt.rq_probs)
    # the one record that calls the sampler when it is built, ahead of the warm-up
    s.set_groups(groups.offsets, groups.members)            # once; the sources size their outputs at their resets
    if opt.grp_rt_on:
        ctx.rt_w = G_mod.rt_weights(groups, ctx.population)
        s.set_group_rt(ctx.rt_w)                            # once, behind the table; sized at the rt reset
        for post in posteriors:
            post.create_dataset("groups/rt_weights", ctx.rt_w)
    if opt.grp_wb_on:
        s.set_group_within_between(True)
    # the sources whose sums are written: the trace's only with summaries on / only (diagnostics alone also summarises
    # every burst, but nothing of it goes to the file); with the group curves alone there is nothing to ask for
    sources = {k: name for k, name, on in (("trace", "the recorded epidemic", summaries != "off"), ("forecast", "the forecast", horizon),
                                           ("check", "the check", check_days)) if on}
    grp_fc, grp_ck, grp_rt, grp_wb = [], [], [], []         # the sampling phase's group sums and curves, kept for the statistics

    def begin():
        if opt.grp_ngm_on:      # the store is sized behind the rt reset (rt_record's begin, which runs first) and set_group_rt
            s.set_group_ngm(ctx.rt_w, total)

    def flush(tr, burst):
        if getattr(tr, "groups", None) is not None:
            g = {k: np.array(v) for k, v in tr.groups.items()}   # the pinned buffer is used again two bursts later
            if "forecast_by_group" in g:
                grp_fc.append((g["forecast_by_group"], g["forecast_group_state0"]))
            if "check_by_group" in g:
                grp_ck.append(g["check_by_group"])
            for c, post in enumerate(posteriors):
                if "seir_by_group" in g:
                    post.write_samples({"seir_by_group": g["seir_by_group"][:, c]}, first_dim_offset=rows["offset"])
                post.write_samples({k: v[:, c] for k, v in g.items() if k.startswith("forecast_")}, first_dim_offset=rows["kept"])
                post.write_samples({k: v[:, c] for k, v in g.items() if k.startswith("check_")}, first_dim_offset=rows["kept"])
        if (opt.grp_rt_on or opt.grp_wb_on) and getattr(tr, "group_curves", None) is not None:
            gc = {k: np.array(v) for k, v in tr.group_curves.items()}   # the pinned buffer is used again two bursts later
            if "rt_by_group" in gc:
                grp_rt.append(gc["rt_by_group"])
                write_rows(ctx, {"R_t_by_group": gc["rt_by_group"]}, rows["kept"])
            if "within_by_group" in gc:
                grp_wb.append((gc["within_by_group"], gc["between_by_group"]))
                write_rows(ctx, {"within_pressure_by_group": gc["within_by_group"],
                                "between_pressure_by_group": gc["between_by_group"]}, rows["kept"])

    def finish():
        if horizon and grp_fc:
            ev = np.concatenate([x[0] for x in grp_fc])     # [nf,B,G,H,3]
            st0 = np.concatenate([x[1] for x in grp_fc])    # [nf,B,G,3]
            state = G_mod.group_state(ev, st0)
            q = None
            if fq_probs:
                planes = G_mod.forecast_planes(ev, st0)     # [3,nf,B,G,H]
                q = {name: (G_mod.quantiles(planes[x], fq_probs),                                    # [K,B,G,H]
                            G_mod.quantiles(planes[x].reshape((-1,) + planes.shape[3:]), fq_probs))   # [K,G,H]
                     for x, name in enumerate(G_mod.PLANES)}
            for c, post in enumerate(posteriors):
                post.write_group_forecast(ev[:, c].mean(axis=0), state[:, c].mean(axis=0),
                                          None if q is None else {k: (v[0][:, c], v[1]) for k, v in q.items()})
        if check_days and grp_ck:
            sim = np.concatenate(grp_ck)                    # [nf,B,G,K,3]
            for c, post in enumerate(posteriors):
                post.write_group_check(G_mod.check_counts(sim[:, c], groups.sum_rows(rows["check"].observed[c])))
        if sources:
            print(G_mod.run_line(groups, list(sources.values())), file=log, flush=True)
        rg = _stack(grp_rt, s.B, groups.G, rt_days)         # [n,B,G,D]; for the matrix: the denominator of the local share
        if opt.grp_rt_on:
            q = None
            if rq_probs and rg.shape[0]:
                q = (draw_quantiles(rg, rq_probs), draw_quantiles(rg.reshape((-1,) + rg.shape[2:]), rq_probs))   # [K,B,G,D], [K,G,D]
            for c, post in enumerate(posteriors):
                post.write_group_rt(*G_mod.curve_moments(rg[:, c]), None if q is None else (q[0][:, c], q[1]))
            print(G_mod.curve_run_line("R_t", groups, rg, "samples/R_t_by_group and rt/group_*"), file=log, flush=True)
        if opt.grp_ngm_on:
            K = s.read_group_ngm(total) if total else np.empty((0, s.B, groups.G, groups.G, rt_days))   # [n,B,G,G,D]
            part = G_mod.is_partition(groups, s.M)
            pooled = None
            if rq_probs and K.shape[0]:
                ps = G_mod.ngm_stats(K.reshape((-1,) + K.shape[2:]), rg.reshape((-1,) + rg.shape[2:]), rq_probs)
                pooled = (ps["K_quantiles"], ps["local_share_quantiles"], ctx.chain_ids)
            for c, post in enumerate(posteriors):
                post.write_group_ngm(rt_days, s.T - rt_days, K[:, c],
                                     G_mod.ngm_stats(K[:, c], rg[:, c], rq_probs if rq_probs and K.shape[0] else None),
                                     pooled, G_mod.spectral_radius(K[:, c]) if part else None)
            print(G_mod.ngm_run_line(groups, K, rg), file=log, flush=True)
        if opt.grp_wb_on:
            wg, bg = (_stack([x[i] for x in grp_wb], s.B, groups.G, wb_days) for i in (0, 1))
            for c, post in enumerate(posteriors):
                post.write_group_within_between(*G_mod.share_stats(wg[:, c], bg[:, c]))
            with np.errstate(divide="ignore", invalid="ignore"):
                share = wg / (wg + bg)
            print(G_mod.curve_run_line("Within share of the infection pressure (between: from outside each member location)",
                                       groups, share, "samples/*_pressure_by_group and within_between/group_*"),
                  file=log, flush=True)
    return Record(begin, flush, finish, dict(groups=("trace",)) if summaries != "off" else {}, dict(groups=tuple(sources)) if sources else {})


def within_between_record(ctx):
    """With Mcmc.within_between = D (`within_between_mode`) the within/between pressure shares of every kept draw of the
    sampling phase over the last D days are formed and folded on the device, behind the burst's summary, forecast, R_t and
    check.  The warm-up is not folded; without the key nothing of it is called."""
    s, wb_days = ctx.s, ctx.opt.wb_days
    if not wb_days:
        return None
    wb_draws = []                                           # the national pressures of every burst: flush keeps, finish reads

    def begin():
        s.reset_within_between(wb_days)                     # once: the sampling phase

    def flush(tr, burst):
        if getattr(tr, "wb", None) is not None:
            wb_draws.append({k: np.array(v) for k, v in tr.wb.items()})   # the pinned buffer is used again two bursts later
            write_rows(ctx, wb_draws[-1], ctx.rows["kept"])

    def finish():
        ws = s.within_between_summary()
        wm, wv, bm, pg = ws.within_mean, ws.within_var, ws.between_mean, ws.p_within_gt_between
        for c, post in enumerate(ctx.posteriors):
            post.write_within_between(wb_days, s.T - wb_days, ws.count[c], ws.defined[c], wm[c], wv[c], bm[c], pg[c])
        wn, bn = (_stack([w[k] for w in wb_draws], s.B, wb_days) for k in ("within_pressure", "between_pressure"))
        print(within_between_run_line(wb_days, s.T, wn, bn, pg), file=ctx.log, flush=True)
    return Record(begin, flush, finish, {}, dict(within_between=True))


# in the order of the resets and the write-up
RECORD_BUILDERS = (summaries_record, forecast_record, rt_record, check_record, groups_record, within_between_record)


def product_records(sampler, config, posteriors, log=sys.stderr, forecast_calendar=None, seed=0, rt_weight=None,
                    check_calendar=None, groups=None, population=None, total=None, results=True, verify=None, *,
                    location_names=None):
    """What `run_mcmc` and `posterior.replay.replay_files` share: the options resolved (`resolve_products`; a resolved section resolves to
    itself) and the missing inputs refused before the first call on the sampler, the products' `Record`s in the order of the resets and
    the write-up, the keywords of the warm-up's and the sampling phase's draws, the diagnostics' marks and the row bookkeeping.
    `total`: the kept draws per chain the products will see (default num_bursts x num_burst_samples: what sizes the draw stores);
    `results=False`: a burst's flush writes the parameters' rows and the marginals only (a replay has no kernel results and no event
    tensor)."""
    config, opt = resolve_products(config)
    opt.windows(getattr(sampler, "T", None))
    if opt.check_days and check_calendar is None:
        raise ValueError("check: run_mcmc needs check_calendar = (W, weekday_c) of the window")
    if opt.rt_days and rt_weight is None:
        raise ValueError("rt: run_mcmc needs rt_weight = N / N.sum()")
    if opt.horizon and forecast_calendar is None:
        raise ValueError("forecast: run_mcmc needs forecast_calendar = (W, weekday_c) of the forecast days")
    opt.require(groups)
    if opt.grp_rt_on and population is None:
        raise ValueError("groups_rt: run_mcmc needs population = N")
    nb, ns = int(config["num_bursts"]), int(config["num_burst_samples"])
    scenarios = resolve_scenarios(config, opt.horizon)      # Mcmc.scenarios: a resolution of its own; empty when the key is absent
    # a targeted specification's members to rows (`location_names`: the input's codes, a callable that reads them, or None), and
    # Mcmc.groups_scenarios held to scenarios and groups -- both before the first call on the sampler
    scenarios = bind_scenarios(scenarios, getattr(sampler, "M", 0), location_names, population)
    grp_sc_on = resolve_scenario_groups(config, scenarios, groups)
    if resolve_verify(config, opt.horizon) is not None and verify is None:   # Mcmc.verify likewise; `verify`: posterior.verify.Truth
        raise ValueError("verify: run_mcmc needs verify = posterior.verify.load_truth(path, data_file, horizon)")
    if verify is not None:
        if not opt.horizon:
            raise ValueError("verify: scoring needs a forecast (set Mcmc.forecast / --forecast H)")
        if np.shape(verify.truth) != (getattr(sampler, "M", np.shape(verify.truth)[0]), opt.horizon):
            raise ValueError(f"verify: truth {np.shape(verify.truth)} is not [M, {opt.horizon}]")
    verify_pooled = True
    if verify is not None and opt.fq_probs:                 # the pair sums' bound, against what is known before the first GPU call
        from .. import _lib as lib_mod
        kept = nb * ns if total is None else int(total)
        if kept > lib_mod.PAIR_ABS_MAX_N:
            raise ValueError(f"verify with forecast_quantiles: {kept} kept draws per chain -- the pair sums of the CRPS hold "
                             f"{lib_mod.PAIR_ABS_MAX_N} values per cell (thin the run, or drop forecast_quantiles for PIT and MAE alone)")
        if sampler.B * kept > lib_mod.PAIR_ABS_MAX_N:
            verify_pooled = False
            print(f"Verify: {sampler.B} chain(s) x {kept} kept draws are {sampler.B * kept} values per pooled cell, above the "
                  f"{lib_mod.PAIR_ABS_MAX_N} the pair sums hold: verify/pooled_pair_sum and pooled_crps are not written (the "
                  "chains' own pair_sum and crps are)", file=log, flush=True)

    ctx = types.SimpleNamespace(
        s=sampler, opt=opt, scenarios=scenarios, grp_sc_on=grp_sc_on, verify=verify, verify_pooled=verify_pooled, posteriors=posteriors, log=log, seed=seed, forecast_calendar=forecast_calendar, rt_weight=rt_weight,
        check_calendar=check_calendar, groups=groups, population=population,
        total=nb * ns if total is None else int(total),     # kept draws per chain that the products will see
        chain_ids=[getattr(sampler, "first_chain_id", 0) + c for c in range(sampler.B)],
        marks=diagnostics_marks(nb) if opt.diagnostics == "on" else {},
        # `offset` counts every written draw, `kept` the sampling phase's: the row of every product's per-draw datasets (a field
        # is in a trace exactly when its keyword was passed: all together, on the sampling phase's bursts); `check`: the
        # check's summary, written by check_record's finish and read by groups_record's, which runs behind it
        rows=dict(offset=0, kept=0, check=None),
        # the weights of the group R_t: written by groups_record when it is built (groups_rt on), read by its begin for the
        # group next-generation matrix -- set whenever it is read, because `require_ngm` holds groups_ngm to groups_rt
        rt_w=None)
    built = {build: build(ctx) for build in RECORD_BUILDERS}   # None: the product is off, nothing of it is called
    records = [r for r in built.values() if r is not None]
    warm_kw, burst_kw = {}, {}                              # the keywords of the warm-up's and the sampling phase's draws
    for r in records:
        warm_kw.update(r.warm_kw)
        burst_kw.update(r.burst_kw)
    # a burst is written out groups first, then last record to first: the order the files have always been written in
    grp = built[groups_record]
    flush_order = ([grp] if grp else []) + [r for r in reversed(records) if r is not grp]
    rows, summaries = ctx.rows, opt.summaries

    def flush(tr, burst=None):
        for r in flush_order:
            r.flush(tr, burst)
        for c, post in enumerate(posteriors):
            if not results:                                 # a replay: the parameters' rows and the marginals, nothing else
                post.write_samples(theta_to_dict(tr.theta[:, c], sampler.M, sampler.T, None if summaries == "off" else tr.marginals, c),
                                   first_dim_offset=rows["offset"])
                continue
            post.write_samples(draws_to_dict(tr.theta, tr.events, c, **({} if summaries == "off" else dict(marginals=tr.marginals))),
                               first_dim_offset=rows["offset"])
            post.write_results(trace_to_dict(tr, c), first_dim_offset=rows["offset"])
        rows["offset"] += tr.theta.shape[0]
        if burst is not None:
            rows["kept"] += tr.theta.shape[0]
        return tr

    return types.SimpleNamespace(records=records, flush=flush, warm_kw=warm_kw, burst_kw=burst_kw, marks=ctx.marks, thin=opt.thin,
                                 nb=nb, ns=ns, rows=rows)


def run_mcmc(sampler: ChainSampler, config, posteriors, log=sys.stderr, pool_step_size=False, forecast_calendar=None,
             seed=0, rt_weight=None, check_calendar=None, groups=None, population=None, verify=None, *, location_names=None):
    """The windowed schedule of inference.py:303-470: fast 200, slow 25*2^k (k<6), fast 50,
    then num_bursts x num_burst_samples with the kernel fixed.  Every draw of the warm-up is
    written, as in the reference (its running variance is formed from every draw of a window);
    the sampling phase keeps every `thin`-th sweep: num_burst_samples kept draws per burst from
    num_burst_samples * thin sweeps (inference.py:455), thinned on the device.

    What each option adds is said at its builder above (`RECORD_BUILDERS`), a product's three parts side by side in a
    `Record`.  A product that is off has no record: nothing of it is called."""
    # 1. resolve the modes and refuse what cannot run -- before the first call on the sampler (product_records)
    pr = product_records(sampler, config, posteriors, log=log, forecast_calendar=forecast_calendar, seed=seed, rt_weight=rt_weight,
                         check_calendar=check_calendar, groups=groups, population=population, verify=verify,
                         location_names=location_names)
    flush, marks, thin, nb, ns = pr.flush, pr.marks, pr.thin, pr.nb, pr.ns

    # 2. warm up
    sampler.set_thin(1)
    first_window_size, last_window_size, slow_window_size, num_slow_windows = 200, 50, 25, 6
    dual_averaging_kwargs = {"target_accept_prob": 0.75}

    def window(n, adapt_mass, running_variance=None):
        sampler.set_adaptation(adapt_step_size=True, adapt_mass=adapt_mass, num_adaptation_steps=n,
                               running_variance=running_variance, **dual_averaging_kwargs)
        tr = flush(sampler.sample(n, **pr.warm_kw))
        return tr, get_weighted_running_variance(unconstrain_theta(tr.theta))

    print(f"Fast window {first_window_size}", file=log, flush=True)
    sampler.set_kernel(step_size=hmc_kernel_kwargs_default()["step_size"])
    tr, running_variance = window(first_window_size, False)
    for k in range(num_slow_windows):
        n = slow_window_size * 2 ** k
        print(f"Slow window {n}", file=log, flush=True)
        tr, running_variance = window(n, True, running_variance)
    print(f"Fast window {last_window_size}", file=log, flush=True)
    tr, _ = window(last_window_size, False)

    # 3. sample
    print("Sampling...", file=log, flush=True)
    step_size = tr.hmc["step_size"][(-last_window_size) // 2:].mean(axis=0)      # inference.py:439-441
    if pool_step_size:
        # build extension (the reference is single-chain): every chain of the job -- all ranks -- samples with
        # the geometric mean of the adapted step sizes; one float64 per chain over RCCL / gloo
        from .. import distributed as D
        step_size = np.full(sampler.B, D.pool_step_sizes(step_size, device=sampler.model.device))
        print(f"Pooled step size over all chains: {step_size[0]:.4g}", file=log, flush=True)
    sampler.set_adaptation(adapt_step_size=False)
    sampler.set_kernel(step_size=step_size, variance=sampler.get_kernel()[1])
    sampler.set_thin(thin)                                  # in force from the first burst's trace reset
    for record in pr.records:
        record.begin()

    def on_burst(tr, i):
        flush(tr, i)
        print(f"  burst {i + 1}/{nb}", file=log, flush=True)
    t0 = time.perf_counter()
    if nb and ns and sampler.cap >= 2 * ns:
        # bursts overlap: while burst k+1 runs, burst k crosses PCIe into page-locked memory and is written
        # to the HDF5 file on a worker thread (ChainSampler.sample_bursts)
        sampler.sample_bursts(nb, ns, on_burst, **pr.burst_kw, **(dict(marks=marks) if marks else {}))
    else:
        for i in range(nb):
            tr = sampler.sample(ns, **pr.burst_kw)
            if i in marks:
                sampler.mark(marks[i])
            on_burst(tr, i)
    dt = time.perf_counter() - t0
    if nb * ns:
        print(f"Sampling: {nb * ns * thin * sampler.B / dt:.1f} sweeps/s, {nb * ns * sampler.B / dt:.1f} kept posterior samples/s "
              f"(thin {thin}, {sampler.B} chain(s), device->host->disk included)", file=log, flush=True)

    # 4. write up
    for record in pr.records:
        record.finish()
    return pr.rows["offset"]


def warmup_size():
    return 200 + 25 * (2 ** 6 - 1) + 50          # inference.py:312-322


def job_layout(num_chains, device=None, env=os.environ):
    """Where this process sits in a multi-GPU job: one process per GPU (torchrun / torch.distributed.run
    sets RANK, WORLD_SIZE, LOCAL_RANK), `num_chains` chains on each.  Read from the environment only --
    nothing here touches the GPU.  Returns dict(rank, world, device, first_chain_id)."""
    rank, world = int(env.get("RANK", "0")), int(env.get("WORLD_SIZE", "1"))
    if not (0 <= rank < world):
        raise ValueError(f"RANK={rank} outside WORLD_SIZE={world}")
    dev = int(env.get("LOCAL_RANK", "0")) if device is None else int(device)
    return dict(rank=rank, world=world, device=dev, first_chain_id=rank * int(num_chains))


def chain_file_name(output_file, chain, total_chains):
    """posterior.hd5 for a single-chain job (the reference); posterior_chain{c}.hd5 with the GLOBAL chain id otherwise."""
    if total_chains == 1:
        return output_file
    root, ext = os.path.splitext(output_file)
    return f"{root}_chain{chain}{ext}"


def dispersed_start(P, chain_ids, scale, seed):
    """Starting points u0[B,P]: the reference's zeros (inference.py:563-573) for global chain 0 and, when
    scale > 0, N(0, scale^2) perturbations for the others, keyed by the GLOBAL chain id so that a chain's
    start does not depend on how the job is sharded (over-dispersed starts for R-hat)."""
    u0 = np.zeros((len(chain_ids), P))
    if scale > 0:
        for b, c in enumerate(chain_ids):
            if c > 0:
                u0[b] = np.random.default_rng([int(seed), 0x5EED, int(c)]).normal(0.0, scale, size=P)
    return u0


def trace_events_dtype(cases, choice="auto"):
    """Width of the event counts in the device-side burst buffer: "u16" halves the buffer and the bytes that cross PCIe
    per draw, but a count above 65535 cannot be held (the read then fails loudly, after the burst has run).  "auto" decides
    from the data before anything runs: the latent S->E / E->I counts of a LAD-day are of the order of its observed
    removals, so 16-bit counts are used while 16 x the largest observed count stays below the limit, int32 otherwise."""
    if choice in ("u16", "int32"):
        return "u16" if choice == "u16" else True
    if choice != "auto":
        raise ValueError(f"events dtype {choice!r}: choose auto, u16 or int32")
    return "u16" if 16.0 * float(np.max(cases, initial=0.0)) < 65535.0 else True


def launch_forms(lay, device_arg, hmc="auto", moves="auto", env=os.environ):
    """The launch forms of the sampler for this process (`ChainSampler(hmc=..., moves=...)`).  "auto": the persistent
    whole-chip launches ("chunk", "paired") when this rank has its GPU to itself, the per-step forms ("chunk-launch",
    "paired-launch") when several ranks of the job were given the SAME device -- an explicit `--device` in a job with more
    than one rank on the node: torchrun hands every rank the same command line -- because two persistent launches cannot
    both be resident on one GPU (include/seir_hip.h, seir_sampler_desc::moves_mode).  Whatever is chosen here, a hand-off
    time-out at run time makes `ChainSampler` fall back by itself."""
    local_world = int(env.get("LOCAL_WORLD_SIZE", lay["world"]))
    shared = lay["world"] > 1 and device_arg is not None and local_world > 1
    return ("chunk-launch" if shared else "chunk") if hmc == "auto" else hmc, \
           ("paired-launch" if shared else "paired") if moves == "auto" else moves


def mcmc(data_file, output_file, config, seed=0, num_chains=1, device=None, pool_step_size=False, init_jitter=0.0,
         events_dtype="auto", hmc="auto", moves="auto", thin=None, summaries=None, diagnostics=None, diagnostics_batch=None,
         forecast=None, forecast_walk=None, rt=None, check=None, forecast_quantiles=None, within_between=None,
         rt_quantiles=None, groups=None, groups_rt=None, groups_within_between=None, groups_ngm=None, scenarios=None, verify=None, *,
         groups_scenarios=None):
    """Constructs and runs the MCMC (covid19uk/inference/inference.py:473-608).

    Multi-GPU: launched as one process per GPU, every rank runs `num_chains` chains with
    global ids rank*num_chains ... (the Philox streams are keyed by the global id, so the draws of chain c
    do not depend on how the job is sharded) and writes its own posterior_chain{c}.hd5; there is no
    data-path collective.  `pool_step_size` adds the one optional exchange: an all_gather of one float64
    per chain after warm-up.  `thin` (every rank is given the same value) and every product keyword override the key of
    their name in `config`; `inference/options.py` says what each accepts and refuses.  `scenarios` (the mapping of a
    `--scenarios FILE.yaml`) likewise takes the place of Mcmc.scenarios."""
    if scenarios is not None:
        config = dict(config, scenarios=scenarios)
    if groups_scenarios is not None:                        # --groups-scenarios: in the place of Mcmc.groups_scenarios
        config = dict(config, groups_scenarios=groups_scenarios)
    if verify is not None:                                  # the path of --verify FILE: in the place of Mcmc.verify
        config = dict(config, verify=verify)
    config, opt = resolve_products(config, thin=thin, summaries=summaries, diagnostics=diagnostics, diagnostics_batch=diagnostics_batch,
                                   forecast=forecast, forecast_walk=forecast_walk, rt=rt, check=check,
                                   forecast_quantiles=forecast_quantiles, within_between=within_between, rt_quantiles=rt_quantiles,
                                   groups=groups, groups_rt=groups_rt, groups_within_between=groups_within_between,
                                   groups_ngm=groups_ngm)          # every option refusal: before the data file is opened
    pending = resolve_scenarios(config, opt.horizon)        # ... the scenarios' too (product_records resolves them again)
    resolve_scenario_groups(config, pending, opt.group_spec)
    truth = None
    if resolve_verify(config, opt.horizon) is not None:     # ... and the truth's: its file is read and held to the fitted one here
        from ..posterior.verify import load_truth
        truth = load_truth(resolve_verify(config, opt.horizon), data_file, opt.horizon, log=sys.stderr)
    lay = job_layout(num_chains, device)                    # before any GPU call
    cov, cases, dates = read_inference_data(data_file)
    rng = np.random.default_rng(seed)                       # same imputation on every rank: one initial state per job
    B = int(num_chains)
    initial_state, events = model_spec.initial_conditions(cases, cov.N, rng)
    M, T = events.shape[0], events.shape[1]
    P = model_spec.num_params(M, T)
    # the table, groups without a source, the windows: refused before any GPU call (no groups: the location coordinate is not opened)
    group_table = opt.bind(cases.shape[0], T, lambda: read_location_names(data_file))
    # ... and the members of a targeted scenario against the same codes (read once, and only when a member is a code or a pattern)
    from ..posterior.scenarios import PendingScenarios
    codes = functools.lru_cache(maxsize=None)(lambda: read_location_names(data_file)) if isinstance(pending, PendingScenarios) else None
    bind_scenarios(pending, cases.shape[0], codes, cov.N)   # ... and a trigger's per-100k thresholds against the populations
    cfg = event_kernel_config(config)
    num_samples = warmup_size() + int(config["num_burst_samples"]) * int(config["num_bursts"])
    cap = max(800, 2 * int(config["num_burst_samples"]))      # two halves: a burst runs while the previous one is written

    if lay["world"] > 1 and pool_step_size:
        import torch
        import torch.distributed as dist
        if not dist.is_initialized():
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            backend = os.environ.get("SEIR_DIST_BACKEND", "nccl")
            if backend == "nccl":
                torch.cuda.set_device(lay["device"])
                dist.init_process_group("nccl", device_id=torch.device("cuda", lay["device"]))
            else:
                dist.init_process_group(backend)
    model = SeirModel(cov, initial_state, max_chains=B, device=lay["device"])
    hmc_form, moves_form = launch_forms(lay, device, hmc, moves)
    if (hmc_form, moves_form) != ("chunk", "paired") and hmc == "auto" and moves == "auto":
        print(f"[rank {lay['rank']}] ranks of this job share device {lay['device']}: launch forms {hmc_form!r}, {moves_form!r} "
              "(one launch per leapfrog step / per pair of event updates)", file=sys.stderr, flush=True)
    sampler = ChainSampler(model, cfg, B, seed=seed, t_range=(max(T - 21, 0), T),
                           num_leapfrog_steps=hmc_kernel_kwargs_default()["num_leapfrog_steps"],
                           trace_capacity=cap, record_events=trace_events_dtype(cases, events_dtype),
                           first_chain_id=lay["first_chain_id"], hmc=hmc_form, moves=moves_form)
    u0 = dispersed_start(P, [lay["first_chain_id"] + c for c in range(B)], float(init_jitter), seed)
    sampler.set_state(u0, np.stack([events] * B))
    print("Initial logpi:", sampler.log_prob(), flush=True)

    total = lay["world"] * B
    names = [chain_file_name(output_file, lay["first_chain_id"] + c, total) for c in range(B)]
    kept = int(config["num_burst_samples"]) * int(config["num_bursts"])
    posteriors = [Posterior(name, M, T, cfg["m"], num_samples, burst=int(config["num_burst_samples"]),
                            **posterior_kwargs(config, opt, group_table, kept))
                  for name in names]
    fc_kw = product_inputs(cov, dates, T, opt, seed, group_table)
    if codes is not None:
        fc_kw["location_names"] = codes
    from ..posterior.scenarios import is_triggered
    if is_triggered(pending):
        fc_kw.setdefault("population", np.asarray(cov.N, dtype=np.float64).reshape(-1))
    if group_table is not None:
        for post in posteriors:
            post.write_groups(group_table, cov.N, initial_state)
    run_mcmc(sampler, config, posteriors, pool_step_size=pool_step_size and total > 1, **fc_kw,
             **({} if truth is None else dict(verify=truth)))
    if sampler.recoveries:
        print(f"{len(sampler.recoveries)} burst(s) were run again after a hand-off time-out (shared GPU?)", flush=True)
    for post in posteriors:
        post.create_dataset("initial_state", initial_state)
        n = max(len(s) for s in dates)
        post.create_dataset("time", np.array(dates, dtype=f"S{n}"))
        print(f"Acceptance theta: {post['results/hmc/is_accepted'].mean()}")
        for key, label in zip(MOVE_KEYS, ("move S->E", "move E->I", "occult S->E", "occult E->I")):
            print(f"Acceptance {label}: {post[f'results/{key}/is_accepted'].mean()}")
        post.close()
    sampler.close()
    model.close()
    if lay["world"] > 1 and pool_step_size:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.barrier()
            dist.destroy_process_group()
    return names


def main(argv=None):
    from argparse import ArgumentParser

    import yaml
    parser = ArgumentParser(description="Run MCMC inference algorithm")
    parser.add_argument("-c", "--config", type=str, help="Config file", required=True)
    parser.add_argument("-o", "--output", type=str, help="Output file", required=True)
    parser.add_argument("data_file", type=str, help="Data NetCDF file")
    parser.add_argument("--seed", type=int, default=0, help="RNG seed (the reference is unseeded)")
    parser.add_argument("--chains", type=int, default=1, help="independent chains on this GPU (per rank under torchrun)")
    parser.add_argument("--device", type=int, default=None, help="HIP device (default: LOCAL_RANK, 0 outside torchrun)")
    parser.add_argument("--pool-step-size", action="store_true",
                        help="sample with the geometric mean of all chains' adapted HMC step sizes (one all_gather)")
    parser.add_argument("--init-jitter", type=float, default=0.0,
                        help="sd of the N(0, sd^2) start of chains 1.. in the unconstrained space (chain 0 starts at 0 as the reference)")
    parser.add_argument("--events-dtype", choices=["auto", "u16", "int32"], default="auto",
                        help="width of the event counts in the device-side burst buffer (auto: 16 bit while 16 x the largest "
                             "observed count fits, else 32)")
    from ..sampler import HMC_MODES, MOVES_MODES
    parser.add_argument("--hmc", choices=["auto"] + sorted(HMC_MODES), default="auto",
                        help="launch form of the HMC update (auto: the persistent whole-trajectory launch, or one launch per "
                             "leapfrog step when ranks share a GPU); what is sampled does not depend on it")
    parser.add_argument("--moves", choices=["auto"] + sorted(MOVES_MODES), default="auto",
                        help="launch form of the event updates (auto: one persistent launch per sweep, or one launch per pair "
                             "of updates when ranks share a GPU)")
    parser.add_argument("--thin", type=int, default=None, metavar="K",
                        help="keep every K-th sweep of the sampling phase, thinned on the device (overrides Mcmc.thin of the "
                             "configuration; the warm-up is never thinned, the shape of the output does not depend on it)")
    add_product_arguments(parser)
    add_scenarios_argument(parser)
    add_verify_argument(parser)
    args = parser.parse_args(argv)
    if args.thin is not None and args.thin < 1:
        parser.error(f"--thin {args.thin}: the thinning interval is >= 1")
    with open(args.config, "r") as f:
        config = yaml.load(f, Loader=yaml.FullLoader)
    always = ("summaries", "diagnostics", "diagnostics_batch", "forecast", "forecast_walk", "rt")   # passed on even when None
    mcmc(args.data_file, args.output, config["Mcmc"], seed=args.seed, num_chains=args.chains, device=args.device,
         pool_step_size=args.pool_step_size, init_jitter=args.init_jitter, events_dtype=args.events_dtype,
         hmc=args.hmc, moves=args.moves, thin=args.thin, **product_overrides(args, always), **scenarios_override(args), **verify_override(args))


if __name__ == "__main__":
    main()

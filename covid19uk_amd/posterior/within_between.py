"""Within-/between-location attributable infection pressure (mirror of
covid19uk/posterior/within_between.py:60-92).  The pressure components run in libseirhip's
k_within_between kernel; this file reduces the sampled events to the last state and
summarises.  Output: a csv with within_mean, between_mean, p_within_gt_between per location.

A run with Mcmc.within_between = D has formed the same product on the device for every kept draw of the sampling phase
(the group within_between/ of every chain's file): `--posterior posterior_chain*.hd5 [--day -1] -o out.csv` pools those
groups over the files and writes the same csv, without a GPU and without samples/seir.
"""
import pickle as pkl

import numpy as np

from .. import model_spec
from ..inference.inference import read_inference_data
from ..seir import SeirModel


def calc_pressure_components(covariates, psi, state_last, device=0, initial_state=None):
    """(within, between) [n,M]; `state_last` [n,M,4] is the state at the last time index."""
    state_last = np.asarray(state_last, dtype=np.float64)
    init = state_last[0] if initial_state is None else initial_state
    W = np.asarray(covariates.W, dtype=np.float64).reshape(-1)
    with SeirModel(covariates, init, max_chains=1, device=device) as model:
        return model.within_between(psi, state_last[..., 2], W[-1])      # t = len(W) clips to len(W)-1


def within_between(input_files, output_file, device=0):
    cov, _, _ = read_inference_data(input_files[0])
    with open(input_files[1], "rb") as f:
        samples = pkl.load(f)
    init_state = np.asarray(samples["initial_state"], dtype=np.float64)
    events = np.asarray(samples["seir"], dtype=np.float64)
    # state at the last time index = init + all increments before it (gemlib compute_state, exclusive cumsum)
    inc = np.einsum("nmtx,xs->nms", events[:, :, :-1, :], model_spec.STOICHIOMETRY)
    state_last = init_state[None] + inc
    within, between = calc_pressure_components(cov, samples["psi"], state_last, device, init_state)
    rows = np.stack([within.mean(0), between.mean(0), (within > between).mean(0)], axis=1)
    write_csv(output_file, rows)
    return within, between


def write_csv(output_file, rows):
    """The reference's csv from rows [M, 3] = within_mean, between_mean, p_within_gt_between: plain decimal numbers that
    read back to the same float64 (the repr of a NumPy scalar is not one)."""
    with open(output_file, "w") as f:
        f.write("location,within_mean,between_mean,p_within_gt_between\n")
        for i, r in enumerate(rows):
            f.write(f"{i},{float(r[0])!r},{float(r[1])!r},{float(r[2])!r}\n")


WB_NAMES = ("days", "first_day", "count", "defined", "within_mean", "between_mean", "p_within_gt_between")


def read_chain_file(path) -> dict:
    """The `within_between/` group of a chain's file (.hd5, or the .npz fallback) as a dict of float64 arrays."""
    if str(path).endswith(".npz"):
        d = np.load(path, allow_pickle=False)
        out = {k: d[f"within_between__{k}"] for k in WB_NAMES if f"within_between__{k}" in d.files}
    else:
        from .. import hdf5io
        with hdf5io.File(path, "r") as f:
            out = {k: f.read(f"/within_between/{k}") for k in WB_NAMES if f.exists(f"/within_between/{k}")}
    missing = [k for k in WB_NAMES if k not in out]
    if missing:
        raise ValueError(f"{path}: no within_between/{missing[0]} -- was the run made with Mcmc.within_between?")
    return out


def pool_posterior(chains: list, day: int = -1) -> np.ndarray:
    """[M, 3] = within_mean, between_mean, p_within_gt_between of window day `day` (an index into [0, D), negative from the
    end: -1 is day T - 1, the reference's product) pooled over `chains` (dicts of `read_chain_file`) with the weights
    `defined`: sum_f defined_f value_f / sum_f defined_f, a file that defines no draw for a location left out; NaN where
    none does."""
    D = int(np.asarray(chains[0]["days"]).reshape(-1)[0])
    for c in chains:
        if int(np.asarray(c["days"]).reshape(-1)[0]) != D or int(np.asarray(c["first_day"]).reshape(-1)[0]) != \
                int(np.asarray(chains[0]["first_day"]).reshape(-1)[0]):
            raise ValueError("the files' within_between/ windows differ")
    if not -D <= int(day) < D:
        raise ValueError(f"--day {day}: the window has {D} day(s), indices {-D} .. {D - 1}")
    w = np.stack([np.asarray(c["defined"], np.float64)[day] for c in chains])                 # [files, M]
    tot = w.sum(axis=0)
    cols = []
    for k in ("within_mean", "between_mean", "p_within_gt_between"):
        v = np.stack([np.asarray(c[k], np.float64)[day] for c in chains])
        num = np.where(w > 0, w * np.where(w > 0, v, 0.0), 0.0).sum(axis=0)
        cols.append(np.where(tot > 0, num / np.where(tot > 0, tot, 1.0), np.nan))
    return np.stack(cols, axis=1)


def within_between_posterior(posterior_files, output_file, day=-1):
    """The reference's csv from the within_between/ groups of `posterior_files`, pooled (`pool_posterior`)."""
    rows = pool_posterior([read_chain_file(name) for name in posterior_files], day)
    write_csv(output_file, rows)
    return rows


def main(argv=None):
    from argparse import ArgumentParser
    parser = ArgumentParser()
    parser.add_argument("-d", "--datafile", type=str, help="Inference-data file")
    parser.add_argument("-s", "--samples", type=str, help="Posterior samples pickle")
    parser.add_argument("--posterior", type=str, nargs="+", metavar="FILE",
                        help="chain files of a run with Mcmc.within_between (posterior_chain*.hd5 or .npz): pool their "
                             "within_between/ groups instead of computing from -d / -s; needs no GPU")
    parser.add_argument("--day", type=int, default=-1,
                        help="with --posterior: the day of the window, as an index into [0, D) (default -1: the last day)")
    parser.add_argument("-o", "--output", type=str, help="Output csv")
    args = parser.parse_args(argv)
    if args.posterior:
        if args.datafile or args.samples:
            parser.error("--posterior stands in for -d / -s: give one or the other")
        if not args.output:
            parser.error("--posterior needs -o")
        return within_between_posterior(args.posterior, args.output, args.day)
    if not args.datafile or not args.samples:
        parser.error("the following arguments are required: -d/--datafile, -s/--samples (or --posterior)")
    within_between([args.datafile, args.samples], args.output)


if __name__ == "__main__":
    main()

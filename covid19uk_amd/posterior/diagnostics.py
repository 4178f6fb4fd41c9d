"""Convergence diagnostics from running accumulators: batch-means effective sample size and split R-hat.

The one place for the host's formulas (include/seir_hip.h, "Convergence diagnostics"; the accumulators' definitions are
covid19uk_amd/csrc/summary_update.h's).  Everything here is NumPy on arrays that are small next to the draws they
describe: the device's exact integer accumulators for the latent epidemic (`ChainSampler.diagnostics()`), or the same
accumulators formed on the host in float64 for the parameter draws (`DrawAccumulator`).  No GPU is needed.

For one chain and one scalar quantity with kept draws x_0 .. x_{n-1}, ref = x_0 and batches of L draws:
    count = n, sum = sum_j (x_j - ref), sumsq = sum_j (x_j - ref)^2                   the moments
    bsum = sum of (x_j - ref) over the open batch, bsumsq = sum_k B_k^2, nbatch = a   the batch sums (closed batches)
    mark w = (count, sum, sumsq) as they stood at some point of the run, w = 0, 1     the marks

  * ESS by batch means: the closed batches' sums B_k have variance L sigma^2_bm when L is long against the autocorrelation
    time, sigma^2_bm being the variance of sqrt(n) x mean; with s^2 the unbiased variance of the draws,
        sigma^2_bm = (bsumsq - (sum - bsum)^2 / a) / ((a - 1) L),     ESS = n s^2 / sigma^2_bm.
    NaN where a < 2 or s^2 = 0 (a cell that never changes: most of the latent tensor).  The relative standard deviation of
    sigma^2_bm is about sqrt(2 / (a - 1)): with a handful of batches the ESS is an order of magnitude, not a figure.
  * Split R-hat (Gelman et al., BDA3 section 11.4) over the half-chains of the chains given: half 0 is the run up to
    mark 0, half 1 the run from mark 1 -- from mark 0 if mark 1 was never taken -- to the end (`run_mcmc` takes them so
    that both are floor(num_bursts / 2) bursts long).  With n draws per half-chain, W the mean of the half-chain variances
    and B / n the variance of the half-chain means,
        R-hat = sqrt(((n - 1) / n W + B / n) / W),        NaN where W = 0.

`python -m covid19uk_amd.posterior.diagnostics posterior_chain*.hd5 -o diagnostics.hd5` pools the `diagnostics/` groups of
any number of chain files -- other ranks' too -- into R-hat over all of them and the summed ESS.
"""
from __future__ import annotations

import dataclasses
import sys

import numpy as np

RHAT_THRESHOLD = 1.05
THETA_HEAD = ("psi", "sigma_space", "beta_area", "gamma0", "gamma1", "alpha_0")


def _per_chain(count, like):
    n = np.asarray(count).astype(np.float64)
    return n.reshape(n.shape + (1,) * (np.ndim(like) - n.ndim))


def _f64(a):
    return np.asarray(a).astype(np.float64)


def mean(count, ref, sum_):
    """ref + sum / n; NaN where n = 0.  `count` broadcasts over the leading axes."""
    n = _per_chain(count, sum_)
    ok = n > 0
    return np.where(ok, _f64(ref) + _f64(sum_) / np.where(ok, n, 1.0), np.nan)


def variance(count, sum_, sumsq):
    """Unbiased variance (sumsq - sum^2 / n) / (n - 1) of the shifted sums; NaN (no warning) where n < 2."""
    n = _per_chain(count, sum_)
    s1, s2 = _f64(sum_), _f64(sumsq)
    ok = n > 1
    nn = np.where(ok, n, 2.0)
    return np.where(ok, (s2 - s1 * s1 / nn) / (nn - 1.0), np.nan)


def batch_means_ess(count, sum_, sumsq, bsum, bsumsq, nbatch, batch_length):
    """ESS = n s^2 / sigma^2_bm per chain and cell; NaN where fewer than two batches are closed or s^2 = 0."""
    s2 = variance(count, sum_, sumsq)
    n, a = _per_chain(count, sum_), _per_chain(nbatch, sum_)
    closed = _f64(np.asarray(sum_) - np.asarray(bsum))              # exact for the integer accumulators
    ok = (a > 1) & (s2 > 0)                                        # NaN compares False
    aa = np.where(a > 1, a, 2.0)
    sig = (_f64(bsumsq) - closed * closed / aa) / ((aa - 1.0) * float(batch_length))
    with np.errstate(divide="ignore", invalid="ignore"):
        ess = n * np.where(ok, s2, 1.0) / sig                      # sigma^2_bm = 0 with s^2 > 0: inf
    return np.where(ok & ~(sig < 0), ess, np.nan)


def half_moments(count, ref, sum_, sumsq, mark_count, mark_sum, mark_sumsq):
    """(half_count [2,B], half_mean [2,B,...], half_var [2,B,...]) from the accumulators at the end and the two marks:
    half 0 is reset .. mark 0, half 1 is mark 1 (mark 0 if mark 1 was not taken) .. end.  Exact differences for integers."""
    count, sum_, sumsq = np.asarray(count), np.asarray(sum_), np.asarray(sumsq)
    mc, ms, mq = np.asarray(mark_count), np.asarray(mark_sum), np.asarray(mark_sumsq)
    late = np.asarray(mc[1] > 0)
    pick = late.reshape(late.shape + (1,) * (sum_.ndim - late.ndim))
    c1, s1, q1 = np.where(late, mc[1], mc[0]), np.where(pick, ms[1], ms[0]), np.where(pick, mq[1], mq[0])
    hc = np.stack([mc[0], count - c1])
    hs, hq = (sum_ - s1), (sumsq - q1)
    hm = np.stack([mean(hc[0], ref, ms[0]), mean(hc[1], ref, hs)])
    hv = np.stack([variance(hc[0], ms[0], mq[0]), variance(hc[1], hs, hq)])
    return hc, hm, hv


def split_rhat(half_count, half_mean, half_var):
    """R-hat over all half-chains given: `half_mean`, `half_var` [2, chains, ...], `half_count` [2, chains] -- the
    half-chains must be equally long.  NaN where the mean within-variance is 0 (or undefined: fewer than 2 draws)."""
    hc = np.asarray(half_count).astype(np.float64).reshape(-1)
    hm, hv = _f64(half_mean), _f64(half_var)
    if hc.size == 0 or (hc != hc[0]).any():
        raise ValueError(f"split R-hat needs half-chains of one length, got {sorted(set(hc.tolist()))} draws")
    n = hc[0]
    hm, hv = hm.reshape((-1,) + hm.shape[2:]), hv.reshape((-1,) + hv.shape[2:])
    k = hm.shape[0]
    if n < 2 or k < 2:
        return np.full(hm.shape[1:], np.nan)
    w = hv.sum(axis=0) / k
    centre = hm.sum(axis=0) / k
    b_over_n = ((hm - centre) ** 2).sum(axis=0) / (k - 1)
    ok = w > 0
    return np.where(ok, np.sqrt(((n - 1.0) / n * w + b_over_n) / np.where(ok, w, 1.0)), np.nan)


@dataclasses.dataclass
class Diagnostics:
    """The accumulators of B chains (leading axis) and the marks; the properties call this module's functions.  For the
    latent epidemic the arrays are the device's integers with trailing axes [M,T,6] (`sampler.SUMMARY_QUANTITIES`), for
    the parameters float64 with trailing axis [P]."""
    batch_length: int
    count: np.ndarray        # [B]
    ref: np.ndarray          # [B,...]
    sum: np.ndarray          # [B,...]
    sumsq: np.ndarray        # [B,...]
    bsum: np.ndarray         # [B,...] the open batch
    bsumsq: np.ndarray       # [B,...]
    nbatch: np.ndarray       # [B] closed batches
    mark_count: np.ndarray   # [2,B]
    mark_sum: np.ndarray     # [2,B,...]
    mark_sumsq: np.ndarray   # [2,B,...]

    @property
    def ess(self) -> np.ndarray:
        return batch_means_ess(self.count, self.sum, self.sumsq, self.bsum, self.bsumsq, self.nbatch, self.batch_length)

    def _halves(self):
        return half_moments(self.count, self.ref, self.sum, self.sumsq, self.mark_count, self.mark_sum, self.mark_sumsq)

    @property
    def half_count(self) -> np.ndarray:
        return self._halves()[0]

    @property
    def half_mean(self) -> np.ndarray:
        return self._halves()[1]

    @property
    def half_var(self) -> np.ndarray:
        return self._halves()[2]

    @property
    def rhat(self) -> np.ndarray:
        hc, hm, hv = self._halves()
        return split_rhat(hc, hm, hv)


class DrawAccumulator:
    """The same accumulators for plain draws on the host, folded as bursts arrive: float64 sums shifted by the first draw,
    the same batches, `mark` where the device's marks are taken.  `fold(x)` takes x [n, B, ...]."""

    def __init__(self, batch_length: int):
        if int(batch_length) < 1:
            raise ValueError(f"batch length {batch_length}: a batch has at least one draw")
        self.L = int(batch_length)
        self.n = 0
        self.ref = None

    def fold(self, x):
        x = np.asarray(x, np.float64)
        if x.shape[0] == 0:
            return
        if self.ref is None:
            self.ref = x[0].copy()
            z = np.zeros_like(self.ref)
            self.sum, self.sumsq, self.bsum, self.bsumsq = z.copy(), z.copy(), z.copy(), z.copy()
            self.marks = [(0, z.copy(), z.copy()), (0, z.copy(), z.copy())]
        d = x - self.ref
        self.sum += d.sum(axis=0)
        self.sumsq += (d * d).sum(axis=0)
        j = 0
        while j < d.shape[0]:
            pos = self.n % self.L
            k = min(self.L - pos, d.shape[0] - j)
            self.bsum += d[j:j + k].sum(axis=0)
            self.n += k
            j += k
            if pos + k == self.L:
                self.bsumsq += self.bsum * self.bsum
                self.bsum[...] = 0.0
        return self

    def mark(self, which: int):
        if which not in (0, 1):
            raise ValueError(f"mark {which}: marks are numbered 0 and 1")
        if self.ref is None:
            raise ValueError("nothing folded yet")
        self.marks[which] = (self.n, self.sum.copy(), self.sumsq.copy())

    def result(self) -> Diagnostics:
        B = self.ref.shape[0]
        full = lambda v: np.full(B, v, np.uint64)                                     # noqa: E731
        return Diagnostics(batch_length=self.L, count=full(self.n), ref=self.ref, sum=self.sum, sumsq=self.sumsq,
                           bsum=self.bsum, bsumsq=self.bsumsq, nbatch=full(self.n // self.L),
                           mark_count=np.stack([full(m[0]) for m in self.marks]),
                           mark_sum=np.stack([m[1] for m in self.marks]), mark_sumsq=np.stack([m[2] for m in self.marks]))


# ---- what goes into a chain's file, and the pooling of such files ---------------------------------------------------------
def theta_names(P, M, T):
    """Names of the P = 6 + (T - 1) + M parameters in the order of the draws (inference.py:541-552)."""
    names = list(THETA_HEAD) + [f"alpha_t[{i}]" for i in range(T - 1)] + [f"spatial_effect[{i}]" for i in range(M)]
    return names[:P] + [f"theta[{i}]" for i in range(len(names), P)]


def evaluate(latent: Diagnostics, theta: Diagnostics) -> dict:
    """Every formula once, for all chains of a process: half moments, ESS and R-hat of the latent epidemic and of the
    parameters (`chain_datasets` slices it per chain, `run_line` words it)."""
    lhc, lhm, lhv = latent._halves()
    thc, thm, thv = theta._halves()
    if not np.array_equal(lhc, thc):
        raise ValueError(f"the parameters' half-chains {thc.tolist()} are not the latent epidemic's {lhc.tolist()}")
    return dict(count=latent.count, batch_length=latent.batch_length, nbatch=latent.nbatch, half_count=lhc,
                latent_half_mean=lhm, latent_half_var=lhv, latent_ess=latent.ess, latent_rhat=split_rhat(lhc, lhm, lhv),
                theta_half_mean=thm, theta_half_var=thv, theta_ess=theta.ess, theta_rhat=split_rhat(thc, thm, thv))


def chain_datasets(ev: dict, chain: int) -> dict:
    """The datasets of the `diagnostics/` group of chain `chain`'s file from `evaluate`'s result.  The *_rhat arrays are
    over all chains evaluated (the chains of one process) and so the same in each of their files."""
    c, con = chain, np.ascontiguousarray
    lhm, lhv, less, lr = ev["latent_half_mean"], ev["latent_half_var"], ev["latent_ess"], ev["latent_rhat"]
    return {
        "count": np.array([float(ev["count"][c])]), "batch_length": np.array([float(ev["batch_length"])]),
        "num_batches": np.array([float(ev["nbatch"][c])]), "half_count": ev["half_count"][:, c].astype(np.float64),
        "seir_half_mean": con(lhm[:, c, ..., :3]), "seir_half_var": con(lhv[:, c, ..., :3]),
        "state_half_mean": con(lhm[:, c, ..., 3:]), "state_half_var": con(lhv[:, c, ..., 3:]),
        "seir_ess": con(less[c, ..., :3]), "state_ess": con(less[c, ..., 3:]),
        "theta_half_mean": con(ev["theta_half_mean"][:, c]), "theta_half_var": con(ev["theta_half_var"][:, c]),
        "theta_ess": con(ev["theta_ess"][c]),
        "seir_rhat": con(lr[..., :3]), "state_rhat": con(lr[..., 3:]), "theta_rhat": ev["theta_rhat"],
    }


def run_line(ev: dict, names=None) -> str:
    """`summary_line` for the chains of one process (ESS summed over them)."""
    return summary_line(ev["theta_rhat"], ev["latent_rhat"], sum_ess(ev["theta_ess"]), sum_ess(ev["latent_ess"]), names)


def sum_ess(ess, axis=0):
    """ESS summed over chains; a chain in which the cell never changed contributes nothing, NaN where none did."""
    ess = _f64(ess)
    some = (~np.isnan(ess)).any(axis=axis)
    return np.where(some, np.nansum(ess, axis=axis), np.nan)


def summary_line(theta_rhat, latent_rhat, theta_ess, latent_ess, names=None) -> str:
    """One line: the largest parameter R-hat and its name, the share of the latent cells that vary with R-hat above
    `RHAT_THRESHOLD`, the smallest ESS of the parameters and of those cells.  `latent_*`: any shape, NaN = constant cell."""
    tr, lr = _f64(theta_rhat).reshape(-1), _f64(latent_rhat).reshape(-1)
    te, le = _f64(theta_ess).reshape(-1), _f64(latent_ess).reshape(-1)
    parts = []
    if np.isfinite(tr).any():
        i = int(np.nanargmax(np.where(np.isfinite(tr), tr, -np.inf)))
        name = names[i] if names is not None and i < len(names) else f"theta[{i}]"
        parts.append(f"largest theta R-hat {tr[i]:.3f} ({name})")
    else:
        parts.append("theta R-hat undefined")
    live = ~np.isnan(lr)
    if live.any():
        parts.append(f"{100.0 * float((lr[live] > RHAT_THRESHOLD).mean()):.1f}% of {int(live.sum())} non-constant latent cells "
                     f"with R-hat > {RHAT_THRESHOLD}")
    else:
        parts.append("no non-constant latent cell")
    fmt = lambda v: f"{np.nanmin(v):.1f}" if (~np.isnan(v)).any() else "undefined"   # noqa: E731
    parts.append(f"smallest ESS theta {fmt(te)}, latent {fmt(le)}")
    return "diagnostics: " + "; ".join(parts)


NAMES = ("count", "batch_length", "num_batches", "half_count", "seir_half_mean", "seir_half_var", "state_half_mean",
         "state_half_var", "seir_ess", "state_ess", "theta_half_mean", "theta_half_var", "theta_ess", "seir_rhat",
         "state_rhat", "theta_rhat")


def read_chain_file(path) -> dict:
    """The `diagnostics/` group of a chain's file (.hd5, or the .npz fallback) as a dict of float64 arrays."""
    if str(path).endswith(".npz"):
        d = np.load(path, allow_pickle=False)
        out = {k: d[f"diagnostics__{k}"] for k in NAMES if f"diagnostics__{k}" in d.files}
    else:
        from .. import hdf5io
        with hdf5io.File(path, "r") as f:
            out = {k: f.read(f"/diagnostics/{k}") for k in NAMES if f.exists(f"/diagnostics/{k}")}
    missing = [k for k in NAMES if k not in out]
    if missing:
        raise ValueError(f"{path}: no diagnostics/{missing[0]} -- was the run made with diagnostics on?")
    return out


def pool(chains: list) -> dict:
    """R-hat over the half-chains of all `chains` (dicts of `read_chain_file`) and their summed ESS, from the stored half
    means, variances and counts alone."""
    hc = np.stack([np.asarray(c["half_count"]).reshape(2) for c in chains], axis=1)           # [2, chains]
    out = {"num_chains": np.array([float(len(chains))]), "half_count": hc[:, 0].astype(np.float64)}
    for k in ("seir", "state", "theta"):
        hm = np.stack([c[f"{k}_half_mean"] for c in chains], axis=1)
        hv = np.stack([c[f"{k}_half_var"] for c in chains], axis=1)
        out[f"{k}_rhat"] = split_rhat(hc, hm, hv)
        out[f"{k}_ess"] = sum_ess(np.stack([c[f"{k}_ess"] for c in chains]))
    return out


def pooled_line(p: dict) -> str:
    M, T = p["seir_rhat"].shape[:2]
    return summary_line(p["theta_rhat"], np.stack([p["seir_rhat"], p["state_rhat"]]), p["theta_ess"],
                        np.stack([p["seir_ess"], p["state_ess"]]), theta_names(p["theta_rhat"].shape[0], M, T))


def write_pooled(path, p: dict):
    if str(path).endswith(".npz"):
        np.savez(path, **p)
        return
    from .. import hdf5io
    with hdf5io.File(path, "w") as f:
        for k, v in p.items():
            v = np.ascontiguousarray(v, np.float64)
            f.create_dataset("/" + k, v.shape, np.float64)
            f.write("/" + k, v)


def main(argv=None):
    import argparse
    parser = argparse.ArgumentParser(description="Pool the diagnostics/ groups of chain files: R-hat over all chains, summed ESS")
    parser.add_argument("chains", nargs="+", help="chain files of runs with diagnostics on (posterior_chain*.hd5 or .npz)")
    parser.add_argument("-o", "--output", required=True, help="output file (.hd5 or .npz)")
    args = parser.parse_args(argv)
    p = pool([read_chain_file(name) for name in args.chains])
    write_pooled(args.output, p)
    print(f"{len(args.chains)} chain(s): " + pooled_line(p), file=sys.stdout, flush=True)
    return p


if __name__ == "__main__":
    main()

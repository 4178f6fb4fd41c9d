"""Scoring the forecast against later data: THE definitions in NumPy (include/seir_hip.h, "Scoring the forecast against
later data"; csrc/verify_update.h, csrc/verify_kernels.h).

Targets, per location m and forecast day s -- planes 0 and 1 of the forecast's draw store:
    cases       the I->R count of the day
    cum_cases   its running total over the horizon
Prevalence is not observed and is not scored.

Truth is `truth[M, H]` int32 with -1 for missing: `cases[:, T:T+H]` of a later input file whose first T dates are the fitted
file's.  Days the file does not reach, NaN and negative cells are missing; `cum_cases` of (m, s) is valid only while every
day <= s of location m is.

Per chain, cell and target over the forecast draws x_1..x_n (integers only, independent of the draws' order):
    lt = #{x_i < y}    eq = #{x_i == y}    abs_sum = sum |x_i - y|    pair_sum D = sum_{i<j} |x_i - x_j|
and from them
    PIT  (lt + eq/2) / n            the mid-p value of the truth under the sample
    MAE  abs_sum / n
    CRPS abs_sum / n - D / n^2      the energy form E|X - y| - E|X - X'|/2 of the EMPIRICAL distribution of the sample:
                                    both expectations over the n draws with replacement, so the denominators are n and
                                    n^2 -- not the "fair" estimator, which divides D by n (n - 1) / 2 twice over.
lt, eq and abs_sum pool over chains and files by a sum; D does not: the pooled D is D of the union of the draws.  A cell
without truth has four zeros and NaN scores, without a warning.
"""
import dataclasses

import numpy as np

TARGETS = ("cases", "cum_cases")
MISSING = -1


def pair_sum(x):
    """D = sum_{i<j} |x_i - x_j| over the LAST axis of integer `x`, in int64: with the values sorted, value k is the larger
    one of k pairs and the smaller one of n - 1 - k."""
    xs = np.sort(np.asarray(x).astype(np.int64), axis=-1)
    n = xs.shape[-1]
    return ((2 * np.arange(n, dtype=np.int64) - n + 1) * xs).sum(axis=-1)


def targets(events):
    """The two scored planes of simulated counts `events` [..., M, H, 3] (se, ei, ir): int64 [..., M, H, 2]."""
    ir = np.asarray(events)[..., 2].astype(np.int64)
    return np.stack([ir, np.cumsum(ir, axis=-1)], axis=-1)


def truth_targets(truth):
    """`truth` [M, H] (negative: missing) as (y [M, H, 2] int64, valid [M, H, 2] bool): the day's count and its running
    total, the latter valid up to a row's first missing day.  y is -1 where not valid."""
    t = np.asarray(truth).astype(np.int64)
    ok = t >= 0
    ok_cum = np.logical_and.accumulate(ok, axis=-1)
    cum = np.cumsum(np.where(ok_cum, t, 0), axis=-1)
    valid = np.stack([ok, ok_cum], axis=-1)
    return np.where(valid, np.stack([t, cum], axis=-1), MISSING), valid


def fold(draws, y, valid):
    """`draws` int [n, ..., 2] against y, valid [..., 2]: dict of lt, eq (uint32) and abs_sum (uint64), zeros where not valid."""
    x = np.asarray(draws).astype(np.int64)
    yy = np.asarray(y).astype(np.int64)
    lt = ((x < yy) & valid).sum(axis=0).astype(np.uint32)
    eq = ((x == yy) & valid).sum(axis=0).astype(np.uint32)
    ab = np.where(valid, np.abs(x - yy), 0).sum(axis=0).astype(np.uint64)
    return dict(lt=lt, eq=eq, abs_sum=ab)


def scores(n, lt, eq, abs_sum, valid, pair=None):
    """PIT, MAE and -- given `pair`, the pair sums of the same draws -- CRPS from the integers of n draws per cell; NaN where
    not valid or n == 0, without a warning.  Every array is broadcast against `valid`."""
    valid = np.asarray(valid, bool) & (n > 0)
    d = float(n) if n > 0 else 1.0
    nan = np.full(np.shape(valid), np.nan)
    out = dict(pit=np.where(valid, (np.asarray(lt, np.float64) + 0.5 * np.asarray(eq, np.float64)) / d, nan),
               mae=np.where(valid, np.asarray(abs_sum, np.float64) / d, nan))
    if pair is not None:
        out["crps"] = np.where(valid, np.asarray(abs_sum, np.float64) / d - np.asarray(pair, np.float64) / (d * d), nan)
    return out


def score_draws(draws, y, valid):
    """`fold`, `pair_sum` and `scores` of `draws` [n, ..., 2] in one: what the host forms for the national and group curves."""
    x = np.asarray(draws).astype(np.int64)
    f = fold(x, y, valid)
    pair = np.where(valid, pair_sum(np.moveaxis(x, 0, -1)), 0) if x.shape[0] else np.zeros(np.shape(valid), np.int64)
    return dict(f, pair_sum=pair, **scores(x.shape[0], f["lt"], f["eq"], f["abs_sum"], valid, pair))


def interval_pairs(probs):
    """The central intervals that `probs` contain: [(i_lo, i_hi, p)] for every p < 1/2 whose 1 - p is there too."""
    probs = [float(p) for p in probs]
    out = []
    for i, p in enumerate(probs):
        if p < 0.5:
            for j, q in enumerate(probs):
                if abs(q - (1.0 - p)) <= 1e-12:
                    out.append((i, j, p))
                    break
    return out


def coverage(q_lo, q_hi, y, valid):
    """The share of valid cells with q_lo <= y <= q_hi, over the location axis: arrays [..., M, H, 2] -> [..., H, 2]; NaN for a
    day and target without a valid cell."""
    valid = np.broadcast_to(np.asarray(valid, bool), np.shape(q_lo))
    hit = (np.asarray(q_lo) <= y) & (y <= np.asarray(q_hi)) & valid
    cnt = valid.sum(axis=-3)
    return np.where(cnt > 0, hit.sum(axis=-3) / np.maximum(cnt, 1), np.nan)


@dataclasses.dataclass(frozen=True)
class Truth:
    """What `extract_truth` found: truth [M, H] int32, the number of cells of the first T days that differ from the fitted
    file's (data get revised), and where it came from."""
    truth: np.ndarray
    revised: int = 0
    path: str = ""

    def __bool__(self):
        return True


def extract_truth(fitted_cases, fitted_dates, later_cases, later_dates, horizon):
    """truth [M, H] int32 from the cases [M, T'] of a later file: columns T .. T + H, -1 where the file does not reach, is
    NaN or negative.  Refuses (ValueError) another M, dates that do not line up, a non-integer value, and no valid cell at
    all; counts the revised cells of the first T days and does not refuse them.  Returns (truth, revised)."""
    fc, lc = np.asarray(fitted_cases, np.float64), np.asarray(later_cases, np.float64)
    M, T = fc.shape
    H = int(horizon)
    if lc.ndim != 2 or lc.shape[0] != M:
        raise ValueError(f"verify: the later file has cases {lc.shape}, the fitted file {M} locations")
    if lc.shape[1] < T or [str(d) for d in later_dates[:T]] != [str(d) for d in fitted_dates]:
        raise ValueError(f"verify: the first {T} dates of the later file ({lc.shape[1]} days) are not the fitted file's "
                         f"({fitted_dates[0]} .. {fitted_dates[-1]})")
    part = lc[:, T:T + H]
    seen = np.isfinite(part)
    if np.any(seen & (part != np.round(np.where(seen, part, 0.0)))):
        raise ValueError("verify: the later file's cases are not integers")
    if np.any(seen & (part >= 2.0 ** 31)):
        raise ValueError("verify: the later file's cases do not fit int32")
    truth = np.full((M, H), MISSING, np.int32)
    ok = seen & (part >= 0)
    truth[:, :part.shape[1]][ok] = part[ok].astype(np.int32)
    if not (truth >= 0).any():
        raise ValueError(f"verify: the later file has no valid cell in the {H} days behind {fitted_dates[-1]}")
    a, b = fc, lc[:, :T]
    revised = int(np.sum(~((a == b) | (np.isnan(a) & np.isnan(b)))))
    return truth, revised


def parse_verify(value, horizon):
    """Mcmc.verify (absent or empty: off) against the forecast's horizon: the path, or None.  Refuses what is no path and
    `verify` without `forecast`."""
    if value is None or value is False or value == "":
        return None
    if not isinstance(value, (str, bytes)) and not hasattr(value, "__fspath__"):
        raise ValueError(f"verify: {value!r} -- the path of a later input file (.nc / .hd5 / .npz)")
    if not horizon:
        raise ValueError("verify: scoring needs a forecast (set Mcmc.forecast / --forecast H)")
    return str(value if not hasattr(value, "__fspath__") else value.__fspath__())


def load_truth(path, data_file, horizon, log=None):
    """`extract_truth` of the input file `path` against the fitted `data_file`, both as `read_inference_data` reads them.
    Logs the revised cells."""
    from ..inference.inference import read_inference_data
    _, fc, fd = read_inference_data(data_file)
    _, lc, ld = read_inference_data(path)
    truth, revised = extract_truth(fc, fd, lc, ld, horizon)
    if log is not None:
        n_ok = int((truth >= 0).sum())
        print(f"Verify: {path}: {n_ok} of {truth.size} cell(s) of the {horizon} forecast day(s) observed; {revised} cell(s) of "
              f"the {fc.shape[1]} fitted day(s) differ from the fitted file (revised data: not refused)", file=log, flush=True)
    return Truth(truth=truth, revised=revised, path=str(path))


def pool(parts):
    """lt, eq, abs_sum and count of several chains or files pooled: a sum (pair_sum is NOT pooled this way)."""
    out = {k: sum(np.asarray(p[k]).astype(np.int64 if k != "abs_sum" else np.uint64) for p in parts) for k in ("lt", "eq", "abs_sum")}
    out["count"] = int(sum(int(p["count"]) for p in parts))
    return out


def run_line(truth, national_draws, pit, crps, valid):
    """The run's one log line: the last valid day, the national cumulative truth against the forecast's median and 0.05 /
    0.95, the mean CRPS over valid cells (`crps` None: no draw store), and the share of cells with mid-p in [0.05, 0.95]."""
    t = np.asarray(truth)
    all_ok = np.logical_and.accumulate((t >= 0).all(axis=0))
    text = "Verify:"
    if all_ok.any():
        last = int(np.nonzero(all_ok)[0][-1])
        y = int(t[:, :last + 1].sum())
        cum = np.cumsum(np.asarray(national_draws)[..., 2].reshape(-1, t.shape[1]), axis=1)[:, last]
        q = np.quantile(cum, [0.05, 0.5, 0.95]) if cum.size else [np.nan] * 3
        text += (f" national cumulative cases to forecast day {last + 1}: observed {y}, forecast median {q[1]:.0f} "
                 f"[{q[0]:.0f}, {q[2]:.0f}];")
    else:
        text += " no forecast day is observed in every location;"
    if crps is None:
        text += " no draw store: set forecast_quantiles for CRPS;"
    else:
        c = np.asarray(crps)[np.broadcast_to(valid, np.shape(crps))]
        text += f" mean CRPS over {c.size} valid cell(s) {np.mean(c) if c.size else np.nan:.4g};"
    p = np.asarray(pit)[np.broadcast_to(valid, np.shape(pit))]
    share = np.mean((p >= 0.05) & (p <= 0.95)) if p.size else np.nan
    return text + f" mid-p within [0.05, 0.95] in {100 * share:.1f} % of them"

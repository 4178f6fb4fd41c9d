"""Quantiles from exact order statistics: the one definition of the rank rule behind `Mcmc: forecast_quantiles` and
`Mcmc: rt_quantiles`.

The device selects order statistics (include/seir_hip.h, "Forecast intervals on the device"); which ones to ask for, and how
two of them become a quantile, is decided here and nowhere else.  For a probability p and n draws

    h = p (n - 1),   lo = floor(h),   hi = ceil(h),   quantile = x[lo] + (h - lo) (x[hi] - x[lo]),

x being the sorted draws: NumPy's default ("linear") method, with h the fp64 product NumPy forms.  Where h is an integer
the quantile is the order statistic itself."""
import math

import numpy as np

MAX_PROBS = 8                     # two ranks each: SEIR_ORDER_STATS_MAX_RANKS = 16


def parse_probs(value, name="forecast_quantiles"):
    """`Mcmc.forecast_quantiles` / `--forecast-quantiles` (or the key `name`): a list of numbers or a comma-separated string
    -> a tuple of 1 to MAX_PROBS probabilities in [0, 1], strictly increasing.  None, False and "off" -> ().  ValueError
    otherwise."""
    if value is None or value is False or (isinstance(value, str) and value.strip().lower() == "off"):
        return ()
    what = f"{name}={value!r}"
    if isinstance(value, str):
        value = [v for v in value.split(",")]
    elif isinstance(value, (int, float, np.integer, np.floating)) and not isinstance(value, bool):
        value = [value]
    if isinstance(value, bool) or not isinstance(value, (list, tuple, np.ndarray)):
        raise ValueError(f"{what}: a list of probabilities, e.g. [0.05, 0.5, 0.95]")
    probs = []
    for v in value:
        if isinstance(v, (bool, np.bool_)):
            raise ValueError(f"{what}: {v!r} is not a number")
        try:
            p = float(v.strip()) if isinstance(v, str) else float(v)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: {v!r} is not a number") from None
        if not 0.0 <= p <= 1.0:                               # a NaN fails this too
            raise ValueError(f"{what}: {v!r} is not a probability in [0, 1]")
        probs.append(p)
    if not probs:
        raise ValueError(f"{what}: the list is empty")
    if len(probs) > MAX_PROBS:
        raise ValueError(f"{what}: at most {MAX_PROBS} probabilities")
    if any(b <= a for a, b in zip(probs, probs[1:])):
        raise ValueError(f"{what}: the probabilities must be strictly increasing")
    return tuple(probs)


def _lo_hi(n, p):
    h = float(p) * (int(n) - 1)
    return h, int(math.floor(h)), int(math.ceil(h))


def quantile_ranks(n, probs):
    """The order statistics that the quantiles `probs` of n draws are made of: sorted, without repeats, int64."""
    n = int(n)
    if n < 1:
        raise ValueError(f"n={n}: a quantile needs at least one draw")
    ranks = set()
    for p in probs:
        if not 0.0 <= float(p) <= 1.0:
            raise ValueError(f"probability {p!r} outside [0, 1]")
        _, lo, hi = _lo_hi(n, p)
        ranks.update((lo, hi))
    return np.array(sorted(ranks), dtype=np.int64)


def interpolate(stats, ranks, n, probs):
    """stats [R, ...]: the order statistics `ranks` (as `quantile_ranks(n, probs)` gives them) -> float64 [K, ...], the
    quantiles `probs`, formed as NumPy forms them: from the lower value below weight 0.5, from the upper one above."""
    stats = np.asarray(stats)
    where = {int(r): i for i, r in enumerate(np.asarray(ranks).reshape(-1))}
    out = np.empty((len(probs),) + stats.shape[1:], np.float64)
    for k, p in enumerate(probs):
        h, lo, hi = _lo_hi(n, p)
        a = stats[where[lo]].astype(np.float64)
        if hi == lo:
            out[k] = a
            continue
        b = stats[where[hi]].astype(np.float64)
        t = h - lo
        out[k] = a + (b - a) * t if t < 0.5 else b - (b - a) * (1.0 - t)
    return out

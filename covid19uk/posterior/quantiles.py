"""The rank rule of the forecast quantiles (the reference has no such module)."""
from covid19uk_amd.posterior.quantiles import *  # noqa: F401,F403
from covid19uk_amd.posterior.quantiles import MAX_PROBS, interpolate, parse_probs, quantile_ranks  # noqa: F401

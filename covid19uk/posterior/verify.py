"""Scoring the forecast against later data: PIT, MAE, CRPS (the reference has no such module)."""
from covid19uk_amd.posterior.verify import *  # noqa: F401,F403
from covid19uk_amd.posterior.verify import (TARGETS, coverage, extract_truth, fold, interval_pairs, load_truth, pair_sum,  # noqa: F401
                                            parse_verify, pool, score_draws, scores, targets, truth_targets)

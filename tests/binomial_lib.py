"""What tests/test_binomial_host.py and tests/test_binomial_gpu.py share: the grid of (n, p) at which the simulator's binomial
sampler is held to the exact law, the C twin's draws at every point (computed once per session) and the statistics.

The protocol is `SeirModel.selftest_binomial`'s: draw id 0, cell = element index, stream RS_SIM_BASE, so the twin's draw i is
the device's draw i."""
import functools

import numpy as np
from scipy import stats

from oracle import c_binding
from oracle import sim_oracle as sim

N_DRAWS = 1 << 20
SEED = 11          # the algorithm alone gave chi-square p >= 0.075 and |z| <= 1.51 over GRID at this seed; another seed
                   # must be re-checked the same way before it is committed
N31 = 2 ** 31 - 1
BINV, BTRS = "binv", "btrs"

# id -> (n, p, branch): each id names the branch the point turns
GRID = {
    # small n, inversion
    "binv,n=1": (1, .25, BINV),
    "binv,n=3,p=half": (3, .5, BINV),
    "binv,n=9,flip": (9, .999, BINV),
    "binv,n=40,flip": (40, .9, BINV),
    "binv,n=50": (50, .1, BINV),
    # the 200-step cap of the inversion: xmax = n below it, 200 above
    "binv,cap,n=199": (199, .05, BINV),
    "binv,cap,n=201": (201, .0497, BINV),
    "binv,n=1000": (1000, .004, BINV),
    # the BINV/BTRS switch at n min(p, q) = 10, and its mirror image
    "switch,below": (1000, .0099999, BINV),
    "switch,at": (1000, .01, BTRS),
    "switch,above": (1000, .0100001, BTRS),
    "switch,flip,at": (1000, .99, BTRS),
    "switch,flip,below": (1000, .9900001, BINV),
    # BTRS at moderate n
    "btrs,n=1000": (1000, .3, BTRS),
    "btrs,n=5000,flip": (5000, .7, BTRS),
    "btrs,n=1e5": (100000, .0005, BTRS),
    "btrs,n=2.5e5": (250000, 4.1e-5, BTRS),
    # either side of p = 1/2
    "btrs,half,below": (1000, .4999, BTRS),
    "btrs,half,at": (1000, .5, BTRS),
    "btrs,half,above,flip": (1000, .5000001, BTRS),
    # the smallest n that reaches BTRS
    "btrs,n=20": (20, .5, BTRS),
    "btrs,n=21": (21, .5, BTRS),
    # UK-sized populations (.2212 ~ 1 - exp(-1/4))
    "uk,n=1.2e5": (120000, .2212, BTRS),
    "uk,n=1.1e6": (1100000, .2212, BTRS),
    "uk,n=1.1e6,p=1e-6": (1100000, 1e-6, BINV),
    "uk,n=1.1e6,switch,below": (1100000, 9.0e-6, BINV),
    "uk,n=1.1e6,switch,above": (1100000, 9.2e-6, BTRS),
    "uk,n=1.1e6,p=.03": (1100000, .03, BTRS),
    "uk,n=1.1e6,p=half": (1100000, .5, BTRS),
    "uk,n=9e6": (9000000, .1, BTRS),
    # the int32 limit
    "int32,p=1e-9": (N31, 1e-9, BINV),
    "int32,switch,below": (N31, 4.6e-9, BINV),
    "int32,switch,above": (N31, 4.7e-9, BTRS),
    "int32,p=1e-6": (N31, 1e-6, BTRS),
    "int32,p=.01": (N31, .01, BTRS),
    "int32,p=half": (N31, .5, BTRS),
    "int32,p=.7,flip": (N31, .7, BTRS),
}


@functools.lru_cache(maxsize=None)
def twin(point):
    """(variate, branch, near_tie, attempts) of the C twin for N_DRAWS draws at GRID[point].  Shared: do not modify."""
    n, p, _ = GRID[point]
    out = c_binding.sim_binomial(n, p, 0, np.arange(N_DRAWS), sim.RS_SIM_BASE, SEED)
    for a in out:
        a.setflags(write=False)
    return out


def law_statistics(x, n, p):
    """x: draws claimed to be Binomial(n, p).  Returns (chi-square p-value, number of bins, z of the mean, z of the variance).

    Chi-square: at most 256 bins of equal width from the 1e-6 to the 1 - 1e-6 quantile plus the two tails, neighbours merged
    until each expects at least 20 draws; the expected counts are scipy.stats.binom's.  Mean: z against n p with variance
    n p q / N.  Variance: the mean square about the KNOWN mean, z against n p q with variance (mu4 - (n p q)^2) / N,
    mu4 = n p q (1 + 3 (n - 2) p q)."""
    x = np.asarray(x, dtype=np.int64)
    N = x.size
    q = 1.0 - p
    lo, hi = int(stats.binom.ppf(1e-6, n, p)), int(stats.binom.ppf(1 - 1e-6, n, p))
    width = -(-(hi - lo + 1) // 256)
    edges = np.arange(lo, hi + width + 1, width)                 # bin j holds edges[j] <= x < edges[j+1]
    cdf = np.concatenate([[0.0], stats.binom.cdf(edges - 1, n, p), [1.0]])
    expected = np.diff(cdf) * N
    idx = np.searchsorted(edges, x, side="right")                # 0: below lo, len(edges): beyond the last edge
    observed = np.bincount(idx, minlength=expected.size)
    assert observed.size == expected.size
    E, O, e_acc, o_acc = [], [], 0.0, 0
    for e, o in zip(expected, observed):
        e_acc += e
        o_acc += o
        if e_acc >= 20:
            E.append(e_acc); O.append(o_acc); e_acc, o_acc = 0.0, 0
    E[-1] += e_acc; O[-1] += o_acc
    E, O = np.array(E), np.array(O)
    assert len(E) >= 2 and O.sum() == N and abs(E.sum() - N) < 1e-6 * N
    chi_p = float(stats.chi2.sf(np.sum((O - E) ** 2 / E), len(E) - 1))
    mu, var = n * p, n * p * q
    d = x - mu
    z_mean = float(d.mean() / np.sqrt(var / N))
    mu4 = var * (1.0 + 3.0 * (n - 2) * p * q)
    z_var = float((np.mean(d * d) - var) / np.sqrt((mu4 - var * var) / N))
    return chi_p, len(E), z_mean, z_var


def assert_law(x, n, p, what):
    chi_p, bins, z_mean, z_var = law_statistics(x, n, p)
    print(f"{what}: n={n} p={p!r} chi-square p={chi_p:.4g} ({bins} bins) z_mean={z_mean:+.3f} z_var={z_var:+.3f}")
    assert x.min() >= 0 and x.max() <= n
    assert chi_p > 1e-4, (what, n, p, chi_p, bins)               # the threshold of tests/test_simulate.py
    assert abs(z_mean) < 5, (what, n, p, z_mean)                 # that file's 5 sigma
    assert abs(z_var) < 5, (what, n, p, z_var)
    return chi_p, z_mean, z_var

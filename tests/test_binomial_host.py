"""The simulator's binomial algorithm against the exact law, on the host: oracle/sim_oracle.c (the C twin of
oracle/sim_oracle.py's `binomial`) draws 2^20 variates at every point of tests/binomial_lib.GRID -- the branch switches, the
inversion cap, p next to 1/2, UK-sized populations and the int32 limit -- and scipy.stats.binom judges them.  The device is
held to the twin draw for draw in tests/test_binomial_gpu.py.

Not constructed here: the re-draw of BINV after its 200-step cap.  It needs a uniform beyond the first 201 terms of a law
whose mean is below 10, a tail of less than 1e-100: no seed reaches it."""
import numpy as np
import pytest

from oracle import c_binding
from oracle import mcmc_oracle as mo
from oracle import sim_oracle as sim
from tests import binomial_lib as BL


@pytest.mark.parametrize("point", list(BL.GRID))
def test_twin_equals_python_oracle(point):
    """40 draws per point, by equality (the Python oracle's lgamma is CPython's own, the twin's is libm's: they agree to
    rounding, and none of these draws is decided by that)."""
    n, p, _ = BL.GRID[point]
    got = BL.twin(point)[0][:40]
    want = [sim.binomial(n, p, lambda att, i=i: tuple(float(x[0]) for x in mo.rng_uniform2(BL.SEED, 0, i, sim.RS_SIM_BASE, att)))
            for i in range(40)]
    assert np.array_equal(got, want)


def test_twin_edges_and_substreams():
    x, branch, tie, att = c_binding.sim_binomial([0, -3, 10, 10, 10, 10, 10], [.5, .5, 0.0, -1.0, float("nan"), 1.0, 1.5],
                                                 0, 0, sim.RS_SIM_BASE, 1)
    assert x.tolist() == [0, 0, 0, 0, 0, 10, 10]
    assert np.all(branch == c_binding.SIM_TRIVIAL) and not tie.any() and not att.any()
    # every counter word and the seed select another substream
    base = c_binding.sim_binomial(1000, .3, 0, np.arange(64), sim.RS_SIM_BASE, 5)[0]
    assert np.array_equal(base, c_binding.sim_binomial(1000, .3, 0, np.arange(64), sim.RS_SIM_BASE, 5)[0])
    for other in (c_binding.sim_binomial(1000, .3, 1, np.arange(64), sim.RS_SIM_BASE, 5),
                  c_binding.sim_binomial(1000, .3, 0, np.arange(64) + 64, sim.RS_SIM_BASE, 5),
                  c_binding.sim_binomial(1000, .3, 0, np.arange(64), sim.RS_SIM_BASE + 1, 5),
                  c_binding.sim_binomial(1000, .3, 0, np.arange(64), sim.RS_SIM_BASE, 5 + 2 ** 32)):
        assert not np.array_equal(base, other[0])


@pytest.mark.parametrize("point", list(BL.GRID))
def test_twin_follows_the_exact_law(point):
    n, p, kind = BL.GRID[point]
    x, branch, tie, att = BL.twin(point)
    counts = np.bincount(branch, minlength=5)
    print(f"{point}: branches {dict(zip(c_binding.SIM_BRANCHES, counts.tolist()))} near-ties {int(tie.sum())} "
          f"max attempts {int(att.max())}")
    assert counts[c_binding.SIM_FALLBACK] == 0 and counts[c_binding.SIM_TRIVIAL] == 0
    assert (n * min(p, 1.0 - p) < sim.BINV_MAX_MEAN) == (kind == BL.BINV)        # the point lies on the side its id says
    if kind == BL.BINV:
        assert counts[c_binding.SIM_BINV] == BL.N_DRAWS
        assert att.max() == 1                                                    # the cap's re-draw: see the module docstring
        assert not tie.any()
    else:
        assert counts[c_binding.SIM_BINV] == 0
        assert counts[c_binding.SIM_BTRS_SQUEEZE] >= 10 ** 5 and counts[c_binding.SIM_BTRS_FULL] >= 10 ** 5
        assert att.max() > 1                                                     # rejections happen
    BL.assert_law(x, n, p, "twin " + point)

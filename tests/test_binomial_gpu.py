"""The device's binomial sampler (csrc/sim_kernels.h: sim_binomial) against its C twin (oracle/sim_oracle.c) draw for draw at
production sizes, through `SeirModel.selftest_binomial` (draw id 0, cell = element index, stream RS_SIM_BASE) and through the
two kernels that call it at UK size (k_simulate, k_forecast_day).

The twin is held to the exact law in tests/test_binomial_host.py.  The device forms log(k!) by Stirling's series and contracts
products into FMAs, the twin uses lgamma and rounds every product: a draw may differ where the twin marks a near-tie
(oracle/sim_oracle.c) and nowhere else, and the marked share is itself bounded.  The device's own draws, exempt ones
included, are judged against the exact law as well."""
import numpy as np
import pytest

from oracle import c_binding
from oracle import seir_oracle as so
from oracle import sim_oracle as sim
from tests import binomial_lib as BL
from tests import helpers as H
from tests.test_sampler_gpu import api  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

MAX_TIE_SHARE = 2e-3               # of a launch's draws
MAX_TIE_SHARE_SMALL_N = 1e-5       # for n <= 2^22, where lfact(m) + lfact(n-m) is small against fp64's spacing of 1
DIVERGENT_SEED = 12


@pytest.fixture(scope="module")
def model(api):  # noqa: F811
    case = H.build_case("micro_3x5", 1)
    with api[0](case["cov"], case["init"], max_chains=1) as m:
        yield m


def _same_but_for_near_ties(got, want, tie, what):
    """Equality on every draw the twin does not mark; returns (marked share, mismatches among the marked)."""
    differ = got != want
    share = float(tie.mean())
    print(f"{what}: near-tie share {share:.3g} ({int(tie.sum())} draws), exempt mismatches {int((differ & tie).sum())}, "
          f"other mismatches {int((differ & ~tie).sum())}")
    bad = np.flatnonzero(differ & ~tie)
    assert bad.size == 0, (what, bad[:10], got[bad[:10]], want[bad[:10]])
    assert share <= MAX_TIE_SHARE, (what, share)
    return share, int((differ & tie).sum())


@pytest.mark.parametrize("point", list(BL.GRID))
def test_device_equals_twin_and_follows_the_exact_law(model, point):
    n, p, _ = BL.GRID[point]
    want, _, tie, _ = BL.twin(point)
    got = model.selftest_binomial(np.full(BL.N_DRAWS, n, np.int32), np.full(BL.N_DRAWS, p), seed=BL.SEED)
    share, _ = _same_but_for_near_ties(got, want, tie, "device " + point)
    if n <= 2 ** 22:
        assert share < MAX_TIE_SHARE_SMALL_N, (point, share)
    BL.assert_law(got, n, p, "device " + point)


def _divergent_inputs(count):
    """Every lane its own (n, p): n log-uniform on 1 .. 2^31 - 1; p log-uniform on 1e-12 .. 1 (70%), uniform within 1e-6 of
    1/2 (25%) or one of 0, 1, 1.5, -0.1, NaN (5%) -- neighbours take different branches and numbers of attempts."""
    rng = np.random.default_rng(DIVERGENT_SEED)
    n = np.clip(np.floor(np.exp(rng.uniform(0.0, np.log(2.0 ** 31), count))), 1, BL.N31).astype(np.int32)
    kind = rng.uniform(size=count)
    p = 10.0 ** rng.uniform(-12.0, 0.0, count)
    half = 0.5 + rng.uniform(-1e-6, 1e-6, count)
    special = rng.choice([0.0, 1.0, 1.5, -0.1, np.nan], count)
    p = np.where(kind < 0.70, p, np.where(kind < 0.95, half, special))
    return n, p


@pytest.fixture(scope="module")
def divergent(model):
    """2^20 + 1 divergent elements: inputs, the device's draws, the twin's report."""
    count = BL.N_DRAWS + 1
    n, p = _divergent_inputs(count)
    got = model.selftest_binomial(n, p, seed=DIVERGENT_SEED)
    ref = c_binding.sim_binomial(n, p, 0, np.arange(count), sim.RS_SIM_BASE, DIVERGENT_SEED)
    for a in (n, p, got) + ref:
        a.setflags(write=False)
    return n, p, got, ref


def test_divergent_waves_equal_twin(model, divergent):
    n, p, got, (want, branch, tie, att) = divergent
    counts = np.bincount(branch, minlength=5)
    print("divergent: branches", dict(zip(c_binding.SIM_BRANCHES, counts.tolist())), "max attempts", int(att.max()))
    assert counts[:4].min() > 10 ** 4 and counts[c_binding.SIM_FALLBACK] == 0    # every branch is in the mixture
    lanes = branch[:BL.N_DRAWS].reshape(-1, 64)
    assert np.mean((lanes != lanes[:, :1]).any(axis=1)) > 0.999                  # and within (nearly) every wave
    _same_but_for_near_ties(got, want, tie, "divergent")
    # the same elements in another order: other neighbours, and every element on another cell's substream -- the device
    # gives what the twin gives for that assignment; the elements that draw nothing keep their values
    perm = np.random.default_rng(DIVERGENT_SEED + 1).permutation(n.size)
    got2 = model.selftest_binomial(n[perm], p[perm], seed=DIVERGENT_SEED)
    want2, branch2, tie2, _ = c_binding.sim_binomial(n[perm], p[perm], 0, np.arange(n.size), sim.RS_SIM_BASE, DIVERGENT_SEED)
    _same_but_for_near_ties(got2, want2, tie2, "divergent, permuted")
    trivial = branch2 == c_binding.SIM_TRIVIAL
    assert np.array_equal(got2[trivial], got[perm][trivial])


@pytest.mark.parametrize("count", [1, 255, 256, 257])
def test_the_count_of_a_launch_changes_no_draw(model, divergent, count):
    """Workgroups of 256: one element, one short of a workgroup, exactly one, one more -- against the launch of 2^20 + 1."""
    n, p, full, _ = divergent
    assert full.size == BL.N_DRAWS + 1
    assert np.array_equal(model.selftest_binomial(n[:count], p[:count], seed=DIVERGENT_SEED), full[:count])


def test_lfact_at_production_arguments(model):
    """log(n!) on the device (Stirling's series above the 64-entry table) where BTRS reaches with UK populations and up to the
    int32 limit, against mpmath with the tolerance of test_logprob_gpu.test_device_math_against_mpmath."""
    import mpmath as mp
    mp.mp.dps = 40
    x = np.array([63.0, 64.0, 65.0, 66.0, 67.0, 100.0, 2.0 ** 21, 9e6, 2.0 ** 31 - 2, 2.0 ** 31 - 1])
    lf = model.selftest_math(x)[2]
    for xi, got in zip(x, lf):
        want = mp.loggamma(mp.mpf(float(xi)) + 1)
        err = abs(mp.mpf(float(got)) - want)
        print(f"lfact({xi:.0f}): error {float(err):.3g}, bound {float(2e-15 * max(1, abs(want))):.3g}")
        assert err <= 2e-15 * max(1, abs(want)), (xi, got)


def _explain(k, par, a_path, spatial, W, wd, init, want, got, seed, first_draw_id):
    """The twin's report on the first cell (in simulation order) at which `got` leaves the oracle's `want`."""
    d, m, s, x = min((tuple(i) for i in np.argwhere(got != want)), key=lambda i: (i[0], i[2], i[1], i[3]))
    state = init[d] + want[d, :, :s, :].sum(axis=1) @ so.STOICHIOMETRY
    lam, nu, rir = sim.day_rates(state, np.concatenate([par[d], spatial[d]]), float(a_path[d][s]), float(W[s]), float(wd[s]), k)
    prob = (sim._prob(float(lam[m]) * so.TIME_DELTA), sim._prob(nu * so.TIME_DELTA), sim._prob(rir * so.TIME_DELTA))[x]
    v, branch, tie, att = c_binding.sim_binomial(int(state[m, x]), prob, first_draw_id + d, s * k.M + m, sim.RS_SIM_BASE + x, seed)
    return (f"first difference at draw {d} day {s} row {m} transition {x}: device {got[d, m, s, x]}, oracle {want[d, m, s, x]}; "
            f"twin: n={int(state[m, x])} p={prob!r} -> {int(v[0])} by {c_binding.SIM_BRANCHES[branch[0]]} in {int(att[0])} "
            f"attempt(s), near-tie={bool(tie[0])}")


def test_simulator_at_uk380_equals_the_python_oracle(model, api):  # noqa: F811
    """k_simulate at UK populations (state of day 200, 2 draws, 4 days: ~9000 variates, most of them BTRS) against
    oracle/sim_oracle.simulate, all days, by equality."""
    from tests.test_simulate import _sim_inputs
    case = H.build_case("uk380", 20210101)
    par, a_path, spatial, W, wd, init = _sim_inputs(case, 2, 4, 8, 200)
    want = sim.simulate(case["k"], par, a_path, spatial, W, wd, init, seed=5, first_draw_id=7)
    with api[0](case["cov"], case["init"], max_chains=1) as uk:
        got = uk.simulate(par, a_path, spatial, W, wd, init, seed=5, first_draw_id=7)
    assert init[..., 0].max() > 2 ** 18 and want.max() > 1000                    # BTRS at large n is what is being run
    assert np.array_equal(got, want), _explain(case["k"], par, a_path, spatial, W, wd, init, want, got, 5, 7)


def test_forecast_at_uk380_equals_the_python_oracle(api):  # noqa: F811
    """k_forecast_day at UK populations: one chain, 2 draws, 3 days, against oracle/sim_oracle.simulate started from the
    draws' recorded state (as test_forecast_gpu.test_forecast_equals_the_independent_cpu_simulator does at micro sizes)."""
    from tests.test_forecast_gpu import _case, _oracle, _reset, _same_marginals, _same_moments, _sampler
    case, u, ev, cfg, eps = _case("uk380", 1)
    n, Hn = 2, 3
    sampler_model, s = _sampler(api, case, cfg, u, ev, eps, n, record_events="u16")
    with sampler_model, s:
        _reset(s, case, Hn)
        tr = s.sample(n, forecast=True)
        want = _oracle(sampler_model, case, tr.theta, tr.events, Hn,
                       simulate=lambda *a, **kw: sim.simulate(case["k"], *a, **kw))
        assert want["sim"].max() > 100
        _same_marginals(tr.forecast, want)
        _same_moments(s.forecast_summary(), want)

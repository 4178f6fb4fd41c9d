"""The stateless entry points at the shapes the host dispatch (covid19uk_amd/csrc/seir_hip.hip) turns on, not at workload
sizes: evaluation (three launch forms, prepare + evaluate, the fp32 contraction), R_it, within/between and the simulator
against the oracles at tile edges, at the LDS limits and past them.

Dispatch of the evaluation, with Mp = ceil64(M), Tp = ceil64(T), Kp = ceil4(M):
  fused / three-launch / one-launch tiles   TN = 96 if Tp % 96 == 0 else 64; Mp / 64 row tiles x Tp / TN day tiles;
                                            K loop in chunks of GSE_KC = 16 over Kp (the last one partial if Kp % 16)
  four-launch and prepare contraction       k_gemm_w8 where Tp % 96 == 0 and 96-day tiles turn > 256 tiles of 64 into
                                            <= 256, else k_gemm<64>: K chunks of 64 over Kp
  one launch                                B a multiple of 8 (and the tiles resident); three launches otherwise
Each case id names what it reaches; a change to these rules makes the ids stale."""
import functools

import numpy as np
import pytest

from covid19uk_amd import synth
from oracle import c_binding
from oracle import rt_oracle as ro
from oracle import seir_oracle as so
from oracle import sim_oracle as sim
from tests import helpers as H

pytestmark = pytest.mark.gpu

RTOL_LOGP = 1e-9
RTOL_GRAD = 1e-6
SEIR_MAX_T = 1088            # include/seir_hip.h


@pytest.fixture(scope="module")
def Model():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import __graft_entry__ as entry
    entry.build()
    from covid19uk_amd.seir import SeirModel
    c_binding.set_threads(8)
    return SeirModel


def _kind(M, T):
    # 'slower_': populations 400 times larger, still running after 1000+ days (and counts beyond 2048)
    return "slower" if T > 200 else "micro"


@functools.lru_cache(maxsize=None)
def _case(M, T, B, seed, kind=None):
    """Case, jittered batch [B] and the C oracle's (log-prob, gradient) of every chain."""
    case = H.build_case(f"{kind or _kind(M, T)}_{M}x{T}", seed, alpha_t_sd=0.005)
    u = synth.jitter_params(case["u"], B, seed=seed, T=T)
    rng = np.random.default_rng(seed)
    # the scalars near the generating ones, as at SYN-2048: dense mobility over 1000+ rows turns a jittered psi into
    # negative rates (an infeasible, NaN, density)
    u[:, :6] = case["u"][:6] + 0.01 * rng.normal(size=(B, 6))
    u[:, 6:6 + T - 1] = 0.005 * rng.normal(size=(B, T - 1))
    ev = np.stack([case["events"]] * B)
    want = [c_binding.evaluate(case["k"], u[b], ev[b], 1, want_grad=True) for b in range(B)]
    return case, u, ev, want


def _check(lp, g, want, rtol_logp=RTOL_LOGP, rtol_grad=RTOL_GRAD):
    for b, (wl, wg) in enumerate(want):
        assert np.isfinite(wl)
        assert abs(lp[b] - wl) <= rtol_logp * abs(wl), (b, lp[b], wl)
        if g is not None:
            scale = np.maximum(np.abs(wg), 1e-6 * np.abs(wg).max())
            err = np.max(np.abs(g[b] - wg) / scale)
            assert err < rtol_grad, (b, err)


# (M, T): Mp, Tp, TN, row tiles x day tiles, Kp and its 16-wide chunks, the four-launch contraction
EVAL_SHAPES = [
    pytest.param(63, 70, id="63x70-Mp64-Tp128-TN64-1x2tiles-Kp64"),
    pytest.param(65, 70, id="65x70-Mp128-Tp128-TN64-2x2tiles-Kp68_partialK16-gemm64_2K"),
    pytest.param(129, 191, id="129x191-Mp192-Tp192-TN96-3x2tiles-Kp132_partialK16-scan_partial_block"),
    pytest.param(128, 193, id="128x193-Mp128-Tp256-TN64-2x4tiles-Kp128"),
    pytest.param(380, 320, id="380x320-Mp384-Tp320-TN64-6x5tiles-Kp380_partialK16-gemm64_6K"),
    pytest.param(380, 385, id="380x385-Mp384-Tp448-TN64-6x7tiles-gemm64_6K"),
    pytest.param(300, 1, id="300x1-Mp320-Tp64-TN64-no_alpha_t"),
    pytest.param(300, 2, id="300x2-Mp320-Tp64-TN64-one_alpha_t"),
    pytest.param(513, 64, id="513x64-Mp576-Tp64-TN64-9x1tiles-T_one_chunk"),
    pytest.param(1024, 1024, id="1024x1024-Mp1024-Tp1024-TN64-16x16tiles"),
    pytest.param(1025, 1025, id="1025x1025-Mp1088-Tp1088-TN64-17x17tiles-Kp1028_partialK16"),
    pytest.param(2048, 64, id="2048x64-Mp2048-Tp64-TN64-32x1tiles"),
    pytest.param(70, 1088, id="70x1088-Mp128-Tp1088-TN64-max_T"),
    pytest.param(2048, 1088, id="2048x1088-Mp2048-Tp1088-TN64-max_M_max_T"),
]
FORMS = ["fused", "three-launch", "four-launch"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("M,T", EVAL_SHAPES)
def test_evaluation_matches_c_oracle(Model, M, T, form):
    case, u, ev, want = _case(M, T, 1, 100 + M + T)
    if T > 1024:
        assert ev[0, :, 1024:, :].sum() > 0, "the epidemic must still run in the day tiles beyond 1024"
    with Model(case["cov"], case["init"], max_chains=1) as model:
        model.set_option(eval_form=form)
        lp, g = model.log_prob_grad(u, ev)
        _check(lp, g, want)
        assert np.array_equal(model.log_prob(u, ev), lp), "value-only and value+grad paths disagree"


@pytest.mark.parametrize("M,T", EVAL_SHAPES)
def test_prepared_evaluation_reproduces_the_four_launch_form(Model, M, T):
    import torch
    case, u, ev, _ = _case(M, T, 1, 100 + M + T)
    dev = torch.device("cuda:0")
    ut, evt = torch.tensor(u, device=dev), torch.tensor(ev, device=dev)
    lp1, lp2 = torch.empty(1, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev)
    g1 = torch.empty(1, u.shape[1], dtype=torch.float64, device=dev)
    g2 = torch.empty_like(g1)
    with Model(case["cov"], case["init"], max_chains=1) as model:
        model.set_option(eval_form="four-launch")
        model.log_prob_dev(ut, evt, lp1, g1)
        model.sync()
        model.prepare_events_dev(evt)
        model.eval_prepared_dev(ut, lp2, g2)
        model.sync()
    assert torch.equal(lp1, lp2) and torch.equal(g1, g2)


@pytest.mark.parametrize("M,T", [pytest.param(65, 70, id="65x70-TN64-2x2tiles"),
                                 pytest.param(129, 191, id="129x191-TN96-3x2tiles"),
                                 pytest.param(380, 320, id="380x320-TN64-6x5tiles")])
def test_eight_chains_one_launch_and_three_launches_give_the_same_bits(Model, M, T):
    """B = 8: the default is the one-launch form (k_eval_all<*, TN>) where the tiles fit the chip at once."""
    case, u, ev, want = _case(M, T, 8, 200 + M + T)
    res = {}
    for form in ("fused", "three-launch"):
        with Model(case["cov"], case["init"], max_chains=8) as model:
            model.set_option(eval_form=form)
            lp, g = model.log_prob_grad(u, ev)
            res[form] = (lp, g, model.log_prob(u, ev))
    _check(res["three-launch"][0], res["three-launch"][1], want)
    for a, b in zip(res["fused"], res["three-launch"]):
        assert np.array_equal(a, b)
    with Model(case["cov"], case["init"], max_chains=8) as model:
        model.set_option(eval_form="four-launch")
        lp, g = model.log_prob_grad(u, ev)
    _check(lp, g, want)


def test_log_factorial_table_edge(Model):
    """Counts on both sides of SCAN_LFT = 2048: the scans take log(n!) from their LDS table below it, from the
    Stirling series above it."""
    M, T = 65, 200
    case, u, ev, want = _case(M, T, 1, 3, kind="slower")
    state = so.compute_state(case["init"], ev[0])
    counts = np.concatenate([ev[0].ravel(), state[..., 1:3].ravel()])      # events, E, I (S is far above 2048)
    assert ((counts > 0) & (counts < 2048)).sum() > 100 and (counts >= 2048).sum() > 10
    for form in FORMS:
        with Model(case["cov"], case["init"], max_chains=1) as model:
            model.set_option(eval_form=form)
            lp, g = model.log_prob_grad(u, ev)
        _check(lp, g, want)


def test_fp32_contraction_at_mp_tp_256(Model):
    """gemm_f32 at Mp = Tp = 256 (two 128 tiles each way): the tolerance of the SYN-2048 test, and not the fp64 bits."""
    case, u, ev, want = _case(200, 250, 1, 31)
    with Model(case["cov"], case["init"], max_chains=1) as model:
        exact = model.log_prob_grad(u, ev)
        model.set_option(gemm_f32=True)
        lp, g = model.log_prob_grad(u, ev)
    assert not np.array_equal(lp, exact[0])
    for b, (wl, wg) in enumerate(want):
        assert abs(lp[b] - wl) <= 1e-8 * abs(wl), (lp[b], wl)
        assert np.max(np.abs(g[b] - wg)) < 2e-6 * np.abs(wg).max()


@pytest.mark.parametrize("T", [SEIR_MAX_T + 1, 1153, 2048])
def test_series_beyond_the_lds_limit_are_refused_at_create(Model, T):
    from covid19uk_amd import _lib
    cov = H.small_covariates(3, T, 1)
    init = np.array([[1000.0, 0.0, 5.0, 0.0]] * 3)
    with pytest.raises(_lib.SeirError, match=f"T <= {SEIR_MAX_T}"):
        Model(cov, init)


# ---------------------------------------------------------------------------------------------
# R_it and within/between
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,T", [pytest.param(511, 9, id="511x9-Mp512-k_rt16"),
                                 pytest.param(512, 9, id="512x9-Mp512-k_rt16_full_LDS"),
                                 pytest.param(513, 9, id="513x9-Mp576-k_rt4"),
                                 pytest.param(2048, 9, id="2048x9-Mp2048-k_rt4"),
                                 pytest.param(70, 1088, id="70x1088-Mp128-k_rt16-68_day_tiles")])
def test_reproduction_number_matches_oracle(Model, M, T):
    case = H.build_case(f"{_kind(M, T)}_{M}x{T}", 40 + M, alpha_t_sd=0.01)
    k = case["k"]
    u = synth.jitter_params(case["u"], 2, scale=0.1, seed=M, T=T)
    theta = so.constrain(u)
    ev = np.stack([case["events"]] * 2)
    want, _ = ro.posterior_rit(theta, ev, k, stable=True)
    with Model(case["cov"], case["init"], max_chains=2) as model:
        got = model.reproduction_number(theta, ev)
    assert got.shape == want.shape
    err = np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-12 * np.abs(want).max()))
    assert err < 1e-11, err


@pytest.mark.parametrize("M", [513, 2048])
def test_within_between_matches_oracle(Model, M):
    case = H.build_case(f"micro_{M}x9", 50 + M)
    k, cov = case["k"], case["cov"]
    rng = np.random.default_rng(M)
    st = np.stack([so.compute_state(k.initial_state, case["events"])[:, -1, :]] * 3)
    st[:, :, 2] += rng.integers(1, 50, size=(3, M))
    # dense mobility over hundreds of rows: psi below the point where `within` turns negative somewhere, so that the
    # fractions stay in [0, 1] (beyond it within + between cancels and the fractions lose all absolute accuracy)
    C = np.array(cov.C, dtype=np.float64)
    np.fill_diagonal(C, 0.0)
    psi = np.array([0.2, 0.5, 0.9]) * np.min(cov.N / (k.W[-1] * C.sum(axis=0)))
    want_w, want_b = ro.pressure_components(psi, st, cov.C, cov.N, k.W[-1])
    assert np.all((want_w >= 0) & (want_w <= 1))
    with Model(cov, case["init"], max_chains=1) as model:
        got_w, got_b = model.within_between(psi, st[:, :, 2], k.W[-1])
    assert max(np.abs(got_w - want_w).max(), np.abs(got_b - want_b).max()) < 1e-12


# ---------------------------------------------------------------------------------------------
# Simulator: SIM_THREADS = 512 rows per stride, SIM_DAYS_STAGED = 8 days per flush, draw chunks of 512 MB
# ---------------------------------------------------------------------------------------------
def _sim_inputs(case, n, S, seed):
    k = case["k"]
    rng = np.random.default_rng(seed)
    from covid19uk_amd.posterior import predict as pp
    theta = so.constrain(synth.jitter_params(case["u"], n, scale=0.05, seed=seed, T=k.T))
    par = theta[:, :5].copy()
    a_path = pp.log_baseline_path(theta[:, 5], theta[:, 6:6 + k.T - 1], 5, S)
    spatial = theta[:, 6 + k.T - 1:]
    W = pp.clipped(k.W, 5, S)
    wd = pp.clipped(k.weekday_c, 5, S)
    init = np.stack([so.compute_state(k.initial_state, case["events"])[:, 5, :]] * n)
    init[:, :, 2] += rng.integers(0, 30, size=init.shape[:2])
    return par, a_path, spatial, W, wd, init


@pytest.mark.parametrize("M", [pytest.param(64, id="64-one_stride"), pytest.param(65, id="65-Mp128"),
                               pytest.param(511, id="511-one_stride"), pytest.param(512, id="512-one_full_stride"),
                               pytest.param(513, id="513-second_stride"), pytest.param(1280, id="1280-max_M")])
def test_simulation_matches_oracle_draw_for_draw(Model, M):
    case = H.build_case(f"micro_{M}x20", 60 + M, alpha_t_sd=0.01)
    with Model(case["cov"], case["init"], max_chains=1) as model:
        for S in (1, 7, 8, 9, 17):             # inside one staged flush, exactly one, one and a bit, two and a bit
            par, a_path, spatial, W, wd, init = _sim_inputs(case, 2, S, S)
            want = sim.simulate(case["k"], par, a_path, spatial, W, wd, init, seed=99, first_draw_id=5)
            got = model.simulate(par, a_path, spatial, W, wd, init, seed=99, first_draw_id=5)
            assert np.array_equal(got, want), (S, np.argwhere(got != want)[:5])
            assert want[..., 0].sum() > 0 and want[..., 2].sum() > 0


def test_simulation_beyond_1280_rows_is_refused(Model):
    from covid19uk_amd import _lib
    case = H.build_case("micro_1281x20", 3)
    par, a_path, spatial, W, wd, init = _sim_inputs(case, 1, 3, 1)
    with Model(case["cov"], case["init"], max_chains=1) as model:
        with pytest.raises(_lib.SeirError, match="LDS"):
            model.simulate(par, a_path, spatial, W, wd, init)


def test_simulation_draws_span_two_device_chunks(Model):
    """1280 rows x 2048 days is 63 MB of events per draw: 8 draws per device chunk, so draw 8 is the first of the
    second chunk and must be what a call that starts at draw id 8 gives.  A sub-critical epidemic keeps the
    mobility sums (which skip zero infectives) short."""
    M, S, n = 1280, 2048, 9
    case = H.build_case(f"micro_{M}x20", 70)
    par, _, spatial, W, wd, init = _sim_inputs(case, n, S, 3)
    a_path = np.full((n, S), np.log(0.05))
    par[:, 3] = np.log(0.25)                   # gamma0: recovery 4 times faster than infection
    W, wd = np.resize(W, S), np.resize(wd, S)
    with Model(case["cov"], case["init"], max_chains=1) as model:
        ev = model.simulate(par, a_path, spatial, W, wd, init, seed=11)
        one = model.simulate(par[8:], a_path[8:], spatial[8:], W, wd, init[8:], seed=11, first_draw_id=8)
    assert np.array_equal(ev[8:], one)
    assert not np.array_equal(ev[7], ev[8])
    assert np.all(ev >= 0) and ev[..., 2].sum() > 0
    for d in (0, 7, 8):
        st = so.compute_state(init[d], ev[d])
        assert np.all(st >= 0)
        assert np.array_equal(st.sum(-1), np.repeat(init[d].sum(-1)[:, None], S, 1))

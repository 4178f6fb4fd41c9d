"""Within/between pressure shares on the device (include/seir_hip.h, "Within/between pressure shares on the device";
covid19uk_amd/csrc/wb_kernels.h): for every kept draw the within- and between-location infection pressure over the window
[T - D, T) is formed from the burst buffer where it lies, its shares folded into per-chain accumulators and the pressures
summed into the national values of the draw.

The reference for every equality is the same run's recorded draws: `tr.theta` and `tr.events` are read back, I_t is formed
in NumPy from the events, and every (draw, day) goes through the stateless `SeirModel.within_between` (k_within_between) of
a context of its own; the shares are folded by a NumPy loop in draw order -- separately rounded operations, and a draw
whose shares are not both finite is left out, as the device's.  n, ref_w, sum_w, sumsq_w, ref_b, sum_b, gt and count are held
to `np.array_equal`.

The national pressures are held to a derived bound against `math.fsum` of the same inputs (`_national`):
    |device - reference| <= 2^-52 (M + 32) sum_m (|I_m| + |psi W Cstar_mm x_m| + sum_{j != m} |psi W Cstar_jm x_j|)
-- at most M + 32 roundings of relative size 2^-53 per path (x, the M terms of the four chains and their combination, the
products with psi W, the 6 levels of the butterfly, the column blocks), with a factor 2 to spare.  The reference's terms are
float64 products of four factors, at most 4 roundings each, which the spare factor covers: (M + 32) + 4 <= 2 (M + 32).

Two micro cases also go through `oracle/rt_oracle.pressure_components`, which shares nothing with the device's
arithmetic, at the tolerance tests/test_rt.py uses for the stateless form."""
import math
import os

import numpy as np
import pytest

from covid19uk_amd import _lib, synth
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.posterior import predict
from covid19uk_amd.posterior import within_between as wbtool
from oracle import rt_oracle as ro
from oracle import seir_oracle as so
from tests import helpers as H
from tests.test_recovery_gpu import _case, _same_bits
from tests.test_sampler_gpu import CFG_REF, CFG_SMALL, api  # noqa: F401  (fixture)
from tests.test_summary_gpu import _cli, _datasets, _sampler

pytestmark = pytest.mark.gpu

WB_DT = 4                     # k_wb_trace's day tile (wb_kernels.h)
ACC = ("count", "defined", "ref_w", "sum_w", "sumsq_w", "ref_b", "sum_b", "gt")


def _infectious(init, events):
    """events [n,B,M,T,3] -> I at the start of every day, [n,B,T,M] float64 (exact integers): init + the exclusive prefix
    of k_ei - k_ir."""
    d = events[..., 1].astype(np.int64) - events[..., 2].astype(np.int64)
    I = np.asarray(init)[:, 2].astype(np.int64)[None, None, :, None] + np.cumsum(d, axis=-1) - d
    return np.moveaxis(I, -1, 2).astype(np.float64)


def _reference(api, case, theta, events, D):
    """theta [n,B,P], events [n,B,M,T,3] of one run -> (within, between) shares [n,B,D,M] over the window, by the stateless
    kernel called per (draw, day), and I [n,B,D,M]."""
    n, B = theta.shape[:2]
    T, M = case["k"].T, case["k"].M
    I = _infectious(case["init"], events)[:, :, T - D:]
    W = np.asarray(case["cov"].W, dtype=np.float64).reshape(-1)
    fw, fb = np.empty((n, B, D, M)), np.empty((n, B, D, M))
    psi = np.ascontiguousarray(theta[:, :, 0]).reshape(-1)
    with api[0](case["cov"], case["init"], max_chains=1) as model:
        for tw in range(D):
            w, b = model.within_between(psi, I[:, :, tw].reshape(n * B, M), W[T - D + tw])
            fw[:, :, tw], fb[:, :, tw] = w.reshape(n, B, M), b.reshape(n, B, M)
    return fw, fb, I


def _fold(fw, fb):
    """Shares [n,B,D,M] -> the accumulators, by the loop the kernel file states."""
    shape = fw.shape[1:]
    n, gt = np.zeros(shape, np.uint32), np.zeros(shape, np.uint32)
    ref_w, sum_w, sumsq_w, ref_b, sum_b = (np.zeros(shape) for _ in range(5))
    with np.errstate(invalid="ignore"):
        for w, b in zip(fw, fb):
            d = np.isfinite(w) & np.isfinite(b)
            first = d & (n == 0)
            ref_w, ref_b = np.where(first, w, ref_w), np.where(first, b, ref_b)
            dw, db = w - ref_w, b - ref_b
            sum_w = np.where(d, sum_w + dw, sum_w)
            sumsq_w = np.where(d, sumsq_w + dw * dw, sumsq_w)
            sum_b = np.where(d, sum_b + db, sum_b)
            gt = gt + (d & (w > b)).astype(np.uint32)
            n = n + d.astype(np.uint32)
    return dict(count=np.full(shape[0], len(fw), np.uint64), defined=n, ref_w=ref_w, sum_w=sum_w, sumsq_w=sumsq_w, ref_b=ref_b,
                sum_b=sum_b, gt=gt)


def _same_acc(ws, want):
    assert ws.count.dtype == np.uint64 and ws.defined.dtype == ws.gt.dtype == np.uint32
    assert ws.ref_w.dtype == ws.sum_w.dtype == ws.sumsq_w.dtype == ws.ref_b.dtype == ws.sum_b.dtype == np.float64
    for k in ACC:
        assert np.array_equal(getattr(ws, k), want[k]), k


def _national(case, theta, I, got, draws=None, days=None):
    """The national pressures `got` = WB_KEYS -> [n,B,D] against math.fsum of the same inputs, at the derived bound of the
    module's docstring.  `draws` / `days` (default: all) choose the (draw, day) pairs that are summed."""
    k = case["k"]
    M, T = k.M, k.T
    n, B, D = I.shape[:3]
    Cs = np.asarray(k.Cstar, np.float64)
    invN = np.array([float(1.0 / v) for v in np.asarray(k.N, np.float64)])
    W = np.asarray(case["cov"].W, dtype=np.float64).reshape(-1)
    off = ~np.eye(M, dtype=bool)
    worst = 0.0
    for j in (range(n) if draws is None else draws):
        for b in range(B):
            psi = float(theta[j, b, 0])
            for tw in (range(D) if days is None else days):
                pw = psi * float(W[T - D + tw])
                x = I[j, b, tw] * invN
                selfs = pw * np.diag(Cs) * x
                cross = (pw * Cs * x[:, None])[off]             # term (j, m): psi W Cstar_jm x_j
                want_w = math.fsum(I[j, b, tw]) + math.fsum(selfs)
                want_b = math.fsum(cross)
                bound = 2.0 ** -52 * (M + 32) * (math.fsum(np.abs(I[j, b, tw])) + math.fsum(np.abs(selfs)) + math.fsum(np.abs(cross)))
                ew = abs(got["within_pressure"][j, b, tw] - want_w)
                eb = abs(got["between_pressure"][j, b, tw] - want_b)
                if bound > 0:
                    worst = max(worst, ew / bound, eb / bound)
                assert ew <= bound and eb <= bound, (j, b, tw, ew, eb, bound)
    print(f"national pressures: largest error / bound = {worst:.3g}")


def _same_run(a, b):
    """(WbSummary, national pressures) of two runs: every bit."""
    for k in ACC:
        assert np.array_equal(getattr(a[0], k), getattr(b[0], k)), k
    for k in a[1]:
        assert np.array_equal(a[1][k], b[1][k]), k


# the case ids name the branch they turn: the chains j mod 4 and the column blocks of 64 (M), the day tile of 4 and the prefix
# over [0, T - D) (D), chains, trace width, one draw and a full burst (n = the buffer's capacity)
CASES = {
    # name, cfg, eps, B, record, n, D
    "M=1,D=tile+1": ("micro_1x70", CFG_SMALL, 0.002, 3, "u16", 6, WB_DT + 1),
    "M=9,T=64,D=tile": ("micro_9x64", CFG_SMALL, 0.0004, 3, "u16", 5, WB_DT),
    "M=65,second_partial_column_block,D=tile-1": ("micro_65x70", CFG_SMALL, 0.0001, 1, "u16", 3, WB_DT - 1),
    "M=520,nine_column_blocks,T=20,D=5": ("slow_520x20", CFG_SMALL, 3e-5, 1, True, 3, 5),
    "M=3,T=1,D=1,the_state_is_init": ("micro_3x1", CFG_SMALL, 0.002, 2, True, 4, 1),
    "T=2,D=T": ("micro_2x2", CFG_SMALL, 0.002, 1, True, 4, 2),
    "T=65,D=T,8_chains,full_burst": ("micro_7x65", CFG_SMALL, 0.0004, 8, True, 8, 65),
    "T=70,D=1,one_draw": ("micro_20x70", CFG_SMALL, 0.0004, 3, "u16", 1, 1),
    "T=70,D=66,prefix_of_4": ("micro_20x70", CFG_SMALL, 0.0004, 3, True, 4, 66),
    "uk380x8,12,D=14": ("uk380", CFG_REF, 1.2e-5, 8, "u16", 12, 14),
}


@pytest.mark.parametrize("case_id", list(CASES))
def test_wb_equals_the_stateless_kernel_on_the_recorded_draws(api, case_id):
    name, cfg, eps, B, record, n, D = CASES[case_id]
    case = H.build_case(name, 43, alpha_t_sd=0.005)
    u = synth.jitter_params(case["u"], B, scale=0.002 if name == "uk380" else 0.01, seed=3, T=case["k"].T)
    ev = np.stack([case["events"]] * B)
    M = case["k"].M
    model, s = _sampler(api, case, cfg, u, ev, eps, n, record_events=record)
    with model, s:
        s.reset_within_between(D)
        tr = s.sample(n, within_between=True)
        ws = s.within_between_summary()
        assert tr.events.dtype == (np.uint16 if record == "u16" else np.int32)
        assert ws.ref_w.shape == (B, D, M) and all(tr.wb[k].shape == (n, B, D) for k in tr.wb)
        fw, fb, I = _reference(api, case, tr.theta, tr.events, D)
        _same_acc(ws, _fold(fw, fb))
        big = M > 65                                           # the exact sums of M^2 terms: first and last draw and day
        _national(case, tr.theta, I, tr.wb, draws=sorted({0, n - 1}) if big else None, days=sorted({0, D - 1}) if big else None)
        if n > 1 and M > 1:
            assert ws.sumsq_w.any(), "every draw has the same shares"
        # a second reset: the last slot alone, with nothing left of the first fold
        s.reset_within_between(D)
        s.within_between(n - 1, 1)
        _same_acc(s.within_between_summary(), _fold(fw[n - 1:], fb[n - 1:]))
        last = s.read_wb_draws(1, first=n - 1)
        for k in last:
            assert np.array_equal(last[k], tr.wb[k][n - 1:]), k
        # ... and another window allocates again
        D2 = 1 if D > 1 else case["k"].T
        s.reset_within_between(D2)
        s.within_between(0, n)
        if D2 <= D:
            fw2, fb2 = fw[:, :, D - D2:], fb[:, :, D - D2:]
        else:
            fw2, fb2, _ = _reference(api, case, tr.theta, tr.events, D2)
        _same_acc(s.within_between_summary(), _fold(fw2, fb2))
        again = s.read_wb_draws(n)
        if D2 <= D:
            for k in again:
                assert np.array_equal(again[k], tr.wb[k][:, :, D - D2:]), k
        assert not s.pair_timeouts().any()


# ---- the preconditions: defined and undefined draws of one cell, within above between and not -----------------------------
def _quiet_case():
    """micro_5x24 with locations 0 and 3 emptied: nobody exposed or infectious there at the start and no recorded event, so
    that their own pressure is (next to) nothing while the others press on them: within <= between there."""
    case = H.build_case("micro_5x24", 43, alpha_t_sd=0.005)
    init, events = case["init"].copy(), case["events"].copy()
    for m in (0, 3):
        init[m] = [init[m].sum(), 0.0, 0.0, 0.0]
        events[m] = 0.0
    return dict(case, init=init, events=events, k=H.oracle_constants(case["cov"], init))


def _flicker_case():
    """One location, 12 days, nobody infectious at the start and three exposed: the first E->I events lie on days 1 and 3,
    so I is 0 on day 0 in every draw and 0 or not on days 1 .. 3 according to where the event-time updates have moved them:
    a cell's draws are some defined, some not."""
    cov = H.small_covariates(1, 12, 43)
    N = float(np.asarray(cov.N).reshape(-1)[0])
    init = np.array([[N - 3.0, 3.0, 0.0, 0.0]])
    events = np.zeros((1, 12, 3))
    events[0, [1, 3, 7, 9], 1] = 1.0                            # E->I
    events[0, [4, 6], 0] = 1.0                                  # S->E, on days with an infective
    events[0, [5, 8, 10], 2] = 1.0                              # I->R
    _, _, truth = synth.simulate_epidemic(cov, 43, alpha_t_sd=0.005, params=dict(alpha_0=-0.5))
    u = synth.unconstrain(synth.pack_params(truth, 1, 12))
    st = so.compute_state(init, events)
    assert st.min() >= 0 and np.all(events[..., 1] <= st[..., 1]) and np.all(events[..., 2] <= st[..., 2])
    return dict(cov=cov, events=events, init=init, u=u, k=H.oracle_constants(cov, init))


FLICKER = dict(B=8, n=16, eps=0.002, seed=13)
QUIET = dict(B=3, n=6, eps=0.0004, seed=13)


def test_within_is_not_above_between_where_a_location_has_no_infective_of_its_own(api):
    case = _quiet_case()
    B, n, D = QUIET["B"], QUIET["n"], case["k"].T
    u = synth.jitter_params(case["u"], B, scale=0.01, seed=3, T=case["k"].T)
    ev = np.stack([case["events"]] * B)
    model, s = _sampler(api, case, CFG_SMALL, u, ev, QUIET["eps"], n, seed=QUIET["seed"])
    with model, s:
        s.reset_within_between(D)
        tr = s.sample(n, within_between=True)
        ws = s.within_between_summary()
    fw, fb, I = _reference(api, case, tr.theta, tr.events, D)
    ok = np.isfinite(fw) & np.isfinite(fb)
    # the precondition: both outcomes of the comparison occur among the defined draws, the emptied locations on the low side
    assert (ok & (fw > fb)).any() and (ok & ~(fw > fb)).any()
    assert (ok[:, :, :, [0, 3]] & ~(fw > fb)[:, :, :, [0, 3]]).any()
    _same_acc(ws, _fold(fw, fb))
    assert ws.gt.max() > 0 and (ws.gt < ws.defined).any()
    assert np.array_equal(ws.p_within_gt_between, _fold(fw, fb)["gt"] / np.where(ok.sum(0) > 0, ok.sum(0), np.nan), equal_nan=True)
    _national(case, tr.theta, I, tr.wb)


def test_a_cell_with_defined_and_undefined_draws_folds_the_defined_ones_alone(api):
    case = _flicker_case()
    B, n, D = FLICKER["B"], FLICKER["n"], case["k"].T
    u = synth.jitter_params(case["u"], B, scale=0.01, seed=3, T=case["k"].T)
    ev = np.stack([case["events"]] * B)
    model, s = _sampler(api, case, CFG_SMALL, u, ev, FLICKER["eps"], n, seed=FLICKER["seed"])
    with model, s:
        s.reset_within_between(D)
        tr = s.sample(n, within_between=True)
        ws = s.within_between_summary()
    fw, fb, I = _reference(api, case, tr.theta, tr.events, D)
    ok = np.isfinite(fw) & np.isfinite(fb)
    k = ok.sum(axis=0)
    # the precondition: a cell with defined and undefined draws, one whose FIRST draw is undefined among them, and a cell
    # without a defined draw at all (day 0)
    mixed = (k > 0) & (k < n)
    assert mixed.any(), "no cell has both defined and undefined draws"
    assert (mixed & ~ok[0]).any(), "no mixed cell starts with an undefined draw"
    assert np.all(k[:, 0] == 0)
    assert np.array_equal(np.isnan(fw), I == 0.0)             # one location: no infective, no pressure, 0 / 0
    _same_acc(ws, _fold(fw, fb))
    assert np.array_equal(ws.defined, k) and np.array_equal(ws.count, np.full(B, n, np.uint64))
    assert np.all(np.isnan(ws.within_mean[:, 0])) and np.all(ws.within_mean[k > 0] == 1.0)
    _national(case, tr.theta, I, tr.wb)
    assert np.array_equal(tr.wb["within_pressure"] == 0.0, (I == 0.0)[..., 0])


@pytest.mark.parametrize("name", ["micro_3x5", "ni11"])
def test_the_mean_of_the_last_day_equals_the_independent_cpu_oracle(api, name):
    """oracle/rt_oracle.pressure_components on the last state of the recorded draws, at the absolute 1e-12 that
    tests/test_rt.py holds the stateless form to (shares in [0, 1]; a mean of values that each meet it meets it too, and
    the fold's rounding over 4 draws is far below it)."""
    case, u, ev, cfg, eps = _case(name, 2)
    n, D = 4, 3
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        s.reset_within_between(D)
        tr = s.sample(n, within_between=True)
        ws = s.within_between_summary()
    k, cov = case["k"], case["cov"]
    for b in range(2):
        st = np.stack([so.compute_state(k.initial_state, tr.events[j, b].astype(np.float64))[:, -1, :] for j in range(n)])
        want_w, want_b = ro.pressure_components(tr.theta[:, b, 0], st, cov.C, cov.N, k.W[-1])
        assert np.all(np.isfinite(want_w)) and np.array_equal(ws.defined[b, -1], np.full(k.M, n))
        err = max(np.abs(ws.within_mean[b, -1] - want_w.mean(axis=0)).max(), np.abs(ws.between_mean[b, -1] - want_b.mean(axis=0)).max())
        print(f"{name} chain {b}: error of the means {err:.3e}")
        assert err < 1e-12, err
        assert np.array_equal(ws.gt[b, -1], (want_w > want_b).sum(axis=0))


# ---- invariances ----------------------------------------------------------------------------------------------------------
def test_cutting_a_burst_into_calls_halves_or_batches_does_not_matter(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    n, D = 11, 9
    model, s = _sampler(api, case, cfg, u, ev, eps, 2 * n)
    with model, s:
        s.reset_within_between(D)
        for first in (0, n):                                   # two bursts in the two halves of the buffer
            s.reset_trace(at=first)
            s.run(n)
            s.within_between(first, n)
        tr = s.read_trace(2 * n)
        halves = (s.within_between_summary(), s.read_wb_draws(2 * n))
        fw, fb, I = _reference(api, case, tr.theta, tr.events, D)
        _same_acc(halves[0], _fold(fw, fb))
        _national(case, tr.theta, I, halves[1])
        s.reset_within_between(D)
        s.within_between(0, 2 * n)                             # one call over everything
        _same_run((s.within_between_summary(), s.read_wb_draws(2 * n)), halves)
        s.reset_within_between(D)
        for first, count in ((0, 3), (3, 1), (4, 9), (13, 2 * n - 13)):
            s.within_between(first, count)
        _same_run((s.within_between_summary(), s.read_wb_draws(2 * n)), halves)
        # the host's own cut: a staging bound of 64 KiB holds 64 KiB / (5 chains x 64 rows x 9 days x 4 B) = 5 slots,
        # so the 22 slots go as batches of 5, 5, 5, 5 and 2 (the bound is read when the window changes)
        model.set_option(rt_staging_kib=64)
        s.reset_within_between(D + 1)
        s.reset_within_between(D)
        s.within_between(0, 2 * n)
        _same_run((s.within_between_summary(), s.read_wb_draws(2 * n)), halves)
        model.set_option(rt_staging_kib=1)                     # less than one slot: one slot per batch
        s.reset_within_between(D + 1)
        s.reset_within_between(D)
        s.within_between(0, 2 * n)
        _same_run((s.within_between_summary(), s.read_wb_draws(2 * n)), halves)


@pytest.mark.parametrize("skew", [1, 2, 3])
def test_results_do_not_depend_on_workgroup_timing_and_repeat(api, skew):
    case, u, ev, cfg, eps = _case("micro_65x70", 2)
    n, D = 4, 6
    res = {}
    for tag, sk in (("a", 0), ("b", 0), ("skew", skew)):
        if tag == "b" and skew != 1:
            continue                                           # the repeat of the plain run is checked once
        model, s = _sampler(api, case, cfg, u, ev, 0.0001, n, skew=sk, record_events="u16")
        with model, s:
            s.reset_within_between(D)
            tr = s.sample(n, within_between=True)
            res[tag] = (s.within_between_summary(), tr.wb, tr)
    assert res["a"][0].sumsq_w.any()
    for tag in res:
        assert np.array_equal(res["a"][2].events, res[tag][2].events)
        _same_run(res[tag], res["a"])


def test_chains_keep_their_numbers_however_they_are_sharded(api):
    """Chains 2 and 3 of a 4-chain sampler against a 2-chain sampler created with first_chain_id = 2."""
    case, u, ev, cfg, eps = _case("micro_20x60", 4)
    n, D = 5, 8
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        s.reset_within_between(D)
        tr4 = s.sample(n, within_between=True)
        ws4 = s.within_between_summary()
    model, s = _sampler(api, case, cfg, u[2:], ev[2:], eps, n, first_chain_id=2)
    with model, s:
        s.reset_within_between(D)
        tr2 = s.sample(n, within_between=True)
        ws2 = s.within_between_summary()
    assert np.array_equal(tr4.events[:, 2:], tr2.events) and np.array_equal(tr4.theta[:, 2:], tr2.theta)
    assert ws2.sumsq_w.any()
    for k in tr2.wb:
        assert np.array_equal(tr4.wb[k][:, 2:], tr2.wb[k]), k
    for k in ACC:
        assert np.array_equal(getattr(ws4, k)[2:], getattr(ws2, k)), k


def test_with_thinning_the_numbers_are_those_of_the_kept_draws(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 4)
    n, D, k = 6, 5, 3
    model, s = _sampler(api, case, cfg, u, ev, eps, n, thin=k)
    with model, s:
        s.reset_within_between(D)
        kept = s.sample(n, within_between=True)
        ws = s.within_between_summary()
    model, s = _sampler(api, case, cfg, u, ev, eps, n * k)
    with model, s:
        every = s.sample(n * k)
    assert np.array_equal(every.events[k - 1::k], kept.events)
    fw, fb, I = _reference(api, case, every.theta[k - 1::k], every.events[k - 1::k], D)
    _same_acc(ws, _fold(fw, fb))
    _national(case, kept.theta, I, kept.wb)


def test_the_chain_and_the_other_products_do_not_notice(api):
    """A sampler that forms the shares behind every burst's summary, forecast, R_t and check against one that never does:
    traces, marginals, forecast, R_t, check, moments, final state and kernel bit for bit."""
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    nb, burst, Hn, D, K, Dw = 4, 5, 6, 7, 5, 6
    N = np.asarray(case["cov"].N, dtype=np.float64).reshape(-1)
    W, wd = predict.forecast_calendar(case["cov"], None, case["k"].T, Hn)
    cW, cwd = predict.check_calendar(case["cov"], None, case["k"].T, K)
    runs = {}
    for on in (False, True):
        model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
        with model, s:
            got = {}
            s.reset_forecast(Hn, W, wd, 77)
            s.reset_rt(D, N / N.sum())
            s.reset_check(K, cW, cwd, 78)
            if on:
                s.reset_within_between(Dw)

            def consume(tr, i, got=got):
                got[i] = (tr.theta.copy(), tr.events.copy(), {k: v.copy() for k, v in tr.hmc.items()},
                          {mk: {kk: v.copy() for kk, v in mv.items()} for mk, mv in tr.moves.items()},
                          {k: v.copy() for k, v in tr.marginals.items()}, {k: v.copy() for k, v in tr.forecast.items()},
                          {k: v.copy() for k, v in tr.check.items()}, {"rt": tr.rt.copy()},
                          None if tr.wb is None else {k: v.copy() for k, v in tr.wb.items()})
            s.sample_bursts(nb, burst, consume, summarize=True, forecast=True, rt=True, check=True,
                            **(dict(within_between=True) if on else {}))
            cs = s.check_summary()
            runs[on] = (got, s.get_state() + s.get_kernel(), s.summary(), s.forecast_summary(), cs.moments, s.rt_summary(), cs,
                        s.within_between_summary() if on else None)
    from types import SimpleNamespace
    for i in range(nb):
        a, b = (SimpleNamespace(theta=x[0], events=x[1], hmc=x[2], moves=x[3]) for x in (runs[False][0][i], runs[True][0][i]))
        _same_bits(a, b)
        assert runs[False][0][i][8] is None
        for part in (4, 5, 6, 7):
            for k in runs[False][0][i][part]:
                assert np.array_equal(runs[False][0][i][part][k], runs[True][0][i][part][k]), k
    for x, y in zip(runs[False][1], runs[True][1]):
        assert np.array_equal(x, y)
    for which in (2, 3, 4):
        for k in ("count", "ref", "sum", "sumsq"):
            assert np.array_equal(getattr(runs[False][which], k), getattr(runs[True][which], k)), k
    for k in ("count", "ref", "sum", "sumsq", "gt1"):
        assert np.array_equal(getattr(runs[False][5], k), getattr(runs[True][5], k)), k
    for k in ("observed", "lt", "eq", "location_lt", "location_eq", "day_lt", "day_eq", "total_lt", "total_eq"):
        assert np.array_equal(getattr(runs[False][6], k), getattr(runs[True][6], k)), k
    got = runs[True][0]
    theta = np.concatenate([got[i][0] for i in range(nb)])
    fw, fb, I = _reference(api, case, theta, np.concatenate([got[i][1] for i in range(nb)]), Dw)
    _same_acc(runs[True][7], _fold(fw, fb))
    _national(case, theta, I, {k: np.concatenate([got[i][8][k] for i in range(nb)]) for k in got[0][8]})   # the asynchronous reader


def test_a_burst_run_again_after_a_time_out_is_counted_once(api):
    """seir_sampler_debug_fail_handoff (the existing test hook, once) in the middle of overlapped bursts: the burst is
    restored -- the accumulators and count included -- and run again one launch form down."""
    case, u, ev, cfg, eps = _case("micro_20x60", 8)
    B, nb, burst, D = 8, 6, 4, 5
    model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
    with model, s:
        got = {}
        s.reset_within_between(D)

        def consume(tr, i):
            got[i] = (tr.events.copy(), {k: v.copy() for k, v in tr.wb.items()}, tr.theta.copy())
            if i == 1 and not s.recoveries:                    # while burst 2 or 3 is in flight
                _lib.check(s._lib.seir_sampler_debug_fail_handoff(s._s, B - 1))
        s.sample_bursts(nb, burst, consume, within_between=True)
        ws, recoveries = s.within_between_summary(), list(s.recoveries)
    assert len(recoveries) == 1, recoveries
    assert sorted(got) == list(range(nb))
    # the run is held to its own draws: every delivered draw folded once, in order
    theta = np.concatenate([got[i][2] for i in range(nb)])
    fw, fb, I = _reference(api, case, theta, np.concatenate([got[i][0] for i in range(nb)]), D)
    _same_acc(ws, _fold(fw, fb))
    _national(case, theta, I, {k: np.concatenate([got[i][1][k] for i in range(nb)]) for k in got[0][1]})


def test_refusals(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 2)
    T = case["k"].T
    model, s = _sampler(api, case, cfg, u, ev, eps, 4, record_events=False)
    with model, s:
        for call in (lambda: s.reset_within_between(3), lambda: s.within_between(0, 1), lambda: s.read_wb_draws(1),
                     lambda: s.within_between_summary()):
            with pytest.raises(_lib.SeirError, match="record_events=0") as e:
                call()
            assert e.value.code == _lib.ERR_INVALID
    model, s = _sampler(api, case, cfg, u, ev, eps, 4)
    with model, s:
        for call in (lambda: s.within_between(0, 1), lambda: s.read_wb_draws(1), lambda: s.within_between_summary()):
            with pytest.raises(_lib.SeirError, match="seir_sampler_wb_reset") as e:         # before a reset
                call()
            assert e.value.code == _lib.ERR_STATE
        with pytest.raises(ValueError, match="before reset_within_between"):
            s.sample(2, within_between=True)
        for D in (0, T + 1, -1):
            with pytest.raises(ValueError):
                s.reset_within_between(D)
            assert s._lib.seir_sampler_wb_reset(s._s, D) == _lib.ERR_INVALID
        s.reset_within_between(3)
        for first, count in ((-1, 1), (0, 5), (4, 1), (3, 2), (0, -1)):
            calls = [lambda: s.within_between(first, count)]
            if count >= 0:
                calls.append(lambda: s.read_wb_draws(count, first=first))
            for call in calls:
                with pytest.raises(_lib.SeirError) as e:
                    call()
                assert e.value.code == _lib.ERR_INVALID, (first, count)
        tr = s.sample(4, within_between=True)                  # and the sampler is as usable as before
        assert np.array_equal(s.within_between_summary().count, [4, 4]) and tr.wb["within_pressure"].shape == (4, 2, 3)


# ---- CLI end to end -------------------------------------------------------------------------------------------------------
PLAIN = {"initial_state", "time"} | {f"samples/{k}" for k in ("psi", "sigma_space", "beta_area", "gamma0", "gamma1", "alpha_0",
                                                                  "alpha_t", "spatial_effect", "seir")} | \
    {f"results/hmc/{k}" for k in ("is_accepted", "target_log_prob", "step_size")} | \
    {f"results/{m}/{k}" for m in inf.MOVE_KEYS for k in ("is_accepted", "target_log_prob", "proposed_delta")}


def test_cli_within_between(api, tmp_path):
    """`--within-between 7` on an NI-11 data set: the group and the two per-draw datasets, equal to the stateless kernel on the
    file's own draws, and the csv tool on the file; `--summaries only --thin 2 --forecast 7 --rt 7 --check 7
    --within-between 7` works without samples/seir; without the flag the file has exactly the datasets of a run before the
    option existed."""
    from covid19uk_amd.sampler import summary_var, wb_mean
    tmp_path = str(tmp_path)
    cov = synth.make_covariates("ni11")
    events, init, _ = synth.simulate_epidemic(cov)
    data = os.path.join(tmp_path, "data.npz")
    inf.write_inference_data(data, cov, events[..., 2])
    wb_path, wb_log = _cli(tmp_path, "wb", data, ["--within-between", "7"])
    wb = _datasets(wb_path)
    both = _datasets(_cli(tmp_path, "both", data, ["--summaries", "only", "--thin", "2", "--forecast", "7", "--rt", "7",
                                                   "--check", "7", "--within-between", "7"])[0])
    plain_path, plain_log = _cli(tmp_path, "plain", data, [])
    plain = _datasets(plain_path)
    new = {f"within_between/{k}" for k in ("days", "first_day", "count", "defined", "within_mean", "within_var", "between_mean",
                                           "p_within_gt_between")} | {"samples/within_pressure", "samples/between_pressure"}
    assert set(plain) == PLAIN and "Within/between" not in plain_log
    assert set(wb) == PLAIN | new
    for k in plain:
        if plain[k].dtype.kind in "fiub":
            assert np.array_equal(plain[k], wb[k], equal_nan=plain[k].dtype.kind == "f"), k
    M, T, D, ns = cov.M, cov.T, 7, 2 * 6
    assert "samples/seir" not in both and new <= set(both)
    assert all(f"{g}/count" in both for g in ("forecast", "summaries", "rt", "check"))
    for f in (wb, both):
        for k in ("within_pressure", "between_pressure"):
            assert f[f"samples/{k}"].shape == (ns, D) and f[f"samples/{k}"].dtype == np.float64 and np.all(f[f"samples/{k}"] > 0.0)
        g = {k: f[f"within_between/{k}"] for k in ("days", "first_day", "count")}
        assert g["days"].reshape(-1)[0] == D and g["first_day"].reshape(-1)[0] == T - D and g["count"].reshape(-1)[0] == ns
        for k in ("defined", "within_mean", "within_var", "between_mean", "p_within_gt_between"):
            assert f[f"within_between/{k}"].shape == (D, M) and np.all(np.isfinite(f[f"within_between/{k}"]))
    assert wb_log.count("Within/between:") == 1 and f"window of {D} day(s) from day {T - D}" in wb_log
    # the reference from the file's own draws: the sampling phase is the last ns rows
    cov2, _, _ = inf.read_inference_data(data)
    case = dict(cov=cov2, init=wb["initial_state"], k=H.oracle_constants(cov2, wb["initial_state"]))
    theta = wb["samples/psi"][-ns:].reshape(ns, 1, 1)
    fw, fb, I = _reference(api, case, theta, wb["samples/seir"][-ns:][:, None], D)
    want = _fold(fw, fb)
    assert np.array_equal(wb["within_between/defined"], want["defined"][0])
    assert np.array_equal(wb["within_between/within_mean"], wb_mean(want["defined"][0], want["ref_w"][0], want["sum_w"][0]))
    assert np.array_equal(wb["within_between/within_var"], summary_var(want["defined"][0], want["sum_w"][0], want["sumsq_w"][0]))
    assert np.array_equal(wb["within_between/between_mean"], wb_mean(want["defined"][0], want["ref_b"][0], want["sum_b"][0]))
    assert np.array_equal(wb["within_between/p_within_gt_between"], wb_mean(want["defined"][0], 0.0, want["gt"][0]))
    _national(case, theta, I, {k: wb[f"samples/{k}"][:, None] for k in ("within_pressure", "between_pressure")})
    # the csv from the file alone: the reference's columns for the last day
    out = os.path.join(tmp_path, "wb.csv")
    rows = wbtool.main(["--posterior", wb_path, "-o", out])
    dfn = wb["within_between/defined"][-1]
    cols = [wb[f"within_between/{k}"][-1] for k in ("within_mean", "between_mean", "p_within_gt_between")]
    # one file: the pooled value is defined x value / defined, two roundings away from the value itself
    assert np.array_equal(rows, np.stack([dfn * c / dfn for c in cols], axis=1))
    np.testing.assert_allclose(rows, np.stack(cols, axis=1), rtol=2.0 ** -51, atol=0.0)
    assert len(open(out).read().splitlines()) == M + 1

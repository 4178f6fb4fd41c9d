"""Convergence diagnostics on the device (include/seir_hip.h, "Convergence diagnostics"; the DIAG instance of k_summarize
in covid19uk_amd/csrc/summary_kernels.h): batch sums and marks next to the moments.

The oracle is NumPy on the recorded events of the same run, as in tests/test_summary_gpu.py: the six quantities are formed
from `tr.events` with `model_spec.compute_state`, and `tests.test_diagnostics_host.accumulate` restates the accumulators'
definitions in int64.  The device's arithmetic is integer arithmetic: every comparison with it is `np.array_equal`."""
import os

import numpy as np
import pytest

from covid19uk_amd import _lib, synth
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.posterior import diagnostics as dm
from tests import helpers as H
from tests.test_diagnostics_host import accumulate, same_accumulators
from tests.test_recovery_gpu import _case, _same_bits
from tests.test_sampler_gpu import CFG_REF, CFG_SMALL, api  # noqa: F401  (fixture)
from tests.test_summary_gpu import MARG, _cli, _datasets, _quantities, _sampler

pytestmark = pytest.mark.gpu


def _chain(dg, b):
    """Chain b of a `Diagnostics` as one of its own."""
    return dm.Diagnostics(dg.batch_length, *(getattr(dg, f)[b:b + 1] for f in ("count", "ref", "sum", "sumsq", "bsum", "bsumsq", "nbatch")),
                          *(getattr(dg, f)[:, b:b + 1] for f in ("mark_count", "mark_sum", "mark_sumsq")))


def _equals_numpy(dg, events, init, L, marks):
    """events [n, B, M, T, 3] recorded -> every accumulator of `dg` equals the restatement, chain by chain (UK-380 x 100
    draws is 0.7 GB of int64 per chain)."""
    assert dg.batch_length == L
    for b in range(events.shape[1]):
        x = _quantities(events[:, b], init)[:, None]
        assert int(np.abs(x - x[:1]).max()) ** 2 * len(x) ** 2 < 2 ** 62         # int64 holds the squared batch sums
        same_accumulators(_chain(dg, b), accumulate(x, L, marks))


def _three_bursts(s, n, L):
    """reset, three bursts of n draws with mark 0 behind the first and mark 1 behind the second."""
    s.reset_diagnostics(L)
    evs = []
    for i in range(3):
        evs.append(s.sample(n, summarize=True).events.copy())
        if i < 2:
            s.mark(i)
    return np.concatenate(evs), s.diagnostics(), {n: 0, 2 * n: 1}


# the case ids name the branch of k_summarize they turn
CASES = {
    "T=1": ("micro_3x1", CFG_SMALL, 0.002, 3, True, 4),
    "M=1": ("micro_1x70", CFG_SMALL, 0.002, 1, "u16", 6),
    # one day chunk exactly / one day past it; one row past and one short of the 8-row block of a workgroup
    "T=64,M=rowblock+1": ("micro_9x64", CFG_SMALL, 0.0004, 3, "u16", 8),
    "T=65,M=rowblock-1": ("micro_7x65", CFG_SMALL, 0.0004, 8, True, 8),
    "M=65": ("micro_65x70", CFG_SMALL, 0.0001, 1, "u16", 8),
    "T=365,int32": ("uk380", CFG_REF, 1.2e-5, 1, True, 6),
}


@pytest.mark.parametrize("case_id", list(CASES))
def test_accumulators_and_marks_equal_numpy_on_the_recorded_events(api, case_id):
    """Batches of 1, 7, a burst and two bursts over three bursts: with 7 and with two bursts the run ends inside an open
    batch, with two bursts a batch spans calls."""
    name, cfg, eps, B, record, n = CASES[case_id]
    case = H.build_case(name, 43, alpha_t_sd=0.005)
    u = synth.jitter_params(case["u"], B, scale=0.002 if name == "uk380" else 0.01, seed=3, T=case["k"].T)
    ev = np.stack([case["events"]] * B)
    model, s = _sampler(api, case, cfg, u, ev, eps, n, record_events=record)
    with model, s:
        moved = False
        for L in (1, 7, n, 2 * n):
            events, dg, marks = _three_bursts(s, n, L)
            assert events.dtype == (np.uint16 if record == "u16" else np.int32)
            assert dg.bsum.dtype == np.int64 and dg.bsumsq.dtype == np.uint64 and dg.nbatch.dtype == np.uint64
            assert np.array_equal(dg.nbatch, np.full(B, 3 * n // L)) and np.array_equal(dg.mark_count, [[n] * B, [2 * n] * B])
            _equals_numpy(dg, events, case["init"], L, marks)
            if (3 * n) % L:
                moved |= bool(dg.bsum.any())
            moved |= bool((events != events[:1]).any())
        if case["k"].T >= 64 and case["k"].M > 1:
            assert moved, "no event update was accepted: all draws equal"
        assert not s.pair_timeouts().any()


@pytest.mark.parametrize("record,B", [("u16", 8), (True, 2)], ids=["uint16-x8", "int32-x2"])
def test_uk380_100_draws(api, record, B):
    """The size users run: one 100-draw burst at UK-380, folded in two calls with mark 0 between them; batches of 7 leave two
    draws in the open batch.  8 chains with the uint16 trace, the trace of a run at this size; the int32 trace with 2 chains,
    which keeps the NumPy restatement (0.7 GB of int64 per chain) to a few seconds -- the int32 instance at T = 365 is in
    CASES above as well."""
    name, n, L = "uk380", 100, 7
    case = H.build_case(name, 43, alpha_t_sd=0.005)
    u = synth.jitter_params(case["u"], B, scale=0.002, seed=3, T=case["k"].T)
    ev = np.stack([case["events"]] * B)
    model, s = _sampler(api, case, CFG_REF, u, ev, 1.2e-5, n, record_events=record)
    with model, s:
        s.reset_diagnostics(L)
        s.reset_trace()
        s.run(n)
        s.summarize(0, 50)
        s.mark(0)
        s.summarize(50, 50)
        tr = s.read_trace(n)
        dg = s.diagnostics()
        assert (tr.events != tr.events[:1]).any() and dg.bsumsq.any() and dg.bsum.any()
        _equals_numpy(dg, tr.events, case["init"], L, {50: 0})
        assert np.array_equal(dg.nbatch, np.full(B, 14))
        ess, rhat = dg.ess, dg.rhat                                   # the formulas hold up on a real latent tensor: no warning
        live = ~np.isnan(rhat)
        assert live.any() and (rhat[live] > 0.5).all() and np.isfinite(ess[~np.isnan(ess)]).any()


def test_the_summaries_and_the_chain_do_not_notice(api):
    """Overlapped bursts with the diagnostics on, with the summaries alone, and with neither: draws bit for bit; moments and
    marginals of the two summarised runs equal."""
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    nb, burst = 4, 5
    runs = {}
    for mode in ("none", "summaries", "diagnostics"):
        model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
        with model, s:
            got = {}

            def consume(tr, i, got=got):
                got[i] = (tr.theta.copy(), tr.events.copy(), {k: v.copy() for k, v in tr.hmc.items()},
                          {mk: {kk: v.copy() for kk, v in mv.items()} for mk, mv in tr.moves.items()},
                          None if tr.marginals is None else {k: v.copy() for k, v in tr.marginals.items()})
            if mode == "diagnostics":
                s.reset_diagnostics(burst)
                s.sample_bursts(nb, burst, consume, summarize=True, marks=inf.diagnostics_marks(nb))
            else:
                s.sample_bursts(nb, burst, consume, summarize=mode == "summaries")
            runs[mode] = (got, s.get_state() + s.get_kernel(), None if mode == "none" else s.summary(),
                          s.diagnostics() if mode == "diagnostics" else None)
    from types import SimpleNamespace
    for other in ("summaries", "diagnostics"):
        for i in range(nb):
            a, b = (SimpleNamespace(theta=x[0], events=x[1], hmc=x[2], moves=x[3]) for x in (runs["none"][0][i], runs[other][0][i]))
            _same_bits(a, b)
        for x, y in zip(runs["none"][1], runs[other][1]):
            assert np.array_equal(x, y)
    sm, sd = runs["summaries"][2], runs["diagnostics"][2]
    for f in ("count", "ref", "sum", "sumsq"):
        assert np.array_equal(getattr(sm, f), getattr(sd, f)), f
    for i in range(nb):
        for k in MARG:
            assert np.array_equal(runs["summaries"][0][i][4][k], runs["diagnostics"][0][i][4][k]), (i, k)
    events = np.concatenate([runs["diagnostics"][0][i][1] for i in range(nb)])
    assert (events != events[:1]).any()
    _equals_numpy(runs["diagnostics"][3], events, case["init"], burst, {2 * burst: 0})


def test_cutting_a_burst_into_calls_or_buffer_halves_does_not_matter(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    n, L = 11, 3
    model, s = _sampler(api, case, cfg, u, ev, eps, 2 * n)
    with model, s:
        # two bursts in the two halves of the buffer, each folded behind its sweeps, mark 0 between them
        s.reset_diagnostics(L)
        for first in (0, n):
            s.reset_trace(at=first)
            s.run(n)
            s.summarize(first, n)
            if first == 0:
                s.mark(0)
        tr = s.read_trace(2 * n)
        halves = s.diagnostics()
        assert (tr.events != tr.events[:1]).any()
        _equals_numpy(halves, tr.events, case["init"], L, {n: 0})
        assert halves.bsum.any() and halves.bsumsq.any()                  # 22 draws: 7 batches and one draw in the open one
        # the same slots in pieces, one of them a single slot, batches closing inside and at the ends of calls
        s.reset_diagnostics(L)
        for first, count in ((0, 3), (3, 1), (4, 7)):
            s.summarize(first, count)
        s.mark(0)
        for first, count in ((11, 2), (13, 2 * n - 13)):
            s.summarize(first, count)
        same_accumulators(s.diagnostics(), halves)
        # a call that folds nothing (marginals only) leaves the batch sums alone; reset_summary starts them again too
        s.summarize(0, 5, accumulate=False)
        same_accumulators(s.diagnostics(), halves)
        s.reset_summary()
        dg = s.diagnostics()
        assert not any(getattr(dg, f).any() for f in ("count", "sum", "sumsq", "bsum", "bsumsq", "nbatch", "mark_count", "mark_sum", "mark_sumsq"))
        s.summarize(2, 9)
        _equals_numpy(s.diagnostics(), tr.events[2:11], case["init"], L, {})


def test_a_call_longer_than_one_launch_holds(api):
    """More draws than one k_summarize launch takes (128), a batch length that straddles the cut."""
    case, u, ev, cfg, eps = _case("micro_5x24", 2)
    n, L = 150, 9
    model, s = _sampler(api, case, cfg, u, ev, 0.002, n)
    with model, s:
        s.reset_diagnostics(L)
        tr = s.sample(n, summarize=True)
        _equals_numpy(s.diagnostics(), tr.events, case["init"], L, {})


def test_with_thinning_the_batches_are_of_kept_draws(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 4)
    n, k = 6, 3
    model, s = _sampler(api, case, cfg, u, ev, eps, n, thin=k)
    with model, s:
        kept, dg, marks = _three_bursts(s, n, 4)
    model, s = _sampler(api, case, cfg, u, ev, eps, 3 * n * k)
    with model, s:
        every = s.sample(3 * n * k)
    assert np.array_equal(every.events[k - 1::k], kept) and (kept != kept[:1]).any()
    _equals_numpy(dg, every.events[k - 1::k], case["init"], 4, marks)


@pytest.mark.parametrize("skew", [2])
def test_diagnostics_do_not_depend_on_workgroup_timing(api, skew):
    """SEIR_OPT_DEBUG_SKEW delays a third of the workgroups of every launch: the same integers."""
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    res = {}
    for sk in (0, skew):
        model, s = _sampler(api, case, cfg, u, ev, eps, 6, skew=sk, record_events="u16")
        with model, s:
            res[sk] = _three_bursts(s, 6, 4)
    assert np.array_equal(res[0][0], res[skew][0])
    same_accumulators(res[skew][1], res[0][1])
    _equals_numpy(res[skew][1], res[0][0], case["init"], 4, res[0][2])


@pytest.mark.parametrize("fail_at", [0, 2])
def test_a_time_out_before_or_after_a_mark_changes_nothing(api, fail_at):
    """seir_sampler_debug_fail_handoff (the existing test hook, once) while overlapped bursts with marks are in flight: seven
    bursts, mark 0 behind burst 2 and mark 1 behind burst 3.  Raised while burst 0 is consumed it hits burst 1 or 2 -- before
    mark 0 or the burst that carries it; while burst 2 is consumed, burst 3 or 4 -- behind mark 0, mark 1's burst or the one
    after.  The burst is restored, accumulators and marks included, and run again: everything equals the undisturbed run."""
    case, u, ev, cfg, eps = _case("micro_20x60", 8)
    B, nb, burst, L = 8, 7, 4, 3
    marks = inf.diagnostics_marks(nb)
    assert marks == {2: 0, 3: 1}
    runs = {}
    for disturb in (False, True):
        model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
        with model, s:
            got = {}

            def consume(tr, i, got=got, s=s, disturb=disturb):
                got[i] = tr.events.copy()
                if disturb and i == fail_at and not s.recoveries:
                    _lib.check(s._lib.seir_sampler_debug_fail_handoff(s._s, B - 1))
            s.reset_diagnostics(L)
            s.sample_bursts(nb, burst, consume, summarize=True, marks=marks)
            runs[disturb] = (got, s.diagnostics(), list(s.recoveries))
    ref, got = runs[False], runs[True]
    assert not ref[2] and len(got[2]) == 1, got[2]
    assert sorted(got[0]) == list(range(nb))
    for i in range(nb):
        assert np.array_equal(ref[0][i], got[0][i]), i
    same_accumulators(got[1], ref[1])
    _equals_numpy(got[1], np.concatenate([ref[0][i] for i in range(nb)]), case["init"], L, {3 * burst: 0, 4 * burst: 1})
    assert np.array_equal(got[1].half_count, np.full((2, B), 3 * burst))


def test_a_reset_drops_what_earlier_snapshots_hold_of_the_accumulators(api):
    """The batch length is no part of a snapshot: one taken under L = 2 and restored after a reset to L = 3 brings the chain
    back and leaves moments, batch sums and marks as the draws folded under L = 3 made them."""
    case, u, ev, cfg, eps = _case("micro_20x60", 2)
    n = 5
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        s.reset_diagnostics(2)
        s.sample(n, summarize=True)
        s.mark(0)
        s.snapshot(1)                                              # slot 0 is `sample`'s own
        s.reset_diagnostics(3)
        tr = s.sample(n, summarize=True)
        before = s.diagnostics()
        s.restore(1)
        after = s.diagnostics()
        assert after.batch_length == 3 and (tr.events != tr.events[:1]).any()
        same_accumulators(after, before)
        _equals_numpy(after, tr.events, case["init"], 3, {})
        assert np.array_equal(s.sample(n).events, tr.events)       # the chain itself did go back


def test_refusals(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 2)
    model, s = _sampler(api, case, cfg, u, ev, eps, 4, record_events=False)
    with model, s:
        for call in (lambda: s.reset_diagnostics(2), lambda: s.mark(0), lambda: s.diagnostics()):
            with pytest.raises(_lib.SeirError) as e:
                call()
            assert e.value.code == _lib.ERR_STATE
    model, s = _sampler(api, case, cfg, u, ev, eps, 4)
    with model, s:
        for call in (lambda: s.mark(0), lambda: s.diagnostics()):
            with pytest.raises(_lib.SeirError, match="seir_sampler_diag_reset") as e:     # before a reset
                call()
            assert e.value.code == _lib.ERR_STATE
        s.reset_summary()                                          # the summaries alone do not enable them
        with pytest.raises(_lib.SeirError, match="seir_sampler_diag_reset"):
            s.mark(1)
        for bad in (0, -1):
            assert s._lib.seir_sampler_diag_reset(s._s, bad) == _lib.ERR_INVALID
            with pytest.raises(ValueError):
                s.reset_diagnostics(bad)
        s.reset_diagnostics(2)
        for which in (-1, 2):
            with pytest.raises(_lib.SeirError) as e:
                s.mark(which)
            assert e.value.code == _lib.ERR_INVALID
            assert s._lib.seir_sampler_read_diag_mark(s._s, which, None, None, None) == _lib.ERR_INVALID
        s.sample(4, summarize=True)                                # and the sampler is as usable as before
        dg = s.diagnostics()
        assert np.array_equal(dg.count, [4, 4]) and np.array_equal(dg.nbatch, [2, 2])


# ---- CLI end to end -------------------------------------------------------------------------------------------------------
def _chain_files(out):
    root, ext = os.path.splitext(out)
    return [f"{root}_chain{c}{ext}" for c in range(2)]


def test_cli_diagnostics_on_with_summaries_off_and_only(api, tmp_path, capsys):
    """`--diagnostics on --chains 2` on an NI-11 data set (2 bursts of 6 draws): the group's datasets and shapes; with
    `--summaries off`, R-hat and ESS in the files equal this module's functions on the files' own samples/*; with `only` the
    event tensors never left the device and the group equals the other run's (same seed); the pooling tool runs on both."""
    tmp_path = str(tmp_path)
    cov = synth.make_covariates("ni11")
    events, init, _ = synth.simulate_epidemic(cov)
    data = os.path.join(tmp_path, "data.npz")
    inf.write_inference_data(data, cov, events[..., 2])
    M, T = cov.M, cov.T
    P = 6 + T - 1 + M
    out, log = _cli(tmp_path, "off", data, ["--diagnostics", "on", "--summaries", "off", "--chains", "2"])
    off = [_datasets(f) for f in _chain_files(out)]
    out_only, _ = _cli(tmp_path, "only", data, ["--diagnostics", "on", "--summaries", "only", "--chains", "2"])
    only = [_datasets(f) for f in _chain_files(out_only)]
    plain = [_datasets(f) for f in _chain_files(_cli(tmp_path, "plain", data, ["--chains", "2"])[0])]
    assert "diagnostics: " in log and "R-hat" in log and "smallest ESS" in log
    group = {f"diagnostics/{k}" for k in dm.NAMES}
    shapes = {"count": (1,), "batch_length": (1,), "num_batches": (1,), "half_count": (2,), "theta_half_mean": (2, P),
              "theta_half_var": (2, P), "theta_ess": (P,), "theta_rhat": (P,)}
    for k in ("seir", "state"):
        shapes.update({f"{k}_half_mean": (2, M, T, 3), f"{k}_half_var": (2, M, T, 3), f"{k}_ess": (M, T, 3), f"{k}_rhat": (M, T, 3)})
    for c in range(2):
        assert set(off[c]) == set(plain[c]) | group             # summaries off: nothing else is added
        assert "samples/seir" not in only[c] and "summaries/seir_mean" in only[c] and group <= set(only[c])
        for k, shp in shapes.items():
            assert off[c][f"diagnostics/{k}"].shape == shp and off[c][f"diagnostics/{k}"].dtype == np.float64, k
            assert np.array_equal(off[c][f"diagnostics/{k}"], only[c][f"diagnostics/{k}"], equal_nan=True), k
        d = off[c]
        assert d["diagnostics/count"][0] == 12 and d["diagnostics/batch_length"][0] == 6 and d["diagnostics/num_batches"][0] == 2
        assert np.array_equal(d["diagnostics/half_count"], [6, 6])
    # the module's functions on the run's own draws, read back from samples/*
    n = off[0]["samples/seir"].shape[0]
    seir = np.stack([off[c]["samples/seir"][n - 12:] for c in range(2)], axis=1)          # [12, 2, M, T, 3]
    assert np.array_equal(seir, np.rint(seir)) and (seir != seir[:1]).any()
    x = np.stack([_quantities(seir[:, c].astype(np.int64), off[c]["initial_state"]) for c in range(2)], axis=1)
    lat = accumulate(x, 6, {6: 0})
    theta = np.stack([np.concatenate([off[c][f"samples/{k}"][n - 12:].reshape(12, -1) for k in
                                      ("psi", "sigma_space", "beta_area", "gamma0", "gamma1", "alpha_0", "alpha_t", "spatial_effect")],
                                     axis=1) for c in range(2)], axis=1)                   # [12, 2, P]
    assert theta.shape == (12, 2, P)
    acc = dm.DrawAccumulator(6)
    acc.fold(theta[:6])
    acc.mark(0)
    acc.fold(theta[6:])
    ev = dm.evaluate(lat, acc.result())
    for c in range(2):
        want = dm.chain_datasets(ev, c)
        for k in dm.NAMES:
            assert np.array_equal(off[c][f"diagnostics/{k}"], want[k], equal_nan=True), (c, k)
    assert np.isfinite(off[0]["diagnostics/theta_rhat"]).all() and np.isfinite(off[0]["diagnostics/seir_rhat"]).any()
    # the pooling tool, on the files that have no samples/seir too
    for files, tag in ((_chain_files(out), "off"), (_chain_files(out_only), "only")):
        pooled = dm.main(files + ["-o", os.path.join(tmp_path, f"pooled_{tag}.hd5")])
        assert "2 chain(s): diagnostics:" in capsys.readouterr().out
        for k in ("seir", "state", "theta"):                    # the two chains of the process are all the chains there are
            assert np.array_equal(pooled[f"{k}_rhat"], off[0][f"diagnostics/{k}_rhat"], equal_nan=True), k
        assert np.array_equal(_datasets(os.path.join(tmp_path, f"pooled_{tag}.hd5"))["theta_rhat"], pooled["theta_rhat"])

"""Summaries of the recorded latent epidemic on the device (include/seir_hip.h, "Summaries of samples/seir on the device";
covid19uk_amd/csrc/summary_kernels.h): per-cell moments of event counts and state over the kept draws, and per-draw marginals.

The oracle is NumPy on the recorded events of the same run: `tr.events` is read back, `model_spec.compute_state` applied
with the context's initial state, and the sums formed in int64 (the quantities are below 2^31 and a burst has at most a
few hundred draws, so int64 holds every sum; `_oracle` checks that with Python integers).  The device's arithmetic is
integer arithmetic too, so every comparison of device results here is `np.array_equal`.  (The one `assert_allclose` of this
file checks the host's float64 formula for mean and variance against NumPy's, after the integers have been compared.)"""
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

from covid19uk_amd import _lib, hdf5io, synth
from covid19uk_amd import model_spec as ms
from covid19uk_amd.inference import inference as inf
from tests import helpers as H
from tests.test_recovery_gpu import _case, _same_bits
from tests.test_sampler_gpu import CFG_REF, CFG_SMALL, api  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARG = ("events_by_day", "events_by_location", "state_by_day")


def _quantities(events, init):
    """events [n, M, T, 3] of one chain -> the six quantities [n, M, T, 6] int64 (k_se, k_ei, k_ir, S, E, I)."""
    ev = events.astype(np.int64)
    st = ms.compute_state(init, ev)[..., :3]
    assert np.array_equal(st, np.rint(st)) and np.abs(st).max() < 2.0 ** 52
    return np.concatenate([ev, st.astype(np.int64)], axis=-1)


def _oracle(events, init, folds=None):
    """events [n, B, M, T, 3] -> moments over the draws `folds` (a slice / index list; None: all) and marginals of every draw."""
    n, B = events.shape[:2]
    out = dict(count=np.zeros(B, np.uint64), ref=[], sum=[], sumsq=[], events_by_day=[], events_by_location=[],
               state_by_day=[])
    for b in range(B):                                    # chain by chain: UK-380 x 100 draws is 0.7 GB of int64 per chain
        x = _quantities(events[:, b], init)
        out["events_by_day"].append(x[..., :3].sum(axis=1))
        out["events_by_location"].append(x[..., :3].sum(axis=2))
        out["state_by_day"].append(x[..., 3:].sum(axis=1))
        f = x if folds is None else x[folds]
        out["count"][b] = len(f)
        d = f - f[0]
        assert int(np.abs(d).max()) ** 2 * len(f) < 2 ** 62      # int64 holds the sums
        out["ref"].append(f[0].astype(np.int32))
        out["sum"].append(d.sum(axis=0))
        out["sumsq"].append((d * d).sum(axis=0).astype(np.uint64))
    for k in ("ref", "sum", "sumsq"):
        out[k] = np.stack(out[k])
    for k in MARG:
        out[k] = np.stack(out[k], axis=1)
    return out


def _same_moments(sm, want):
    assert sm.count.dtype == np.uint64 and sm.ref.dtype == np.int32 and sm.sum.dtype == np.int64 and sm.sumsq.dtype == np.uint64
    assert np.array_equal(sm.count, want["count"])
    assert np.array_equal(sm.ref, want["ref"])
    assert np.array_equal(sm.sum, want["sum"])
    assert np.array_equal(sm.sumsq, want["sumsq"])


def _same_marginals(m, want, rows=slice(None)):
    for k in MARG:
        assert m[k].dtype == np.int64
        assert np.array_equal(m[k], want[k][rows]), k


def _sampler(api, case, cfg, u, ev, eps, cap, seed=13, skew=0, **kw):
    model = api[0](case["cov"], case["init"], max_chains=u.shape[0])
    if skew:
        model.set_option(debug_skew=skew)
    s = api[1](model, cfg, u.shape[0], seed=seed, trace_capacity=cap, **kw)
    s.set_state(u, ev)
    s.set_kernel(step_size=eps)
    return model, s


# the case ids name the branch of k_summarize they turn
CASES = {
    # degenerate shapes, for the indexing (exempt from the "something moved" condition)
    "T=1": ("micro_3x1", CFG_SMALL, 0.002, 2, True, 4),
    "M=1": ("micro_1x70", CFG_SMALL, 0.002, 3, "u16", 6),
    # one day chunk exactly / one day past it; one row short of and one past the 8-row block of a workgroup
    "T=64,M=rowblock+1": ("micro_9x64", CFG_SMALL, 0.0004, 3, "u16", 8),
    "T=65,M=rowblock-1": ("micro_7x65", CFG_SMALL, 0.0004, 8, True, 8),
    "M=65": ("micro_65x70", CFG_SMALL, 0.0001, 1, "u16", 8),
    "M=520": ("slow_520x70", CFG_SMALL, 3e-5, 2, True, 6),
    "T=800": ("slower_4x800", CFG_REF, 3e-5, 3, True, 8),
    "T=800,u16": ("slower_4x800", CFG_REF, 3e-5, 1, "u16", 8),
    # the size users run: a 100-draw burst of 8 chains at UK-380 (T = 365), and one chain
    "uk380x8,100": ("uk380", CFG_REF, 1.2e-5, 8, "u16", 100),
    "uk380x1,int32": ("uk380", CFG_REF, 1.2e-5, 1, True, 12),
}


@pytest.mark.parametrize("case_id", list(CASES))
def test_moments_and_marginals_equal_numpy_on_the_recorded_events(api, case_id):
    name, cfg, eps, B, record, n = CASES[case_id]
    case = H.build_case(name, 43, alpha_t_sd=0.005)
    u = synth.jitter_params(case["u"], B, scale=0.002 if name == "uk380" else 0.01, seed=3, T=case["k"].T)
    ev = np.stack([case["events"]] * B)
    model, s = _sampler(api, case, cfg, u, ev, eps, n, record_events=record)
    with model, s:
        tr = s.sample(n, summarize=True)                      # a full burst in one call
        sm = s.summary()
        assert tr.events.dtype == (np.uint16 if record == "u16" else np.int32)
        if case["k"].T >= 64 and case["k"].M > 1:
            assert any(tr.moves[k]["is_accepted"].any() for k in tr.moves), "no event update was accepted: all draws equal"
            assert (tr.events != tr.events[:1]).any()
        want = _oracle(tr.events, case["init"])
        _same_moments(sm, want)
        _same_marginals(tr.marginals, want)
        # count = 1: the last slot alone, after a reset, becomes ref
        s.reset_summary()
        s.summarize(n - 1, 1)
        one = _oracle(tr.events, case["init"], folds=slice(n - 1, n))
        _same_moments(s.summary(), one)
        assert not s.summary().sum.any() and not s.summary().sumsq.any()
        _same_marginals(s.read_marginals(1, first=n - 1), want, slice(n - 1, n))
        assert not s.pair_timeouts().any()


def test_cutting_a_burst_into_calls_or_buffer_halves_does_not_matter(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    n = 11
    model, s = _sampler(api, case, cfg, u, ev, eps, 2 * n)
    with model, s:
        # two bursts in the two halves of the buffer, each summarised behind its sweeps
        s.reset_summary()
        for first in (0, n):
            s.reset_trace(at=first)
            s.run(n)
            s.summarize(first, n)
        tr = s.read_trace(2 * n)
        halves, marg = s.summary(), s.read_marginals(2 * n)
        want = _oracle(tr.events, case["init"])
        assert (tr.events != tr.events[:1]).any()
        _same_moments(halves, want)
        _same_marginals(marg, want)
        # one call over everything
        s.reset_summary()
        s.summarize(0, 2 * n)
        _same_moments(s.summary(), want)
        _same_marginals(s.read_marginals(2 * n), want)
        # pieces, one of them a single slot
        s.reset_summary()
        for first, count in ((0, 3), (3, 1), (4, 9), (13, 2 * n - 13)):
            s.summarize(first, count)
        _same_moments(s.summary(), want)
        _same_marginals(s.read_marginals(2 * n), want)


def test_a_call_longer_than_one_launch_holds(api):
    """More draws than one k_summarize launch takes (128): the host cuts the call, the integers are the same."""
    case, u, ev, cfg, eps = _case("micro_5x24", 2)
    n = 150
    model, s = _sampler(api, case, cfg, u, ev, 0.002, n)
    with model, s:
        tr = s.sample(n, summarize=True)
        want = _oracle(tr.events, case["init"])
        _same_moments(s.summary(), want)
        _same_marginals(tr.marginals, want)


def test_accumulate_0_writes_marginals_only_and_reset_starts_again(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 3)
    n = 8
    model, s = _sampler(api, case, cfg, u, ev, eps, n)
    with model, s:
        tr = s.sample(n, summarize="marginals")
        want = _oracle(tr.events, case["init"])
        _same_marginals(tr.marginals, want)
        sm = s.summary()
        assert not sm.count.any() and not sm.ref.any() and not sm.sum.any() and not sm.sumsq.any()
        s.summarize(0, 5)                                      # folds draws 0..4
        five = _oracle(tr.events, case["init"], folds=slice(0, 5))
        _same_moments(s.summary(), five)
        s.summarize(5, 3, accumulate=False)                    # marginals again; accumulators and count stay
        _same_moments(s.summary(), five)
        _same_marginals(s.read_marginals(n), want)
        s.reset_summary()
        sm = s.summary()
        assert not sm.count.any() and not sm.ref.any() and not sm.sum.any() and not sm.sumsq.any()
        s.summarize(2, 4)                                      # after a reset the next draw folded becomes ref
        late = _oracle(tr.events, case["init"], folds=slice(2, 6))
        assert np.array_equal(late["ref"], _oracle(tr.events[2:3], case["init"])["ref"])
        _same_moments(s.summary(), late)


@pytest.mark.parametrize("k", [3])
def test_with_thinning_the_summary_is_over_the_kept_draws(api, k):
    case, u, ev, cfg, eps = _case("micro_20x60", 4)
    n = 6
    model, s = _sampler(api, case, cfg, u, ev, eps, n, thin=k)
    with model, s:
        kept = s.sample(n, summarize=True)
        sm = s.summary()
    model, s = _sampler(api, case, cfg, u, ev, eps, n * k)
    with model, s:
        every = s.sample(n * k)
    assert np.array_equal(every.events[k - 1::k], kept.events)
    want = _oracle(every.events[k - 1::k], case["init"])
    _same_moments(sm, want)
    _same_marginals(kept.marginals, want)


def test_the_chain_does_not_notice_being_summarised(api):
    """A sampler that summarises every burst against one that never does: traces bit for bit, final state and kernel."""
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    nb, burst = 4, 5
    runs = {}
    for summarize in (False, True):
        model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
        with model, s:
            got = {}

            def consume(tr, i, got=got):
                got[i] = (tr.theta.copy(), tr.events.copy(), {k: v.copy() for k, v in tr.hmc.items()},
                          {mk: {kk: v.copy() for kk, v in mv.items()} for mk, mv in tr.moves.items()},
                          None if tr.marginals is None else {k: v.copy() for k, v in tr.marginals.items()})
            s.sample_bursts(nb, burst, consume, summarize=summarize)
            runs[summarize] = (got, s.get_state() + s.get_kernel(), s.summary() if summarize else None)
    from types import SimpleNamespace
    for i in range(nb):
        a, b = (SimpleNamespace(theta=x[0], events=x[1], hmc=x[2], moves=x[3]) for x in (runs[False][0][i], runs[True][0][i]))
        _same_bits(a, b)
        assert runs[False][0][i][4] is None
    for x, y in zip(runs[False][1], runs[True][1]):
        assert np.array_equal(x, y)
    events = np.concatenate([runs[True][0][i][1] for i in range(nb)])
    want = _oracle(events, case["init"])
    _same_moments(runs[True][2], want)
    _same_marginals({k: np.concatenate([runs[True][0][i][4][k] for i in range(nb)]) for k in MARG}, want)


@pytest.mark.parametrize("skew", [1, 2, 3])
def test_summaries_do_not_depend_on_workgroup_timing(api, skew):
    """SEIR_OPT_DEBUG_SKEW delays a third of the workgroups of every launch: the same integers."""
    case, u, ev, cfg, eps = _case("micro_20x60", 5)
    n = 6
    res = {}
    for sk in (0, skew):
        model, s = _sampler(api, case, cfg, u, ev, eps, n, skew=sk, record_events="u16")
        with model, s:
            tr = s.sample(n, summarize=True)
            res[sk] = (tr, s.summary())
    assert np.array_equal(res[0][0].events, res[skew][0].events)
    _same_moments(res[skew][1], _oracle(res[0][0].events, case["init"]))
    for k in MARG:
        assert np.array_equal(res[0][0].marginals[k], res[skew][0].marginals[k])
    _same_marginals(res[skew][0].marginals, _oracle(res[0][0].events, case["init"]))


def test_a_burst_run_again_after_a_time_out_is_not_counted_twice(api):
    """seir_sampler_debug_fail_handoff (the existing test hook, once) in the middle of overlapped bursts with
    summarize=True: the burst is restored -- accumulators included -- and run again one launch form down.  Events, marginals
    and final moments equal those of the undisturbed run; event counts are exact across launch forms, so this is an
    equality too."""
    case, u, ev, cfg, eps = _case("micro_20x60", 8)
    B, nb, burst = 8, 6, 4
    runs = {}
    for disturb in (False, True):
        model, s = _sampler(api, case, cfg, u, ev, eps, 2 * burst, log=None)
        with model, s:
            got = {}

            def consume(tr, i, got=got, s=s, disturb=disturb):
                got[i] = (tr.events.copy(), {k: v.copy() for k, v in tr.marginals.items()})
                if disturb and i == 1 and not s.recoveries:    # while burst 2 or 3 is in flight
                    _lib.check(s._lib.seir_sampler_debug_fail_handoff(s._s, B - 1))
            s.sample_bursts(nb, burst, consume, summarize=True)
            runs[disturb] = (got, s.summary(), list(s.recoveries), s.get_state())
    ref, got = runs[False], runs[True]
    assert not ref[2] and len(got[2]) == 1, got[2]
    assert sorted(got[0]) == list(range(nb))
    for i in range(nb):
        assert np.array_equal(ref[0][i][0], got[0][i][0]), i
        for k in MARG:
            assert np.array_equal(ref[0][i][1][k], got[0][i][1][k]), (i, k)
    want = _oracle(np.concatenate([ref[0][i][0] for i in range(nb)]), case["init"])
    _same_moments(ref[1], want)
    _same_moments(got[1], want)
    assert np.array_equal(ref[3][1], got[3][1])


def test_refusals(api):
    case, u, ev, cfg, eps = _case("micro_20x60", 2)
    model, s = _sampler(api, case, cfg, u, ev, eps, 4, record_events=False)
    with model, s:
        for call in (lambda: s.reset_summary(), lambda: s.summarize(0, 1), lambda: s.read_marginals(1), lambda: s.summary()):
            with pytest.raises(_lib.SeirError) as e:
                call()
            assert e.value.code == _lib.ERR_STATE
    model, s = _sampler(api, case, cfg, u, ev, eps, 4)
    with model, s:
        for call in (lambda: s.summarize(0, 1), lambda: s.read_marginals(1), lambda: s.summary()):
            with pytest.raises(_lib.SeirError, match="seir_sampler_summary_reset") as e:    # before a reset
                call()
            assert e.value.code == _lib.ERR_STATE
        s.reset_summary()
        for first, count in ((-1, 1), (0, 5), (4, 1), (3, 2), (0, -1)):
            calls = [lambda: s.summarize(first, count)]
            if count >= 0:                                     # (NumPy refuses a negative count before the library is asked)
                calls.append(lambda: s.read_marginals(count, first=first))
            for call in calls:
                with pytest.raises(_lib.SeirError) as e:
                    call()
                assert e.value.code == _lib.ERR_INVALID, (first, count)
        s.sample(4, summarize=True)                            # and the sampler is as usable as before
        assert np.array_equal(s.summary().count, [4, 4])


# ---- CLI end to end -------------------------------------------------------------------------------------------------------
def _cli(tmp_path, tag, data, extra):
    cfg = dict(Mcmc=dict(dmax=84, nmax=25, m=2, occult_nmax=15, num_event_time_updates=5,
                         num_bursts=2, num_burst_samples=6, thin=1))
    cpath = os.path.join(tmp_path, f"{tag}.yaml")
    with open(cpath, "w") as f:
        yaml.safe_dump(cfg, f)
    out = os.path.join(tmp_path, f"{tag}.h5")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "covid19uk_amd.inference.inference", "-c", cpath, "-o", out, data] + extra,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    return out, r.stderr


def _datasets(path):
    out = {}
    with hdf5io.File(path, "r") as f:
        def walk(group):
            for link in f._links(group or "/"):
                name = f"{group}/{link}"
                if f._links(name):
                    walk(name)
                else:
                    out[name[1:]] = f.read(name)
        walk("")
    return out


def test_cli_summaries_on_only_off(api, tmp_path):
    """`python -m covid19uk_amd.inference.inference --summaries {on,only,off}` on an NI-11 data set: with `on`, the file's
    summaries/* and marginal datasets equal NumPy over the file's own samples/seir; `only` has no samples/seir and every
    other dataset of the `on` run (same seed); `off` has the layout of a run without the option."""
    tmp_path = str(tmp_path)
    cov = synth.make_covariates("ni11")
    events, init, _ = synth.simulate_epidemic(cov)
    data = os.path.join(tmp_path, "data.npz")
    inf.write_inference_data(data, cov, events[..., 2])
    on = _datasets(_cli(tmp_path, "on", data, ["--summaries", "on"])[0])
    only_path, only_log = _cli(tmp_path, "only", data, ["--summaries", "only"])
    only = _datasets(only_path)
    off = _datasets(_cli(tmp_path, "off", data, ["--summaries", "off"])[0])
    plain = _datasets(_cli(tmp_path, "plain", data, [])[0])

    new = {"samples/seir_by_day", "samples/seir_by_location", "samples/state_by_day", "summaries/count",
           "summaries/seir_mean", "summaries/seir_var", "summaries/state_mean", "summaries/state_var"}
    assert set(on) - set(off) == new and set(off) <= set(on)
    assert set(off) == set(plain)
    for k in off:
        if off[k].dtype.kind in "fiub":
            assert np.array_equal(off[k], plain[k], equal_nan=off[k].dtype.kind == "f"), k
    assert "samples/seir" in on and "samples/seir" not in only
    assert set(only) == set(on) - {"samples/seir"}
    for k in only:
        if only[k].dtype.kind in "fiub":
            assert np.array_equal(only[k], on[k], equal_nan=only[k].dtype.kind == "f"), k
    for word in ("samples/seir", "thin_posterior", "predict", "reproduction_number"):
        assert word in only_log, word

    # the file's summaries against NumPy over the file's own samples/seir
    from covid19uk_amd.sampler import summary_mean, summary_var
    seir = on["samples/seir"]                                 # [n, M, T, 3] float64, warm-up rows first
    n = seir.shape[0]
    assert np.array_equal(seir, np.rint(seir))
    x = _quantities(seir.astype(np.int64), on["initial_state"])
    for k in ("samples/seir_by_day", "samples/seir_by_location", "samples/state_by_day"):
        assert on[k].dtype == np.int64
    assert np.array_equal(on["samples/seir_by_day"], x[..., :3].sum(axis=1))
    assert np.array_equal(on["samples/seir_by_location"], x[..., :3].sum(axis=2))
    assert np.array_equal(on["samples/state_by_day"], x[..., 3:].sum(axis=1))
    ns = int(np.asarray(on["summaries/count"]).reshape(-1)[0])
    assert ns == 2 * 6                                        # bursts x burst: the sampling-phase rows of this chain's file
    xs = x[n - ns:]
    assert (xs != xs[:1]).any()
    d = xs - xs[:1]
    cnt = np.array(ns, np.uint64)
    mean = summary_mean(cnt, xs[0], d.sum(axis=0))            # the integers are NumPy's; the float64 formula is the host's
    var = summary_var(cnt, d.sum(axis=0), (d * d).sum(axis=0))
    assert np.array_equal(on["summaries/seir_mean"], mean[..., :3]) and np.array_equal(on["summaries/state_mean"], mean[..., 3:])
    assert np.array_equal(on["summaries/seir_var"], var[..., :3]) and np.array_equal(on["summaries/state_var"], var[..., 3:])
    # ... and that formula against NumPy's own mean and variance of the float64 rows, to rounding
    xf = xs.astype(np.float64)
    np.testing.assert_allclose(mean, xf.mean(axis=0), rtol=1e-13, atol=0.0)
    np.testing.assert_allclose(var, xf.var(axis=0, ddof=1), rtol=1e-9, atol=1e-9)

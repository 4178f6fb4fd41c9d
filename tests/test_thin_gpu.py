"""Thinning on the device (seir_sampler_desc::thin, seir_sampler_set_thin; the reference's Mcmc.thin,
example_config.yaml:33): the device records the last sweep of every group of `thin` sweeps and skips the trace writes of the
others, while the chain, its random streams and its adaptation see every sweep.

Every comparison is between two samplers with the same seed: A with thin = 1 records n * k sweeps, B with thin = k records
n.  B's trace equals A[k-1::k] BIT FOR BIT and both end in the same state -- both run the same launch form and nothing in
the arithmetic depends on k, so no tolerance is involved (except where a recovery re-runs a burst in another launch form,
and against the CPU oracle: the tolerances tests/test_sampler_gpu.py / tests/test_recovery_gpu.py use there)."""
import ctypes
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import yaml

from covid19uk_amd import _lib, hdf5io, synth
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.sampler import MOVE_KEYS
from oracle import mcmc_oracle as mo
from tests import helpers as H
from tests.test_recovery_gpu import _case, _same_bits, _same_draws
from tests.test_sampler_gpu import CFG_REF, CFG_SMALL, _compare, _start, api  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def _rows(tr, sl):
    """Rows `sl` of a trace, as a trace."""
    return SimpleNamespace(theta=tr.theta[sl], events=None if tr.events is None else tr.events[sl],
                           hmc={k: v[sl] for k, v in tr.hmc.items()},
                           moves={mk: {k: v[sl] for k, v in mv.items()} for mk, mv in tr.moves.items()})


def _copy(tr):
    return SimpleNamespace(theta=tr.theta.copy(), events=None if tr.events is None else tr.events.copy(),
                           hmc={k: v.copy() for k, v in tr.hmc.items()},
                           moves={mk: {k: v.copy() for k, v in mv.items()} for mk, mv in tr.moves.items()})


def _cat(trs):
    return SimpleNamespace(theta=np.concatenate([t.theta for t in trs]), events=np.concatenate([t.events for t in trs]),
                           hmc={k: np.concatenate([t.hmc[k] for t in trs]) for k in trs[0].hmc},
                           moves={mk: {k: np.concatenate([t.moves[mk][k] for t in trs]) for k in trs[0].moves[mk]}
                                  for mk in trs[0].moves})


def _same_state(a, b):
    """get_state() (u, events, running log-prob) and get_kernel() (step size, variances) of two samplers."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def _adaptation(s, u, B, P, steps):
    s.set_adaptation(adapt_step_size=True, adapt_mass=True, num_adaptation_steps=steps,
                     running_variance=(np.full(B, 5.0), np.tile(u.mean(0), (B, 1)), np.full((B, P), 0.5)))


def _run(api, case, cfg, u, ev, eps, thin, kept, adapt=False, seed=13, skew=0, **kw):
    """`kept` draws of a fresh sampler with thinning interval `thin` -> (trace, state + kernel afterwards)."""
    B = u.shape[0]
    with api[0](case["cov"], case["init"], max_chains=B) as model:
        if skew:
            model.set_option(debug_skew=skew)
        with api[1](model, cfg, B, seed=seed, trace_capacity=kept, thin=thin, **kw) as s:
            assert s.thin == thin
            s.set_state(u, ev)
            s.set_kernel(step_size=eps)
            if adapt:
                _adaptation(s, u, B, case["k"].P, kept * thin)        # the window spans every sweep, kept or not
            tr = s.sample(kept)
            assert not s.pair_timeouts().any()
            return tr, s.get_state() + s.get_kernel()


def _check_slice(api, case, cfg, u, ev, eps, k, n, **kw):
    a, st_a = _run(api, case, cfg, u, ev, eps, 1, n * k, **kw)
    b, st_b = _run(api, case, cfg, u, ev, eps, k, n, **kw)
    _same_bits(_rows(a, slice(k - 1, None, k)), b)
    _same_state(st_a, st_b)
    assert a.hmc["is_accepted"].any() and any(a.moves[mk]["is_accepted"].any() for mk in a.moves)
    return a, b, st_a


FORMS = [("chunk", "paired"), ("chunk-launch-fold", "paired-launch"), ("chunk-stage", "paired"),
         ("chunk-split", "paired-delta"), ("single", "split")]


# ---- 4. launch forms ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("form", FORMS, ids=["+".join(f) for f in FORMS])
@pytest.mark.parametrize("name,record,adapt", [("micro_20x60", True, True), ("ni11", "u16", False), ("ni11", True, True)])
def test_thinned_trace_is_a_slice_of_the_unthinned_one(api, name, record, adapt, form, k):
    """Five chains, every launch form.  With dual averaging and the running variance on, the step size and the variances the
    two samplers end with are the same bits: the adaptation saw the dropped sweeps."""
    case, u, ev, cfg, eps = _case(name, 5)
    a, b, st = _check_slice(api, case, cfg, u, ev, eps, k, 4, adapt=adapt, record_events=record, hmc=form[0], moves=form[1])
    assert b.events.dtype == (np.uint16 if record == "u16" else np.int32)
    if adapt:
        assert not np.array_equal(st[3], np.full_like(st[3], eps)) and not np.allclose(st[4], 1.0)


# ---- 5. the sizes that run the persistent launches for real ---------------------------------------------------------------
@pytest.mark.parametrize("B,adapt", [(8, False), (16, False), (1, True)])
def test_thinned_trace_at_uk380(api, B, adapt):
    case, u, ev, cfg, eps = _case("uk380", B)
    _check_slice(api, case, cfg, u, ev, eps, 4, 8, adapt=adapt)


def test_thinned_run_without_the_event_trace(api):
    """record_events = 0: the closing step applies the last F band without a copy; the running log-prob must agree."""
    case, u, ev, cfg, eps = _case("uk380", 8)
    _check_slice(api, case, cfg, u, ev, eps, 4, 4, record_events=False)


# ---- 6. against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cfg,seed,eps,k,n", [("micro_5x24", CFG_SMALL, 1, 0.002, 3, 4), ("ni11", CFG_REF, 2, 0.002, 2, 4)])
def test_kept_sweeps_match_the_oracles_kept_sweeps(api, name, cfg, seed, eps, k, n):
    """oracle/mcmc_oracle.py runs every sweep; the sweeps it would keep, against the device's thinned trace."""
    case = H.build_case(name, seed, alpha_t_sd=0.005)
    B = 2
    u, ev = _start(case, B, seed)
    oracles = []
    for b in range(B):
        ch = mo.OracleChain(case["k"], cfg, u[b], ev[b], seed=77, chain_id=5 + b)
        ch.eps = eps
        every = [ch.sweep_once() for _ in range(n * k)]
        oracles.append(every[k - 1::k])
    tr, _ = _run(api, case, cfg, u, ev, eps, k, n, seed=77, first_chain_id=5)
    _compare(tr, oracles, n, B, cfg)


# ---- 7. graph replay, chain groups, skewed workgroups ---------------------------------------------------------------------
@pytest.mark.parametrize("how", ["graph", "groups", "skew1", "skew2", "skew3"])
def test_launch_geometries_with_thinning(api, how):
    """As tests/test_sampler_gpu.py::test_launch_geometries_give_identical_chains / ..._workgroup_timing, with k = 3: the bits
    of the plain thinned run."""
    case = H.build_case("micro_17x70", 9, alpha_t_sd=0.005)
    B, k, n = 8, 3, 4
    u, ev = _start(case, B, 9)
    kw = dict(graph=dict(use_graph=True), groups=dict(chain_groups=2), skew1=dict(skew=1), skew2=dict(skew=2),
              skew3=dict(skew=3))[how]
    plain, st_plain = _run(api, case, CFG_SMALL, u, ev, 0.0004, k, n, seed=5)
    got, st_got = _run(api, case, CFG_SMALL, u, ev, 0.0004, k, n, seed=5, **kw)
    _same_bits(plain, got)
    _same_state(st_plain, st_got)
    every, _ = _run(api, case, CFG_SMALL, u, ev, 0.0004, 1, n * k, seed=5, **kw)
    _same_bits(_rows(every, slice(k - 1, None, k)), got)


def test_set_thin_on_a_captured_graph_takes_effect(api):
    case = H.build_case("micro_17x70", 9, alpha_t_sd=0.005)
    B, k = 4, 3
    u, ev = _start(case, B, 9)
    with api[0](case["cov"], case["init"], max_chains=B) as model:
        with api[1](model, CFG_SMALL, B, seed=5, trace_capacity=12, use_graph=True) as s:
            s.set_state(u, ev)
            s.set_kernel(step_size=0.0004)
            head = _copy(s.sample(3))                          # captures the sweep with thin = 1
            s.set_thin(k)
            assert s.thin == k
            rest = _copy(s.sample(4))                          # 12 sweeps, 4 kept
            st = s.get_state()
            s.set_thin(1)
            tail = _copy(s.sample(2))
        with api[1](model, CFG_SMALL, B, seed=5, trace_capacity=17, use_graph=True) as s:
            s.set_state(u, ev)
            s.set_kernel(step_size=0.0004)
            every = _copy(s.sample(17))
    _same_bits(_rows(every, slice(0, 3)), head)
    _same_bits(_rows(every, slice(3 + k - 1, 15, k)), rest)
    _same_bits(_rows(every, slice(15, 17)), tail)
    assert st[0].shape == u.shape


# ---- 8. bursts ------------------------------------------------------------------------------------------------------------
def test_overlapped_bursts_with_thinning(api):
    """sample_bursts(4, 10) with thin = 3: in burst order, rows [2::3] of one sample(120) with thin = 1."""
    case = H.build_case("micro_17x70", 9, alpha_t_sd=0.005)
    B, burst, nb, k = 3, 10, 4, 3
    u, ev = _start(case, B, 9)
    with api[0](case["cov"], case["init"], max_chains=B) as model:
        with api[1](model, CFG_SMALL, B, seed=5, trace_capacity=burst * nb * k) as s:
            s.set_state(u, ev)
            s.set_kernel(step_size=0.0004)
            ref = _copy(s.sample(burst * nb * k))
            st_ref = s.get_state()
        got = {}
        with api[1](model, CFG_SMALL, B, seed=5, trace_capacity=2 * burst, thin=k) as s:
            s.set_state(u, ev)
            s.set_kernel(step_size=0.0004)
            s.sample_bursts(nb, burst, lambda tr, i: got.__setitem__(i, _copy(tr)))
            st = s.get_state()
    assert sorted(got) == list(range(nb))
    _same_bits(_rows(ref, slice(k - 1, None, k)), _cat([got[i] for i in range(nb)]))
    _same_state(st_ref, st)


def test_reset_trace_at_starts_a_fresh_group_at_that_slot(api):
    """reset_trace(at=h) counts h in slots; whatever part of a group was under way before it is dropped."""
    case = H.build_case("micro_17x70", 9, alpha_t_sd=0.005)
    B, k, h = 3, 3, 5
    u, ev = _start(case, B, 9)
    with api[0](case["cov"], case["init"], max_chains=B) as model:
        with api[1](model, CFG_SMALL, B, seed=5, trace_capacity=8) as s:
            s.set_state(u, ev)
            s.set_kernel(step_size=0.0004)
            ref = _copy(s.sample(8))
        with api[1](model, CFG_SMALL, B, seed=5, trace_capacity=8, thin=k) as s:
            s.set_state(u, ev)
            s.set_kernel(step_size=0.0004)
            s.reset_trace()
            s.run(2)                                           # two sweeps of a group of three: nothing recorded
            s.reset_trace(at=h)
            s.run(2 * k)                                       # sweeps 2..7: kept are 4 and 7, in slots h and h + 1
            got = _copy(s.read_trace(2, first=h))
            with pytest.raises(_lib.SeirError):
                s.reset_trace(at=8)                            # a slot, whatever the interval
    _same_bits(_rows(ref, [4, 7]), got)


# ---- 9. warm-up windows at 1, then set_thin -------------------------------------------------------------------------------
def test_set_thin_after_unthinned_adaptation_windows(api):
    """The schedule of run_mcmc in small: two adaptation windows with every draw kept, then the fixed kernel thinned by 4 --
    against the same history continued unthinned."""
    case, u, ev, cfg, eps = _case("ni11", 5)
    B, P, k, n = 5, case["k"].P, 4, 5
    out = {}
    for thin in (1, k):
        with api[0](case["cov"], case["init"], max_chains=B) as model:
            with api[1](model, cfg, B, seed=13, trace_capacity=n * k) as s:
                s.set_state(u, ev)
                s.set_kernel(step_size=eps)
                s.set_adaptation(adapt_step_size=True, num_adaptation_steps=10)
                w1 = _copy(s.sample(10))
                _adaptation(s, u, B, P, 10)
                w2 = _copy(s.sample(10))
                s.set_adaptation(adapt_step_size=False)
                s.set_thin(thin)
                rest = _copy(s.sample(n * k // thin))
                out[thin] = (w1, w2, rest, s.get_state() + s.get_kernel())
    _same_bits(out[1][0], out[k][0])
    _same_bits(out[1][1], out[k][1])
    _same_bits(_rows(out[1][2], slice(k - 1, None, k)), out[k][2])
    _same_state(out[1][3], out[k][3])


def test_thin_argument_errors(api):
    case = H.build_case("micro_5x24", 8)
    with api[0](case["cov"], case["init"], max_chains=1) as model:
        with pytest.raises(ValueError):
            api[1](model, CFG_SMALL, 1, thin=0)
        with api[1](model, CFG_SMALL, 1, thin=2) as s:
            with pytest.raises(ValueError):
                s.set_thin(0)
            assert s._lib.seir_sampler_set_thin(s._s, -1) == -1          # SEIR_ERR_INVALID
            got = ctypes.c_int32()
            _lib.check(s._lib.seir_sampler_thin(s._s, ctypes.byref(got)))
            assert got.value == 2 == s.thin
        desc = _lib.SeirSamplerDesc(num_chains=1, dmax=8, nmax=6, m=2, occult_nmax=5, num_event_time_updates=3, t_range_lo=0,
                                    t_range_hi=case["k"].T, num_leapfrog_steps=4, trace_capacity=4, thin=-1)
        ptr = ctypes.c_void_p()
        assert _lib.load().seir_sampler_create(model._ctx, ctypes.byref(desc), ctypes.byref(ptr)) == -1


# ---- 10. recovery ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,adapt", [("uk380", 8, False), ("micro_20x60", 5, True)])
def test_restore_reproduces_a_thinned_burst(api, name, B, adapt):
    case, u, ev, cfg, eps = _case(name, B)
    n, k = 4, 3
    with api[0](case["cov"], case["init"], max_chains=B) as model:
        with api[1](model, cfg, B, seed=13, trace_capacity=n, auto_recover=False, thin=k) as s:
            s.set_state(u, ev)
            s.set_kernel(step_size=eps)
            if adapt:
                _adaptation(s, u, B, case["k"].P, 3 * n * k)
            s.sample(2)
            s.snapshot(1)
            first, st_first = _copy(s.sample(n)), s.get_state() + s.get_kernel()
            s.restore(1)
            again, st_again = _copy(s.sample(n)), s.get_state() + s.get_kernel()
            _same_bits(first, again)
            _same_state(st_first, st_again)
            assert not s.pair_timeouts().any()


def test_sampler_recovers_from_a_time_out_with_thinning(api):
    """tests/test_recovery_gpu.py::test_sampler_recovers_from_a_time_out_by_itself with thin = 3: a time-out injected in the
    middle of overlapped bursts (the existing hook: the chain's counter raised as a timed-out wait leaves it) costs the burst
    it happened in, which is run again -- all its n * thin sweeps -- one launch form down; the run ends with the draws of the
    undisturbed thinned run."""
    name, B, k = "micro_20x60", 8, 3
    case, u, ev, cfg, eps = _case(name, B)
    nb, burst = 6, 4
    runs = {}
    for disturb in (False, True):
        with api[0](case["cov"], case["init"], max_chains=B) as model:
            with api[1](model, cfg, B, seed=13, trace_capacity=2 * burst, log=None, thin=k) as s:
                s.retry_after = 2
                s.set_state(u, ev)
                s.set_kernel(step_size=eps)
                got = {}

                def consume(tr, i, s=s, got=got, disturb=disturb):
                    got[i] = _copy(tr)
                    if disturb and i == 1 and not s.recoveries:
                        _lib.check(s._lib.seir_sampler_debug_fail_handoff(s._s, B - 1))
                s.sample_bursts(nb, burst, consume)
                tail = _copy(s.sample(burst))
                runs[disturb] = (got, tail, list(s.recoveries), s.get_state())
    ref, got = runs[False], runs[True]
    tol = dict(rtol=1e-3, atol=1e-6)             # (the micro case: see test_recovery_gpu.py)
    assert not ref[2] and len(got[2]) == 1, got[2]
    assert got[2][0]["failed_form"] == ("chunk", "paired") and got[2][0]["rerun_form"] == ("chunk-launch", "paired-launch")
    assert sorted(got[0]) == list(range(nb))
    for i in range(nb):
        _same_draws(ref[0][i], got[0][i], **tol)
    _same_draws(ref[1], got[1], **tol)
    assert np.array_equal(ref[3][1], got[3][1])
    # and the undisturbed thinned run is the slice of the unthinned one
    every, _ = _run(api, case, cfg, u, ev, eps, 1, (nb + 1) * burst * k)
    _same_bits(_rows(every, slice(k - 1, None, k)), _cat([ref[0][i] for i in range(nb)] + [ref[1]]))


# ---- 11. CLI end to end ---------------------------------------------------------------------------------------------------
DATASETS = ["samples/psi", "samples/sigma_space", "samples/beta_area", "samples/gamma0", "samples/gamma1", "samples/alpha_0",
            "samples/alpha_t", "samples/spatial_effect", "samples/seir", "results/hmc/is_accepted",
            "results/hmc/target_log_prob", "results/hmc/step_size"] + \
           [f"results/{mk}/{f}" for mk in MOVE_KEYS for f in ("is_accepted", "target_log_prob", "proposed_delta")]
W = inf.warmup_size()


def _write_case(tmp_path):
    cov = synth.make_covariates("ni11")
    events, init, truth = synth.simulate_epidemic(cov)
    data = str(tmp_path / "inferencedata.nc")
    inf.write_inference_data(data, cov, events[..., 2])
    return data


def _config(tmp_path, tag, **mcmc):
    cfg = {"Mcmc": dict(dmax=84, nmax=25, m=2, occult_nmax=15, num_event_time_updates=5, **mcmc)}
    path = str(tmp_path / f"config_{tag}.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path


def _cli(cfg_path, out, data, *extra, env=None):
    env = dict(os.environ, PYTHONPATH=H.ROOT) if env is None else env
    return subprocess.run([sys.executable, "-m", "covid19uk.inference.inference", "-c", cfg_path, "-o", out, "--seed", "4",
                           *extra, data], cwd=H.ROOT, env=env, capture_output=True, text=True, timeout=900)


def _read_all(path):
    with hdf5io.File(path, "r") as f:
        return {name: f.read("/" + name) for name in DATASETS}


def test_cli_thin_in_the_configuration_and_on_the_command_line(tmp_path):
    data = _write_case(tmp_path)
    x = _config(tmp_path, "x", num_bursts=2, num_burst_samples=40, thin=1)
    y = _config(tmp_path, "y", num_bursts=2, num_burst_samples=10, thin=4)
    z = _config(tmp_path, "z", num_bursts=2, num_burst_samples=10, thin=1)
    outs = {}
    for tag, cfg, extra in (("x", x, ()), ("y", y, ()), ("z", z, ("--thin", "4"))):
        out = str(tmp_path / f"posterior_{tag}.hd5")
        r = _cli(cfg, out, data, *extra)
        assert r.returncode == 0, r.stderr[-2000:]
        assert f"thin {1 if tag == 'x' else 4}," in r.stderr, r.stderr[-500:]
        outs[tag] = _read_all(out)
    for name in DATASETS:
        X, Y, Z = outs["x"][name], outs["y"][name], outs["z"][name]
        assert X.shape[0] == W + 80 and Y.shape[0] == W + 20, name
        assert np.array_equal(X[:W], Y[:W]), name                     # the warm-up is not thinned
        assert np.array_equal(X[W:][3::4], Y[W:]), name               # the sampling rows: every fourth
        assert Y.dtype == Z.dtype and np.array_equal(Y, Z), name      # --thin 4 over a configuration that says 1
    assert outs["x"]["results/hmc/is_accepted"][W:].any()
    r = _cli(x, str(tmp_path / "bad.hd5"), data, "--thin", "-2")
    assert r.returncode == 2 and "--thin -2" in r.stderr
    r = _cli(_config(tmp_path, "bad", num_bursts=1, num_burst_samples=1, thin=0), str(tmp_path / "bad.hd5"), data)
    assert r.returncode != 0 and "thin=0" in r.stderr and not os.path.exists(str(tmp_path / "bad.hd5"))


def test_two_rank_job_with_thinning_equals_one_process(tmp_path):
    """tests/test_cli_gpu.py::test_two_rank_job_equals_one_process_with_all_chains with `thin: 4`: every rank uses the same
    interval, the files of chains {0..3} are the same bits however the job is split."""
    import socket
    data = _write_case(tmp_path)
    cfg_path = _config(tmp_path, "y", num_bursts=2, num_burst_samples=10, thin=4)
    base = [sys.executable, "-m", "covid19uk.inference.inference", "-c", cfg_path, "--seed", "11", "--pool-step-size",
            "--device", "0"]
    env = dict(os.environ, PYTHONPATH=H.ROOT)
    one, two = tmp_path / "one", tmp_path / "two"
    one.mkdir(), two.mkdir()
    r = subprocess.run(base + ["--chains", "4", "--hmc", "chunk-launch", "--moves", "paired-launch",
                               "-o", str(one / "posterior.hd5"), data], cwd=H.ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for rank in range(2):
        e = dict(env, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                 MASTER_PORT=str(port), SEIR_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen(base + ["--chains", "2", "-o", str(two / "posterior.hd5"), data], cwd=H.ROOT,
                                      env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    for p in procs:
        out, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-2000:]
        assert "thin 4," in err
    for c in range(4):
        a, b = _read_all(str(one / f"posterior_chain{c}.hd5")), _read_all(str(two / f"posterior_chain{c}.hd5"))
        for name in DATASETS:
            assert a[name].shape[0] == W + 20 and np.array_equal(a[name], b[name]), (c, name)

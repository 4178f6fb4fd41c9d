"""Host side of the thinning interval (Mcmc.thin, example_config.yaml:33) without a GPU: `run_mcmc` keeps the warm-up
windows unthinned, sets the interval before the first burst, asks every burst for num_burst_samples KEPT draws and writes
them at the offsets of an unthinned run; `ChainSampler.sample` / `sample_bursts` enqueue n * thin sweeps and read n slots,
also when a burst is run again after a hand-off time-out.  The device is a stand-in, as in tests/test_recovery_host.py."""
import numpy as np
import pytest

from covid19uk_amd import _lib
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.sampler import MOVE_KEYS, ChainSampler, Trace
from tests.test_recovery_host import FakeDevice, _Buf

B, P, M, T, MM = 2, 9, 2, 4, 1


class StubSampler:
    """What run_mcmc calls, recorded.  A sweep advances an integer state; a kept draw carries the state it was taken at."""

    def __init__(self, cap=800):
        self.B, self.cap = B, cap
        self.calls = []
        self.thin = 1
        self.state = 0

    def set_thin(self, k):
        assert int(k) >= 1
        self.thin = int(k)
        self.calls.append(("set_thin", int(k)))

    def set_kernel(self, step_size=None, variance=None):
        pass

    def get_kernel(self):
        return np.ones(B), np.ones((B, P))

    def set_adaptation(self, **kw):
        self.calls.append(("set_adaptation", bool(kw.get("adapt_step_size")), bool(kw.get("adapt_mass"))))

    def _trace(self, n):
        states = self.state + self.thin * (1 + np.arange(n))           # the last sweep of every group of `thin`
        self.state += n * self.thin
        theta = np.ones((n, B, P)) * states[:, None, None] + 1.0
        ev = np.zeros((n, B, M, T, 3), dtype=np.int32)
        hmc = dict(is_accepted=np.ones((n, B), bool), target_log_prob=np.zeros((n, B)), step_size=np.full((n, B), 0.1))
        mv = {k: dict(is_accepted=np.ones((n, B), bool), target_log_prob=np.zeros((n, B)),
                      proposed_delta=np.zeros((n, B, 4, MM), np.int64)) for k in MOVE_KEYS}
        return Trace(theta=theta, events=ev, hmc=hmc, moves=mv)

    def sample(self, n):
        self.calls.append(("sample", int(n), self.thin))
        return self._trace(n)

    def sample_bursts(self, nb, n, consume):
        for i in range(nb):
            self.calls.append(("burst", int(n), self.thin))
            consume(self._trace(n), i)


class StubPosterior:
    def __init__(self):
        self.writes = []          # (offset, rows, first theta value)

    def write_samples(self, samples, first_dim_offset):
        self.writes.append((first_dim_offset, len(samples["psi"]), float(samples["psi"][0])))

    def write_results(self, results, first_dim_offset):
        assert self.writes[-1][0] == first_dim_offset


def _run(config, cap=800):
    s, posts = StubSampler(cap), [StubPosterior() for _ in range(B)]
    n = inf.run_mcmc(s, config, posts, log=open("/dev/null", "w"))
    return s, posts, n


CFG = dict(num_bursts=3, num_burst_samples=10)
WINDOWS = [200] + [25 * 2 ** k for k in range(6)] + [50]


@pytest.mark.parametrize("cap", [800, 10])       # overlapped bursts (sample_bursts) / one blocking sample per burst
def test_warm_up_runs_at_1_and_the_bursts_at_thin(cap):
    s, posts, n = _run(dict(CFG, thin=4), cap)
    kind = "burst" if cap >= 20 else "sample"
    sampling = [c for c in s.calls if c[0] in ("sample", "burst")]
    assert sampling[:len(WINDOWS)] == [("sample", w, 1) for w in WINDOWS]                 # every warm-up draw is kept
    assert sampling[len(WINDOWS):] == [(kind, 10, 4)] * 3                                 # num_burst_samples KEPT draws each
    # set_thin(4) comes after the last window and before the first burst, and nothing but 1 was in force before
    names = [c[0] if c[0] != "sample" or c[2] == 1 else "burst" for c in s.calls]
    i4 = s.calls.index(("set_thin", 4))
    assert all(c != "burst" for c in names[:i4]) and names[i4 + 1:] == ["burst"] * 3
    assert [c for c in s.calls[:i4] if c[0] == "set_thin"] in ([], [("set_thin", 1)])
    assert s.state == inf.warmup_size() + 3 * 10 * 4                                      # sweeps the chain made
    assert n == inf.warmup_size() + 30                                                    # rows written


def test_offsets_are_those_of_an_unthinned_run():
    _, p1, n1 = _run(dict(CFG, thin=1))
    _, p4, n4 = _run(dict(CFG, thin=4))
    assert n1 == n4
    for a, b in zip(p1, p4):
        assert [(o, r) for o, r, _ in a.writes] == [(o, r) for o, r, _ in b.writes]
        nw = len(WINDOWS)
        assert a.writes[:nw] == b.writes[:nw]                                             # the warm-up rows are the same rows
        w0 = inf.warmup_size()
        # first kept draw of burst i: sweep w0 + 10 i + 1 unthinned, sweep w0 + 40 i + 4 thinned
        assert [v for _, _, v in a.writes[nw:]] == [w0 + 10 * i + 1 + 1.0 for i in range(3)]
        assert [v for _, _, v in b.writes[nw:]] == [w0 + 40 * i + 4 + 1.0 for i in range(3)]


def test_a_configuration_without_the_key_is_thin_1():
    s0, p0, _ = _run(dict(CFG))
    s1, p1, _ = _run(dict(CFG, thin=1))
    assert [c for c in s0.calls if c[0] != "set_thin"] == [c for c in s1.calls if c[0] != "set_thin"]
    assert all(c[1] == 1 for c in s0.calls if c[0] == "set_thin")
    assert [p.writes for p in p0] == [p.writes for p in p1]
    assert inf.thin_interval({}) == 1 and inf.thin_interval({"thin": 5}) == 5 and inf.thin_interval({"thin": 5}, 2) == 2


@pytest.mark.parametrize("bad", [0, -1])
def test_thin_below_1_is_refused_before_anything_runs(bad):
    s, posts = StubSampler(), [StubPosterior()]
    with pytest.raises(ValueError, match="thin"):
        inf.run_mcmc(s, dict(CFG, thin=bad), posts, log=open("/dev/null", "w"))
    assert s.calls == [] and posts[0].writes == []
    # mcmc() refuses it before it reads the data file or opens a device: the file named here does not exist
    with pytest.raises(ValueError, match="thin"):
        inf.mcmc("/nonexistent/data.nc", "/nonexistent/out.hd5", dict(CFG, thin=bad))
    with pytest.raises(ValueError, match="thin"):
        inf.mcmc("/nonexistent/data.nc", "/nonexistent/out.hd5", dict(CFG, thin=3), thin=bad)


def test_the_command_line_refuses_thin_minus_2(tmp_path, capsys):
    cfg = tmp_path / "c.yaml"
    cfg.write_text("Mcmc:\n  num_bursts: 1\n  num_burst_samples: 1\n")
    with pytest.raises(SystemExit) as e:
        inf.main(["-c", str(cfg), "-o", str(tmp_path / "o.hd5"), "--thin", "-2", str(tmp_path / "none.nc")])
    assert e.value.code == 2 and "--thin -2" in capsys.readouterr().err


def test_the_command_line_value_overrides_the_configuration(tmp_path, monkeypatch):
    cfg = tmp_path / "c.yaml"
    cfg.write_text("Mcmc:\n  num_bursts: 1\n  num_burst_samples: 1\n  thin: 7\n")
    seen = {}
    monkeypatch.setattr(inf, "mcmc", lambda data, out, config, **kw: seen.update(config=config, **kw))
    inf.main(["-c", str(cfg), "-o", "o.hd5", "--thin", "4", "d.nc"])
    assert seen["thin"] == 4 and inf.thin_interval(seen["config"], seen["thin"]) == 4
    inf.main(["-c", str(cfg), "-o", "o.hd5", "d.nc"])
    assert seen["thin"] is None and inf.thin_interval(seen["config"], seen["thin"]) == 7


# --- ChainSampler.sample / sample_bursts: n kept draws = n * thin sweeps, re-runs included --------------------------------
class ThinFake(FakeDevice):
    """tests/test_recovery_host.FakeDevice with the device's thinning rule: the last sweep of every group is recorded."""

    def reset_trace(self, at=0):
        self.slot, self.group = at, 0

    def run(self, n):
        if self.poisoned:
            self._fail()
        self.runs.append(n)
        for _ in range(n):
            self.state += 1
            if self.state in self.fail_at and self.form in self.fail_forms:
                self.fail_at.discard(self.state)
                self.poisoned_pending = True
            self.group += 1
            if self.group % self._thin == 0:
                self.trace[self.slot] = -1 if getattr(self, "poisoned_pending", False) else self.state
                self.slot += 1


@pytest.fixture
def pinned(monkeypatch):
    import covid19uk_amd.sampler as S
    monkeypatch.setattr(S, "PinnedTrace", lambda sampler, burst, events=True: _Buf())


def test_a_sampler_built_by_hand_samples_every_sweep():
    s = FakeDevice(cap=8)                      # never ran ChainSampler.__init__
    assert s.thin == 1 and ChainSampler._thin == 1
    assert s.sample(4) == [1, 2, 3, 4]


@pytest.mark.parametrize("fail_at", [(), (2,), (13,), (30, 31), (5, 40, 70)])
def test_bursts_and_their_re_runs_make_n_times_thin_sweeps(pinned, fail_at):
    nb, burst, k = 6, 4, 3
    s = ThinFake(fail_at=fail_at, cap=2 * burst)
    s._thin, s.runs = k, []
    got = {}

    def consume(tr, i):
        assert i not in got
        got[i] = list(tr)
    s.sample_bursts(nb, burst, consume)
    assert set(s.runs) == {burst * k}
    for i in range(nb):
        assert got[i] == [k * (i * burst + j + 1) for j in range(burst)], (i, got[i])     # rows [k-1::k] of the unthinned run
    assert s.state == nb * burst * k
    assert bool(s.recoveries) == bool(fail_at)


def test_blocking_sample_re_runs_the_same_sweeps(pinned):
    s = ThinFake(fail_at=(7,), cap=8)
    s._thin, s.runs = 3, []
    assert s.sample(4) == [3, 6, 9, 12]
    assert s.runs == [12, 12] and len(s.recoveries) == 1
    assert s.sample(2) == [15, 18]

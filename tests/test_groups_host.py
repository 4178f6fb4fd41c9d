"""Region totals, the host's half (covid19uk_amd/posterior/groups.py, `Mcmc: groups` / `--groups`, the datasets) and what can
be said about the device's half without a GPU: the entry points' declarations and bindings and the compiler's account of
k_group_sums.  The device's results are held to NumPy and to `SeirModel.simulate` in tests/test_groups_gpu.py."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from covid19uk_amd import _lib, hdf5io, synth
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.posterior import groups as G
from covid19uk_amd.sampler import GROUP_KEYS, GROUP_SOURCES, ChainSampler
from covid19uk_amd.seir import SeirModel
from tests import helpers as H
from tests.abi_lib import check_symbols
from tests.test_check_host import CheckStub
from tests.test_summary_host import CFG, _read

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "seir_sampler_groups_set": "seir_sampler *s, int32_t G, const int32_t *offsets, const int32_t *members",
    "seir_sampler_read_group_marginals": "seir_sampler *s, int32_t which, int32_t first, int32_t count, "
                                         "int64_t *events_by_group, int64_t *state0_by_group",
    "seir_sampler_read_group_marginals_async": "seir_sampler *s, int32_t which, int32_t first, int32_t count, "
                                               "int64_t *events_by_group, int64_t *state0_by_group",
    "seir_group_sums": "seir_ctx *ctx, const int32_t *events, int64_t n, int32_t M, int32_t L, int32_t G, "
                       "const int32_t *offsets, const int32_t *members, int64_t *out",
}


# ---- 1. the symbols ------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound_with_the_headers_types():
    lib = check_symbols(NEW)
    raw = open(os.path.join(ROOT, "include", "seir_hip.h")).read()
    assert re.search(r"#define SEIR_GROUPS_MAX 256\b", raw) and _lib.GROUPS_MAX == G.MAX_GROUPS == 256
    # a null sampler / context is refused before anything touches a device
    one = (ctypes.c_int32 * 2)(0, 1)
    out = (ctypes.c_int64 * 3)()
    assert lib.seir_sampler_groups_set(None, 1, one, one) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_group_marginals(None, 0, 0, 1, out, None) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_group_marginals_async(None, 0, 0, 1, out, None) == _lib.ERR_INVALID
    assert lib.seir_group_sums(None, one, 1, 1, 1, 1, one, one, out) == _lib.ERR_INVALID
    for name in ("set_groups", "read_group_marginals", "read_group_marginals_async"):
        assert callable(getattr(ChainSampler, name))
    assert callable(SeirModel.group_sums)
    assert GROUP_KEYS == ("seir_by_group", "forecast_by_group", "forecast_group_state0", "check_by_group", "check_group_state0")
    assert [v[0] for v in GROUP_SOURCES.values()] == [0, 1, 2]


# ---- 2. group specifications ---------------------------------------------------------------------------------------------
def test_nations_on_the_bundled_codes():
    codes = [str(x) for x in np.load(synth._DATA)["lad19cd"]]
    tab = G.parse_groups("nations", len(codes), codes)
    assert tab.names == ["E", "S", "W", "N"]
    assert np.array_equal(np.diff(tab.offsets), [315, 32, 22, 11]) and tab.offsets[0] == 0
    assert tab.offsets.dtype == tab.members.dtype == np.int32
    for g, letter in enumerate(tab.names):
        assert np.array_equal(tab.rows(g), [m for m, c in enumerate(codes) if c[0] == letter])
    assert np.array_equal(np.sort(tab.members), np.arange(380))                # a partition
    # letters that are none of the four follow, in order of first appearance
    tab = G.parse_groups("nations", 5, ["X1", "N1", "A1", "E1", "X2"])
    assert tab.names == ["E", "N", "X", "A"] and np.array_equal(tab.offsets, [0, 1, 2, 4, 5])
    assert np.array_equal(tab.members, [3, 1, 0, 4, 2])


def test_a_mapping_with_codes_prefixes_indices_and_overlap():
    codes = ["E06000001", "E06000002", "E07000001", "S12000005", "W06000001", "N09000001", "E09000001"]
    spec = {"England": ["E0*"], "unitary": ["E06*", "W06000001"], "mixed": [5, "S12000005", 0], "one": 6, "code": "N09000001"}
    tab = G.parse_groups(spec, 7, codes)
    assert tab.names == ["England", "unitary", "mixed", "one", "code"] and tab.G == 5
    assert np.array_equal(tab.offsets, [0, 4, 7, 10, 11, 12])
    assert np.array_equal(tab.members, [0, 1, 2, 6, 0, 1, 4, 0, 3, 5, 6, 5])  # ascending within a group; groups overlap
    # indices alone need no codes
    tab = G.parse_groups({"a": [2, 0], "b": [1]}, 3)
    assert np.array_equal(tab.offsets, [0, 2, 3]) and np.array_equal(tab.members, [0, 2, 1])
    x = np.arange(12).reshape(3, 4)
    assert np.array_equal(tab.sum_rows(x), [x[0] + x[2], x[1]])
    assert np.array_equal(tab.sum_rows(x.T, axis=1), np.stack([x[0] + x[2], x[1]], axis=1))
    for off in (None, False, "off"):
        assert G.parse_groups(off, 3) is None


def test_every_refusal_before_any_gpu_call(tmp_path):
    codes = ["E01", "E02", "S01"]
    bad = [({"a": []}, "empty"), ({"a": ["E03"]}, "unknown location code"), ({"a": ["E01", 0]}, "more than once"),
           ({"a": ["E0*", "E01"]}, "more than once"), ({"a": [3]}, "outside"), ({"a": [-1]}, "outside"),
           ({"a": ["Q*"]}, "matches no"), ({"a": [1.5]}, "no member"), ({"a": [True]}, "no member"), ({}, "no group"),
           ({str(i): [0] for i in range(257)}, "at most 256"), ("regions", "'nations' or a mapping"), (7, "'nations' or a mapping"),
           ({"a": {"b": 1}}, "a list of")]
    for spec, word in bad:
        with pytest.raises(ValueError, match=word):
            G.parse_groups(spec, 3, codes)
    assert G.parse_groups({str(i): [0] for i in range(256)}, 3, codes).G == 256
    with pytest.raises(ValueError, match="location codes"):
        G.parse_groups("nations", 3)
    with pytest.raises(ValueError, match="location codes"):
        G.parse_groups({"a": ["E0*"]}, 3)
    with pytest.raises(ValueError, match="unknown location code"):
        G.parse_groups({"a": ["E01"]}, 3)
    with pytest.raises(ValueError, match="2 location names for M=3"):
        G.parse_groups("nations", 3, codes[:2])
    # mcmc(): `nations` on an .npz input (it carries no codes), a bad table, and groups without a source -- all before a
    # model or a sampler exists (this test runs without a GPU)
    cov = synth.make_covariates("ni11")
    events, _, _ = synth.simulate_epidemic(cov)
    data = str(tmp_path / "data.npz")
    inf.write_inference_data(data, cov, events[..., 2])
    out = str(tmp_path / "out.npz")
    with pytest.raises(ValueError, match="location codes"):
        inf.mcmc(data, out, dict(CFG, summaries="only", groups="nations"))
    with pytest.raises(ValueError, match="location codes"):
        inf.mcmc(data, out, dict(CFG, summaries="only"), groups="nations")
    with pytest.raises(ValueError, match="outside"):
        inf.mcmc(data, out, dict(CFG, summaries="only", groups={"a": [11]}))
    with pytest.raises(ValueError, match="no effect"):
        inf.mcmc(data, out, dict(CFG, groups={"a": [0, 1]}))
    with pytest.raises(ValueError, match="no effect"):
        inf.mcmc(data, out, dict(CFG, rt=3, within_between=3, groups={"a": [0, 1]}))
    assert not os.path.exists(out)
    with pytest.raises(ValueError, match="no effect"):
        G.require_source(G.parse_groups({"a": [0]}, 3), "off", 0, 0)
    for ok in (("on", 0, 0), ("only", 0, 0), ("off", 7, 0), ("off", 0, 7)):
        G.require_source(G.parse_groups({"a": [0]}, 3), *ok)
    G.require_source(None, "off", 0, 0)


def test_the_input_files_location_coordinate_is_read(tmp_path):
    assert hdf5io.available(), "the HDF5 writer is part of what this project needs"
    cov = synth.make_covariates("ni11")
    events, _, _ = synth.simulate_epidemic(cov)
    codes = ["E%02d" % m for m in range(6)] + ["W%02d" % m for m in range(5)]
    data = str(tmp_path / "data.h5")
    inf.write_inference_data(data, cov, events[..., 2], locations=codes)
    assert inf.read_location_names(data) == codes
    cov2, cases, _ = inf.read_inference_data(data)
    assert np.array_equal(cases, events[..., 2]) and np.array_equal(cov2.N, cov.N)
    tab = G.parse_groups("nations", 11, inf.read_location_names(data))
    assert tab.names == ["E", "W"] and np.array_equal(tab.offsets, [0, 6, 11])


def test_the_cli_flag_parses(tmp_path, monkeypatch):
    import yaml
    cpath, gpath = str(tmp_path / "c.yaml"), str(tmp_path / "g.yaml")
    with open(cpath, "w") as f:
        yaml.safe_dump(dict(Mcmc=CFG), f)
    with open(gpath, "w") as f:
        yaml.safe_dump({"north": ["E0*", 4], "one": [0]}, f)
    seen = {}
    monkeypatch.setattr(inf, "mcmc", lambda *a, **kw: (seen.clear(), seen.update(kw)))
    inf.main(["-c", cpath, "-o", "x", "--summaries", "only", "--groups", "nations", "data.nc"])
    assert seen["groups"] == "nations"
    inf.main(["-c", cpath, "-o", "x", "--summaries", "only", "--groups", gpath, "data.nc"])
    assert seen["groups"] == {"north": ["E0*", 4], "one": [0]}
    inf.main(["-c", cpath, "-o", "x", "--summaries", "only", "data.nc"])
    assert "groups" not in seen                              # absent: mcmc is called as before the option existed


# ---- 3. the statistics ---------------------------------------------------------------------------------------------------
def test_group_state_planes_and_check_counts_equal_a_numpy_restatement():
    rng = np.random.default_rng(5)
    n, B, Gn, L = 7, 2, 3, 9
    ev = rng.integers(0, 50, size=(n, B, Gn, L, 3))
    s0 = rng.integers(500, 900, size=(n, B, Gn, 3))
    st = G.group_state(ev, s0)
    assert st.dtype == np.int64 and st.shape == ev.shape
    want = np.empty_like(st)
    for i in np.ndindex(n, B, Gn):
        S, E, I = (int(v) for v in s0[i])
        for t in range(L):
            want[i][t] = (S, E, I)
            a, b, c = (int(v) for v in ev[i][t])
            S, E, I = S - a, E + a - b, I + b - c
    assert np.array_equal(st, want)
    with pytest.raises(TypeError):
        G.group_state(ev.astype(np.float64), s0)
    pl = G.forecast_planes(ev, s0)
    assert pl.shape == (3, n, B, Gn, L) and G.PLANES == ("cases", "cum_cases", "prevalence")
    assert np.array_equal(pl[0], ev[..., 2]) and np.array_equal(pl[1], np.cumsum(ev[..., 2], axis=-1))
    assert np.array_equal(pl[2], want[..., 2])
    sim = rng.integers(0, 4, size=(n, Gn, L, 3))
    obs = rng.integers(0, 4, size=(Gn, L))
    cc = G.check_counts(sim, obs)
    assert set(cc) == {"group_observed", "group_lt", "group_eq", "group_window_lt", "group_window_eq", "group_pit",
                       "group_window_pit"}
    for g in range(Gn):
        tot = [int(sim[j, g, :, 2].sum()) for j in range(n)]
        assert cc["group_window_lt"][g] == sum(v < obs[g].sum() for v in tot)
        assert cc["group_window_eq"][g] == sum(v == obs[g].sum() for v in tot)
        for s in range(L):
            assert cc["group_lt"][g, s] == sum(sim[j, g, s, 2] < obs[g, s] for j in range(n))
            assert cc["group_eq"][g, s] == sum(sim[j, g, s, 2] == obs[g, s] for j in range(n))
    assert cc["group_lt"].any() and cc["group_eq"].any() and (n - cc["group_lt"] - cc["group_eq"]).any()
    assert np.array_equal(cc["group_observed"], obs)
    # raw counts pool over chains by a sum
    both = G.check_counts(np.concatenate([sim, sim[::-1]]), obs)
    assert np.array_equal(both["group_lt"], 2 * cc["group_lt"]) and np.array_equal(both["group_window_eq"], 2 * cc["group_window_eq"])


def test_mid_p_equals_the_exact_fraction():
    rng = np.random.default_rng(9)
    for n in (1, 3, 7, 1000, 2 ** 20 - 1):
        lt = rng.integers(0, n + 1, size=50)
        eq = np.array([rng.integers(0, n - a + 1) for a in lt])
        got = G.mid_p(n, lt, eq)
        for a, b, v in zip(lt, eq, got):
            assert v == float(Fraction(2 * int(a) + int(b), 2 * n)), (n, a, b)
    assert np.isnan(G.mid_p(0, np.zeros(2), np.zeros(2))).all()
    sim = rng.integers(0, 3, size=(11, 2, 4, 3))
    obs = rng.integers(0, 3, size=(2, 4))
    cc = G.check_counts(sim, obs)
    for idx in np.ndindex(2, 4):
        assert cc["group_pit"][idx] == float(Fraction(2 * int(cc["group_lt"][idx]) + int(cc["group_eq"][idx]), 22))
    for g in range(2):
        assert cc["group_window_pit"][g] == float(Fraction(2 * int(cc["group_window_lt"][g]) + int(cc["group_window_eq"][g]), 22))


def test_quantiles_equal_numpy_quantile():
    rng = np.random.default_rng(3)
    probs = (0.0, 0.05, 1.0 / 3.0, 0.5, 0.95, 1.0)
    for n in (1, 2, 7, 100):
        x = rng.integers(0, 10 ** 6, size=(n, 2, 5))
        np.testing.assert_allclose(G.quantiles(x, probs), np.quantile(x.astype(np.float64), probs, axis=0), rtol=1e-12, atol=0)


# ---- 4. run_mcmc with a stub sampler -------------------------------------------------------------------------------------
TABLE = G.parse_groups({"all": [0, 1, 2], "ends": [0, 2]}, 3)


class QuantileStub(CheckStub):
    """CheckStub with the forecast's draw store: a sampler that has never heard of groups."""

    def keep_forecast_draws(self, cap):
        self.calls.append(("keep_forecast_draws", cap))

    def forecast_quantiles(self, probs, pooled=False):
        self.calls.append(("forecast_quantiles", tuple(probs), pooled))
        q = np.quantile(np.asarray(self.forecast_rows, np.float64), probs)
        cell = q[:, None, None, None] + np.zeros((1, 3, self.M, self.H))
        return cell if pooled else np.repeat(cell[:, None], self.B, axis=1)


class GroupStub(QuantileStub):
    """QuantileStub with the group table: a draw's group sums are functions of its sweep number, the group and the day."""

    def set_groups(self, offsets, members):
        self.calls.append(("set_groups", np.asarray(offsets).copy(), np.asarray(members).copy()))
        self.G = len(offsets) - 1

    def _rows(self, idx, L):
        g, t, x = np.arange(self.G)[:, None, None], np.arange(L)[None, :, None], np.arange(3)[None, None, :]
        one = (idx[:, None, None, None] * (g + 1) + 3 * t + x) % 11
        return np.repeat(one[:, None], self.B, axis=1).astype(np.int64) + np.arange(self.B)[None, :, None, None, None]

    def _trace(self, n, events=True, summarize=False, forecast=False, rt=False, check=False, groups=False):
        tr = super()._trace(n, events=events, summarize=summarize, forecast=forecast, rt=rt, check=check)
        if groups:
            idx = self.sweeps - n + np.arange(n)
            tr.groups = {}
            assert groups is True or all(dict(trace=summarize, forecast=forecast, check=check)[k] for k in groups)
            summarize, forecast, check = (on and (groups is True or k in groups)
                                          for k, on in (("trace", summarize), ("forecast", forecast), ("check", check)))
            if summarize:
                tr.groups["seir_by_group"] = self._rows(idx, self.T)
            if forecast:
                tr.groups["forecast_by_group"] = self._rows(idx, self.H)
                tr.groups["forecast_group_state0"] = 1000 + self._rows(idx, 1)[:, :, :, 0]
            if check:
                tr.groups["check_by_group"] = self._rows(idx, self.K)
                tr.groups["check_group_state0"] = 2000 + self._rows(idx, 1)[:, :, :, 0]
        return tr


def _run(tmp_path, tag, config, ext=".npz", cap=800, stub=GroupStub, groups=None):
    s = stub()
    s.cap = cap
    nb, ns = config["num_bursts"], config["num_burst_samples"]
    Hn, _ = inf.forecast_mode(config)
    K = inf.check_mode(config)
    names = [str(tmp_path / f"{tag}_{c}{ext}") for c in range(s.B)]
    kw = {} if config.get("summaries", "off") == "off" else dict(summaries=config["summaries"])
    for key, v in (("forecast", Hn), ("check", K)):
        if v:
            kw[key] = (v, nb * ns)
    if groups is not None:
        kw["groups"] = groups.G
    posts = [inf.Posterior(name, s.M, s.T, 2, inf.warmup_size() + nb * ns, **kw) for name in names]
    logname = str(tmp_path / f"{tag}.log")
    fkw = dict(seed=21)
    if Hn:
        fkw["forecast_calendar"] = (np.arange(Hn) + 0.5, np.arange(Hn) - 1.0)
    if K:
        fkw["check_calendar"] = (np.arange(K) + 0.25, np.arange(K) - 2.0)
    if groups is not None:
        fkw["groups"] = groups
        for p in posts:
            p.write_groups(groups, np.array([10.0, 20.0, 40.0]), np.arange(12.0).reshape(3, 4))
    with open(logname, "w") as log:
        inf.run_mcmc(s, config, posts, log=log, **fkw)
    for p in posts:
        p.close()
    return s, [_read(n) for n in names], open(logname).read()


def _untimed(log):
    return [ln for ln in log.splitlines() if not ln.startswith("Sampling: ")]      # that line carries a wall-clock rate


def _stripped(calls):
    """The calls without set_groups and without the groups keyword."""
    out = []
    for c in calls:
        if c[0] == "set_groups":
            continue
        if c[0] in ("sample", "burst"):
            c = (c[0], c[1], {k: v for k, v in c[2].items() if k != "groups"})
        out.append(c)
    return out


def _same_calls(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x[0] == y[0] and len(x) == len(y), (x, y)
        if x[0] in ("sample", "burst"):
            assert x[1] == y[1] and set(x[2]) == set(y[2]), (x, y)
            assert all(callable(v) or v == y[2][k] for k, v in x[2].items()), (x, y)


FULL = dict(CFG, num_bursts=3, num_burst_samples=4, forecast=6, forecast_quantiles=[0.05, 0.5, 0.95], check=2)


def test_absent_calls_nothing_new_and_writes_todays_datasets(tmp_path):
    cfg = dict(FULL, summaries="only")
    s0, f0, log0 = _run(tmp_path, "parent", cfg, stub=QuantileStub)        # a sampler that has never heard of groups
    s1, f1, log1 = _run(tmp_path, "absent", cfg)
    _same_calls(s1.calls, s0.calls)
    assert not any(c[0] == "set_groups" for c in s1.calls)
    assert not any("groups" in c[2] for c in s1.calls if c[0] in ("sample", "burst"))
    assert "Groups:" not in log1 and _untimed(log1) == _untimed(log0)
    for c in range(2):
        assert set(f1[c]) == set(f0[c]) and not any("group" in k for k in f1[c])
        for k in f0[c]:
            assert np.array_equal(f1[c][k], f0[c][k], equal_nan=True), k
    with pytest.raises(ValueError, match="no effect"):
        _run(tmp_path, "nosource", dict(CFG, rt=None), groups=TABLE)


@pytest.mark.parametrize("summaries,overlap,ext", [("only", True, ".hd5"), ("on", False, ".npz"), ("off", True, ".npz")])
def test_the_table_is_set_once_and_the_datasets_are_written(tmp_path, summaries, overlap, ext):
    assert hdf5io.available(), "the HDF5 writer is part of what this project needs"
    cfg = dict(FULL, summaries=summaries)
    nb, ns, Hn, K, probs = 3, 4, 6, 2, (0.05, 0.5, 0.95)
    cap = 800 if overlap else ns
    s, files, log = _run(tmp_path, "on", cfg, ext=ext, cap=cap, groups=TABLE)
    base, bf, blog = _run(tmp_path, "base", cfg, ext=ext, cap=cap)
    names = [c[0] for c in s.calls]
    # once, before the first draw
    assert names.count("set_groups") == 1 and names.index("set_groups") < min(i for i, n in enumerate(names) if n == "sample")
    call = s.calls[names.index("set_groups")]
    assert np.array_equal(call[1], TABLE.offsets) and np.array_equal(call[2], TABLE.members)
    # the others' calls and keyword sets are untouched; `groups` rides on the warm-up only where summaries summarises it
    _same_calls(_stripped(s.calls), base.calls)
    warm = [c for c in s.calls if c[0] == "sample" and "forecast" not in c[2]]
    assert len(warm) == 8 and all(c[2].get("groups") == (("trace",) if summaries != "off" else None) for c in warm)
    # the sampling phase asks for the sources that are written: the trace's only with summaries on / only
    src = (("trace",) if summaries != "off" else ()) + ("forecast", "check")
    assert all(c[2].get("groups") == src for c in s.calls if c[0] in ("sample", "burst") and "forecast" in c[2])
    W, n_all = inf.warmup_size(), inf.warmup_size() + nb * ns
    idx_all, idx_fc = np.arange(n_all), W + np.arange(nb * ns)
    new = {"groups/" + k for k in ("names", "offsets", "members", "population", "initial_state")}
    new |= {"samples/" + k for k in GROUP_KEYS if summaries != "off" or k != "seir_by_group"}
    new |= {"forecast/" + k for k in ["group_seir_mean", "group_state_mean"] +
            [f"{p}group_{x}_quantiles" for p in ("", "pooled_") for x in G.PLANES]}
    new |= {"check/group_" + k for k in ("observed", "lt", "eq", "window_lt", "window_eq", "pit", "window_pit")}
    for c, f in enumerate(files):
        assert set(f) == set(bf[c]) | new
        for k in bf[c]:
            assert np.array_equal(f[k], bf[c][k], equal_nan=True), k
        assert [x.decode() for x in f["groups/names"]] == ["all", "ends"]
        assert np.array_equal(f["groups/offsets"], [0, 3, 5]) and np.array_equal(f["groups/members"], [0, 1, 2, 0, 2])
        assert np.array_equal(f["groups/population"], [70.0, 50.0])
        assert np.array_equal(f["groups/initial_state"], [[12, 15, 18, 21], [8, 10, 12, 14]])
        if summaries != "off":
            sg = f["samples/seir_by_group"]
            assert sg.dtype == np.int64 and sg.shape == (n_all, 2, s.T, 3)
            assert np.array_equal(sg, s._rows(idx_all, s.T)[:, c])                       # warm-up rows included
        fg, f0 = f["samples/forecast_by_group"], f["samples/forecast_group_state0"]
        assert fg.dtype == f0.dtype == np.int64 and fg.shape == (nb * ns, 2, Hn, 3) and f0.shape == (nb * ns, 2, 3)
        assert np.array_equal(fg, s._rows(idx_fc, Hn)[:, c]) and np.array_equal(f0, 1000 + s._rows(idx_fc, 1)[:, c, :, 0])
        cg = f["samples/check_by_group"]
        assert np.array_equal(cg, s._rows(idx_fc, K)[:, c]) and cg.shape == (nb * ns, 2, K, 3)
        assert np.array_equal(f["samples/check_group_state0"], 2000 + s._rows(idx_fc, 1)[:, c, :, 0])
        assert np.array_equal(f["forecast/group_seir_mean"], fg.mean(axis=0))
        assert np.array_equal(f["forecast/group_state_mean"], G.group_state(fg, f0).mean(axis=0))
        pl = G.forecast_planes(fg, f0)
        allc = G.forecast_planes(s._rows(idx_fc, Hn), 1000 + s._rows(idx_fc, 1)[:, :, :, 0])     # [3,n,B,G,H]
        for x, name in enumerate(G.PLANES):
            own, pooled = f[f"forecast/group_{name}_quantiles"], f[f"forecast/pooled_group_{name}_quantiles"]
            assert own.shape == pooled.shape == (3, 2, Hn) and own.dtype == np.float64
            np.testing.assert_allclose(own, np.quantile(pl[x].astype(np.float64), probs, axis=0), rtol=1e-12, atol=0)
            np.testing.assert_allclose(pooled, np.quantile(allc[x].reshape(-1, 2, Hn).astype(np.float64), probs, axis=0),
                                       rtol=1e-12, atol=0)
        want = G.check_counts(cg, TABLE.sum_rows(np.full((s.M, K), 9)))                  # the stub's observed counts are 9
        for k, v in want.items():
            assert np.array_equal(f["check/" + k], np.asarray(v, np.float64)), k
        assert np.array_equal(f["check/group_observed"], [[27, 27], [18, 18]])
    assert log.count("Groups: 2 group(s)") == 1 and "all (3), ends (2)" in log
    assert [ln for ln in _untimed(log) if not ln.startswith("Groups:")] == _untimed(blog)      # one line more


def test_with_diagnostics_alone_the_traces_sums_are_not_asked_for(tmp_path):
    """`diagnostics: on` with `summaries: off` summarises every burst, but nothing of the trace's group sums would be
    written: only the forecast's and the check's cross."""
    cfg = dict(FULL, summaries="off", diagnostics="on")
    s = GroupStub()
    seen = []
    orig = s._trace

    def spy(n, **kw):
        seen.append(kw)
        return orig(n, **{k: v for k, v in kw.items() if k != "marks"})
    s._trace = spy
    s.reset_diagnostics = lambda L: s.reset_summary()
    s.mark = lambda which: None
    class EndOfSampling(Exception):
        pass

    def diagnostics():
        raise EndOfSampling
    s.diagnostics = diagnostics
    posts = [inf.Posterior(str(tmp_path / f"d_{c}.npz"), s.M, s.T, 2, inf.warmup_size() + 12, forecast=(6, 12), check=(2, 12),
                           groups=TABLE.G) for c in range(s.B)]
    with pytest.raises(EndOfSampling):                       # the run up to the end of the sampling phase is what is examined
        inf.run_mcmc(s, cfg, posts, log=open(os.devnull, "w"), seed=21, groups=TABLE,
                     forecast_calendar=(np.arange(6) + 0.5, np.arange(6) - 1.0),
                     check_calendar=(np.arange(2) + 0.25, np.arange(2) - 2.0))
    bursts = [kw for kw in seen if kw.get("forecast")]
    assert len(bursts) == 3 and all(kw["summarize"] is True and kw["groups"] == ("forecast", "check") for kw in bursts)
    assert all("groups" not in kw for kw in seen if not kw.get("forecast"))


# ---- 5. the compiler's account of the new kernel ---------------------------------------------------------------------------
def test_the_new_kernel_is_these_instances_without_scratch_at_full_occupancy():
    res = H.kernel_account("groups")
    new = ["k_group_sums<0>", "k_group_sums<1>"]
    assert sorted(res) == new, sorted(res)
    for k in new:
        assert res[k]["scratch_bytes_per_lane"] == 0 and res[k]["vgpr_spill"] == 0 and res[k]["sgpr_spill"] == 0, (k, res[k])
        # the LDS tile [64 days][3] and the three state sums, 64-bit
        assert res[k]["lds_bytes_per_block"] == (64 * 3 + 3) * 8, (k, res[k])
        assert res[k]["occupancy_waves_per_simd"] == 8

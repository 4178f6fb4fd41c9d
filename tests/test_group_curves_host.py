"""Group curves (include/seir_hip.h, "Group curves on the device"): everything that needs no GPU -- the symbols, the NumPy
definition of a group sum (`posterior.groups.weighted_sum_rows`) held three ways, the refusals before any GPU call,
run_mcmc's calls and datasets with a stub sampler, and the compiler's account of the new kernels."""
import ctypes
import math
import os

import numpy as np
import pytest

from covid19uk_amd import _lib, hdf5io, synth
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.posterior import groups as G
from covid19uk_amd.sampler import GROUP_CURVE_KEYS, GROUP_KEYS, GROUP_SOURCES, ChainSampler, PinnedTrace, Trace
from covid19uk_amd.seir import SeirModel
from tests import helpers as H
from tests.abi_lib import check_symbols
from tests.test_rt_quantiles_host import RtqStub
from tests.test_summary_host import CFG, _read
from tests.test_wb_host import WbStub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "seir_sampler_group_rt": "seir_sampler *s, const double *weights",
    "seir_sampler_group_wb": "seir_sampler *s, int32_t on",
    "seir_sampler_read_group_rt": "seir_sampler *s, int32_t first, int32_t count, double *Rg",
    "seir_sampler_read_group_rt_async": "seir_sampler *s, int32_t first, int32_t count, double *Rg",
    "seir_sampler_read_group_wb": "seir_sampler *s, int32_t first, int32_t count, double *Wg, double *Bg",
    "seir_sampler_read_group_wb_async": "seir_sampler *s, int32_t first, int32_t count, double *Wg, double *Bg",
    "seir_group_wsums": "seir_ctx *ctx, const double *v, int64_t nd, int32_t L, int32_t M, int32_t G, const int32_t *offsets, "
                        "const int32_t *members, const double *weights, double *out",
}


# ---- 1. the symbols ------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound_with_the_headers_types():
    lib = check_symbols(NEW)
    # a null sampler / context is refused before anything touches a device
    one = (ctypes.c_double * 2)(0.0, 1.0)
    idx = (ctypes.c_int32 * 2)(0, 1)
    assert lib.seir_sampler_group_rt(None, one) == _lib.ERR_INVALID
    assert lib.seir_sampler_group_wb(None, 1) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_group_rt(None, 0, 1, one) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_group_rt_async(None, 0, 1, one) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_group_wb(None, 0, 1, one, one) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_group_wb_async(None, 0, 1, one, one) == _lib.ERR_INVALID
    assert lib.seir_group_wsums(None, one, 1, 1, 1, 1, idx, idx, None, one) == _lib.ERR_INVALID
    for name in ("set_group_rt", "set_group_within_between", "read_group_rt", "read_group_wb"):
        assert callable(getattr(ChainSampler, name))
    assert callable(SeirModel.group_wsums)
    assert GROUP_CURVE_KEYS == ("rt_by_group", "within_by_group", "between_by_group")
    # the region totals' constants are what they were
    assert GROUP_KEYS == ("seir_by_group", "forecast_by_group", "forecast_group_state0", "check_by_group", "check_group_state0")
    assert [v[0] for v in GROUP_SOURCES.values()] == [0, 1, 2]
    assert "group_curves" in Trace.__dataclass_fields__ and "group_curves" in PinnedTrace.__init__.__code__.co_varnames
    # no new keyword on sample / sample_bursts: the sampler's state decides
    for fn in (ChainSampler.sample, ChainSampler.sample_bursts):
        assert not any("curve" in v or v.startswith("group_") for v in fn.__code__.co_varnames[:fn.__code__.co_argcount])
    # the definition is written once in the kernel file and names no fused multiply-add
    src = open(os.path.join(ROOT, "covid19uk_amd", "csrc", "group_curve_kernels.h")).read()
    assert "a_l = a_l + a_{l xor o}" in src and src.count("#pragma clang fp contract(off)") >= 3


# ---- 2. the NumPy definition, held three ways ------------------------------------------------------------------------------
def _one(n, M=None):
    M = n if M is None else M
    return G.GroupTable(["g"], np.array([0, n], np.int32), np.arange(n, dtype=np.int32))


def _loop(members, v, w=None):
    """The lane / butterfly rule, plainly: Python floats, one operation per line."""
    a = [0.0] * 64
    for lane in range(64):
        k = lane
        while k < len(members):
            p = float(v[members[k]])
            if w is not None:
                p = float(w[k]) * p
            a[lane] = a[lane] + p
            k += 64
    for o in (32, 16, 8, 4, 2, 1):
        a = [a[lane] + a[lane ^ o] for lane in range(64)]
    return a[0]


def test_the_definition_against_hand_cases():
    # n = 1: the value itself (and +0.0 for -0.0: the lane starts from +0.0)
    assert G.weighted_sum_rows(_one(1), np.array([3.5]))[0] == 3.5
    assert not np.signbit(G.weighted_sum_rows(_one(1), np.array([-0.0]))[0])
    assert G.weighted_sum_rows(_one(1), np.array([3.0]), np.array([0.1]))[0] == 0.1 * 3.0
    # n = 64: a lane a member, the butterfly alone.  1 + 2^-53 + 2^-53 ...: pairs (l, l ^ 32) first
    v = np.zeros(64)
    v[0], v[32], v[1], v[33] = 1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53
    # lane 0: 1 + 2^-53 = 1 (ties to even); lane 1: 2^-53 + 2^-53 = 2^-52; then 1 + 2^-52
    assert G.weighted_sum_rows(_one(64), v)[0] == 1.0 + 2.0 ** -52
    v = np.zeros(64)
    v[0], v[1], v[2] = 1.0, 2.0 ** -53, 2.0 ** -53             # lanes 0, 1, 2 meet as (0 + 1) + (2 + 3): 1 + 2^-53 = 1, twice
    assert G.weighted_sum_rows(_one(64), v)[0] == 1.0
    assert float(np.sum(v[[1, 2, 0]])) == 1.0 + 2.0 ** -52      # another order, other bits
    # n = 65: member 64 is lane 0's second term, added BEFORE the butterfly
    v = np.zeros(65)
    v[0], v[64], v[32] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert G.weighted_sum_rows(_one(65), v)[0] == 1.0           # (1 + 2^-53) = 1, then + 2^-53 = 1
    v[0], v[64], v[32] = 2.0 ** -53, 2.0 ** -53, 1.0
    assert G.weighted_sum_rows(_one(65), v)[0] == 1.0 + 2.0 ** -52
    # n = 129: lane 0 takes members 0, 64, 128 in ascending order
    v = np.zeros(129)
    v[0], v[64], v[128] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert G.weighted_sum_rows(_one(129), v)[0] == 1.0
    v[0], v[64], v[128] = 2.0 ** -53, 2.0 ** -53, 1.0
    assert G.weighted_sum_rows(_one(129), v)[0] == 1.0 + 2.0 ** -52
    # the weight is one rounding of its own, not fused into the add
    v, w = np.array([1.0 + 2.0 ** -30, -1.0]), np.array([1.0 + 2.0 ** -30, 1.0])
    assert G.weighted_sum_rows(_one(2), v, w)[0] == (1.0 + 2.0 ** -29) - 1.0       # the product's 2^-60 is rounded away


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 380])
def test_the_definition_against_fsum_and_a_plain_loop(n):
    rng = np.random.default_rng(n)
    M = n + 7
    members = np.sort(rng.choice(M, size=n, replace=False)).astype(np.int32)
    tab = G.GroupTable(["g", "all"], np.array([0, n, n + M], np.int32), np.concatenate([members, np.arange(M, dtype=np.int32)]))
    differs = False
    for trial in range(6):
        v = rng.standard_normal(M) * 10.0 ** rng.integers(-8, 9, size=M)      # mixed signs, 16 decades
        w = rng.standard_normal(n + M) * 10.0 ** rng.integers(-3, 4, size=n + M)
        for weights in (None, w):
            got = G.weighted_sum_rows(tab, v, weights)
            assert got.shape == (2,) and got.dtype == np.float64
            for g, mem in enumerate((members, np.arange(M))):
                wg = None if weights is None else weights[tab.offsets[g]:tab.offsets[g + 1]]
                assert got[g] == _loop(mem, v, wg)                            # every bit
                terms = v[mem] if wg is None else wg * v[mem]
                # derived: at most ceil(n / 64) adds in a lane and 6 in the butterfly, each within 2^-53 relative of a
                # partial sum that is at most sum |terms| in magnitude (to first order)
                bound = (math.ceil(len(mem) / 64) + 6) * 2.0 ** -53 * math.fsum(np.abs(terms))
                assert abs(got[g] - math.fsum(terms)) <= bound
                if float(np.sum(terms[::-1])) != got[g]:
                    differs = True
    assert differs or n <= 2, "the data does not tell one order from another"


def test_axes_batches_singletons_and_the_weights_shape():
    rng = np.random.default_rng(5)
    tab = G.parse_groups({"a": [0, 2, 4], "b": [1], "all": list(range(6))}, 6)
    v = rng.standard_normal((3, 4, 6))
    w = rng.standard_normal(10)
    got = G.weighted_sum_rows(tab, v, w)
    assert got.shape == (3, 4, 3)
    for i in range(3):
        for t in range(4):
            for g in range(3):
                assert got[i, t, g] == _loop(tab.rows(g), v[i, t], w[tab.offsets[g]:tab.offsets[g + 1]])
    assert np.array_equal(G.weighted_sum_rows(tab, np.moveaxis(v, -1, 0), w, axis=0), np.moveaxis(got, -1, 0))
    # singletons with weight 1.0 return the input bits
    single = G.parse_groups({str(m): [m] for m in range(6)}, 6)
    assert np.array_equal(G.weighted_sum_rows(single, v, np.ones(6)).view(np.uint64), v.view(np.uint64))
    assert np.array_equal(G.weighted_sum_rows(single, v).view(np.uint64), v.view(np.uint64))
    with pytest.raises(ValueError, match="aligned"):
        G.weighted_sum_rows(tab, v, np.ones(9))
    # the population weights sum to one within a group and are aligned with the members
    N = np.array([10.0, 20.0, 40.0, 5.0, 25.0, 100.0])
    pw = G.rt_weights(tab, N)
    assert pw.shape == (10,) and np.array_equal(pw[:3], N[[0, 2, 4]] / 75.0) and pw[3] == 1.0
    assert np.array_equal(pw[4:], N / N.sum())


def test_the_statistics_of_the_curves():
    rng = np.random.default_rng(9)
    rg = rng.uniform(0.5, 1.5, size=(7, 2, 3))
    mean, var, p1 = G.curve_moments(rg)
    assert np.array_equal(mean, rg.mean(0)) and np.array_equal(var, rg.var(0)) and np.array_equal(p1, (rg > 1).mean(0))
    assert all(np.all(np.isnan(x)) and x.shape == (2, 3) for x in G.curve_moments(np.empty((0, 2, 3))))
    wg = np.array([[3.0, 0.0], [1.0, 0.0], [0.0, 0.0]])
    bg = np.array([[1.0, 0.0], [3.0, 2.0], [0.0, 0.0]])
    d, share, gt = G.share_stats(wg, bg)                       # the third draw is undefined in both cells
    assert np.array_equal(d, [2.0, 1.0]) and np.array_equal(share, [(0.75 + 0.25) / 2, 0.0]) and np.array_equal(gt, [0.5, 0.0])
    d, share, gt = G.share_stats(np.zeros((4, 2)), np.zeros((4, 2)))
    assert np.array_equal(d, [0.0, 0.0]) and np.all(np.isnan(share)) and np.all(np.isnan(gt))


# ---- 3. the refusals, all before any GPU call -----------------------------------------------------------------------------
def test_every_refusal_before_any_gpu_call(tmp_path):
    cov = synth.make_covariates("ni11")
    events, _, _ = synth.simulate_epidemic(cov)
    data = str(tmp_path / "data.npz")
    inf.write_inference_data(data, cov, events[..., 2])
    out = str(tmp_path / "out.npz")
    grp = {"a": [0, 1]}
    for cfg, kw, word in (
            (dict(CFG, rt=3, groups_rt="on"), {}, "groups_rt given without groups"),
            (dict(CFG, rt=3), dict(groups_rt=True), "groups_rt given without groups"),
            (dict(CFG, groups=grp, groups_rt=True, summaries="only"), {}, "groups_rt given without rt"),
            (dict(CFG, within_between=3, groups_within_between="on"), {}, "groups_within_between given without groups"),
            (dict(CFG, groups=grp, summaries="only"), dict(groups_within_between=True), "groups_within_between given without within_between"),
            (dict(CFG, groups=grp, rt=3, groups_within_between=True), {}, "groups_within_between given without within_between"),
            (dict(CFG, groups=grp, rt=3, groups_rt="sometimes"), {}, "on or off"),
            # (rt, within_between, groups) without the new keys is still "no effect"
            (dict(CFG, rt=3, within_between=3, groups=grp), {}, "no effect"),
            (dict(CFG, rt=3, within_between=3, groups=grp, groups_rt="off", groups_within_between=False), {}, "no effect")):
        with pytest.raises(ValueError, match=word):
            inf.mcmc(data, out, cfg, **kw)
    assert not os.path.exists(out)
    tab = G.parse_groups(grp, 3)
    with pytest.raises(ValueError, match="no effect"):
        G.require_source(tab, "off", 0, 0)                     # the four-positional-argument form behaves as before
    G.require_source(tab, "off", 0, 0, groups_rt=True)
    G.require_source(tab, "off", 0, 0, groups_within_between=True)
    G.require_source(None, "off", 0, 0)
    G.require_curves(tab, True, 3, True, 3)
    G.require_curves(None, False, 0, False, 0)
    for v, want in ((None, False), (False, False), (True, True), ("on", True), ("off", False), (" On ", True)):
        assert G.switch(v, "x") is want
    for bad in (1, "yes", 0.5):
        with pytest.raises(ValueError, match="on or off"):
            G.switch(bad, "x")


def test_the_cli_flags_parse(tmp_path, monkeypatch):
    import yaml
    cpath = str(tmp_path / "c.yaml")
    with open(cpath, "w") as f:
        yaml.safe_dump(dict(Mcmc=CFG), f)
    seen = {}
    monkeypatch.setattr(inf, "mcmc", lambda *a, **kw: (seen.clear(), seen.update(kw)))
    inf.main(["-c", cpath, "-o", "x", "--rt", "7", "--within-between", "7", "--groups", "nations", "--groups-rt",
              "--groups-within-between", "data.nc"])
    assert seen["groups_rt"] is True and seen["groups_within_between"] is True and seen["groups"] == "nations"
    inf.main(["-c", cpath, "-o", "x", "--rt", "7", "--groups", "nations", "--groups-rt", "data.nc"])
    assert seen["groups_rt"] is True and "groups_within_between" not in seen
    inf.main(["-c", cpath, "-o", "x", "--rt", "7", "--groups", "nations", "data.nc"])
    assert "groups_rt" not in seen and "groups_within_between" not in seen       # absent: mcmc is called as before


# ---- 4. run_mcmc with a stub sampler --------------------------------------------------------------------------------------
TABLE = G.parse_groups({"all": [0, 1, 2], "ends": [0, 2]}, 3)
POP = np.array([10.0, 20.0, 40.0])


class BaseStub(WbStub):
    """WbStub with the draw store of the R_t quantiles and the group table: a sampler that has never heard of the curves."""
    keep_rt_draws = RtqStub.keep_rt_draws
    rt_quantiles = RtqStub.rt_quantiles

    def set_groups(self, offsets, members):
        self.calls.append(("set_groups", np.asarray(offsets).copy(), np.asarray(members).copy()))
        self.G = len(offsets) - 1

    def _trace(self, n, groups=False, **kw):
        tr = super()._trace(n, **kw)
        if groups:
            assert tuple(groups) == ("trace",) and kw.get("summarize")
            idx = self.sweeps - n + np.arange(n)
            tr.groups = {"seir_by_group": np.broadcast_to(idx[:, None, None, None, None], (n, self.B, self.G, self.T, 3)).astype(np.int64)}
        return tr


class CurveStub(BaseStub):
    """BaseStub with the switches: a draw's group curves are functions of its sweep number, the chain, the group and the day."""
    rt_on = wb_on = False

    def set_group_rt(self, weights):
        self.calls.append(("set_group_rt", np.asarray(weights).copy()))
        self.rt_on = True

    def set_group_within_between(self, on):
        self.calls.append(("set_group_within_between", on))
        self.wb_on = bool(on)

    def curve(self, idx, D, scale):
        b, g, t = np.arange(self.B)[None, :, None, None], np.arange(self.G)[None, None, :, None], np.arange(D)[None, None, None, :]
        return scale * (0.5 + ((idx[:, None, None, None] * 7 + 3 * b + 5 * g + t) % 13) / 12.0)

    def _trace(self, n, **kw):
        tr = super()._trace(n, **kw)
        idx = self.sweeps - n + np.arange(n)
        gc = {}
        if kw.get("rt") and self.rt_on:
            gc["rt_by_group"] = self.curve(idx, self.D, 1.0)
        if kw.get("within_between") and self.wb_on:
            gc["within_by_group"] = self.curve(idx, self.Dw, 3.0)
            gc["between_by_group"] = self.curve(idx + 1, self.Dw, 2.0)
            gc["within_by_group"][:, 1, 0, 0] = gc["between_by_group"][:, 1, 0, 0] = 0.0      # chain 1: a cell that is never defined
        tr.group_curves = gc or None
        return tr


def _run(tmp_path, tag, config, ext=".npz", cap=800, stub=CurveStub, groups=None):
    s = stub()
    s.cap = cap
    nb, ns = config["num_bursts"], config["num_burst_samples"]
    D, Dw = inf.rt_mode(config), inf.within_between_mode(config)
    names = [str(tmp_path / f"{tag}_{c}{ext}") for c in range(s.B)]
    kw = {} if config.get("summaries", "off") == "off" else dict(summaries=config["summaries"])
    for key, v in (("rt", D), ("within_between", Dw)):
        if v:
            kw[key] = (v, nb * ns)
    curves = {k: (d, nb * ns) for k, key, d in (("rt", "groups_rt", D), ("within_between", "groups_within_between", Dw))
              if config.get(key)}
    if groups is not None:
        kw["groups"] = groups.G
        if curves:
            kw["group_curves"] = curves
    posts = [inf.Posterior(name, s.M, s.T, 2, inf.warmup_size() + nb * ns, **kw) for name in names]
    logname = str(tmp_path / f"{tag}.log")
    fkw = dict(seed=21)
    if D:
        fkw["rt_weight"] = POP / POP.sum()
    if groups is not None:
        fkw["groups"] = groups
        fkw["population"] = POP
        for p in posts:
            p.write_groups(groups, POP, np.arange(12.0).reshape(3, 4))
    with open(logname, "w") as log:
        inf.run_mcmc(s, config, posts, log=log, **fkw)
    for p in posts:
        p.close()
    return s, [_read(n) for n in names], open(logname).read()


def _untimed(log):
    return [ln for ln in log.splitlines() if not ln.startswith("Sampling: ")]      # that line carries a wall-clock rate


FULL = dict(CFG, num_bursts=3, num_burst_samples=4, rt=3, rt_quantiles=[0.05, 0.5, 0.95], within_between=2, summaries="only")
CURVE_SETS = {"groups/rt_weights", "samples/R_t_by_group", "samples/within_pressure_by_group", "samples/between_pressure_by_group",
              "rt/group_R_t_mean", "rt/group_R_t_var", "rt/group_prob_gt1", "rt/group_R_t_quantiles", "rt/pooled_group_R_t_quantiles",
              "within_between/group_defined", "within_between/group_within_share_mean", "within_between/group_p_within_gt_between"}


def test_absent_calls_nothing_new_and_writes_todays_datasets(tmp_path):
    s0, f0, log0 = _run(tmp_path, "parent", FULL, stub=BaseStub, groups=TABLE)   # a sampler that has never heard of the curves
    s1, f1, log1 = _run(tmp_path, "absent", FULL, groups=TABLE)
    assert [c[0] for c in s1.calls] == [c[0] for c in s0.calls]
    assert not any(c[0] in ("set_group_rt", "set_group_within_between") for c in s1.calls)
    for a, b in zip(s1.calls, s0.calls):
        if a[0] in ("sample", "burst"):
            assert a[1] == b[1] and a[2] == b[2]
    assert "by group, last day" not in log1 and _untimed(log1) == _untimed(log0)
    for c in range(2):
        assert set(f1[c]) == set(f0[c]) and not (CURVE_SETS & set(f1[c]))
        for k in f0[c]:
            assert np.array_equal(f1[c][k], f0[c][k], equal_nan=f0[c][k].dtype.kind == "f"), k
    # the switches "off" are absent too
    s2, f2, log2 = _run(tmp_path, "off", dict(FULL, groups_rt="off", groups_within_between=False), groups=TABLE)
    assert [c[0] for c in s2.calls] == [c[0] for c in s0.calls] and _untimed(log2) == _untimed(log0)
    # and the refusals of run_mcmc itself
    with pytest.raises(ValueError, match="groups_rt given without groups"):
        _run(tmp_path, "r1", dict(FULL, groups_rt=True))
    with pytest.raises(ValueError, match="groups_rt given without rt"):
        _run(tmp_path, "r2", dict(FULL, rt=None, rt_quantiles=None, groups_rt=True), groups=TABLE)
    with pytest.raises(ValueError, match="groups_within_between given without within_between"):
        _run(tmp_path, "r3", dict(FULL, within_between=None, groups_within_between=True), groups=TABLE)
    with pytest.raises(ValueError, match="no effect"):
        _run(tmp_path, "r4", dict(FULL, summaries="off"), groups=TABLE)


@pytest.mark.parametrize("summaries,overlap,ext,which", [("only", True, ".hd5", "both"), ("off", False, ".npz", "both"),
                                                         ("on", True, ".npz", "rt"), ("off", True, ".npz", "wb")])
def test_the_switches_are_set_once_behind_the_table_and_the_datasets_are_written(tmp_path, summaries, overlap, ext, which):
    assert hdf5io.available(), "the HDF5 writer is part of what this project needs"
    nb, ns, D, Dw, probs = 3, 4, 3, 2, (0.05, 0.5, 0.95)
    rt_on, wb_on = which in ("both", "rt"), which in ("both", "wb")
    cfg = dict(FULL, summaries=summaries, **(dict(groups_rt="on") if rt_on else {}),
               **(dict(groups_within_between=True) if wb_on else {}))
    cap = 800 if overlap else ns
    s, files, log = _run(tmp_path, "on", cfg, ext=ext, cap=cap, groups=TABLE)
    names = [c[0] for c in s.calls]
    # once each, behind the table and before the first draw
    first_draw = min(i for i, n in enumerate(names) if n == "sample")
    assert names.count("set_groups") == 1
    for key, on in (("set_group_rt", rt_on), ("set_group_within_between", wb_on)):
        assert names.count(key) == (1 if on else 0)
        if on:
            assert names.index("set_groups") < names.index(key) < first_draw
    if rt_on:
        assert np.array_equal(s.calls[names.index("set_group_rt")][1], G.rt_weights(TABLE, POP))
    if wb_on:
        assert s.calls[names.index("set_group_within_between")][1] is True
    # no new keyword on the draws: the calls are those of a run without the switches
    if summaries != "off":
        base, bf, blog = _run(tmp_path, "base", {k: v for k, v in cfg.items() if not k.startswith("groups_")}, ext=ext, cap=cap,
                              stub=BaseStub, groups=TABLE)
        stripped = [c for c in s.calls if c[0] not in ("set_group_rt", "set_group_within_between")]
        assert [c[0] for c in stripped] == [c[0] for c in base.calls]
        for a, b in zip(stripped, base.calls):
            if a[0] in ("sample", "burst"):
                assert a[1] == b[1] and a[2] == b[2]
    else:
        assert all("groups" not in c[2] for c in s.calls if c[0] in ("sample", "burst"))   # the curves alone: no sums to ask for
        assert "Groups:" not in log
        bf = None
    W = inf.warmup_size()
    idx = W + np.arange(nb * ns)
    new = set()
    if rt_on:
        new |= {k for k in CURVE_SETS if k.startswith(("rt/", "samples/R_t", "groups/rt"))}
    if wb_on:
        new |= {k for k in CURVE_SETS if "within" in k or "between" in k}
    for c, f in enumerate(files):
        assert CURVE_SETS & set(f) == new
        if bf is not None:
            assert set(f) == set(bf[c]) | new
            for k in bf[c]:
                assert np.array_equal(f[k], bf[c][k], equal_nan=bf[c][k].dtype.kind == "f"), k
        if rt_on:
            assert np.array_equal(f["groups/rt_weights"], G.rt_weights(TABLE, POP))
            rg_all = s.curve(idx, D, 1.0)                      # [n,B,G,D]
            rg = f["samples/R_t_by_group"]
            assert rg.dtype == np.float64 and rg.shape == (nb * ns, 2, D) and np.array_equal(rg, rg_all[:, c])
            assert np.array_equal(f["rt/group_R_t_mean"], rg.mean(0)) and np.array_equal(f["rt/group_R_t_var"], rg.var(0))
            assert np.array_equal(f["rt/group_prob_gt1"], (rg > 1.0).mean(0))
            own, pooled = f["rt/group_R_t_quantiles"], f["rt/pooled_group_R_t_quantiles"]
            assert own.shape == pooled.shape == (3, 2, D)
            np.testing.assert_allclose(own, np.quantile(rg, probs, axis=0), rtol=1e-12, atol=0)
            np.testing.assert_allclose(pooled, np.quantile(rg_all.reshape(-1, 2, D), probs, axis=0), rtol=1e-12, atol=0)
        if wb_on:
            wg, bg = f["samples/within_pressure_by_group"], f["samples/between_pressure_by_group"]
            assert wg.shape == bg.shape == (nb * ns, 2, Dw)
            want_w, want_b = s.curve(idx, Dw, 3.0)[:, c], s.curve(idx + 1, Dw, 2.0)[:, c]
            if c == 1:
                want_w[:, 0, 0] = want_b[:, 0, 0] = 0.0
            assert np.array_equal(wg, want_w) and np.array_equal(bg, want_b)
            d, share, gt = G.share_stats(wg, bg)
            assert np.array_equal(f["within_between/group_defined"], d)
            assert np.array_equal(f["within_between/group_within_share_mean"], share, equal_nan=True)
            assert np.array_equal(f["within_between/group_p_within_gt_between"], gt, equal_nan=True)
            assert d[0, 0] == (0 if c == 1 else nb * ns) and np.isnan(share[0, 0]) == (c == 1)
            np.testing.assert_allclose(share[1], (wg[:, 1] / (wg[:, 1] + bg[:, 1])).mean(0), rtol=1e-15)
    # one log line per product, with every group's last-day value and its 0.05 / 0.95 quantiles
    assert log.count("R_t by group, last day") == (1 if rt_on else 0)
    assert log.count("Within share of the infection pressure") == (1 if wb_on else 0)
    if rt_on:
        line = [ln for ln in log.splitlines() if ln.startswith("R_t by group")][0]
        last = s.curve(idx, D, 1.0)[..., -1].reshape(-1, 2)
        q = np.quantile(last, [0.05, 0.95], axis=0)
        assert f"all {last[:, 0].mean():.3g} [{q[0, 0]:.3g}, {q[1, 0]:.3g}]" in line and "ends " in line
    if wb_on:
        assert "from outside each member location" in log


# ---- 5. the compiler's account of the new kernels ---------------------------------------------------------------------------
def test_the_new_kernels_are_these_instances_with_their_parents_occupancy_behind_everything_else():
    res = H.kernel_account("group_curves")
    new = ["k_group_wsums<0>", "k_group_wsums<1>", "k_rt_cells_from_keep", "k_rt_trace_cells<4>", "k_wb_trace_cells<4>"]
    assert sorted(res) == new, sorted(res)
    for k in new:
        assert res[k]["scratch_bytes_per_lane"] == 0 and res[k]["vgpr_spill"] == 0 and res[k]["sgpr_spill"] == 0, (k, res[k])
        assert res[k]["lds_bytes_per_block"] == 0, (k, res[k])   # k_group_wsums shares nothing between its waves; the two
        #                                                          trace kernels' LDS is dynamic, as their parents'
    base = H.kernel_account("base")
    wb = H.kernel_account("wb")
    # the heavy kernels keep their parents' occupancy
    assert res["k_rt_trace_cells<4>"]["occupancy_waves_per_simd"] == base["k_rt_trace<4>"]["occupancy_waves_per_simd"] == 5
    assert res["k_wb_trace_cells<4>"]["occupancy_waves_per_simd"] == wb["k_wb_trace<4>"]["occupancy_waves_per_simd"]
    assert res["k_group_wsums<0>"]["occupancy_waves_per_simd"] == res["k_group_wsums<1>"]["occupancy_waves_per_simd"] == 8
    # the existing kernels' text is what it was: the new file restates the loops and is included behind everything else
    hip = open(os.path.join(ROOT, "covid19uk_amd", "csrc", "seir_hip.hip")).read()
    assert hip.count('#include "group_curve_kernels.h"') == 1
    assert hip.index('#include "group_curve_kernels.h"') > hip.index("static void groups_launch(const Dims &d, hipStream_t st, const GroupTable &gt, bool ev16, const void *ev, int M, int L,\n                          long long ev_d0, long long out_d0, long long nd, int64_t *out, const int *St0, long long plane, int ndp,\n                          int64_t *state0) {")

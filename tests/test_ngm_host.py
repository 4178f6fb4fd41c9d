"""Group next-generation matrix (include/seir_hip.h, "Group next-generation matrix on the device"): everything that needs
no GPU -- the symbols, the NumPy definition (`posterior.groups.ngm_rows`, `group_ngm`) against plain Python loops, the
statistics against exact rationals, the spectral radius against hand cases, the refusals before any GPU call, run_mcmc's
calls and datasets with a stub sampler, and the compiler's account of the new kernel."""
import ctypes
import os
import warnings
from fractions import Fraction

import numpy as np
import pytest

from covid19uk_amd import _lib, hdf5io, synth
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.posterior import groups as G
from covid19uk_amd.sampler import BURST_PRODUCTS, GROUP_CURVE_KEYS, ChainSampler
from covid19uk_amd.seir import SeirModel
from tests import helpers as H
from tests.abi_lib import check_symbols
from tests.test_group_curves_host import FULL, POP, TABLE, BaseStub, CurveStub, _loop, _run, _untimed
from tests.test_summary_host import CFG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "seir_sampler_group_ngm": "seir_sampler *s, const double *weights, int64_t cap",
    "seir_sampler_read_group_ngm": "seir_sampler *s, int64_t first_draw, int64_t count, double *out",
    "seir_group_ngm_rows": "seir_ctx *ctx, int32_t n, const double *theta, const int32_t *events, int32_t days, int32_t G, "
                           "const int32_t *offsets, const int32_t *members, double *out",
}


# ---- 1. the symbols ------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound_with_the_headers_types():
    lib = check_symbols(NEW)
    # a null sampler / context is refused before anything touches a device
    one = (ctypes.c_double * 2)(0.0, 1.0)
    idx = (ctypes.c_int32 * 6)(0, 1, 0, 0, 0, 0)
    assert lib.seir_sampler_group_ngm(None, one, 4) == _lib.ERR_INVALID
    assert lib.seir_sampler_read_group_ngm(None, 0, 1, one) == _lib.ERR_INVALID
    assert lib.seir_group_ngm_rows(None, 1, one, idx, 1, 1, idx, idx, one) == _lib.ERR_INVALID
    for name in ("set_group_ngm", "read_group_ngm"):
        assert callable(getattr(ChainSampler, name))
    assert callable(SeirModel.group_ngm_rows)
    assert ChainSampler.__new__(ChainSampler)._state().ngm_cap == 0   # without a handle: a subclass that never runs __init__
    # not a burst product: the tables of the products are what they were
    assert GROUP_CURVE_KEYS == ("rt_by_group", "within_by_group", "between_by_group")
    assert not any("ngm" in p.field for p in BURST_PRODUCTS)
    for fn in (ChainSampler.sample, ChainSampler.sample_bursts):
        assert not any("ngm" in v for v in fn.__code__.co_varnames[:fn.__code__.co_argcount])
    # the definition is written once in the kernel file, which is included once, behind the group curves' launches
    src = open(os.path.join(ROOT, "covid19uk_amd", "csrc", "ngm_kernels.h")).read()
    assert "member POSITIONS k = p, p + 4, ..." in src and "rt_combine(p0, p1, p2, p3, period)" in src
    assert "fma" not in src.lower().replace("no fma", "") and "atomic" not in src.lower().replace("no floating-point atomics", "")
    hip = open(os.path.join(ROOT, "covid19uk_amd", "csrc", "seir_hip.hip")).read()
    assert hip.count('#include "ngm_kernels.h"') == 1
    assert hip.index('#include "ngm_kernels.h"') > hip.index("static void gcurve_lds_attributes(int Mp) {")


# ---- 2. the NumPy definition against plain loops ----------------------------------------------------------------------------
def _mixed(rng, shape):
    """Mixed signs, magnitudes over 16 decades: another order of the adds gives other bits."""
    return rng.standard_normal(shape) * 10.0 ** rng.integers(-8, 9, size=shape)


def _rows_loop(members, terms, t, j, period):
    """The position-mod-4 rule, plainly: Python floats, one operation per line."""
    p = [0.0, 0.0, 0.0, 0.0]
    for k, m in enumerate(members):
        p[k % 4] = p[k % 4] + float(terms[m, t, j])
    v = (p[0] + p[1]) + (p[2] + p[3])
    return v * period


@pytest.mark.parametrize("n", [1, 3, 4, 5, 64, 65])
def test_the_definition_against_plain_loops_at_every_group_size(n):
    rng = np.random.default_rng(n)
    M, D = n + 3, 2
    members = np.sort(rng.choice(M, size=n, replace=False)).astype(np.int32)
    tab = G.GroupTable(["g", "all", "last"], np.array([0, n, n + M, n + M + 1], np.int32),
                       np.concatenate([members, np.arange(M, dtype=np.int32), [M - 1]]).astype(np.int32))
    terms = _mixed(rng, (M, D, M))
    w = _mixed(rng, tab.members.shape)
    period = 1.0 + 2.0 ** -20
    P = G.ngm_rows(terms, tab, period)
    assert P.shape == (3, D, M) and P.dtype == np.float64
    for g in range(3):
        for t in range(D):
            for j in range(M):
                assert P[g, t, j] == _rows_loop(tab.rows(g), terms, t, j, period)
    assert np.array_equal(P[2].view(np.uint64), ((terms[M - 1] + 0.0) * period).view(np.uint64))    # a singleton: the term itself
    K = G.group_ngm(P, tab, w)
    assert K.shape == (3, 3, D) and K.flags["C_CONTIGUOUS"]
    for g in range(3):
        for h in range(3):
            for t in range(D):
                assert K[g, h, t] == _loop(tab.rows(h), P[g, t], w[tab.offsets[h]:tab.offsets[h + 1]])
    # leading axes are carried: [draws, chains, ...]
    tb = _mixed(rng, (2, 3, M, D, M))
    Pb = G.ngm_rows(tb, tab)
    assert np.array_equal(Pb[1, 2], G.ngm_rows(tb[1, 2], tab)) and np.array_equal(G.group_ngm(Pb, tab, w)[1, 2], G.group_ngm(Pb[1, 2], tab, w))
    if n >= 5:
        # the data does tell orders apart: a plain ascending sum over the members differs somewhere
        assert not np.array_equal(terms[members].sum(axis=0) * period, P[0])


def test_the_definition_hand_cases():
    one = G.GroupTable(["g"], np.array([0, 5], np.int32), np.arange(5, dtype=np.int32))
    t = np.zeros((5, 1, 1))
    # positions 0 and 4 share partial 0 and meet FIRST: (1 + 2^-53) = 1, then 1 + 2^-53 (position 1) = 1
    t[0], t[4], t[1] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert G.ngm_rows(t, one)[0, 0, 0] == 1.0
    # positions 1 and 2 are different partials: p1 = 2^-53 joins p0 = 1 (lost), p2 = 2^-53 alone, then 1 + 2^-53 = 1
    t[:] = 0.0
    t[0], t[1], t[2] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert G.ngm_rows(t, one)[0, 0, 0] == 1.0
    # positions 2 and 3 meet as (p2 + p3) = 2^-52 before they join (p0 + p1) = 1
    t[:] = 0.0
    t[0], t[2], t[3] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert G.ngm_rows(t, one)[0, 0, 0] == 1.0 + 2.0 ** -52
    # fewer than four members: the other partials stay +0.0, and -0.0 comes back as +0.0
    assert not np.signbit(G.ngm_rows(np.full((5, 1, 1), -0.0), one)[0, 0, 0])
    # the period is one multiplication at the end
    assert G.ngm_rows(np.full((5, 1, 1), 0.1), one, 3.0)[0, 0, 0] == (((0.1 + 0.1) + 0.1) + (0.1 + 0.1)) * 3.0
    assert G.is_partition(G.parse_groups({"a": [0, 2], "b": [1]}, 3), 3)
    assert not G.is_partition(G.parse_groups({"a": [0, 2], "b": [0, 1]}, 3), 3)
    assert not G.is_partition(G.parse_groups({"a": [0, 2]}, 3), 3)


# ---- 3. the statistics against exact rationals -------------------------------------------------------------------------------
def test_ngm_stats_against_fractions_and_numpy_quantiles():
    rng = np.random.default_rng(4)
    n, Gn, D, probs = 9, 3, 2, (0.05, 0.5, 0.95)
    K = rng.integers(1, 1 << 20, (n, Gn, Gn, D)) / float(1 << 10)
    R = K.sum(axis=1) * 1.25                                       # [n, h, D]: column sums and then some
    st = G.ngm_stats(K, R, probs)
    assert set(st) == {"K_mean", "K_var", "local_share", "local_share_mean", "K_quantiles", "local_share_quantiles"}
    for g in range(Gn):
        for h in range(Gn):
            for t in range(D):
                x = [Fraction(float(v)) for v in K[:, g, h, t]]
                mean = sum(x) / n
                var = sum((v - mean) ** 2 for v in x) / n
                assert abs(Fraction(float(st["K_mean"][g, h, t])) - mean) <= abs(mean) * Fraction(1, 10 ** 12)
                assert abs(Fraction(float(st["K_var"][g, h, t])) - var) <= var * Fraction(1, 10 ** 12)
    share = np.empty((n, Gn, D))
    for i in range(n):
        for h in range(Gn):
            for t in range(D):
                share[i, h, t] = float(K[i, h, h, t]) / float(R[i, h, t])
    assert np.array_equal(st["local_share"], share)
    for h in range(Gn):
        for t in range(D):
            mean = sum(Fraction(float(v)) for v in share[:, h, t]) / n
            assert abs(Fraction(float(st["local_share_mean"][h, t])) - mean) <= mean * Fraction(1, 10 ** 12)
    np.testing.assert_allclose(st["K_quantiles"], np.quantile(K, probs, axis=0), rtol=1e-12, atol=0)
    np.testing.assert_allclose(st["local_share_quantiles"], np.quantile(share, probs, axis=0), rtol=1e-12, atol=0)
    assert "K_quantiles" not in G.ngm_stats(K, R)
    # a draw with R_t_by_group == 0 gives NaN, without a warning; the other cells are untouched
    R0 = R.copy()
    R0[3, 1, 0] = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s0 = G.ngm_stats(K, R0, probs)
        none = G.ngm_stats(K[:0], R[:0], probs)
    assert np.isnan(s0["local_share"][3, 1, 0]) and np.isnan(s0["local_share"]).sum() == 1
    assert np.isnan(s0["local_share_mean"][1, 0]) and np.isnan(s0["local_share_quantiles"][:, 1, 0]).all()
    keep = np.ones((Gn, D), bool)
    keep[1, 0] = False
    assert np.array_equal(s0["local_share_mean"][keep], st["local_share_mean"][keep])
    assert np.array_equal(s0["local_share_quantiles"][:, keep], st["local_share_quantiles"][:, keep])
    assert np.array_equal(s0["K_mean"], st["K_mean"])
    assert all(np.all(np.isnan(none[k])) for k in ("K_mean", "K_var", "local_share_mean", "K_quantiles", "local_share_quantiles"))
    assert none["K_quantiles"].shape == (3, Gn, Gn, D) and none["local_share"].shape == (0, Gn, D)
    with pytest.raises(ValueError, match="need"):
        G.ngm_stats(K, R[:, :2])


def test_spectral_radius_hand_cases():
    rng = np.random.default_rng(8)
    # diagonal: the largest entry
    d = rng.uniform(0.1, 3.0, size=(4, 5))                         # [G, D]
    K = np.zeros((4, 4, 5))
    K[np.arange(4), np.arange(4)] = d
    np.testing.assert_allclose(G.spectral_radius(K), d.max(axis=0), rtol=1e-14)
    # rank one u v^T: the trace v . u
    u, v = rng.uniform(0.1, 2.0, size=(2, 6, 3))
    K = u[:, None, :] * v[None, :, :]
    np.testing.assert_allclose(G.spectral_radius(K), (u * v).sum(axis=0), rtol=1e-13)
    # leading axes are carried, a single group is its entry
    Kb = rng.uniform(0.0, 2.0, size=(3, 2, 5, 5, 4))
    rho = G.spectral_radius(Kb)
    assert rho.shape == (3, 2, 4) and np.array_equal(rho[2, 1], G.spectral_radius(Kb[2, 1]))
    assert np.array_equal(G.spectral_radius(np.full((1, 1, 2), 0.7)), [0.7, 0.7])
    assert G.spectral_radius(np.empty((0, 3, 3, 2))).shape == (0, 2)
    # the Perron root of a positive matrix is monotone in its entries: (1 +- eps) A <= A' <= ... brackets it by (1 +- eps)
    eps = 1e-3
    A = rng.uniform(0.5, 1.5, size=(5, 5, 1))
    Ap = A * (1.0 + eps * rng.uniform(-1.0, 1.0, size=A.shape))
    r, rp = G.spectral_radius(A)[0], G.spectral_radius(Ap)[0]
    slack = 1e-13
    assert (1.0 - eps) * r * (1.0 - slack) <= rp <= (1.0 + eps) * r * (1.0 + slack)
    with pytest.raises(ValueError, match="G, G, D"):
        G.spectral_radius(np.zeros((2, 3, 4)))


# ---- 4. the refusals, all before any GPU call -----------------------------------------------------------------------------
def test_every_refusal_before_any_gpu_call(tmp_path):
    cov = synth.make_covariates("ni11")
    events, _, _ = synth.simulate_epidemic(cov)
    data = str(tmp_path / "data.npz")
    inf.write_inference_data(data, cov, events[..., 2])
    out = str(tmp_path / "out.npz")
    grp = {"a": [0, 1]}
    for cfg, kw, word in (
            (dict(CFG, rt=3, groups_ngm="on"), {}, "groups_ngm given without groups"),
            (dict(CFG, rt=3), dict(groups_ngm=True), "groups_ngm given without groups"),
            (dict(CFG, groups=grp, groups_ngm=True, summaries="only"), {}, "groups_ngm given without rt"),
            (dict(CFG, groups=grp, rt=3, groups_ngm=True), {}, "groups_ngm given without groups_rt"),
            (dict(CFG, groups=grp, rt=3, groups_rt="off"), dict(groups_ngm=True), "groups_ngm given without groups_rt"),
            (dict(CFG, groups=grp, rt=3, groups_rt=True, groups_ngm="sometimes"), {}, "on or off"),
            # off with nothing else set has no effect, as the group curves
            (dict(CFG, rt=3, groups=grp, groups_ngm="off"), {}, "no effect"),
            (dict(CFG, rt=3, groups=grp, groups_rt=False, groups_ngm=False), {}, "no effect")):
        with pytest.raises(ValueError, match=word):
            inf.mcmc(data, out, cfg, **kw)
    assert not os.path.exists(out)
    tab = G.parse_groups(grp, 3)
    G.require_ngm(tab, True, 3, True)
    G.require_ngm(None, False, 0, False)
    G.require_ngm(tab, False, 0, False)
    # the signatures of the others are what they were
    G.require_source(tab, "off", 0, 0, groups_rt=True)
    G.require_curves(tab, True, 3, True, 3)
    assert G.require_source.__code__.co_argcount == 6 and G.require_curves.__code__.co_argcount == 5


def test_the_cli_flag_parses(tmp_path, monkeypatch):
    import yaml
    cpath = str(tmp_path / "c.yaml")
    with open(cpath, "w") as f:
        yaml.safe_dump(dict(Mcmc=CFG), f)
    seen = {}
    monkeypatch.setattr(inf, "mcmc", lambda *a, **kw: (seen.clear(), seen.update(kw)))
    inf.main(["-c", cpath, "-o", "x", "--rt", "7", "--groups", "nations", "--groups-rt", "--groups-ngm", "data.nc"])
    assert seen["groups_ngm"] is True and seen["groups_rt"] is True and seen["groups"] == "nations"
    inf.main(["-c", cpath, "-o", "x", "--rt", "7", "--groups", "nations", "--groups-rt", "data.nc"])
    assert "groups_ngm" not in seen                                # absent: mcmc is called as before


# ---- 5. run_mcmc with a stub sampler --------------------------------------------------------------------------------------
PART = G.parse_groups({"north": [0, 1], "south": [2]}, 3)


class NgmStub(CurveStub):
    """CurveStub with the switch: a draw's K is a function of its position, the chain, the two groups and the day."""
    ngm_cap = 0

    def set_group_ngm(self, weights, cap):
        self.calls.append(("set_group_ngm", np.asarray(weights).copy(), cap))
        self.ngm_cap = cap

    def K(self, idx):
        b, g = np.arange(self.B)[None, :, None, None, None], np.arange(self.G)[None, None, :, None, None]
        h, t = np.arange(self.G)[None, None, None, :, None], np.arange(self.D)[None, None, None, None, :]
        return 0.05 + ((idx[:, None, None, None, None] * 5 + 3 * b + 7 * g + 2 * h + t) % 11) / 40.0

    def read_group_ngm(self, count, first=0):
        self.calls.append(("read_group_ngm", count, first))
        assert count <= self.ngm_cap
        return self.K(first + np.arange(count))


ON = dict(FULL, groups_rt="on", groups_ngm="on")
NGM_SETS = {"samples/ngm_by_group", "samples/ngm_spectral_radius", "ngm/days", "ngm/first_day", "ngm/count", "ngm/K_mean", "ngm/K_var",
            "ngm/local_share_mean", "ngm/K_quantiles", "ngm/local_share_quantiles", "ngm/pooled_K_quantiles",
            "ngm/pooled_local_share_quantiles", "ngm/pooled_chains"}


def test_absent_calls_nothing_new_and_writes_todays_datasets(tmp_path):
    base = dict(FULL, groups_rt="on")
    s0, f0, log0 = _run(tmp_path, "parent", base, stub=CurveStub, groups=TABLE)      # a sampler that has never heard of the matrix
    for tag, cfg in (("absent", base), ("off", dict(base, groups_ngm="off")), ("false", dict(base, groups_ngm=False))):
        s1, f1, log1 = _run(tmp_path, tag, cfg, stub=NgmStub, groups=TABLE)
        assert [c[0] for c in s1.calls] == [c[0] for c in s0.calls]
        for a, b in zip(s1.calls, s0.calls):
            if a[0] in ("sample", "burst"):
                assert a[1] == b[1] and a[2] == b[2]
        assert "Local share" not in log1 and _untimed(log1) == _untimed(log0)
        for c in range(2):
            assert set(f1[c]) == set(f0[c]) and not (NGM_SETS & set(f1[c]))
            for k in f0[c]:
                assert np.array_equal(f1[c][k], f0[c][k], equal_nan=f0[c][k].dtype.kind == "f"), k
    # the refusals of run_mcmc itself
    with pytest.raises(ValueError, match="groups_ngm given without groups"):
        _run(tmp_path, "r1", dict(FULL, groups_ngm=True), stub=NgmStub)
    with pytest.raises(ValueError, match="groups_ngm given without rt"):
        _run(tmp_path, "r2", dict(FULL, rt=None, rt_quantiles=None, groups_ngm=True), stub=NgmStub, groups=TABLE)
    with pytest.raises(ValueError, match="groups_ngm given without groups_rt"):
        _run(tmp_path, "r3", dict(FULL, groups_ngm=True), stub=NgmStub, groups=TABLE)


@pytest.mark.parametrize("table,overlap,ext,quant", [("overlapping", True, ".hd5", True), ("partition", False, ".npz", True),
                                                     ("partition", True, ".hd5", False)])
def test_the_switch_is_set_once_read_once_and_the_datasets_are_written(tmp_path, table, overlap, ext, quant):
    assert hdf5io.available(), "the HDF5 writer is part of what this project needs"
    nb, ns, D, probs = 3, 4, 3, (0.05, 0.5, 0.95)
    tab = TABLE if table == "overlapping" else PART
    cfg = dict(ON) if quant else {k: v for k, v in ON.items() if k != "rt_quantiles"}
    cap = 800 if overlap else ns
    s, files, log = _run(tmp_path, "on", cfg, ext=ext, cap=cap, stub=NgmStub, groups=tab)
    names = [c[0] for c in s.calls]
    # set once, behind set_group_rt and the rt reset, before the first kept draw; read once, behind the last burst
    assert names.count("set_group_ngm") == 1 and names.count("read_group_ngm") == 1
    i = names.index("set_group_ngm")
    assert names.index("set_group_rt") < names.index("reset_rt") < i
    last_draw = max(k for k, n in enumerate(names) if n in ("sample", "burst"))
    first_kept = min(k for k, n in enumerate(names) if n in ("sample", "burst") and k > names.index("reset_rt"))
    assert i < first_kept and names.index("read_group_ngm") > last_draw
    assert np.array_equal(s.calls[i][1], G.rt_weights(tab, POP)) and s.calls[i][2] == nb * ns
    assert s.calls[names.index("read_group_ngm")][1:] == (nb * ns, 0)
    # the others' calls and keyword sets are those of a run without the switch
    base, bf, blog = _run(tmp_path, "base", {k: v for k, v in cfg.items() if k != "groups_ngm"}, ext=ext, cap=cap,
                          stub=CurveStub, groups=tab)
    stripped = [c for c in s.calls if c[0] not in ("set_group_ngm", "read_group_ngm")]
    assert [c[0] for c in stripped] == [c[0] for c in base.calls]
    for a, b in zip(stripped, base.calls):
        if a[0] in ("sample", "burst"):
            assert a[1] == b[1] and a[2] == b[2]
    part = table == "partition"
    new = set(NGM_SETS)
    if not part:
        new.discard("samples/ngm_spectral_radius")
    if not quant:
        new = {k for k in new if "quantiles" not in k and k != "ngm/pooled_chains"}
    W = inf.warmup_size()
    K_all = s.K(np.arange(nb * ns))                                # [n,B,G,G,D]
    rg_all = s.curve(W + np.arange(nb * ns), D, 1.0)               # [n,B,G,D]
    pooled = G.ngm_stats(K_all.reshape(-1, s.G, s.G, D), rg_all.reshape(-1, s.G, D), probs)
    for c, f in enumerate(files):
        assert set(f) == set(bf[c]) | new
        for k in bf[c]:
            assert np.array_equal(f[k], bf[c][k], equal_nan=bf[c][k].dtype.kind == "f"), k
        K = f["samples/ngm_by_group"]
        assert K.dtype == np.float64 and K.shape == (nb * ns, s.G, s.G, D) and np.array_equal(K, K_all[:, c])
        assert np.array_equal(f["samples/R_t_by_group"], rg_all[:, c])
        assert f["ngm/days"][0] == D and f["ngm/first_day"][0] == s.T - D and f["ngm/count"][0] == nb * ns
        assert np.array_equal(f["ngm/K_mean"], K.mean(0)) and np.array_equal(f["ngm/K_var"], K.var(0))
        share = K[:, np.arange(s.G), np.arange(s.G)] / rg_all[:, c]
        assert f["ngm/local_share_mean"].shape == (s.G, D) and np.array_equal(f["ngm/local_share_mean"], share.mean(0))
        if quant:
            np.testing.assert_allclose(f["ngm/K_quantiles"], np.quantile(K, probs, axis=0), rtol=1e-12, atol=0)
            np.testing.assert_allclose(f["ngm/local_share_quantiles"], np.quantile(share, probs, axis=0), rtol=1e-12, atol=0)
            assert np.array_equal(f["ngm/pooled_K_quantiles"], pooled["K_quantiles"])
            assert np.array_equal(f["ngm/pooled_local_share_quantiles"], pooled["local_share_quantiles"])
            assert np.array_equal(f["ngm/pooled_chains"], s.first_chain_id + np.arange(2.0))
            assert np.array_equal(f["ngm/pooled_chains"], f["rt/pooled_chains"])
        if part:
            rho = f["samples/ngm_spectral_radius"]
            assert rho.shape == (nb * ns, D) and np.array_equal(rho, G.spectral_radius(K))
            assert np.all(rho >= K[:, np.arange(s.G), np.arange(s.G)].max(axis=1) * (1 - 1e-12))   # a non-negative matrix
    # one log line: every group's last-day local share with its 0.05 / 0.95 quantiles, and the largest export
    assert log.count("Local share of R_t by group") == 1
    line = [ln for ln in log.splitlines() if ln.startswith("Local share of R_t by group")][0]
    last = (K_all[..., -1][:, :, np.arange(s.G), np.arange(s.G)] / rg_all[..., -1]).reshape(-1, s.G)
    q = np.quantile(last, [0.05, 0.95], axis=0)
    for g, name in enumerate(tab.names):
        assert f"{name} {last[:, g].mean():.3g} [{q[0, g]:.3g}, {q[1, g]:.3g}]" in line
    off = K_all[..., -1].reshape(-1, s.G, s.G).mean(axis=0)
    off[np.arange(s.G), np.arange(s.G)] = -np.inf
    g, h = np.unravel_index(int(np.argmax(off)), off.shape)
    assert f"largest export {tab.names[h]} -> {tab.names[g]}: {off[g, h]:.3g}" in line


# ---- 6. the compiler's account of the new kernel ----------------------------------------------------------------------------
def test_the_new_kernel_is_this_instance_without_scratch_at_its_parents_occupancy():
    res = H.kernel_account("ngm")
    assert sorted(res) == ["k_ngm_rows<4>"], sorted(res)
    k = res["k_ngm_rows<4>"]
    assert k["scratch_bytes_per_lane"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
    assert k["lds_bytes_per_block"] == 0, k                         # its LDS is dynamic, as its parent's
    base = H.kernel_account("base")
    # the same loop with fewer live registers (no fold): at least the parent's occupancy
    assert k["occupancy_waves_per_simd"] >= base["k_rt_trace<4>"]["occupancy_waves_per_simd"]

"""The references of tests/devmath_lib.py on the CPU: the restatement of the device math in exact-fma arithmetic keeps every
bound of the table in devmath_lib (with the margin the device is allowed on top), and the grids reach every branch they
name, on both sides of each switch, counted from the restatement's branch predicates alone.  No GPU."""
import hashlib
import math

import mpmath as mp
import numpy as np
import pytest

from tests import devmath_lib as D


def _ratio(name, got, x, y=None):
    return D.worst_ratio(name, got, D.reference(name, x, y), x, y)


# ---- fast_log / mv_log / fast_rcp ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def log_grid():
    g = D.grid_log()
    x = D.cat(g)
    return g, x, np.array([D.fast_log_r(float(v)) for v in x])


def test_log_table_is_the_rule_of_seir_create():
    with mp.workdps(D.DPS):
        for i, (invc, logc) in enumerate(D.TAB):
            c = 1 + (mp.mpf(i) + mp.mpf(1) / 2) / 128
            assert abs(mp.mpf(invc) * c - 1) < 2.0 ** -52, i
            assert abs(mp.mpf(logc) + mp.log(mp.mpf(invc))) <= D.ulp(logc), i


def test_fast_log_grid_reaches_every_cell_and_both_signs_of_the_exponent(log_grid):
    g, x, _ = log_grid
    cells = {D.log_cell(float(v)) for v in x}
    assert {c[0] for c in cells} == set(range(128))
    ks = {c[1] for c in cells}
    assert min(ks) == -997 and max(ks) == 30 and 0 in ks and -1 in ks           # 1 - 1 ulp and 1e-300 sit below 2^0 / 2^-996
    for i in range(128):                                                       # each cell edge from both sides
        e = 1.0 + i / 128.0
        assert D.log_cell(D.up(e))[0] == i and D.log_cell(e)[0] == i
        assert D.log_cell(D.down(e)) == ((i - 1, 0) if i else (127, -1))
    assert (x == 1.0).any() and (x != 1.0).any()                               # mv_log's switch
    assert set(g) == {"dense[1,2)", "cell-edge", "cell-edge-1ulp", "cell-edge+1ulp", "one", "pow2", "integers", "series-min"}
    assert D.INT_MAX in g["integers"] and g["pow2"][0] == 2.0 ** -996 and g["pow2"][-1] == 2.0 ** 30


def test_fast_log_restatement_keeps_the_headers_bound(log_grid):
    _, x, got = log_grid
    worst, at = _ratio("fast_log", got, x)
    print(f"fast_log restatement: worst |err| / (2e-16 + ulp) = {worst:.3f} at x = {x[at]!r}")
    assert worst <= 1.0
    # the excess over one ulp of the result, the figure the header's 2e-16 is about
    with mp.workdps(D.DPS):
        excess = max(float(abs(mp.mpf(float(g)) - mp.log(mp.mpf(float(v))))) - D.ulp(mp.log(mp.mpf(float(v))))
                     for g, v in zip(got, x))
    print(f"fast_log restatement: worst abs err - 1 ulp(result) = {excess:.2e}")
    assert excess < 1e-16


def test_fast_log_restatement_is_pinned_bit_for_bit(log_grid):
    """A polynomial literal off by 1e-12 moves fast_log by at most f^2 1e-12 < 2e-17: less than the bound allows and less
    than an ulp of most results, so no bound can see it.  The restatement's own bits on the grid are therefore pinned: an
    edit of a literal, the table rule or the order of operations changes this digest.  (On the device fast_log_k and
    fast_log are held to each other bit for bit.)"""
    _, x, got = log_grid
    assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest()[:16] == FAST_LOG_DIGEST


FAST_LOG_DIGEST = "c68f2b16bd82a0df"


def test_reciprocal_reference_is_within_an_ulp_of_itself(log_grid):
    _, x, _ = log_grid
    worst, _ = _ratio("fast_rcp", [D.rcp(float(v)) for v in x[::5]], x[::5])
    assert worst <= 0.5


# ---- softplus ----------------------------------------------------------------------------------------------------------------
def test_softplus_tab_restatement_keeps_the_absolute_bound_and_not_the_relative_one():
    g = D.grid_softplus()
    x = D.cat(g)
    e = np.array([D.exp_cr(-abs(float(v))) for v in x])
    # both sides of every switch: the sign select, 1 + e rounding to 1, the absolute floor showing (below about -8)
    assert (x >= 0).any() and (x < 0).any() and (1.0 + e == 1.0).any() and (1.0 + e != 1.0).any()
    assert ((1.0 + e == 1.0) & (x > 0)).any() and ((1.0 + e == 1.0) & (x < 0)).any()
    assert (x < -8).any() and ((x > -8) & (x < 0)).any() and 36.7 in x and -36.7 in x
    got = np.array([D.softplus_tab_r(float(v)) for v in x])
    worst, at = _ratio("softplus_tab", got, x)
    print(f"softplus_tab restatement: worst |err| / (2 ulp + 2^-59) = {worst:.3f} at x = {x[at]!r}")
    assert worst <= 1.0
    # ... while "good to the last bit or two" does not hold of the RELATIVE error once the value is below the floor
    with mp.workdps(D.DPS):
        rel = {xv: float(abs(mp.mpf(D.softplus_tab_r(xv)) / mp.log1p(mp.exp(mp.mpf(xv))) - 1)) for xv in (-20.0, -30.0)}
        ab = {xv: float(abs(mp.mpf(D.softplus_tab_r(xv)) - mp.log1p(mp.exp(mp.mpf(xv))))) for xv in (-20.0, -30.0)}
    print("softplus_tab restatement: relative error", rel, "absolute", ab)
    assert rel[-30.0] > 1e-9 and rel[-20.0] > 1e-13 and max(ab.values()) < 2.0 ** -59


# ---- lfact / lbinom ----------------------------------------------------------------------------------------------------------
def test_lbinom_restatement_and_its_grid():
    n, k = D.grid_lbinom()
    # both sides of every switch, inside one wave of 64 elements
    for lo in range(0, n.size - 63, 64):
        w = slice(lo, lo + 64)
        assert (k[w] < 0).any() and (k[w] > n[w]).any() and ((k[w] >= 0) & (k[w] <= n[w])).any(), lo
        assert (n[w] < 64).any() and (n[w] >= 64).any(), lo
    for v in (63.0, 64.0, 65.0):
        assert ((k == v) & (k <= n)).any() and ((n - k == v) & (k >= 0)).any(), v
    assert set(n) == set(D.N_LIST) and (k == n).any() and (k == n + 1).any() and (k == n - 1).any() and (k == 0).any()
    got = np.array([D.lbinom_bf_r(float(a), float(b)) for a, b in zip(n, k)])
    assert not np.isnan(got).any()
    assert np.array_equal(np.isneginf(got), (k < 0) | (k > n))
    worst, at = _ratio("lbinom_bf", got, n, k)
    print(f"lbinom_bf restatement: worst |err| / bound = {worst:.3f} at n, k = {n[at]!r}, {k[at]!r}")
    assert worst <= 1.0
    # the branching form returns the same bits
    br = np.array([D.lbinom_r(float(a), float(b)) for a, b in zip(n, k)])
    assert np.array_equal(br.view(np.int64), got.view(np.int64))
    x = D.grid_lfact()
    worst, _ = _ratio("lfact_bf", [D.lfact_bf_r(float(v)) for v in x], x)
    assert worst <= 1.0 and (x < 64).any() and (x >= 64).any() and 63.0 in x and 64.0 in x and 0.0 in x


# ---- log(1 - e^-r) and 1 / expm1(r) ------------------------------------------------------------------------------------------
def test_series_restatement_and_its_grid():
    g = D.grid_l1me()
    x = D.cat(g)
    ins = np.array([D.in_series(float(v)) for v in x])
    assert ins.any() and (x > D.L1ME_SERIES_MAX).any() and ((x < D.L1ME_SERIES_MIN) & (x > 0)).any()
    assert (x < 0).any() and (x == 0).any()
    assert D.in_series(D.L1ME_SERIES_MAX) and not D.in_series(D.up(D.L1ME_SERIES_MAX)) and D.in_series(D.down(D.L1ME_SERIES_MAX))
    assert D.in_series(D.L1ME_SERIES_MIN) and not D.in_series(D.down(D.L1ME_SERIES_MIN))
    assert x[ins].min() <= 1e-11 and x.max() > 4.0
    xs = x[ins]
    LI = [D.l1me_inv_series_r(float(v)) for v in xs]
    refs = D.reference("l1me_inv_series", xs)
    wl, _ = D.worst_ratio("l1me_L", [a for a, _ in LI], [r[0] for r in refs], xs)
    wi, _ = D.worst_ratio("l1me_inv", [b for _, b in LI], [r[1] for r in refs], xs)
    print(f"series restatement: worst L {wl:.3f}, inv {wi:.3f} of the bound")
    assert wl <= 1.0 and wi <= 1.0
    # the references of the other arguments: NaN below 0, -inf at 0
    refs = D.reference("log1mexp_tab", np.array([-1.0, 0.0]))
    assert mp.isnan(refs[0]) and refs[1] == mp.ninf


# ---- band_delta and the own-rows piece ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def band():
    g = D.grid_band()
    rows = np.concatenate(list(g.values()))
    return g, rows


def test_band_grid_reaches_every_branch_on_both_sides_of_each_switch(band):
    g, rows = band
    seen = {"series": 0, "slow": 0, "either": 0, "linear": 0}
    z_in, z_out, a_pos, a_neg = 0, 0, 0, 0
    for row in rows:
        r0q, aq = D.band_exact(row)
        r0, a = float(r0q), float(aq)
        _, _, branch = D.delta_reference("band", row)
        seen[branch] += 1
        if row[2] != 0.0 and D.in_series(r0) and D.in_series(r0 + a):
            z = D.band_parts(r0, a)[1]
            z_in += abs(z) <= D.Z_SWITCH
            z_out += abs(z) > D.Z_SWITCH
        a_pos += a > 0
        a_neg += a < 0
    assert all(v > 0 for v in seen.values()), seen
    assert z_in > 100 and z_out >= 10 and a_pos > 100 and a_neg > 100
    r0 = rows[:, 5] * (rows[:, 1] + rows[:, 6] * rows[:, 3])
    r1 = r0 + rows[:, 5] * rows[:, 6] * rows[:, 4]
    k = rows[:, 2] != 0
    assert (k & (r0 <= 0.125) & (r1 > 0.125)).any() and (k & (r0 > 0.125)).any()               # r1 and r0 across the maximum
    assert (k & (r1 > 0) & (r1 < 1e-300)).any() and (k & (r1 < 0)).any() and (k & (r1 == 0)).any()
    assert (~k & (r1 < 0)).any() and (rows[:, 4] == 0).any() and (rows[:, 0] == rows[:, 2]).any()
    assert r0[k].min() < 1e-8 and (rows[:, 1] != 0).any()
    for scale in ("1", "0.001", "1e-06", "1e-09"):
        assert f"z+0.1x{scale}" in g and f"z-0.1x{scale}" in g, sorted(g)
    # the switch itself: elements within 4 ulp of |z| = 0.1 on both sides, and just outside that on both sides
    zs = [D.band_parts(*map(float, D.band_exact(r)))[1] for r in g["z-switch"]]
    d = np.array([(abs(z) - D.Z_SWITCH) / D.ulp(D.Z_SWITCH) for z in zs])
    assert (d > 0).any() and (d <= 0).any() and (d > 4).any() and (d < -4).any()


def test_band_delta_restatement_errs_by_less_than_two_units_of_four(band):
    """The bound's constant 4 is a bit over twice the restatement's worst: the restatement must stay below 2 units
    (half the bound), or the margin left for the device's reciprocal and exp is gone."""
    _, rows = band
    worst = {"series": 0.0, "linear": 0.0}
    n = 0
    for row in rows:
        ref, b, branch = D.delta_reference("band", row)
        r0q, aq = D.band_exact(row)
        got = D.band_delta_r(float(row[0]), float(row[2]), float(r0q), float(aq))
        if branch in ("slow", "either") or got is None:
            assert branch != "series"
            continue
        n += 1
        worst[branch] = max(worst[branch], D.err_ratio(got, ref, b))
    print(f"band_delta restatement: worst {4 * worst['series']:.2f} eps units over {n} cells (linear: {4 * worst['linear']:.2f})")
    assert n > 500 and worst["series"] <= 0.5 and worst["linear"] <= 0.5


def test_own_rows_restatement_errs_by_less_than_two_units_of_four(band):
    _, rows = band
    worst, n = {"own_ei": 0.0, "own_ei_formed": 0.0}, {"own_ei": 0, "own_ei_formed": 0}
    for row in rows:
        for which in worst:
            if which == "own_ei" and not D.own_ei_exact_applies(row):
                continue
            ref, b, branch = D.delta_reference(which, row)
            if branch != "series":
                continue
            r0q, aq = D.band_exact(row)
            r0 = float(r0q)
            got = D.own_ei_r(float(row[0]), float(row[2]), r0, r0 + float(aq))
            n[which] += 1
            worst[which] = max(worst[which], D.err_ratio(got, ref, b))
    print(f"own-rows E->I restatement: worst {4 * worst['own_ei']:.2f} eps units over {n['own_ei']} cells against exact r0 + a, "
          f"{4 * worst['own_ei_formed']:.2f} over {n['own_ei_formed']} against the rates as formed")
    assert n["own_ei"] > 500 and n["own_ei_formed"] > n["own_ei"] and max(worst.values()) <= 0.5
    rows = D.own_se_rows()
    worst, seen = 0.0, set()
    for row in rows:
        ref, b, branch = D.own_se_reference(row)
        seen.add(branch)
        if branch == "series":
            got = D.own_se_r(float(row[2]), float(row[2] + row[4]), float(row[0] - row[4]), float(row[3]))
            worst = max(worst, D.err_ratio(got, ref, b))
    print(f"own-rows S->E restatement: worst {4 * worst:.2f} eps units")
    assert seen == {"series", "slow"} and worst <= 0.5
    assert (rows[:, 2] == 0).any() and (rows[:, 2] + rows[:, 4] == 0).any() and (rows[:, 4] < 0).any() and (rows[:, 4] > 0).any()


# ---- the wave scan's DPP steps -----------------------------------------------------------------------------------------------
def test_wave_scan_restatement_of_the_dpp_steps_is_a_prefix_sum():
    """wave_incl_scan's six DPP steps (row_shr 1, 2, 4, 8; row_bcast 15 under row mask 0xa; row_bcast 31 under 0xc) restated
    lane by lane give the prefix sum for every input of the GPU test -- and the inputs tell a wrong row mask apart."""
    for dtype in (np.int32, np.float64):
        for name, v in D.wave_inputs(dtype).items():
            for w in v.reshape(-1, 64):
                assert np.array_equal(D.wave_scan_dpp(w), np.cumsum(w)), name
    ones = np.ones(64, np.int64)
    for bad in ((0xf, 0xf, 0xf, 0xf, 0xa, 0x8), (0xf, 0xf, 0xf, 0xf, 0xe, 0xc), (0xf, 0x7, 0xf, 0xf, 0xa, 0xc)):
        assert not np.array_equal(D.wave_scan_dpp(ones, bad), np.cumsum(ones)), bad


def test_wave_expected_values():
    v = np.arange(512, dtype=np.float64)
    out, tot = D.wave_expected("block_excl_scan_256", v)
    assert out[0] == 0 and out[256] == 0 and out[255] == sum(range(255)) and tot[0] == sum(range(256)) and tot[511] == sum(range(256, 512))
    out, _ = D.wave_expected("wave_incl_suffix_scan", v)
    assert out[0] == sum(range(64)) and out[63] == 63 and out[64] == sum(range(64, 128))
    assert math.fsum(v) == D.wave_expected("block_sum_256", v)[0].reshape(-1, 256)[:, 0].sum()


# ---- the per-cell terms of the mpmath density (oracle/seir_oracle.py) --------------------------------------------------------
def test_per_cell_terms_sum_to_the_difference_of_the_full_mpmath_densities():
    from oracle import seir_oracle as so
    from tests import helpers as H
    case = H.build_case("micro_5x24", 3, alpha_t_sd=0.005)
    k, u, ev = case["k"], case["u"], case["events"]
    full = so.joint_log_prob_mp(u, ev, k)
    for comp in (0, 1):                                          # an S->E and an E->I event moved by two days
        m, t = [c for c in np.argwhere(ev[..., comp] > 0) if c[1] + 2 < k.T][3]
        ev2 = ev.copy()
        ev2[m, t, comp] -= 1
        ev2[m, t + 2, comp] += 1
        cells = so.changed_cells(ev, ev2, k)
        assert 0 < len(cells) < k.M * k.T and (m, t) in cells
        cache = {}
        a, b = so.likelihood_cells_mp(u, ev, k, cells, cache=cache), so.likelihood_cells_mp(u, ev2, k, cells, cache=cache)
        fresh = so.likelihood_cells_mp(u, ev2, k, cells)
        full2 = so.joint_log_prob_mp(u, ev2, k)
        with mp.workdps(50):
            assert all(b[c] == fresh[c] for c in cells)                                    # the cache changes nothing
            d = sum((b[c][0] - a[c][0] for c in cells), mp.mpf(0))
            assert abs((full2 - full) - d) < mp.mpf(10) ** -40
            assert all(b[c][1] >= abs(b[c][0]) for c in cells)                             # the scale bounds the term
            # every cell outside `cells` has the same term in both states
            rest = [(i, j) for i in range(k.M) for j in range(k.T) if (i, j) not in set(cells)]
            ra, rb = so.likelihood_cells_mp(u, ev, k, rest, cache=cache), so.likelihood_cells_mp(u, ev2, k, rest, cache=cache)
            assert all(ra[c] == rb[c] for c in rest)
    with pytest.raises(AssertionError):
        so.likelihood_cells_mp(u + 1e-3, ev, k, cells, cache=cache)                        # one cache per u

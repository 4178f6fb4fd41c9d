"""References, grids and bounds for the scalar device math (csrc/device_math.h), the delta log-ratios of the event updates
(csrc/sampler_kernels.h: band_delta, the S->E piece of own_rows_delta) and the wave primitives.

Two kinds of reference, neither of them the device:
 * mpmath at 50 digits for every function;
 * a restatement in Python of fast_log (with the table rule of seir_hip.hip), softplus_tab, the series of l1me_inv /
   log1mexp_series, band_delta's series branch and the own-rows piece, operation by operation in IEEE double with an exact
   fused multiply-add (exact rational arithmetic, rounded once: Python before 3.13 has no math.fma).  Where the C++ writes
   a * b + c the restatement uses the fma, as the device compiler contracts it; the reciprocal and exp are the correctly
   rounded ones (the device's Newton reciprocal and libm exp may differ from them by an ulp).
The host test (test_devmath_host.py) holds the restatement to BOUNDS on the grids below and counts the branches the grids
reach; the GPU test (test_devmath_gpu.py) holds the device to the same BOUNDS on the same grids.

BOUNDS and where each comes from (eps = 2^-52; ulp(v) = spacing of doubles at |v|):
 fast_log, mv_log       |err| <= 2e-16 + 1 ulp(result)            the header's own claim
 fast_rcp               |err| <= 1 ulp(1/x)                       v_rcp_f64 + two Newton steps
 softplus_tab value     |err| <= 2 ulp(value) + 2^-59             fast_log(w), w in [1, 1 + 2^-7), cancels two addends of at
                                                                  most 2^-8, each rounded at 2^-61: times 4
 sigmoid                |err| <= 4 ulp                            e, 1 + e, the reciprocal and a product
 softplus (libm)        |err| <= 4 ulp
 lbinom*                |err| <= 2e-15 max(1, |lfact n| + |lfact k| + |lfact(n - k)|); -inf exactly where k < 0 or k > n,
                        never NaN                                 the suite's per-lfact bound, summed
 lfact_bf               the same with one term; bit-equal to lfact(n, tab); lbinom_bf bit-equal to lbinom(n, k, tab)
 log1mexp*, series, l1me_* L   rel 2e-15 or abs 2e-16; inv rel 2e-15      the suite's existing bound
 l1me_inv_k == l1me_inv, l1me_inv_series_k == l1me_inv_series (inside the series' range), fast_log_k == fast_log: bits
 band_delta series      |err| <= 4 eps (K0 (|dL| + (r0 + r1)/2) + |S - K0| |a|) against L(r0 + a) - L(r0) with EXACT r0 + a:
                        the restatement's worst is 1.87 of these units on the grid below (the host test fails above 2)
 own-rows piece (E->I)  the same with |L0| + |L1| for |dL| + (r0 + r1)/2: the restatement's worst is 0.97.  Held to it twice:
                        against exact r0 + a on the rows of `own_ei_exact_applies`, and on every row against the rates as
                        the piece is handed them (rr1 = fl(r0 + a), rr1 - rr0 for a)
 own-rows piece (S->E)  |err| <= 4 eps ((|k1| + |kse|) |L0| + |dS - dk0| r0): L0 within ~1.5 eps |L0| taken twice, two
                        products and two sums of half an ulp each
 slow branch            |err| <= 2e-15 (|L0| + |L1|) K0 + 4 eps |S - K0| |a|   (log1mexp_diff_slow alone: S = K0 = 1)
 an element within 4 ulp of band_delta's |z| = 0.1 switch may take either branch on the device (its reciprocal may differ
 by an ulp): it is held to the larger of the two branches' bounds
"""
import struct
from fractions import Fraction

import mpmath as mp
import numpy as np

DPS = 50
EPS = 2.0 ** -52
L1ME_SERIES_MAX, L1ME_SERIES_MIN = 0.125, 1e-300
LOGTAB_N = 128
INT_MAX = 2.0 ** 31 - 1


def ulp(v):
    return float(np.spacing(abs(float(v)))) if np.isfinite(float(v)) else float("inf")


def up(x, n=1):
    for _ in range(n):
        x = np.nextafter(x, np.inf)
    return float(x)


def down(x, n=1):
    for _ in range(n):
        x = np.nextafter(x, -np.inf)
    return float(x)


# ---- exact-fma arithmetic and the restatement ------------------------------------------------------------------------------
def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _mp(x):
    return mp.mpf(float(x))


def rcp(x):
    """correctly rounded 1 / x"""
    return float(Fraction(1) / Fraction(x))


def exp_cr(x):
    with mp.workdps(DPS):
        return float(mp.exp(_mp(x)))


def log_table():
    """The table seir_create uploads: c_i = 1 + (i + 1/2)/128, (fl(1/c_i), -log(fl(1/c_i))), through an x87 long double."""
    tab = []
    for i in range(LOGTAB_N):
        cc = Fraction(2 * i + 1, 2 * LOGTAB_N) + 1
        with mp.workprec(64):
            invc = float(mp.mpf(cc.denominator) / mp.mpf(cc.numerator))
            logc = float(-mp.log(mp.mpf(invc)))
        tab.append((invc, logc))
    return tab


TAB = log_table()
_G = (-0.125, 0.14285714285714285, -0.16666666666666666, 0.2, -0.25, 0.33333333333333331, -0.5)
LN2HI, LN2LO = 0.69314718055994529, 2.3190468138462996e-17
_LC = (4.1666666666666664e-2, 3.4722222222222224e-4, 5.5114638447971785e-6, 1.0333994708994709e-7)
_IC = (8.3333333333333329e-2, 1.3888888888888889e-3, 3.3068783068783071e-5, 8.2671957671957672e-7)
_AT = (2.0, 0.66666666666666663, 0.4, 0.2857142857142857, 0.22222222222222221, 0.18181818181818182, 0.15384615384615385,
       0.13333333333333333)
Z_SWITCH = 0.1


def log_cell(x):
    bits = struct.unpack("<q", struct.pack("<d", x))[0]
    return (bits >> 45) & 127, ((bits >> 52) & 0x7ff) - 1023


def fast_log_r(x, g=_G, tab=TAB):
    bits = struct.unpack("<q", struct.pack("<d", x))[0]
    i, k = log_cell(x)
    m = struct.unpack("<d", struct.pack("<q", (bits & 0x000fffffffffffff) | 0x3ff0000000000000))[0]
    invc, logc = tab[i]
    f = fma(m, invc, -1.0)
    p = fma(f, g[0], g[1])
    for c in g[2:]:
        p = fma(f, p, c)
    p = fma(f * f, p, f)
    kd = float(k)
    return fma(kd, LN2HI, logc) + fma(kd, LN2LO, p)


def softplus_tab_r(x):
    e = exp_cr(-abs(x))
    wv = 1.0 + e
    return max(x, 0.0) + fma(e - (wv - 1.0), rcp(wv), fast_log_r(wv))


def _g_series(r):
    """r (-1/2 + r (c1 - r2 (c2 - r2 (c3 - r2 c4)))) as the compiler contracts it"""
    r2 = r * r
    q = fma(-r2, _LC[3], _LC[2])
    q = fma(-r2, q, _LC[1])
    q = fma(-r2, q, _LC[0])
    return r * fma(r, q, -0.5)


def l1me_inv_series_r(r):
    r2 = r * r
    q = fma(-r2, _LC[3], _LC[2])
    q = fma(-r2, q, _LC[1])
    q = fma(-r2, q, _LC[0])
    L = fma(r, fma(r, q, -0.5), fast_log_r(r))
    q = fma(-r2, _IC[3], _IC[2])
    q = fma(-r2, q, _IC[1])
    q = fma(-r2, q, _IC[0])
    inv = fma(r, q, rcp(r) - 0.5)
    return L, inv


def in_series(r):
    return L1ME_SERIES_MIN <= r <= L1ME_SERIES_MAX


def band_parts(r0, a, z_switch=Z_SWITCH):
    """(r1, z, branch) of band_delta for a cell of K0 != 0: the restatement's branch predicate"""
    r1 = r0 + a
    z = a * rcp(r0 + r1) if r0 + r1 != 0.0 else float("nan")
    series = in_series(r0) and in_series(r1) and abs(z) <= z_switch
    return r1, z, "series" if series else "slow"


def band_delta_r(S, K0, r0, a, z_switch=Z_SWITCH):
    """band_delta's series branch restated (None where the restatement's predicate takes the slow branch)"""
    out = -(S - K0) * a
    if K0 == 0.0:
        return out
    r1, z, branch = band_parts(r0, a, z_switch)
    if branch != "series":
        return None
    z2 = z * z
    p = _AT[7]
    for c in _AT[6::-1]:
        p = fma(z2, p, c)
    at = z * p
    dL = at + (_g_series(r1) - _g_series(r0))
    return fma(K0, dL, out)


def log1mexp_series_r(r):
    return l1me_inv_series_r(r)[0]


def own_ei_r(S, K0, r0, r1):
    """S->E piece of own_rows_delta for an E->I-type update, both rates inside the series' range"""
    lin = (S - K0) * (r1 - r0)
    if K0 == 0.0:
        return 0.0 - lin
    return fma(K0, log1mexp_series_r(r1) - log1mexp_series_r(r0), -lin)


def own_se_r(K0, k1, dsk, r0):
    L0 = log1mexp_series_r(r0)
    a = k1 * L0 if k1 != 0.0 else 0.0
    b = K0 * L0 if K0 != 0.0 else 0.0
    return fma(-dsk, r0, a - b)


LFACT_TABLE = 64
with mp.workdps(DPS):
    LFACT = [float(mp.loggamma(i + 1)) for i in range(LFACT_TABLE)]
_ST = (8.333333333333333e-2, 2.777777777777778e-3, 7.936507936507937e-4, 5.952380952380952e-4)


def lfact_stirling_r(n):
    x = n + 1.0
    if not x > 0.0:
        return float("nan")                        # lfact_bf evaluates it for every n and selects it only for n >= 64
    xi = rcp(x)
    xi2 = xi * xi
    q = fma(-xi2, _ST[3], _ST[2])
    q = fma(-xi2, q, _ST[1])
    q = fma(-xi2, q, _ST[0])
    return fma(x - 0.5, fast_log_r(x), -x) + 0.9189385332046727 + xi * q


def lfact_r(n):
    return LFACT[int(n)] if n < LFACT_TABLE else lfact_stirling_r(n)


def lfact_bf_r(n):
    small = n < LFACT_TABLE
    tv = LFACT[(int(n) if n > 0.0 else 0) if small else 0]
    st = lfact_stirling_r(n)
    return tv if small else st


def lbinom_r(n, k):
    if k < 0.0 or k > n:
        return float("-inf")
    return lfact_r(n) - lfact_r(k) - lfact_r(n - k)


def lbinom_bf_r(n, k):
    v = lfact_bf_r(n) - lfact_bf_r(k) - lfact_bf_r(n - k)
    return float("-inf") if (k < 0.0 or k > n) else v


# ---- mpmath references -----------------------------------------------------------------------------------------------------
def L_mp(r):
    """log(1 - e^-r) of an mpf / Fraction r: -inf at 0, nan below"""
    r = mp.mpf(r.numerator) / mp.mpf(r.denominator) if isinstance(r, Fraction) else mp.mpf(r)
    if r < 0:
        return mp.nan
    if r == 0:
        return mp.ninf
    return mp.log(-mp.expm1(-r))


def lfact_mp(n):
    return mp.loggamma(_mp(n) + 1)


def lbinom_terms(n, k):
    return lfact_mp(n), lfact_mp(k), lfact_mp(n - k)


def reference(name, x, y=None):
    """mpmath value(s) of function `name` at each element: a list of mpf (or of pairs for a function with two results)"""
    out = []
    with mp.workdps(DPS):
        for j, xv in enumerate(np.asarray(x, dtype=np.float64)):
            v = _mp(xv)
            if name in ("fast_log", "mv_log", "fast_log_k"):
                out.append(mp.log(v))
            elif name == "fast_rcp":
                out.append(1 / v)
            elif name in ("softplus_tab", "softplus"):
                out.append(mp.log1p(mp.exp(v)))
            elif name == "softplus_sigmoid_tab":
                out.append((mp.log1p(mp.exp(v)), 1 / (1 + mp.exp(-v))))
            elif name == "lfact_bf":
                out.append(lfact_mp(xv))
            elif name in ("lbinom_tab", "lbinom_const", "lbinom_bf"):
                k = float(y[j])
                if k < 0 or k > xv:
                    out.append(mp.ninf)
                else:
                    a, b, c = lbinom_terms(xv, k)
                    out.append(a - b - c)
            elif name in ("log1mexp_tab", "log1mexp", "log1mexp_series"):
                out.append(L_mp(v))
            elif name in ("l1me_inv_series", "l1me_inv_k", "l1me_inv_series_k"):
                out.append((L_mp(v), 1 / mp.expm1(v) if v != 0 else mp.inf))
            elif name == "log1mexp_diff_slow":
                out.append(L_mp(v) - L_mp(_mp(y[j])))
            else:
                raise KeyError(name)
    return out


def _rel_or_abs(ref):
    return max(2e-15 * abs(ref), mp.mpf(2e-16))


def bound(name, ref, x, y=None):
    """BOUNDS (module docstring): the allowed |err| of one element, from its reference value"""
    with mp.workdps(DPS):
        if name in ("fast_log", "mv_log", "fast_log_k"):
            return 2e-16 + ulp(ref)
        if name == "fast_rcp":
            return ulp(ref)
        if name == "softplus_tab":
            return 2 * ulp(ref) + 2.0 ** -59
        if name == "softplus":
            return 4 * ulp(ref)
        if name == "sigmoid":
            return 4 * ulp(ref)
        if name == "lfact_bf":
            return 2e-15 * max(1, abs(ref))
        if name in ("lbinom_tab", "lbinom_const", "lbinom_bf"):
            a, b, c = lbinom_terms(x, y)
            return 2e-15 * max(1, abs(a) + abs(b) + abs(c))
        if name in ("log1mexp_tab", "log1mexp", "log1mexp_series", "l1me_L"):
            return _rel_or_abs(ref)
        if name == "l1me_inv":
            return 2e-15 * abs(ref)
        if name == "log1mexp_diff_slow":
            return 2e-15 * (abs(L_mp(_mp(x))) + abs(L_mp(_mp(y))))
    raise KeyError(name)


def worst_ratio(name, got, refs, x, y=None):
    """max |got - ref| / bound over the elements whose reference is finite; the others must match exactly (-inf) or be NaN
    (NaN reference).  Returns (worst ratio, index of the worst)."""
    worst, at = 0.0, -1
    with mp.workdps(DPS):
        for j, (g, r) in enumerate(zip(got, refs)):
            g = float(g)
            if mp.isnan(r):
                assert np.isnan(g), (name, j, float(x[j]), g)
                continue
            if mp.isinf(r):
                assert g == float(r), (name, j, float(x[j]), g)
                continue
            assert np.isfinite(g), (name, j, float(x[j]), g)
            b = bound(name, r, float(x[j]), None if y is None else float(y[j]))
            q = float(abs(_mp(g) - r) / b)
            if q > worst:
                worst, at = q, j
    return worst, at


# ---- grids: {branch id: array}; the ids name the branch or the edge a segment is there for ---------------------------------
def _rng(seed):
    return np.random.default_rng(seed)


def grid_log():
    edges = np.array([1.0 + i / 128.0 for i in range(128)])
    return {
        "dense[1,2)": np.concatenate([np.linspace(1.0, 2.0, 1024, endpoint=False), _rng(1).uniform(1.0, 2.0, 512)]),
        "cell-edge": edges, "cell-edge-1ulp": np.array([down(e) for e in edges]), "cell-edge+1ulp": np.array([up(e) for e in edges]),
        "one": np.array([down(1.0), 1.0, up(1.0)]),
        "pow2": np.array([2.0 ** e for e in range(-996, 31)]),
        "integers": np.concatenate([np.arange(1.0, 301.0), [INT_MAX]]),
        "series-min": np.array([L1ME_SERIES_MIN]),
    }


def grid_softplus():
    edge = np.concatenate([np.arange(36.0, 37.5, 0.05), [36.7, 36.73, 36.74, 36.75]])
    return {
        "integers": np.arange(-45.0, 46.0),
        "around0": np.array([0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300, 1e-16, -1e-16, 1e-8, -1e-8, 0.5, -0.5]),
        "around-8": np.linspace(-9.0, -7.0, 81),
        "1+e==1": np.concatenate([edge, -edge]),
        "random": _rng(2).uniform(-45.0, 45.0, 600),
    }


N_LIST = [0.0, 1.0, 62.0, 63.0, 64.0, 65.0, 2047.0, 2048.0, 1.2e6, 6.7e7, INT_MAX]


def grid_lbinom():
    n, k = [], []
    for nv in N_LIST:
        for kv in (-1.0, 0.0, 1.0, nv - 1, nv, nv + 1, 63.0, 64.0, 65.0, nv - 63, nv - 64, nv - 65):
            n.append(nv)
            k.append(kv)
    n, k = np.array(n), np.array(k)
    perm = _rng(3).permutation(n.size)             # all mixed inside one wave
    return n[perm], k[perm]


def grid_lfact():
    return _rng(4).permutation(np.concatenate([np.arange(0.0, 131.0), N_LIST]))


def grid_l1me():
    return {
        "log-uniform": np.exp(_rng(5).uniform(np.log(1e-12), np.log(5.0), 1500)),
        "series-max": np.array([down(L1ME_SERIES_MAX), L1ME_SERIES_MAX, up(L1ME_SERIES_MAX)]),
        "series-min": np.array([L1ME_SERIES_MIN, down(L1ME_SERIES_MIN)]),
        "negative": np.array([-1e-300, -1e-3, -1.0]),
        "zero": np.array([0.0]),
    }


def cat(grid):
    return np.concatenate(list(grid.values()))


def grid_band():
    """Cells of band_delta / the own-rows piece.  Columns S, I, K0, F, dF, ee, psiW; rate_floor = 0, dt = DT.  ee = psiW = 1,
    I = 0 (and DT = 1) make r0 = F and a = dF exactly, whatever the order and contraction of the device's products; the
    `scaled` segment has power-of-two factors and F, dF on a 2^-40 grid, which are exact too.  Returns {id: rows}."""
    rng = _rng(6)
    g = {}

    def rows(r0, a, K0=None, SmK=None):
        r0, a = np.atleast_1d(np.asarray(r0, float)), np.atleast_1d(np.asarray(a, float))
        n = r0.size
        K0 = rng.choice([1.0, 3.0, 50.0], n) if K0 is None else np.full(n, float(K0))
        SmK = rng.choice([0.0, 7.0, 1000.0], n) if SmK is None else np.full(n, float(SmK))
        one, zero = np.ones(n), np.zeros(n)
        return np.stack([K0 + SmK, zero, K0, r0, a, one, one], axis=1)

    r0 = np.exp(rng.uniform(np.log(1e-9), np.log(0.125), 120))
    for scale in (1.0, 1e-3, 1e-6, 1e-9):
        for sgn in (1.0, -1.0):
            z = sgn * 0.1 * scale * rng.uniform(0.5, 1.0, r0.size)
            g[f"z{'+' if sgn > 0 else '-'}0.1x{scale:g}"] = rows(r0, 2.0 * r0 * z / (1.0 - z))
    # the |z| = 0.1 switch and a few ulps either side of it
    sw = []
    for r in (1e-6, 3e-4, 0.01, 0.1):
        for sgn in (1.0, -1.0):
            a0 = 2.0 * r * sgn * 0.1 / (1.0 - sgn * 0.1)
            for step in (-8, -2, -1, 0, 1, 2, 8):
                a = a0
                for _ in range(abs(step)):
                    a = np.nextafter(a, np.inf if step > 0 else -np.inf)
                sw.append((r, float(a)))
    sw = np.array(sw)
    g["z-switch"] = rows(sw[:, 0], sw[:, 1])
    g["z>0.1"] = rows([1e-5, 1e-3, 0.05, 0.02], [1e-5, -4e-4, 0.05, -0.01])
    g["r1-crosses-max"] = rows([0.12, L1ME_SERIES_MAX, 0.124], [0.01, up(L1ME_SERIES_MAX) - L1ME_SERIES_MAX, 0.002])
    g["r0-above-max"] = rows([0.13, 0.5, 2.0], [-0.01, 0.01, -0.5])
    g["r1-below-min"] = rows([1e-300, 2e-300], [-5e-301, -1.5e-300])
    g["r1-zero"] = rows([1e-5], [-1e-5])
    g["r1-negative"] = rows([1e-5, 0.01], [-2e-5, -0.5])
    g["K0=0"] = rows([1e-5, 1e-5, 0.01, 0.3], [-2e-5, 1e-6, -0.5, 0.1], K0=0.0, SmK=7.0)
    g["dF=0"] = rows([1e-6, 0.01, 0.5], [0.0, 0.0, 0.0])
    g["S=K0"] = rows(r0[:20], r0[:20] * rng.uniform(-0.15, 0.15, 20), SmK=0.0)
    # power-of-two factors: ee = 2^-10, psiW = 2, dt = 1 (the caller passes DT): r0 = 2^-10 (I + 2 F), a = 2^-9 dF
    n = 40
    F = np.round(rng.uniform(0.0, 4.0, n) * 2.0 ** 40) / 2.0 ** 40
    dFv = np.round(rng.uniform(-0.3, 0.3, n) * 2.0 ** 40) / 2.0 ** 40
    K0 = rng.choice([1.0, 3.0, 50.0], n)
    g["scaled"] = np.stack([K0 + rng.choice([0.0, 7.0], n), np.full(n, 3.0), K0, F, dFv, np.full(n, 2.0 ** -10), np.full(n, 2.0), ], axis=1)
    return g


DT = 1.0


def band_exact(row):
    """(r0, a) of a grid row as exact rationals; both must be doubles (the grids are built that way)"""
    S, I, K0, F, dF, ee, psiW = (Fraction(float(v)) for v in row)
    r0 = ee * (I + psiW * F) * Fraction(DT)
    a = ee * psiW * dF * Fraction(DT)
    assert Fraction(float(r0)) == r0 and Fraction(float(a)) == a, row
    return r0, a


def delta_reference(which, row):
    """(mpmath value, bound, branch) of one grid row for which = "band" | "own_ei" (exact r0 + a) | "own_ei_formed" (the
    own-rows piece against the rates it is handed, rr1 = fl(r0 + a), and rr1 - rr0 for a).  branch: "series", "slow",
    "either" (within 4 ulp of the |z| switch: band only), "linear" (K0 = 0)."""
    S, I, K0, F, dF, ee, psiW = (float(v) for v in row)
    r0q, aq = band_exact(row)
    r0, a = float(r0q), float(aq)
    with mp.workdps(DPS):
        if which == "own_ei_formed":               # the rates as the piece is handed them: rr1 = fl(r0 + a), a = rr1 - rr0
            aq = Fraction(r0 + a) - r0q
            a = float(aq)
            which = "own_ei"
        lin = -(_mp(S) - _mp(K0)) * (mp.mpf(aq.numerator) / mp.mpf(aq.denominator))
        lin_b = 4 * EPS * abs(S - K0) * abs(float(aq))
        if K0 == 0.0:
            return lin, lin_b, "linear"
        L0, L1 = L_mp(r0q), L_mp(r0q + aq)
        ref = _mp(K0) * (L1 - L0) + lin
        if mp.isnan(L1) or mp.isinf(L1):
            return (mp.nan if mp.isnan(L1) else mp.ninf), 0.0, "slow"
        r1 = r0 + a
        slow_b = 2e-15 * float(abs(L0) + abs(L1)) * K0 + lin_b
        if which == "band":
            _, z, branch = band_parts(r0, a)
            series_b = 4 * EPS * K0 * (float(abs(L1 - L0)) + (r0 + r1) / 2) + lin_b
            if in_series(r0) and in_series(r1) and abs(abs(z) - Z_SWITCH) <= 4 * ulp(Z_SWITCH):
                return ref, max(series_b, slow_b), "either"
            return ref, series_b if branch == "series" else slow_b, branch
        series = in_series(r0) and in_series(r1)
        series_b = 4 * EPS * K0 * float(abs(L0) + abs(L1)) + lin_b
        return ref, series_b if series else slow_b, "series" if series else "slow"


def own_ei_exact_applies(row):
    """Whether the own-rows piece of this row is held to the reference with EXACT r0 + a.  The piece is handed rr1 = fl(r0 + a)
    -- in the sampler the new F is a stored double -- so against exact r0 + a its linear term carries |S - K0| ulp(r1)/2 that
    is the input's rounding, not the function's error, and that the bound (which has |S - K0| |a| only) does not know.  The
    rows where that can reach a quarter of a unit, |S - K0| r1 / 2 > K0 (|L0| + |L1|) / 4, and |L| >= 2.07 here, are held
    to the as-formed reference alone ("own_ei_formed": every row is)."""
    S, I, K0, F, dF, ee, psiW = (float(v) for v in row)
    r0q, aq = band_exact(row)
    return abs(S - K0) * abs(float(r0q + aq)) <= 2.0 * K0


def own_se_rows():
    """Rows for the S->E-type piece: column S holds dS, column dF holds dk0 (include/seir_hip.h)"""
    rng = _rng(7)
    r0 = np.concatenate([np.exp(rng.uniform(np.log(1e-9), np.log(0.125), 60)), [0.125, up(0.125), 0.3, 2.0, 1e-300]])
    n = r0.size
    K0 = rng.choice([0.0, 1.0, 3.0, 50.0], n)
    dk0 = rng.choice([-1.0, 0.0, 1.0, 2.0], n)
    dk0 = np.where(K0 + dk0 < 0, 0.0, dk0)
    dS = rng.choice([-2.0, -1.0, 0.0, 1.0, 2.0], n)
    return np.stack([dS, np.zeros(n), K0, r0, dk0, np.ones(n), np.ones(n)], axis=1)


def own_se_reference(row):
    dS, I, K0, r0, dk0, ee, psiW = (float(v) for v in row)
    with mp.workdps(DPS):
        L0 = L_mp(_mp(r0))
        ref = _mp(dk0) * L0 - (_mp(dS) - _mp(dk0)) * _mp(r0)
        b = 4 * EPS * ((abs(K0 + dk0) + abs(K0)) * float(abs(L0)) + abs(dS - dk0) * r0)
        if not in_series(r0):
            b = max(b, 2e-15 * (abs(K0 + dk0) + abs(K0)) * float(abs(L0)) + 4 * EPS * abs(dS - dk0) * r0)
        return ref, b, "series" if in_series(r0) else "slow"


def err_ratio(got, ref, b):
    """|got - ref| / b for a finite reference; exact agreement required of an infinite one, NaN of a NaN one"""
    got = float(got)
    with mp.workdps(DPS):
        if mp.isnan(ref):
            assert np.isnan(got), got
            return 0.0
        if mp.isinf(ref):
            assert got == float(ref), got
            return 0.0
        assert np.isfinite(got), got
        e = abs(_mp(got) - ref)
        if b == 0.0:
            assert e == 0, (got, ref)
            return 0.0
        return float(e / b)


# ---- wave and block primitives in numpy --------------------------------------------------------------------------------------
def wave_expected(name, v):
    """(out, total) the primitive must hand back for the input v [nblocks * 256] (exact for integer-valued input)"""
    w, b = v.reshape(-1, 64), v.reshape(-1, 256)
    zero = np.zeros_like(v)
    if name == "wave_sum":
        return np.repeat(w.sum(axis=1), 64), zero
    if name == "wave_min":
        return np.repeat(w.min(axis=1), 64), zero
    if name == "wave_incl_scan":
        return np.cumsum(w, axis=1).reshape(-1), zero
    if name == "wave_incl_suffix_scan":
        return np.cumsum(w[:, ::-1], axis=1)[:, ::-1].reshape(-1), zero
    tot = np.repeat(b.sum(axis=1), 256)
    if name == "block_excl_scan_256":
        return (np.cumsum(b, axis=1) - b).reshape(-1), tot
    if name == "block_incl_suffix_scan_256":
        return np.cumsum(b[:, ::-1], axis=1)[:, ::-1].reshape(-1), tot
    if name == "block_sum_256":
        return tot, zero
    raise KeyError(name)


def wave_inputs(dtype, nblocks=4):
    """{id: input}: a single 1 at each lane / thread position, all ones, random integers of either sign below 2^20"""
    n = nblocks * 256
    out = {"ones": np.ones(n, dtype)}
    out["random"] = _rng(8).integers(-(2 ** 20) + 1, 2 ** 20, n).astype(dtype)
    for lane in range(64):
        v = np.zeros(n, dtype)
        v.reshape(-1, 64)[:, lane] = 1
        out[f"lane{lane}"] = v
    for t in range(256):
        v = np.zeros(n, dtype)
        v[(t % nblocks) * 256 + t] = 1
        out[f"thread{t}"] = v
    return out


def wave_scan_dpp(v, row_masks=(0xf, 0xf, 0xf, 0xf, 0xa, 0xc)):
    """wave_incl_scan restated on one wave of 64 values: row_shr 1, 2, 4, 8 inside each row of 16 (a source outside the row
    gives 0), then row_bcast 15 and row_bcast 31 under their row masks"""
    v = np.array(v).copy()
    lanes = np.arange(64)
    for step, sh in enumerate((1, 2, 4, 8)):
        src = np.where((lanes % 16) >= sh, v[np.maximum(lanes - sh, 0)], 0)
        v = v + np.where((row_masks[step] >> (lanes // 16)) & 1, src, 0)
    src = np.where(lanes >= 16, v[np.maximum((lanes // 16) * 16 - 1, 0)], 0)          # row_bcast 15: lane 15 of the row before
    v = v + np.where((row_masks[4] >> (lanes // 16)) & 1, src, 0)
    src = np.where(lanes >= 32, v[31], 0)                                               # row_bcast 31: lane 31 into rows 2, 3
    v = v + np.where((row_masks[5] >> (lanes // 16)) & 1, src, 0)
    return v

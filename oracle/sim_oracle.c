/* C twin of oracle/sim_oracle.py's `binomial`: the same operations in the same order on the same Philox stream, fast
 * enough for 2^20 draws per point, and with a report on how each variate came about.
 *
 * TEST INFRASTRUCTURE ONLY: built into oracle/libseir_oracle.so, loaded by tests/ (oracle/c_binding.py), never by the
 * product package.  PARITY UNPINNED, like the Python file it follows: the draw protocol is the build's own.
 *
 * Protocol (oracle/sim_oracle.py): Philox4x32-10, key = seed, counter = (attempt, stream, cell, draw id); one call gives
 * the uniform pair (u, v) of one attempt.  Binomial(n, p): trivial cases, the flip at p > 1/2, sequential inversion (BINV)
 * for n min(p, q) < 10, BTRS (Hormann 1993) from 10 on.  log(k!) is libm's lgamma(k + 1): no Stirling series here, so that
 * the device's series is checked against something else.  The Makefile compiles with -std=c11 -ffp-contract=off: every
 * product is rounded before it is added, as in the Python oracle (the device contracts them into FMAs).
 *
 * Pinned to oracle/sim_oracle.py by equality and to scipy.stats.binom by chi-square and moments
 * (tests/test_binomial_host.py).
 *
 * Near-ties.  A variate can differ between two correctly rounded fp64 evaluations of this algorithm in two places only:
 * where the BTRS candidate floor((2a/us + b) u + c) has its argument next to an integer, and where the acceptance test
 * v <= h - lfact(k) - lfact(n-k) + (k-m) lpq is decided by less than the rounding of its log-factorials.  A draw is
 * marked when, in any attempt,
 *     |t - rint(t)| <= 4 ulp(t)                         for the pre-floor value t, or
 *     |v - rhs| <= 16 * 2^-52 * (lfact(m) + lfact(n-m)) for the two sides of the acceptance test.
 */
#include <math.h>
#include <stdint.h>

#define SIM_BINV_MAX_MEAN 10.0
#define SIM_BINV_MAX_X 200
#define SIM_MAX_ATTEMPTS 64

enum { SIM_TRIVIAL = 0, SIM_BINV = 1, SIM_BTRS_SQUEEZE = 2, SIM_BTRS_FULL = 3, SIM_FALLBACK = 4 };

static void philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
    const uint64_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = M0 * c0, p1 = M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
static double u01(uint32_t hi, uint32_t lo) {
    const uint64_t x = (((uint64_t)hi << 32) | lo) >> 12;
    return ((double)x + 0.5) * 2.220446049250313e-16;
}

typedef struct { uint32_t k0, k1, draw, cell, stream; } sim_key;

static void uniform2(const sim_key *k, uint32_t attempt, double *u, double *v) {
    uint32_t r[4];
    philox(attempt, k->stream, k->cell, k->draw, k->k0, k->k1, r);
    *u = u01(r[0], r[1]);
    *v = u01(r[2], r[3]);
}
static double lfact(double k) { int sign; return lgamma_r(k + 1.0, &sign); }
static double ulp(double x) { x = fabs(x); return nextafter(x, INFINITY) - x; }

static int binomial(int n, double p, const sim_key *key, int *branch, int *tie, int *attempts) {
    *branch = SIM_TRIVIAL; *tie = 0; *attempts = 0;
    if (n <= 0 || !(p > 0.0)) return 0;
    if (p >= 1.0) return n;
    const int flip = p > 0.5;
    const double pp = flip ? 1.0 - p : p, q = 1.0 - pp;
    const double nd = (double)n;
    int x = -1;
    if (nd * pp < SIM_BINV_MAX_MEAN) {
        const double s = pp / q, a = (nd + 1.0) * s, r0 = exp(nd * log1p(-pp));
        const int xmax = n < SIM_BINV_MAX_X ? n : SIM_BINV_MAX_X;
        for (int att = 0; att < SIM_MAX_ATTEMPTS && x < 0; ++att) {
            double u, v;
            uniform2(key, (uint32_t)att, &u, &v);
            *attempts = att + 1;
            double r = r0;
            int k = 0;
            while (u > r && k <= xmax) {
                u -= r;
                ++k;
                r *= a / (double)k - s;
            }
            if (k <= xmax) x = k;
        }
        *branch = SIM_BINV;
        if (x < 0) { x = (int)(nd * pp); *branch = SIM_FALLBACK; }
    } else {
        const double spq = sqrt(nd * pp * q);
        const double b = 1.15 + 2.53 * spq;
        const double a = -0.0873 + 0.0248 * b + 0.01 * pp;
        const double c = nd * pp + 0.5;
        const double vr = 0.92 - 4.2 / b;
        const double alpha = (2.83 + 5.1 / b) * spq;
        const double m = floor((nd + 1.0) * pp);
        const double lpq = log(pp / q);
        const double h = lfact(m) + lfact(nd - m);
        const double tol = 16.0 * 2.220446049250313e-16 * h;
        for (int att = 0; att < SIM_MAX_ATTEMPTS && x < 0; ++att) {
            double u, v;
            uniform2(key, (uint32_t)att, &u, &v);
            *attempts = att + 1;
            u -= 0.5;
            const double us = 0.5 - fabs(u);
            const double t = (2.0 * a / us + b) * u + c;
            if (fabs(t - rint(t)) <= 4.0 * ulp(t)) *tie = 1;
            const double k = floor(t);
            if (k < 0.0 || k > nd) continue;
            if (us >= 0.07 && v <= vr) { x = (int)k; *branch = SIM_BTRS_SQUEEZE; break; }
            v = log(v * alpha / (a / (us * us) + b));
            const double rhs = h - lfact(k) - lfact(nd - k) + (k - m) * lpq;
            if (fabs(v - rhs) <= tol) *tie = 1;
            if (v <= rhs) { x = (int)k; *branch = SIM_BTRS_FULL; }
        }
        if (x < 0) { x = (int)m; *branch = SIM_FALLBACK; }
    }
    return flip ? n - x : x;
}

/* ---- public (ctypes) ----
 * count elements (n_i, p_i) on the substream (draw_i, cell_i, stream_i) of `seed`; stream_i is the counter word itself
 * (the simulator's transition x uses 64 + x).  out: the variate; branch: SIM_TRIVIAL .. SIM_FALLBACK; tie: 1 for a
 * near-tie (above); attempts: uniform pairs consumed (0 for a trivial case) -- the last three may be NULL. */
void sim_oracle_binomial(int64_t count, const int32_t *n, const double *p, const uint32_t *draw, const uint32_t *cell,
                         const uint32_t *stream, uint64_t seed, int32_t *out, uint8_t *branch, uint8_t *tie,
                         int32_t *attempts) {
#pragma omp parallel for schedule(static, 4096)
    for (int64_t i = 0; i < count; ++i) {
        const sim_key key = {(uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32), draw[i], cell[i], stream[i]};
        int br, ti, at;
        out[i] = binomial(n[i], p[i], &key, &br, &ti, &at);
        if (branch) branch[i] = (uint8_t)br;
        if (tie) tie[i] = (uint8_t)ti;
        if (attempts) attempts[i] = at;
    }
}

"""Region totals: the one definition of what `Mcmc: groups` / `--groups` means on the host.

The device forms, for every kept draw, exact integer sums of the event counts over each group's members
(include/seir_hip.h, "Region totals on the device"): of the recorded epidemic, of the forecast and of the in-sample check.
Everything that is made of those sums is defined here and nowhere else:

  - `parse_groups`: a group specification -> names and a CSR pair (offsets [G+1], members [nnz]);
  - `group_state`: the state at the start of every day from the summed events and the summed initial state,
    state0 + exclusive cumsum of stoichiometry . events, in exact integers -- `model_spec.compute_state`'s rule;
  - `forecast_planes`: cases, cumulative cases and prevalence per group, with the definitions of forecast/*_quantiles;
  - `check_counts`: the counts of draws below / at the observed removals per group and day and over the window, and
    their mid-p values.

The locations of a draw are correlated through the commuting matrix: none of this can be had from per-location moments
or quantiles, which is why the sums are formed per draw.

The group curves (`Mcmc: groups_rt`, `groups_within_between`; include/seir_hip.h, "Group curves on the device") are sums of
fp64 values, whose bits depend on the order of the adds.  `weighted_sum_rows` is the one host definition of that order --
the device's (csrc/group_curve_kernels.h), restated in NumPy -- and `rt_weights`, `curve_moments`, `share_stats` are what
the run makes of the curves.

The group next-generation matrix (`Mcmc: groups_ngm`; include/seir_hip.h, "Group next-generation matrix on the device") is
K[g][h][t], the expected infections in group g caused by one typical infective of group h on day t: `ngm_rows` and
`group_ngm` restate the device's definition (csrc/ngm_kernels.h), `ngm_stats` and `spectral_radius` are what the run makes
of the draws, `require_ngm` its refusals."""
from dataclasses import dataclass

import numpy as np

MAX_GROUPS = 256                  # SEIR_GROUPS_MAX
PLANES = ("cases", "cum_cases", "prevalence")
NATIONS = ("E", "S", "W", "N")    # England, Scotland, Wales, Northern Ireland: the first letter of a GSS code


@dataclass
class GroupTable:
    names: list                   # [G] str
    offsets: np.ndarray           # [G+1] int32, offsets[0] = 0, strictly increasing
    members: np.ndarray           # [nnz] int32 rows, ascending and unique within a group

    @property
    def G(self) -> int:
        return len(self.names)

    def rows(self, g: int) -> np.ndarray:
        return self.members[self.offsets[g]:self.offsets[g + 1]]

    def sum_rows(self, x, axis=0):
        """x with `axis` indexed by location -> the same with that axis indexed by group (sums over the members)."""
        x = np.moveaxis(np.asarray(x), axis, 0)
        return np.moveaxis(np.stack([x[self.rows(g)].sum(axis=0) for g in range(self.G)]), 0, axis)


WAVE = 64                         # lanes of the fixed order of `weighted_sum_rows`


def weighted_sum_rows(table, v, weights=None, axis=-1):
    """The group sums of fp64 values in the device's fixed order: `v` float64 with `axis` indexed by location -> the same
    with that axis indexed by group; `weights` [nnz] aligned with `table.members`, or None.

    For one group with members m_0 < ... < m_{n-1} in CSR order: lane l in [0, 64) starts from +0.0 and adds, for
    k = l, l + 64, ... < n ascending, p = w_k * v[m_k] (one rounding; unweighted p = v[m_k]), one rounding per add; then for
    o = 32, 16, 8, 4, 2, 1, all lanes at once, a_l = a_l + a_{l xor o}; the result is a_0.  No fused multiply-add."""
    x = np.moveaxis(np.asarray(v, np.float64), axis, -1)
    w = None if weights is None else np.asarray(weights, np.float64).reshape(-1)
    if w is not None and w.shape != np.shape(table.members):
        raise ValueError(f"weights {w.shape}: aligned with the table's members {np.shape(table.members)}")
    lanes = np.arange(WAVE)
    out = np.empty(x.shape[:-1] + (table.G,))
    for g in range(table.G):
        beg, end = int(table.offsets[g]), int(table.offsets[g + 1])
        p = x[..., table.members[beg:end]]
        if w is not None:
            p = w[beg:end] * p
        a = np.zeros(x.shape[:-1] + (WAVE,))
        for k0 in range(0, end - beg, WAVE):
            c = p[..., k0:k0 + WAVE]
            a[..., :c.shape[-1]] = a[..., :c.shape[-1]] + c
        for o in (32, 16, 8, 4, 2, 1):
            a = a + a[..., lanes ^ o]
        out[..., g] = a[..., 0]
    return np.moveaxis(out, -1, axis)


def rt_weights(table, N):
    """The weights of the population-weighted group R_t: N[members] / the group's population, float64 [nnz].  The array
    handed to the device is the definition (groups/rt_weights)."""
    N = np.asarray(N, np.float64).reshape(-1)
    pop = table.sum_rows(N)
    return np.concatenate([N[table.rows(g)] / pop[g] for g in range(table.G)])


def curve_moments(curves):
    """Per-draw curves [n, ...] -> (mean, var (ddof 0), P(curve > 1)) over the draws, each [...]; NaN without draws."""
    c = np.asarray(curves, np.float64)
    if c.shape[0] == 0:
        nan = np.full(c.shape[1:], np.nan)
        return nan, nan.copy(), nan.copy()
    return c.mean(axis=0), c.var(axis=0), (c > 1.0).mean(axis=0)


def share_stats(within, between):
    """Per-draw group pressures [n, ...] -> (defined, within_share_mean, p_within_gt_between), each [...]: the share is
    Wg / (Wg + Bg); a draw with Wg + Bg == 0 (or a share that is not finite) is undefined and left out; NaN where no draw is
    defined."""
    wg, bg = np.asarray(within, np.float64), np.asarray(between, np.float64)
    tot = wg + bg
    with np.errstate(divide="ignore", invalid="ignore"):
        share = wg / tot
    ok = (tot != 0.0) & np.isfinite(share)
    n = ok.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(ok, share, 0.0).sum(axis=0) / n
        gt = (ok & (wg > bg)).sum(axis=0) / n
    return n.astype(np.float64), np.where(n > 0, mean, np.nan), np.where(n > 0, gt, np.nan)


NGM_PARTIALS = 4                  # partial sums of a rows-plane cell: member positions p, p + 4, ...


def ngm_rows(terms, table, period=1.0):
    """The rows plane of the group next-generation matrix in the device's fixed order (csrc/ngm_kernels.h): `terms` float64
    [..., M, D, M], terms[i][t][j] = S_it (1 - exp(-rate_ij)) of destination row i, day t and source column j (what the
    device returns for a table of singletons when the infectious period is exactly 1) -> P [..., G, D, M].

    For a group with members m_0 < ... < m_{n-1}: partial sum p in {0, 1, 2, 3} starts from +0.0 and adds the member
    POSITIONS k = p, p + 4, ... ascending, one rounding per add; P = ((p0 + p1) + (p2 + p3)) * period.  The device adds a
    term by the fused multiply-add of rt_cell, acc + S * prob with one rounding: this restatement has its bits wherever
    S * prob is exact (S a power of two, or 0), and is within one rounding per add of it everywhere else."""
    x = np.asarray(terms, np.float64)
    out = np.empty(x.shape[:-3] + (table.G,) + x.shape[-2:])
    for g in range(table.G):
        rows = table.rows(g)
        part = []
        for p in range(NGM_PARTIALS):
            acc = np.zeros(x.shape[:-3] + x.shape[-2:])
            for k in range(p, len(rows), NGM_PARTIALS):
                acc = acc + x[..., rows[k], :, :]
            part.append(acc)
        out[..., g, :, :] = ((part[0] + part[1]) + (part[2] + part[3])) * period
    return out


def group_ngm(rows, table, weights):
    """K from a rows plane: `rows` float64 [..., G, D, M] (P[g][t][j]; `SeirModel.group_ngm_rows`, or `ngm_rows`) ->
    K [..., G, G, D] (destination g, source h, day): the group sum of P[g][t][.] over the members of h with `weights` [nnz],
    in the one order of `weighted_sum_rows`."""
    k = weighted_sum_rows(table, np.asarray(rows, np.float64), weights, axis=-1)      # [..., g, D, h]
    return np.ascontiguousarray(np.moveaxis(k, -1, -2))


def is_partition(table, M):
    """Every location of [0, M) is a member of exactly one group."""
    return np.array_equal(np.sort(np.asarray(table.members)), np.arange(int(M)))


def ngm_stats(K, R_by_group, probs=None):
    """One chain's draws K [n, G, G, D] and the per-draw group curve R_by_group [n, G, D] (samples/R_t_by_group: the column
    sums of K's fine-grained matrix over ALL destinations) -> dict:
      K_mean, K_var [G, G, D]    over the draws (ddof 0); NaN without draws;
      local_share [n, G, D]      K[h][h][t] / R_by_group[h][t] per draw: the part of a region's R that stays inside it; NaN
                                 (without a warning) where R_by_group == 0;
      local_share_mean [G, D]    over the draws, NaN where any draw is undefined;
      K_quantiles [k, G, G, D], local_share_quantiles [k, G, D]    at `probs`, by the one rank rule
                                 (`posterior.quantiles`), when `probs` is given."""
    K = np.asarray(K, np.float64)
    R = np.asarray(R_by_group, np.float64)
    n, G = K.shape[0], K.shape[1]
    if K.ndim != 4 or K.shape[2] != G or R.shape != (n, G, K.shape[3]):
        raise ValueError(f"K {K.shape} and R_by_group {R.shape}: need [n, G, G, D] and [n, G, D]")
    diag = K[:, np.arange(G), np.arange(G), :]                     # [n, G, D]
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(R != 0.0, diag / np.where(R != 0.0, R, 1.0), np.nan)
    out = {"local_share": share}
    if n == 0:
        out["K_mean"], out["K_var"] = np.full(K.shape[1:], np.nan), np.full(K.shape[1:], np.nan)
        out["local_share_mean"] = np.full(R.shape[1:], np.nan)
    else:
        out["K_mean"], out["K_var"], out["local_share_mean"] = K.mean(axis=0), K.var(axis=0), share.mean(axis=0)
    if probs is not None:
        if n == 0:
            out["K_quantiles"] = np.full((len(probs),) + K.shape[1:], np.nan)
            out["local_share_quantiles"] = np.full((len(probs),) + R.shape[1:], np.nan)
        else:
            out["K_quantiles"] = quantiles(K, probs)
            undefined = np.isnan(share).any(axis=0)
            q = quantiles(np.where(undefined, 0.0, share), probs)
            out["local_share_quantiles"] = np.where(undefined, np.nan, q)
    return out


def spectral_radius(K):
    """K [..., G, G, D] -> max |eigenvalue| of K[..., :, :, t] per (draw, day), float64 [..., D].  For a table that
    partitions the locations this is the dominant eigenvalue of the next-generation matrix aggregated under
    population-distributed infectives (the weights of `rt_weights` spread a group's typical infective over its members by
    population), and of the next-generation matrix itself for a table of singletons.  It is formed only for a partition
    (`is_partition`): with overlapping groups or locations left out, K is not a next-generation matrix of anything."""
    K = np.asarray(K, np.float64)
    if K.ndim < 3 or K.shape[-3] != K.shape[-2]:
        raise ValueError(f"K {K.shape}: need [..., G, G, D]")
    if K.size == 0:
        return np.empty(K.shape[:-3] + K.shape[-1:])
    return np.abs(np.linalg.eigvals(np.moveaxis(K, -1, -3))).max(axis=-1)


def ngm_run_line(table, K, R_by_group):
    """One log line for K [n, B, G, G, D] with R_by_group [n, B, G, D]: every group's last-day local share with its 0.05 /
    0.95 quantiles over all draws and chains of this process, and the largest off-diagonal entry of the last day's mean with
    its (source -> destination) names."""
    K, R = np.asarray(K, np.float64), np.asarray(R_by_group, np.float64)
    if K.shape[0] == 0:
        return "Group next-generation matrix: no draws; ngm/* and samples/ngm_by_group written"
    G = K.shape[2]
    last = K[..., -1].reshape(-1, G, G)
    st = ngm_stats(last[..., None], R[..., -1].reshape(-1, G)[..., None], (0.05, 0.95))
    mean, q = st["local_share_mean"][:, 0], st["local_share_quantiles"][:, :, 0]
    shown = ", ".join(f"{name} {mean[g]:.3g} [{q[0, g]:.3g}, {q[1, g]:.3g}]"
                      for g, name in list(enumerate(table.names))[:6]) + (", ..." if G > 6 else "")
    line = (f"Local share of R_t by group (infections that stay inside the group), last day, mean [0.05, 0.95] over "
            f"{last.shape[0]} draw(s): {shown}")
    if G > 1:
        off = st["K_mean"][:, :, 0].copy()
        off[np.arange(G), np.arange(G)] = -np.inf
        g, h = np.unravel_index(int(np.argmax(off)), off.shape)
        line += f"; largest export {table.names[h]} -> {table.names[g]}: {off[g, h]:.3g}"
    return line + "; formed per draw on the device; ngm/* and samples/ngm_by_group written"


def curve_run_line(what, table, curves, dataset):
    """One log line for a per-draw group curve [n, B, G, D]: every group's last-day mean with its 0.05 / 0.95 quantiles
    over all draws and chains of this process."""
    c = np.asarray(curves, np.float64)
    if c.shape[0] == 0:
        return f"{what} by group: no draws; {dataset} written"
    last = c[..., -1].reshape(-1, c.shape[2])              # [n * B, G]
    q = quantiles(last, (0.05, 0.95))
    shown = ", ".join(f"{name} {last[:, g].mean():.3g} [{q[0, g]:.3g}, {q[1, g]:.3g}]"
                      for g, name in list(enumerate(table.names))[:6]) + (", ..." if table.G > 6 else "")
    return (f"{what} by group, last day, mean [0.05, 0.95] over {last.shape[0]} draw(s): {shown}; formed per draw on the "
            f"device; {dataset} written")


def _table(named_rows, what):
    if not named_rows:
        raise ValueError(f"{what}: no group at all")
    if len(named_rows) > MAX_GROUPS:
        raise ValueError(f"{what}: {len(named_rows)} groups, at most {MAX_GROUPS}")
    names, offsets, members = [], [0], []
    for name, rows in named_rows:
        if not rows:
            raise ValueError(f"{what}: group {name!r} is empty")
        if len(set(rows)) != len(rows):
            dup = sorted(r for r in set(rows) if rows.count(r) > 1)
            raise ValueError(f"{what}: group {name!r} names location index {dup[0]} more than once")
        names.append(str(name))
        members.extend(sorted(rows))
        offsets.append(len(members))
    return GroupTable(names, np.asarray(offsets, np.int32), np.asarray(members, np.int32))


def is_off(spec):
    """None, False and "off": no groups."""
    return spec is None or spec is False or (isinstance(spec, str) and spec.strip().lower() == "off")


def parse_groups(spec, M, location_names=None):
    """`Mcmc.groups`: "nations" (group by the first letter of the location code: `NATIONS` in that order, then any other
    letter in order of first appearance; needs `location_names`) or a mapping name -> list of members, a member being a
    location code, a prefix pattern "E0*" or an integer index.  None, False and "off" -> None.  ValueError for everything else: an unknown code, a pattern that
    matches nothing, an index outside [0, M), an empty group, a member named twice within a group, more than MAX_GROUPS."""
    if is_off(spec):
        return None
    M = int(M)
    names = None if location_names is None else [str(x) for x in location_names]
    if names is not None and len(names) != M:
        raise ValueError(f"groups: {len(names)} location names for M={M} locations")
    if isinstance(spec, str):
        if spec.strip().lower() != "nations":
            raise ValueError(f"groups={spec!r}: 'nations' or a mapping name -> members")
        if names is None:
            raise ValueError("groups='nations' needs the input file's location codes: the input has no `location` coordinate "
                             "(an .npz input carries none)")
        by_letter = {}
        for m, code in enumerate(names):
            if not code:
                raise ValueError(f"groups='nations': location {m} has an empty code")
            by_letter.setdefault(code[0], []).append(m)
        order = [c for c in NATIONS if c in by_letter] + [c for c in by_letter if c not in NATIONS]
        return _table([(c, by_letter[c]) for c in order], "groups='nations'")
    if not isinstance(spec, dict):
        raise ValueError(f"groups={spec!r}: 'nations' or a mapping name -> members")
    index = {} if names is None else {c: m for m, c in enumerate(names)}
    named_rows = []
    for gname, mem in spec.items():
        if isinstance(mem, (str, int, np.integer)) and not isinstance(mem, bool):
            mem = [mem]
        if not isinstance(mem, (list, tuple)):
            raise ValueError(f"groups: group {gname!r}: a list of location codes, prefix patterns or indices, not {mem!r}")
        rows = []
        for x in mem:
            if isinstance(x, bool):
                raise ValueError(f"groups: group {gname!r}: {x!r} is no member")
            if isinstance(x, (int, np.integer)):
                if not 0 <= int(x) < M:
                    raise ValueError(f"groups: group {gname!r}: index {int(x)} outside [0, M={M})")
                rows.append(int(x))
            elif isinstance(x, str) and x.endswith("*"):
                if names is None:
                    raise ValueError(f"groups: group {gname!r}: the pattern {x!r} needs the input file's location codes")
                hit = [m for m, c in enumerate(names) if c.startswith(x[:-1])]
                if not hit:
                    raise ValueError(f"groups: group {gname!r}: the pattern {x!r} matches no location code")
                rows.extend(hit)
            elif isinstance(x, str):
                if x not in index:
                    raise ValueError(f"groups: group {gname!r}: unknown location code {x!r}")
                rows.append(index[x])
            else:
                raise ValueError(f"groups: group {gname!r}: {x!r} is no member")
        named_rows.append((gname, rows))
    return _table(named_rows, "groups")


def load_spec(value):
    """The command line's `--groups SPEC`: "nations", or a path to a YAML mapping name -> members."""
    if isinstance(value, str) and value.strip().lower() in ("nations", "off"):
        return value.strip().lower()
    import yaml
    with open(value, "r") as f:
        spec = yaml.safe_load(f)
    if not isinstance(spec, dict):
        raise ValueError(f"--groups {value}: the file does not hold a mapping name -> members")
    return spec


def require_source(table, summaries, horizon, check_days, groups_rt=False, groups_within_between=False):
    """`groups` without any of summaries on / only, forecast, check -- or one of the group curves `groups_rt`,
    `groups_within_between` -- would launch and write nothing: refused."""
    if table is not None and summaries == "off" and not horizon and not check_days and not groups_rt and not groups_within_between:
        raise ValueError("groups given without any of summaries on/only, forecast, check: it would have no effect")


def require_curves(table, groups_rt, rt_days, groups_within_between, wb_days):
    """`groups_rt` needs `groups` and `rt`, `groups_within_between` needs `groups` and `within_between`: refused otherwise."""
    for on, key, need, days in ((groups_rt, "groups_rt", "rt", rt_days),
                                (groups_within_between, "groups_within_between", "within_between", wb_days)):
        if on and table is None:
            raise ValueError(f"{key} given without groups: there is no table of groups to form the curves over")
        if on and not days:
            raise ValueError(f"{key} given without {need}: it would have no effect")


def require_ngm(table, groups_ngm, rt_days, groups_rt):
    """`groups_ngm` needs `groups`, `rt` and `groups_rt` (whose per-draw curve is the denominator of the local share):
    refused otherwise."""
    if not groups_ngm:
        return
    if table is None:
        raise ValueError("groups_ngm given without groups: there is no table of groups to form the matrix over")
    if not rt_days:
        raise ValueError("groups_ngm given without rt: it would have no effect")
    if not groups_rt:
        raise ValueError("groups_ngm given without groups_rt: the group curve R_t_by_group is the denominator of the local share")


def switch(value, name):
    """An on / off key of the configuration (absent: off): True, False, "on", "off"."""
    if value is None or value is False:
        return False
    if value is True:
        return True
    if isinstance(value, str) and value.strip().lower() in ("on", "off"):
        return value.strip().lower() == "on"
    raise ValueError(f"{name}={value!r}: on or off")


def group_state(events_by_group, state0):
    """events_by_group [..., L, 3] and state0 [..., 3] (S, E, I at the window's start), integers -> int64 [..., L, 3]: the
    state at the START of every day, state0 + exclusive cumsum over days of stoichiometry . events."""
    ev = np.asarray(events_by_group)
    s0 = np.asarray(state0)
    if ev.dtype.kind not in "iu" or s0.dtype.kind not in "iu":
        raise TypeError("group_state is exact: integer arrays only")
    ev = ev.astype(np.int64)
    ex = np.cumsum(ev, axis=-2) - ev
    s0 = s0.astype(np.int64)[..., None, :]
    return np.stack([s0[..., 0] - ex[..., 0], s0[..., 1] + ex[..., 0] - ex[..., 1], s0[..., 2] + ex[..., 1] - ex[..., 2]], axis=-1)


def forecast_planes(events_by_group, state0):
    """The three planes of forecast/*_quantiles per group: [..., L, 3] and [..., 3] -> int64 [3, ..., L] in the order
    `PLANES`: cases k_ir, cumulative cases (inclusive), prevalence = I at the start of the day."""
    ev = np.asarray(events_by_group)
    st = group_state(ev, state0)
    cases = ev[..., 2].astype(np.int64)
    return np.stack([cases, np.cumsum(cases, axis=-1), st[..., 2]])


def mid_p(count, lt, eq):
    """(lt + eq / 2) / count, the rule of check/pit (`sampler.mid_p`); NaN where count = 0."""
    n = np.asarray(count, np.float64)
    num = 2.0 * np.asarray(lt, np.float64) + np.asarray(eq, np.float64)
    ok = n > 0
    return np.where(ok, num / np.where(ok, 2.0 * n, 1.0), np.nan)


def check_counts(check_by_group, observed_by_group):
    """check_by_group [n, G, K, 3] (one chain's draws) against observed_by_group [G, K] (the observed removals summed over
    the members): the raw counts, which pool over chains by a sum, and their mid-p values.  Keys: group_observed, group_lt,
    group_eq [G, K]; group_window_lt, group_window_eq [G] (the window's total); group_pit [G, K], group_window_pit [G]."""
    sim = np.asarray(check_by_group)[..., 2].astype(np.int64)
    obs = np.asarray(observed_by_group).astype(np.int64)
    n = sim.shape[0]
    out = {"group_observed": obs,
           "group_lt": (sim < obs).sum(axis=0), "group_eq": (sim == obs).sum(axis=0),
           "group_window_lt": (sim.sum(axis=-1) < obs.sum(axis=-1)).sum(axis=0),
           "group_window_eq": (sim.sum(axis=-1) == obs.sum(axis=-1)).sum(axis=0)}
    out["group_pit"] = mid_p(n, out["group_lt"], out["group_eq"])
    out["group_window_pit"] = mid_p(n, out["group_window_lt"], out["group_window_eq"])
    return out


def quantiles(x, probs):
    """Quantiles `probs` over the first axis of x [n, ...] by the one rank rule (`posterior.quantiles`): float64 [K, ...]."""
    from . import quantiles as Q
    x = np.asarray(x, np.float64)
    ranks = Q.quantile_ranks(x.shape[0], probs)
    return Q.interpolate(np.sort(x, axis=0)[ranks], ranks, x.shape[0], probs)


def run_line(table, sources):
    sizes = [int(table.offsets[g + 1] - table.offsets[g]) for g in range(table.G)]
    shown = ", ".join(f"{n} ({s})" for n, s in list(zip(table.names, sizes))[:6]) + (", ..." if table.G > 6 else "")
    return (f"Groups: {table.G} group(s) of locations -- {shown}; per-draw sums of {', '.join(sources)} formed on the device; "
            "groups/* and samples/*_by_group written")

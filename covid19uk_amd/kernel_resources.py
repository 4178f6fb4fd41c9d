"""The compiler's account of the library's kernels: parser of `hipcc -Rpass-analysis=kernel-resource-usage` remarks
(registers, scratch, spills, LDS, occupancy per kernel), and the table of which product owns which kernel.
`__graft_entry__.build()` keeps the account of every kernel next to the library as kernel_resources.json (the tracked copy:
profiles/kernel_resources.json); `owned` takes one owner's kernels out of it.  tests/test_resources.py holds the fresh
account to the tracked copy and the hot-path instances to their budgets; tools/dev/resources.py prints it."""
import re


def demangle(name):
    """`_ZN4seir6k_leapILi1ELi6ELi1ELi6EEEv...` -> `k_leap<1,6,1,6>` (the library's kernels only take integer and bool
    template arguments; anything else is returned as it is)."""
    m = re.match(r"_ZN4seir(\d+)", name)
    if not m:
        m = re.match(r"_Z(\d+)", name)
        if not m:
            return name
    n = int(m.group(1))
    base = name[m.end():m.end() + n]
    rest = name[m.end() + n:]
    if not rest.startswith("I"):
        return base
    args, i = [], 1
    while i < len(rest) and rest[i] != "E":
        a = re.match(r"L([ibjlmxy])(n?)(\d+)E", rest[i:])
        if not a:
            return base + "<?>"
        v = ("-" if a.group(2) else "") + a.group(3)
        args.append({"b": {"0": "false", "1": "true"}.get(v, v)}.get(a.group(1), v) if a.group(1) == "b" else v)
        i += a.end()
    return f"{base}<{','.join(args)}>"


FIELDS = {"sgpr": "TotalSGPRs", "vgpr": "VGPRs", "agpr": "AGPRs", "scratch_bytes_per_lane": r"ScratchSize \[bytes/lane\]",
          "occupancy_waves_per_simd": r"Occupancy \[waves/SIMD\]", "sgpr_spill": "SGPRs Spill", "vgpr_spill": "VGPRs Spill",
          "lds_bytes_per_block": r"LDS Size \[bytes/block\]"}


def parse(text):
    out = {}
    for blk in re.split(r"remark: [^\n]*Function Name: ", text)[1:]:
        name = demangle(blk.split()[0])
        ent = {}
        for key, pat in FIELDS.items():
            m = re.search(r"remark:\s+" + pat + r": (\d+)", blk)
            ent[key] = int(m.group(1)) if m else None
        out[name] = ent
    return out


BASE = "base"
# owner -> the kernels it brought, by base name (templates: every instance).  Every kernel that no owner names belongs to
# BASE: the sampler's kernels and the products up to the in-sample check
OWNERS = {
    "forecast_quantiles": ("k_forecast_keep", "k_order_stats"),   # forecast_kernels.h, order_stats_kernels.h
    "selftest": ("k_selftest_fn", "k_selftest_delta", "k_selftest_wave"),   # the device math's self-tests (selftest_kernels.h)
    "wb": ("k_wb_prepare", "k_wb_trace", "k_wb_finish"),          # the within/between pressure shares (wb_kernels.h)
    "rt_quantiles": ("k_rt_trace_keep", "k_order_stats_f64"),     # the R_t intervals (rt_keep_kernels.h, order_stats_kernels.h)
    "groups": ("k_group_sums",),                                  # the region totals (group_kernels.h)
    "group_curves": ("k_group_wsums", "k_rt_trace_cells", "k_rt_cells_from_keep", "k_wb_trace_cells"),   # group_curve_kernels.h
    "ngm": ("k_ngm_rows",),                                       # the group next-generation matrix (ngm_kernels.h)
    "replay": ("k_trace_load", "k_trace_load_theta"),             # stored draws into trace slots (trace_load_kernels.h)
    "scenarios": ("k_scenario_begin", "k_scenario_day", "k_scenario_diff"),   # scenarios riding on the forecast (scenario_kernels.h)
    "scenarios_local": ("k_scenario_local_begin", "k_scenario_local_day"),   # per-location operands (scenario_local_kernels.h)
    # measures that switch on case counts (scenario_trigger_kernels.h)
    "scenario_triggers": ("k_trigger_begin", "k_scenario_trigger_day", "k_trigger_fold"),
    "verify": ("k_verify_fold", "k_pair_abs"),                    # the forecast scored against later data (verify_kernels.h)
    # the event-update kernels for every m <= 4; their plain names (BASE) are the instances for m <= 2 (moves_kernel.h)
    "moves_m4": ("k_move_pairs_m4", "k_move_pair_m4", "k_move_pa2_m4", "k_move_delta_m4", "k_record_m4", "k_apply_fpend_m4"),
}


def move_instance_names(mm, nch):
    """The event-update kernels of sub-move bound `mm` (seir_move_instance: 2 or 4) and `nch` 64-day chunks per row (6, 12
    or 16), as the account spells them."""
    suf = {2: "", 4: "_m4"}[mm]
    return [f"k_move_pairs{suf}<{nch}>", f"k_move_pair{suf}<{nch}>", f"k_move_pa2{suf}<{nch}>", f"k_move_delta{suf}<false>",
            f"k_move_delta{suf}<true>", f"k_record{suf}", f"k_apply_fpend{suf}"]


def owned(res, owner):
    """The kernels of `res` (an account: instance -> figures) that belong to `owner`: a key of OWNERS, or BASE."""
    if owner == BASE:
        named = {b for names in OWNERS.values() for b in names}
        return {k: v for k, v in res.items() if k.split("<")[0] not in named}
    return {k: v for k, v in res.items() if k.split("<")[0] in OWNERS[owner]}

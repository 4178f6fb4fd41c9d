"""The sampler sweep's launch plan (covid19uk_amd/csrc/sweep_plan.h: plan_sweep, which enqueue_sweep executes) at the shapes
and placements that turn its decisions: a small host driver around the header, compiled as plain C++ -- seconds, no GPU.
The GPU tests hold every form to the same draws, so only this table notices when a sweep stops taking the form it should."""
import subprocess

import pytest

import __graft_entry__ as entry
from tests import helpers as H
from tests.test_resources import HOT_PATH

DRIVER = r"""
#include <cstdio>
#include "sweep_plan.h"
int main() {
    seir::SweepInputs in;
    int xl, og, ug, pl;
    while (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &in.M, &in.Mp, &in.Tp, &in.ntc, &in.nmt,
                      &in.nrb_d, &in.nb, &in.L, &in.n_scans, &in.record_events, &in.hmc_mode, &in.moves_mode, &in.leap_rows,
                      &xl, &og, &ug, &in.affinity, &in.cus, &in.leap_occ24, &in.leap_occ32, &pl) == 21) {
        in.xcd_local = xl; in.one_group = og; in.use_graph = ug; in.pairs_lds = pl;
        const seir::SweepPlan p = seir::plan_sweep(in);
        std::printf("hmc=%d inner=%d ts_mode=%d end_in_leap=%d chunk_aff=%d final_aff=%d per=%d nbv=%d nlive=%d leap_nst=%d "
                    "leap_nmt=%d leap_wgs=%d leap_nbv=%d leap_nlive=%d leap_launches=%d section_launches=%d section_evals=%d "
                    "moves=%d pre=%d nband=%d nbk=%d pair_nlive=%d nch=%d move_aff=%d fpend=%d record=%d advance=%d\n",
                    p.hmc, p.inner, p.ts_mode, p.end_in_leap, p.chunk_aff, p.final_aff, p.per, p.nbv, p.nlive, p.leap_nst,
                    p.leap_nmt, p.leap_wgs, p.leap_nbv, p.leap_nlive, p.leap_launches, p.section_launches, p.section_evals,
                    p.moves, p.pre, p.nband, p.nbk, p.pair_nlive, p.nch, p.move_aff, p.fpend, p.record, p.advance);
    }
}
"""
HMC = ("fold", "tailfold", "stage")
INNER = ("single", "leap", "se_chunk", "split")
MOVES = ("pairs", "pair", "split")
FPEND = (None, "k_move_pairs", "k_record", "k_apply_fpend")

# (M, T) of the BASELINE workloads (synth.py); any other shape is named as tests.helpers.build_case names it: "slow_MxT"
SHAPES = {"uk380": (380, 365), "ni11": (11, 32), "syn2048": (2048, 730)}
# the chip: 256 CUs; workgroups per CU of k_leap<1,6,1,6> (four) and of the 32-row instances k_leap<TSM,NTC,2,4> by their TSM:
# three with the column scalars alone, TWO with all four tile scalars (Mp > 512: 172 VGPRs) -- the compiler's figures, which
# test_resources.HOT_PATH holds the instances to and the library asks the driver for.  k_move_pairs granted its LDS; chains
# XCD-local, one group, stream launches, affinity 3; bench's MCMC_CONFIG and L = 16
LEAP_OCC24, LEAP_OCC32 = 4, {1: 3, 2: 2}
BASE = dict(nb=8, L=16, n_scans=5, record_events=1, hmc_mode=0, moves_mode=0, leap_rows=0, xcd_local=1, one_group=1,
            use_graph=0, affinity=3, cus=256, leap_occ24=LEAP_OCC24, leap_occ32=None, pairs_lds=1)
FIELDS = ("M", "Mp", "Tp", "ntc", "nmt", "nrb_d") + tuple(BASE)


def shape_of(shape):
    return SHAPES[shape] if shape in SHAPES else tuple(int(v) for v in shape.split("_")[1].split("x"))


def inputs(shape="uk380", **kw):
    M, T = shape_of(shape)
    Mp, Tp = (M + 63) // 64 * 64, (T + 63) // 64 * 64
    row = dict(BASE, M=M, Mp=Mp, Tp=Tp, ntc=Tp // 64, nmt=Mp // 16, nrb_d=(M + 7) // 8)
    row.update(kw)
    if row["leap_occ32"] is None:                     # the occupancy of THIS shape's instance (chunk_ts_mode of sweep_plan.h)
        row["leap_occ32"] = LEAP_OCC32[1 if Mp <= 512 else 2]
    return " ".join(str(int(row[f])) for f in FIELDS)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    try:
        hipcc = entry._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("sweep_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", entry.CSRC, "-o", str(exe), str(src)],
                   check=True, capture_output=True, text=True)

    def run(shape="uk380", **kw):
        out = subprocess.run([str(exe)], input=inputs(shape, **kw) + "\n", check=True, capture_output=True, text=True).stdout
        p = dict((k, int(v)) for k, v in (f.split("=") for f in out.split()))
        p["hmc"], p["inner"], p["moves"], p["fpend"] = HMC[p["hmc"]], INNER[p["inner"]], MOVES[p["moves"]], FPEND[p["fpend"]]
        return p
    return run


def leap_name(p):
    return "k_leap<1,6,1,6>" if p["leap_nst"] == 1 else f"k_leap<{p['ts_mode']},{p['ntc']},2,4>"


def hot_instances(p, ntc):
    """The template instances of a plan whose residency the launch arithmetic relies on (test_resources.HOT_PATH)."""
    p = dict(p, ntc=ntc)
    names = []
    if p["hmc"] == "fold" or p["inner"] == "leap":
        names.append(leap_name(p))
    if p["hmc"] == "tailfold" or p["inner"] == "se_chunk":
        names.append(f"k_se_chunk<{p['ts_mode']},{ntc}>")
    names.append(f"k_move_pairs<{p['nch']}>" if p["moves"] == "pairs" else f"k_move_pair<{p['nch']}>")
    if p["moves"] == "pair" and p["nband"] == 0:
        names.append("k_move_delta<false>")
    if p["record"]:
        names.append("k_record")
    return names


def check(p, **want):
    got = {k: p[k] for k in want}
    assert got == want


# --- [HMC] ---------------------------------------------------------------------------------------------------------------

def test_uk380_x8_one_persistent_launch_of_24_row_tiles(plan):
    p = plan(nb=8)
    check(p, hmc="fold", end_in_leap=1, ts_mode=1, leap_nst=1, leap_nmt=16, leap_wgs=96, leap_nbv=8, leap_nlive=0,
          leap_launches=1, per=12, section_launches=1, section_evals=17)
    assert leap_name(dict(p, ntc=6)) == "k_leap<1,6,1,6>"


@pytest.mark.parametrize("nb", [1, 3])
def test_uk380_fewer_chains_take_the_layout_of_8(plan, nb):
    p = plan(nb=nb)
    check(p, hmc="fold", leap_nst=1, leap_nbv=8, leap_nlive=nb, leap_launches=1, nbv=8, nlive=nb, section_launches=1,
          section_evals=17)
    check(p, moves="pairs", nband=24, nbk=8, pair_nlive=nb)


def test_uk380_x16_two_launches_of_8(plan):
    p = plan(nb=16)
    check(p, hmc="fold", leap_nst=1, leap_nbv=8, leap_nlive=0, leap_launches=2, section_launches=2, section_evals=17)


@pytest.mark.parametrize("nb,launches", [(16, 2), (8, 1)])
def test_uk380_leap_rows_32_takes_the_32_row_instance(plan, nb, launches):
    p = plan(nb=nb, leap_rows=32)
    check(p, hmc="fold", leap_nst=2, leap_nmt=24, leap_wgs=72, leap_nbv=8, leap_launches=launches,
          section_launches=launches, section_evals=17)
    assert leap_name(dict(p, ntc=6)) == "k_leap<1,6,2,4>"


def test_uk380_leap_rows_24_where_24_rows_do_not_fit_is_the_per_step_form(plan):
    check(plan(nb=32, leap_rows=24), hmc="tailfold")


def test_uk380_x32_per_step_launches_with_the_ends_by_the_roles(plan):
    p = plan(nb=32)
    check(p, hmc="tailfold", ts_mode=1, nbv=32, nlive=0, final_aff=1, section_launches=18, section_evals=17)


def test_ni11_x16_one_launch_of_the_32_row_instance(plan):
    p = plan("ni11", nb=16)
    check(p, hmc="fold", ts_mode=1, per=2, leap_nst=2, leap_wgs=2, leap_nbv=16, leap_launches=1, section_launches=1,
          section_evals=17)
    assert leap_name(dict(p, ntc=1)) == "k_leap<1,1,2,4>"


def test_syn2048_per_step_launches_with_all_four_tile_scalars(plan):
    p = plan("syn2048", nb=8)
    check(p, hmc="tailfold", ts_mode=2, per=44, section_launches=18, section_evals=17)


@pytest.mark.parametrize("hmc_mode,want", [
    (5, dict(hmc="fold", end_in_leap=0, leap_nst=1, leap_nmt=16, section_launches=1, section_evals=17)),
    (4, dict(hmc="stage", inner="leap", leap_nst=1, leap_launches=1, section_launches=1, section_evals=15)),
    (3, dict(hmc="stage", inner="se_chunk", section_launches=15, section_evals=15)),
    (2, dict(hmc="stage", inner="split", chunk_aff=1, section_launches=30, section_evals=15)),
    (6, dict(hmc="tailfold", section_launches=18, section_evals=17)),
    (1, dict(hmc="stage", inner="single", ts_mode=0, section_launches=0, section_evals=0)),
], ids=["chunk-stage", "chunk-leap", "chunk-launch", "chunk-split", "chunk-launch-fold", "single"])
def test_uk380_x8_hmc_modes(plan, hmc_mode, want):
    p = plan(nb=8, hmc_mode=hmc_mode)
    check(p, **want)
    check(p, moves="pairs", nband=24)


def test_uk380_x16_chunk_leap_reports_one_launch_of_two(plan):
    check(plan(nb=16, hmc_mode=4), hmc="stage", inner="leap", leap_nbv=8, leap_launches=2, section_launches=1,
          section_evals=15)


def test_mode_0_never_takes_the_stage_path_with_chunk_roles(plan):
    for nb in (1, 2, 3, 4, 5, 8, 11, 12, 16, 24, 32, 64):
        for shape in SHAPES:
            assert plan(shape, nb=nb)["hmc"] in ("fold", "tailfold") or plan(shape, nb=nb)["inner"] == "split", (shape, nb)


# --- placement -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw,nb", [(dict(use_graph=1), 8), (dict(one_group=0), 4), (dict(xcd_local=0), 8)],
                         ids=["graph", "two-groups", "not-xcd-local"])
def test_uk380_without_in_launch_hand_offs(plan, kw, nb):
    p = plan(nb=nb, **kw)
    check(p, hmc="stage", inner="split", chunk_aff=1, section_launches=30, section_evals=15)
    check(p, moves="pair", pre=1, nband=0, nbk=nb, pair_nlive=0)
    assert "k_move_delta<false>" in hot_instances(p, 6)


def test_uk380_affinity_0(plan):
    p = plan(nb=8, affinity=0)
    check(p, hmc="stage", inner="split", chunk_aff=0, section_launches=30, section_evals=15)
    check(p, moves="pairs", nband=24, move_aff=0)      # the band test does not read affinity bit 1


def test_hmc_final_grid(plan):
    check(plan(nb=3, hmc_mode=6), hmc="tailfold", nbv=8, nlive=3, final_aff=0)   # 12 roles x 3 chains: the 2-D grid
    check(plan(nb=32, affinity=1), hmc="tailfold", final_aff=1, move_aff=0)


def test_uk380_x8_two_leapfrog_steps_are_not_chunked(plan):
    check(plan(nb=8, L=2), hmc="stage", inner="single", ts_mode=0, section_launches=0, moves="pairs")


def test_persistent_pairs_need_their_lds(plan):
    check(plan(nb=8, pairs_lds=0), moves="pair", nband=24, pre=1)


def test_leap_needs_the_occupancy(plan):
    check(plan(nb=8, leap_occ24=3), hmc="fold", leap_nst=2, leap_launches=1)     # 108 x 8 > 768: the 32-row shape
    check(plan(nb=8, leap_occ24=3, leap_occ32=2), hmc="tailfold")


# --- event updates ---------------------------------------------------------------------------------------------------------

def test_uk380_x8_one_launch_for_every_pair(plan):
    p = plan(nb=8)
    check(p, moves="pairs", nband=24, nbk=8, pair_nlive=0, nch=6, move_aff=1, fpend="k_move_pairs", record=0, advance=0)


def test_uk380_x16_32_row_band_workgroups(plan):
    check(plan(nb=16), moves="pairs", nband=12, nbk=16, fpend="k_move_pairs")


def test_uk380_x32_one_launch_per_pair(plan):
    p = plan(nb=32)
    check(p, moves="pair", pre=1, nband=0, nbk=32, fpend="k_record", record=1, advance=0)


def test_ni11_x16_band(plan):
    check(plan("ni11", nb=16), moves="pairs", nband=1, nbk=16, nch=6)


def test_syn2048_no_band(plan):
    check(plan("syn2048", nb=8), moves="pair", pre=1, nband=0, nch=12, fpend="k_record", record=1)


@pytest.mark.parametrize("moves_mode,want", [
    (4, dict(moves="pair", pre=1, nband=24, nbk=8)),
    (3, dict(moves="pair", pre=1, nband=0, nbk=8)),
    (2, dict(moves="pair", pre=0, nband=24, nbk=8)),
    (1, dict(moves="split", pre=0, nband=0, fpend=None, record=1)),
], ids=["paired-launch", "paired-delta", "paired-nopre", "split"])
def test_uk380_x8_moves_modes(plan, moves_mode, want):
    check(plan(nb=8, moves_mode=moves_mode), **want)


def test_fpend_without_recorded_events(plan):
    check(plan(nb=32, record_events=0), moves="pair", fpend="k_apply_fpend", record=0)
    check(plan(nb=8, record_events=0), moves="pairs", fpend="k_move_pairs", record=0)


@pytest.mark.parametrize("moves_mode", range(5))
def test_more_than_30_scans_take_the_split_form(plan, moves_mode):
    p = plan(nb=8, n_scans=31, moves_mode=moves_mode)
    check(p, hmc="fold", section_launches=1, section_evals=17, moves="split")
    check(plan(nb=8, n_scans=30, moves_mode=moves_mode), moves={0: "pairs", 1: "split"}.get(moves_mode, "pair"))


def test_no_scans(plan):
    check(plan(nb=8, n_scans=0), hmc="fold", section_launches=1, section_evals=17, moves="pair", fpend=None, record=1,
          advance=1)


# --- the BASELINE configurations' instances are the ones test_resources holds to their occupancy ---------------------------

@pytest.mark.parametrize("shape,nb", [("uk380", 1), ("uk380", 8), ("uk380", 16), ("uk380", 32), ("ni11", 16), ("syn2048", 8)])
def test_baseline_instances_are_on_the_hot_path(plan, shape, nb):
    M, T = SHAPES[shape]
    names = hot_instances(plan(shape, nb=nb), ntc=(T + 63) // 64)
    missing = [n for n in names if n not in HOT_PATH]
    assert not missing, missing


# --- the shapes at which the plan turns to another instance of the persistent kernels ---------------------------------------

# (shape, leap_rows, sweeps, the plan): tests/test_sampler_shapes_gpu.py runs every row against the oracle -- three chains,
# its move configuration's three scans -- and holds the sampler's own seir_sampler_sweep_plan to the same members
_LEAP12 = dict(hmc="fold", inner="leap", ts_mode=1, leap_nst=2, leap_nmt=12, nch=12, moves="pairs")
SAMPLER_SHAPE_CASES = [
    # k_leap<1,6,2,4> by default (Mp no multiple of 24); no padding in rows or days
    ("slow_64x384", 0, 3, dict(hmc="fold", inner="leap", ts_mode=1, leap_nst=2, leap_nmt=4, nch=6)),
    # ... one live row in the second 64-row block
    ("slow_65x330", 0, 3, dict(hmc="fold", inner="leap", ts_mode=1, leap_nst=2, leap_nmt=8)),
    # k_leap<1,6,1,6> at Mp = 192: two of eight 24-row tiles are all padding, one live day in chunk 6; and in 32-row tiles
    ("slow_130x321", 0, 3, dict(hmc="fold", inner="leap", ts_mode=1, leap_nst=1, leap_nmt=8)),
    ("slow_130x321", 32, 3, dict(hmc="fold", inner="leap", ts_mode=1, leap_nst=2, leap_nmt=12)),
    # 24-row tiles with no padding anywhere
    ("slow_192x384", 0, 3, dict(hmc="fold", inner="leap", leap_nst=1, leap_nmt=8)),
    ("slow_192x384", 32, 3, dict(hmc="fold", inner="leap", leap_nst=2, leap_nmt=12)),
    # k_leap<1,12,2,4>: one live day in chunk 12 and one live row in block 3; the largest shape it fits, no padding
    ("slow_129x705", 0, 2, _LEAP12),
    ("slow_192x768", 0, 2, _LEAP12),
    # one row past: k_se_chunk<1,12> + k_hmc_final<12>
    ("slow_193x705", 0, 2, dict(hmc="tailfold", inner="se_chunk", ts_mode=1, nch=12)),
    # k_se_chunk<2,6> + k_hmc_final<6>
    ("slow_513x321", 0, 2, dict(hmc="tailfold", inner="se_chunk", ts_mode=2, nch=6, moves="pairs", nband=17)),
    # k_leap<2,1,2,4>; T is exactly one chunk
    ("slow_577x64", 0, 3, dict(hmc="fold", inner="leap", ts_mode=2, leap_nst=2, leap_nmt=40)),
    # nmt at its limit; event updates without band workgroups
    ("slow_1024x33", 0, 3, dict(hmc="fold", inner="leap", ts_mode=2, leap_nmt=64, moves="pair", nband=0)),
    # one row past: k_se_chunk<2,1> + k_hmc_final<1>
    ("slow_1025x33", 0, 3, dict(hmc="tailfold", inner="se_chunk", ts_mode=2)),
]
SHAPE_IDS = [f"{name}-rows{rows}" if rows else name for name, rows, _, _ in SAMPLER_SHAPE_CASES]


def shape_plan(plan, name, rows, nb=3):
    return plan(name, nb=nb, n_scans=3, leap_rows=rows)


@pytest.mark.parametrize("name,rows,n,want", SAMPLER_SHAPE_CASES, ids=SHAPE_IDS)
def test_sampler_shape_cases(plan, name, rows, n, want):
    p = shape_plan(plan, name, rows)
    check(p, **want)
    check(p, nbv=8, nlive=3, leap_launches=1)


def test_sampler_shape_cases_run_every_instance_the_plan_turns_to(plan):
    ran = set()
    for name, rows, _, _ in SAMPLER_SHAPE_CASES:
        p, ntc = shape_plan(plan, name, rows), (shape_of(name)[1] + 63) // 64
        ran.update(hot_instances(p, ntc) + ([f"k_hmc_final<{ntc}>"] if p["hmc"] == "tailfold" else []))
    want = {"k_leap<1,12,2,4>", "k_se_chunk<1,12>", "k_hmc_final<12>", "k_se_chunk<2,6>", "k_hmc_final<6>", "k_se_chunk<2,1>",
            "k_hmc_final<1>", "k_leap<2,1,2,4>", "k_leap<1,6,1,6>", "k_leap<1,6,2,4>"}
    assert want <= ran, want - ran
    # ... and the launches whose workgroups must all be resident are held to their occupancy
    missing = [k for k in want if k not in HOT_PATH and not k.startswith("k_hmc_final")]
    assert not missing, missing


def test_slow_129x705_x16_two_launches_of_8(plan):
    check(shape_plan(plan, "slow_129x705", 0, nb=16), hmc="fold", leap_nst=2, leap_nmt=12, leap_nbv=8, leap_launches=2)


def test_the_edges_of_the_shape_cases(plan):
    # one row or one day to either side of where an instance ends
    check(shape_plan(plan, "slow_192x769", 0), hmc="stage", inner="split")          # 13 day chunks: no roles
    check(shape_plan(plan, "slow_192x704", 0), hmc="stage", inner="split")          # 11
    check(shape_plan(plan, "slow_512x321", 0), hmc="tailfold", ts_mode=1)
    check(shape_plan(plan, "slow_576x64", 0), hmc="fold", ts_mode=2, leap_nmt=36)
    check(shape_plan(plan, "slow_512x64", 0), hmc="fold", ts_mode=1, leap_nmt=32)
    check(shape_plan(plan, "slow_1024x65", 0), hmc="stage", inner="split")          # 2 day chunks


def test_two_workgroups_per_cu_decide_at_sixteen_wide_chains(plan):
    """Where the occupancy of the ts_mode-2 instance turns the plan: 960 x 33, sixteen chains are (30 + 16) x 16 = 736
    workgroups -- one launch at three per CU, which the instance does not reach; at its two, two launches of 8."""
    check(plan("slow_960x33", nb=16), hmc="fold", ts_mode=2, leap_nbv=8, leap_launches=2)
    check(plan("slow_960x33", nb=16, leap_occ32=3), hmc="fold", ts_mode=2, leap_nbv=16, leap_launches=1)


def test_all_four_tile_scalars_never_take_k_leap_with_6_or_12_day_chunks(plan):
    """k_leap<2,6,2,4> and k_leap<2,12,2,4> are compiled and unreachable on 256 CUs: the smallest shape they would serve
    (Mp = 576, six chunks) is (108 + 15) x 8 = 984 workgroups against 2 x 256 places."""
    for M in range(64, 1025, 64):
        for ntc in (6, 12):
            for nb in (1, 8, 16):
                p = plan(f"slow_{M}x{64 * ntc}", nb=nb)
                assert p["ts_mode"] == (1 if M <= 512 else 2), (M, ntc, nb)
                if p["ts_mode"] == 2:
                    assert p["inner"] != "leap" and p["hmc"] == "tailfold", (M, ntc, nb, p)
                else:
                    assert p["hmc"] in ("fold", "tailfold"), (M, ntc, nb, p)


def test_the_occupancies_fed_to_the_plan_are_the_compilers():
    """LEAP_OCC24 / LEAP_OCC32 against the resource remarks of this build (256-thread workgroups: one wave per SIMD each,
    so waves per SIMD are workgroups per CU), and against what test_resources holds the instances to."""
    res = H.kernel_account("base")
    assert res["k_leap<1,6,1,6>"]["occupancy_waves_per_simd"] == LEAP_OCC24 == HOT_PATH["k_leap<1,6,1,6>"][1]
    seen = 0
    for name, r in res.items():
        if name.startswith("k_leap<") and name.endswith(",2,4>"):
            ts = int(name[len("k_leap<")])
            assert r["occupancy_waves_per_simd"] == LEAP_OCC32[ts], (name, r)
            assert HOT_PATH.get(name, (0, LEAP_OCC32[ts]))[1] == LEAP_OCC32[ts], name
            seen += 1
    assert seen == 6

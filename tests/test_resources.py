"""The compiler's account of the kernels (`hipcc -Rpass-analysis=kernel-resource-usage`, kept by `__graft_entry__.build()`
as covid19uk_amd/kernel_resources.json; the tracked copy is profiles/kernel_resources.json): the instances
that a BASELINE.json configuration launches on its hot path must not acquire scratch -- a spill inside a persistent launch's
step loop is paid in every step -- and must keep the occupancy their launches' residency arithmetic relies on.  And what holds
across the products (covid19uk_amd/kernel_resources.py: who owns which kernel): a fresh build gives the tracked copy, every
owner's kernels are there, no kernel has two owners.  What a product asks of its own kernels is in its tests/test_*_host.py."""
import json
import os

import pytest

import __graft_entry__ as entry
from covid19uk_amd import kernel_resources
from tests import helpers as H

TRACKED = os.path.join(entry.ROOT, "profiles", "kernel_resources.json")

# instance -> (max VGPRs, min waves per SIMD) the host's launch logic assumes; scratch must be 0 for all of them
HOT_PATH = {
    # UK-380 x 8 / x 1 chains (BASELINE configs 3, 4): the two persistent launches of a sweep
    "k_leap<1,6,1,6>": (128, 4),       # 24-row tiles: 96 + 12 workgroups per XCD need four waves per SIMD
    "k_leap<1,6,2,4>": (168, 3),       # 32-row tiles (the fall-back shape)
    "k_move_pairs<6>": (256, 2),
    # NI-11 x 16 chains (config 2)
    "k_leap<1,1,2,4>": (168, 3),
    # the per-step forms (16+ chains per GPU, a shared GPU, SYN-2048: config 5)
    "k_se_chunk<1,6>": (128, 4), "k_se_chunk<1,1>": (128, 4), "k_se_chunk<2,12>": (168, 3),
    "k_move_pair<6>": (168, 3), "k_move_pair<12>": (168, 3), "k_move_delta<false>": (128, 4),
    "k_hmc_step<0,1,1>": (256, 2), "k_hmc_step<2,1,1>": (256, 2), "k_hmc_step<0,2,4>": (256, 2), "k_hmc_step<2,2,4>": (256, 2),
    "k_se<true,1,0>": (128, 4), "k_se<true,1,1>": (128, 4), "k_se<true,1,2>": (128, 4), "k_record": (128, 4),
    "k_gemm_f32": (168, 3),
    # the instances the plan turns to beyond the BASELINE shapes (tests/test_sampler_shapes_gpu.py runs each of them): 12 day
    # chunks with few rows; all four tile scalars (Mp > 512: 172 VGPRs, TWO workgroups per CU -- what plan_sweep is told by
    # the driver, and what tests/test_sweep_plan.py tells it)
    "k_leap<1,12,2,4>": (168, 3), "k_leap<2,1,2,4>": (192, 2),
    "k_se_chunk<1,12>": (168, 3), "k_se_chunk<2,6>": (168, 3), "k_se_chunk<2,1>": (168, 3),
    # the stateless evaluation (seir_log_prob_dev) at UK-380 / SYN-2048 (96-day tiles) and NI-11 (64)
    "k_eval_all<true,96>": (128, 4), "k_eval_all<false,96>": (128, 4), "k_eval_tiles<true,96>": (128, 4),
    "k_eval_tiles<false,96>": (128, 4), "k_state_params": (128, 4), "k_finish<true>": (128, 4), "k_finish<false>": (128, 4),
}


@pytest.fixture(scope="module")
def resources():
    return H.kernel_account()


def test_every_hot_path_instance_is_compiled(resources):
    missing = [k for k in HOT_PATH if k not in resources]
    assert not missing, missing


@pytest.mark.parametrize("kernel", sorted(HOT_PATH))
def test_hot_path_instances_have_no_scratch_and_keep_their_occupancy(resources, kernel):
    r = resources[kernel]
    vmax, occ = HOT_PATH[kernel]
    assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0, (kernel, r)
    assert r["vgpr"] <= vmax and r["occupancy_waves_per_simd"] >= occ, (kernel, r)


def test_launches_fit_the_lds_at_the_shape_limits(resources):
    """Static LDS (the compiler's figure) + the dynamic LDS the host asks for, at the largest shape each launch is made
    for, within the 160 KiB of a gfx950 workgroup: the evaluation kernels at T = SEIR_MAX_T, k_rt's two day tiles at
    the largest Mp each is picked for, the simulator at M = 1280."""
    import re
    hdr = open(os.path.join(entry.ROOT, "include", "seir_hip.h")).read()
    t_max = int(re.search(r"#define SEIR_MAX_T (\d+)", hdr).group(1))
    tp = (t_max + 63) // 64 * 64
    assert tp == t_max
    scan = (8 * tp * 2 + 2048) * 8                                   # [SCAN_WAVES][Tp][2] | SCAN_LFT table
    cols = 8 * tp * 2 * 8

    def tiles(tn):                                                   # eval_tiles_lds_bytes<TN>
        panels = (2 * 16 * (80 + tn + 16) + 2) * 8
        epi = (64 * (tn + 2) + 4 * tn + 2 * 64 + 16) * 8
        return max(panels, epi, 2048 * 8)
    dynamic = {"k_scan<0>": scan, "k_scan<1>": scan, "k_scan_params": scan, "k_state_params": cols,
               "k_eval_all<true,64>": max(tiles(64), cols), "k_eval_all<false,64>": max(tiles(64), cols),
               "k_eval_all<true,96>": max(tiles(96), cols // tp * 960), "k_eval_all<false,96>": max(tiles(96), cols // tp * 960),
               "k_finish<true>": tp * 8, "k_finish<false>": tp * 8,
               "k_rt<16>": (2 * 16 * 512 + 4 * 16 * 64) * 8, "k_rt<4>": (2 * 4 * 2048 + 4 * 4 * 64) * 8,
               "k_simulate": 124 * 1280}
    over = {k: resources[k]["lds_bytes_per_block"] + v for k, v in dynamic.items()
            if resources[k]["lds_bytes_per_block"] + v > 160 * 1024}
    assert not over, over
    # ... and the limit is the largest such T: one more 64-day chunk does not fit the state scan
    assert resources["k_scan_params"]["lds_bytes_per_block"] + scan + 2 * 8 * 64 * 8 > 160 * 1024


def test_the_committed_copy_is_this_rounds(resources):
    """profiles/kernel_resources.json is the tracked copy the docs cite: it must list the same kernels, and agree with a
    fresh build on what the hot path is held to (scratch)."""
    doc = json.load(open(TRACKED))
    assert set(doc) == set(resources)
    for k in HOT_PATH:
        assert doc[k]["scratch_bytes_per_lane"] == resources[k]["scratch_bytes_per_lane"], k


def test_a_fresh_build_gives_the_committed_account_kernel_for_kernel_and_field_for_field(resources):
    """Every kernel of the library and every figure of each: a change to any kernel's registers, LDS, scratch, spills or
    occupancy, a kernel more or a kernel less, shows here, whichever product owns it."""
    doc = json.load(open(TRACKED))
    assert sorted(doc) == sorted(resources)
    wrong = {k: (resources[k], doc[k]) for k in doc if resources[k] != doc[k]}
    assert not wrong, wrong
    assert all(sorted(v) == sorted(kernel_resources.FIELDS) and None not in v.values() for v in resources.values())


def test_every_owner_has_its_kernels_and_no_kernel_has_two_owners(resources):
    named = [b for names in kernel_resources.OWNERS.values() for b in names]
    assert len(named) == len(set(named)), sorted(b for b in set(named) if named.count(b) > 1)
    assert kernel_resources.BASE not in kernel_resources.OWNERS
    compiled = {k.split("<")[0] for k in resources}
    assert not [b for b in named if b not in compiled]
    # ... so the owners' accounts, the base owner's included, are disjoint and together the whole account
    parts = [kernel_resources.owned(resources, o) for o in (kernel_resources.BASE, *kernel_resources.OWNERS)]
    assert all(parts) and sum(len(p) for p in parts) == len(resources)
    assert {k: v for p in parts for k, v in p.items()} == resources

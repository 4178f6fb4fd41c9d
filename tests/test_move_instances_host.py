"""The two sets of event-update instances (covid19uk_amd/csrc/moves_kernel.h, sampler_kernels.h: the kernels' plain names are
compiled for updates of m <= 2 sub-moves, the `_m4` kernels for every m <= 4), without a GPU: both sets are built, the m <= 2
instances of the hot path cost no more than their generic twins, the library resolves m and the option to the right set,
and the seeds of tests/test_move_instances_gpu.py do what they were chosen for on the C oracle."""
import re
import os

import pytest

import __graft_entry__ as entry
from covid19uk_amd import _lib, kernel_resources
from tests import helpers as H
from tests import move_instances_lib as L


@pytest.fixture(scope="module")
def resources():
    return H.kernel_account()


@pytest.fixture(scope="module")
def lib():
    entry.build()
    return _lib.load()


def test_the_bounds_are_the_headers(lib):
    src = open(os.path.join(entry.CSRC, "sampler_kernels.h")).read()
    assert int(re.search(r"constexpr int MMAX = (\d+);", src).group(1)) == _lib.MMAX == 4
    assert int(re.search(r"constexpr int MM_SMALL = (\d+);", src).group(1)) == _lib.MM_SMALL == 2


@pytest.mark.parametrize("nch", [6, 12, 16])
def test_both_sets_of_instances_are_compiled(resources, nch):
    for mm in (_lib.MM_SMALL, _lib.MMAX):
        missing = [k for k in kernel_resources.move_instance_names(mm, nch) if k not in resources]
        assert not missing, missing
    # the generic set has an owner of its own in the account; the plain names stay the base owner's
    m4 = kernel_resources.owned(resources, "moves_m4")
    assert set(kernel_resources.move_instance_names(_lib.MMAX, nch)) <= set(m4)
    assert not set(kernel_resources.move_instance_names(_lib.MM_SMALL, nch)) & set(m4)


@pytest.mark.parametrize("kernel", ["k_move_pairs", "k_move_pair"])
def test_the_small_instances_of_the_hot_path_cost_no_more_than_their_generic_twins(resources, kernel):
    small, generic = resources[f"{kernel}<6>"], resources[f"{kernel}_m4<6>"]
    print(kernel, "m <= 2:", small, "every m:", generic)
    assert small["scratch_bytes_per_lane"] == 0 and small["vgpr_spill"] == 0
    assert small["vgpr"] <= generic["vgpr"]
    assert small["sgpr_spill"] <= generic["sgpr_spill"]


@pytest.mark.parametrize("m,generic,mm", [(1, 0, 2), (2, 0, 2), (3, 0, 4), (4, 0, 4), (1, 1, 4), (2, 1, 4), (3, 1, 4)])
def test_m_and_the_option_resolve_to_the_instances(lib, resources, m, generic, mm):
    """seir_move_instance is the rule the sampler's launches follow (seir_sampler_move_instance reads it with the sampler's
    own m and its context's option; tests/test_move_instances_gpu.py holds a live sampler to it): m = 3 resolves to the
    generic names, m = 2 to the specialised ones -- unless SEIR_OPT_GENERIC_MOVES forces the generic ones."""
    assert lib.seir_move_instance(m, generic) == mm
    names = kernel_resources.move_instance_names(lib.seir_move_instance(m, generic), 6)
    assert all(("_m4" in k) == (mm == 4) for k in names) and all(k in resources for k in names)
    assert ("k_move_pairs<6>" in names) == (mm == 2) and ("k_move_pairs_m4<6>" in names) == (mm == 4)


@pytest.mark.parametrize("m", [0, 5, -1])
def test_an_m_the_library_does_not_serve_is_refused(lib, m):
    assert lib.seir_move_instance(m, 0) == _lib.ERR_INVALID
    assert b"outside [1, 4]" in lib.seir_last_error()


def test_the_instance_query_refuses_null(lib):
    import ctypes
    mm = ctypes.c_int32(-7)
    assert lib.seir_sampler_move_instance(None, ctypes.byref(mm)) == _lib.ERR_INVALID and mm.value == -7


@pytest.mark.parametrize("case_id", sorted(L.CASES))
def test_the_gpu_cases_seeds_accept_and_reject_every_update_kind_on_the_oracle(case_id):
    acc = L.oracle_decisions(case_id)
    print(case_id, "accepted of", acc.shape[0] * acc.shape[1], ":", dict(zip(L.MOVE_KEYS, acc.reshape(-1, 4).sum(axis=0))))
    assert L.both_ways(acc)

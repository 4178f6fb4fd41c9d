"""The sampler's device memory has one owner (covid19uk_amd/csrc/dev_mem.h; DESIGN.md, "Who owns the device memory"): what the
products allocate goes when they are resized, switched off, refused or closed, and a fresh allocation is zeroed before anything
that is enqueued behind it can write to it.  The case and the builders are those of tests/test_product_state_gpu.py: the
smallest shapes at which every product has buffers."""
import dataclasses

import numpy as np
import pytest
import torch

from covid19uk_amd import _lib
from tests import test_check_gpu as CG
from tests import test_forecast_gpu as FG
from tests.test_groups_gpu import _set
from tests.test_recovery_gpu import _case
from tests.test_rt_device_gpu import _weight
from tests.test_sampler_gpu import api  # noqa: F401  (fixture)
from tests.test_summary_gpu import _sampler

pytestmark = pytest.mark.gpu

CAP, N = 8, 4                                                   # trace capacity; draws of the one burst
STORE = 256 << 20                                               # what the R_it draw store alone takes, at least
SLACK = 64 << 20                                                # other tenants of a shared device (tests/test_rt_quantiles_gpu.py)


def _cycle(api, built):
    """Create, switch every product on, one burst through all of them, every extent changed, one refusal by size, close."""
    case, u, ev, cfg, eps = built
    w, M = _weight(case), case["k"].M
    model, s = _sampler(api, case, cfg, u, ev, eps, CAP)
    with model, s:
        s.reset_summary()
        s.reset_diagnostics(2)
        FG._reset(s, case, 5)
        CG._reset(s, case, 4)
        s.reset_rt(3, w)
        s.reset_within_between(6)
        s.keep_forecast_draws(CAP)
        keep = -(-STORE // (s.B * 3 * M * 8))                   # B x D x M x stride x 8 bytes, stride >= cap
        assert s.B * 3 * M * keep * 8 >= STORE and keep <= 1 << 20
        s.keep_rt_draws(keep)
        _set(s, [[0, 1, 2], [19]])
        s.set_group_rt(np.ones(4))
        s.set_group_within_between(True)
        s.set_group_ngm(np.ones(4), CAP)
        st = s._state()
        assert (st.summary_on, st.diag_batch_len, st.forecast_H, st.check_K, st.rt_D, st.wb_D) == (1, 2, 5, 4, 3, 6)
        assert (st.fc_keep_cap, st.rt_keep_cap, st.groups_G, st.group_L) == (CAP, keep, 2, (60, 5, 4))
        assert (st.group_rt_D, st.group_wb_D, st.ngm_cap, st.ngm_D) == (3, 6, CAP, 3)
        tr = s.sample(N, summarize=True, forecast=True, rt=True, check=True, within_between=True, groups=True)
        assert tr.rt.shape == (N, s.B, 3) and s.read_group_ngm(N).shape == (N, s.B, 2, 2, 3)
        assert (s._state().fc_j, s._state().ck_j, s._state().rt_j) == (N, N, N)
        # another D (twice), another H, another K, another table
        s.reset_rt(5, w)
        s.reset_within_between(4)
        FG._reset(s, case, 7)
        CG._reset(s, case, 3)
        _set(s, [[m] for m in range(M)])
        st = s._state()
        assert (st.forecast_H, st.check_K, st.rt_D, st.wb_D, st.rt_keep_cap, st.ngm_cap) == (7, 3, 5, 4, 0, 0)
        assert (st.groups_G, st.group_L, st.group_rt_on, st.group_wb_D) == (M, (60, 7, 3), 0, 4)
        # one refusal by size, as tests/test_ngm_gpu.py
        s.reset_rt(60, w)
        cap = 1 << 20
        assert cap * s.B * M * M * 60 * 8 > torch.cuda.mem_get_info()[0] / 2
        with pytest.raises(_lib.SeirError, match=r"next-generation matrix needs \d+ bytes .* more than half of the \d+ bytes free") as e:
            s.set_group_ngm(np.ones(M), cap)
        assert e.value.code == _lib.ERR_INVALID and s._state().ngm_cap == 0
        # no table
        s.set_groups(None, None)
        assert (s._state().groups_G, s._state().group_L) == (0, (0, 0, 0))
        assert not s.pair_timeouts().any()


def test_nothing_is_left_behind(api):
    """Four cycles of a sampler's life with every product on, each with an R_it draw store of at least 256 MiB: after the
    first (the warm-up: the runtime's own pools, the code object, the bindings' buffers) the free memory of the device is
    read, and after three more it is within 64 MiB of that reading -- the allowance for other tenants of a shared device.  A
    store leaked once per cycle would show as 768 MiB.  The test cannot see the leak of a small buffer: the table's device
    copy, a set of weights or a shadow of a few KiB per cycle disappears in the allowance."""
    built = _case("micro_20x60", 3)
    _cycle(api, built)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        _cycle(api, built)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    print(f"free after the warm-up cycle {free0}, after three more {free1}, difference {free1 - free0}")
    assert abs(free1 - free0) < SLACK


def _arrays(x, name=""):
    """Every array of a (nested) summary dataclass, by name."""
    if dataclasses.is_dataclass(x):
        return [a for f in dataclasses.fields(x) for a in _arrays(getattr(x, f.name), f"{name}.{f.name}")]
    return [(name, np.asarray(x))]


# product -> (its reset on (s, case), its call on slots, its blocking read)
PRODUCTS = {
    "rt": (lambda s, case: s.reset_rt(3, _weight(case)), "rt", "rt_summary"),
    "within_between": (lambda s, case: s.reset_within_between(6), "within_between", "within_between_summary"),
    "forecast": (lambda s, case: FG._reset(s, case, 5), "forecast", "forecast_summary"),
    "check": (lambda s, case: CG._reset(s, case, 4), "check", "check_summary"),
}


@pytest.mark.parametrize("product", PRODUCTS)
def test_a_product_folded_right_behind_its_first_reset_starts_from_zero(api, product):
    """The first reset allocates the product's accumulators and the product is enqueued behind it with no synchronising call
    of the test's in between: what is read then equals, bit for bit, what the same slots give after a second reset (which
    allocates nothing) and a synchronisation -- the zeroing of a fresh allocation is done before anything can be folded."""
    reset, call, read = PRODUCTS[product]
    case, u, ev, cfg, eps = _case("micro_20x60", 3)
    model, s = _sampler(api, case, cfg, u, ev, eps, CAP)
    with model, s:
        s.sample(N)
        reset(s, case)
        getattr(s, call)(0, N)
        first = _arrays(getattr(s, read)())
        reset(s, case)
        model.sync()
        getattr(s, call)(0, N)
        again = _arrays(getattr(s, read)())
        assert len(first) >= 4 and [k for k, _ in first] == [k for k, _ in again]
        assert int(first[0][1].max()) == N, first[0]                               # count: the draws were folded
        for (k, a), (_, b) in zip(first, again):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), k        # the bits: a NaN equals itself

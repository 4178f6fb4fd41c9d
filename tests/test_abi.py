"""CPU-only: the C-ABI library builds, loads and exports every symbol that
include/seir_hip.h declares; the host-side model spec matches the oracle's
derived constants.  No compute calls (no GPU here)."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
from covid19uk_amd import _lib, model_spec as ms, synth
from oracle import seir_oracle as so
from tests import abi_lib
from tests import helpers as H

ROOT = H.ROOT


@pytest.fixture(scope="module")
def lib():
    entry.build()
    return _lib.load()


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "seir_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(seir_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported(lib):
    declared = _declared_symbols()
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in seir_hip.h but not exported"
    assert sorted(declared) == _lib.exported_symbols()


def test_every_prototype_is_bound_with_the_headers_types(lib):
    """All of them, not only those a product's test pins (tests/abi_lib.py: check_symbols): the return type is the header's;
    an argument is the header's type, or a void pointer (to a void pointer) where the header declares a pointer -- the binding
    passes device pointers and handles that way on purpose."""
    declared = abi_lib.prototypes()
    assert sorted(declared) == _declared_symbols() and len(declared) == len(_lib._SIGNATURES)
    opaque = (ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p))
    for name, (ret, params) in declared.items():
        fn = getattr(lib, name)
        assert fn.restype is abi_lib.CTYPE[ret], (name, ret, fn.restype)
        assert len(fn.argtypes) == len(params), (name, params, fn.argtypes)
        for p, got in zip(params, fn.argtypes):
            assert got is abi_lib.CTYPE[abi_lib.c_type(p)] or (got in opaque and ("*" in p or "[" in p)), (name, p, got)


def test_abi_version_4_and_the_handoff_status(lib):
    text = open(os.path.join(ROOT, "include", "seir_hip.h")).read()
    declared = int(re.search(r"#define\s+SEIR_ABI_VERSION\s+(\d+)", text).group(1))
    assert lib.seir_abi_version() == declared == _lib.ABI_VERSION == 4
    # v4: hand-off time-outs have a status of their own, and the binding knows them by that status alone
    code = int(re.search(r"SEIR_ERR_HANDOFF\s*=\s*(-\d+)", text).group(1))
    assert code == _lib.ERR_HANDOFF == -4
    with pytest.raises(_lib.HandoffTimeout):
        _lib.check(code)
    with pytest.raises(_lib.SeirError) as e:
        _lib.check(-3)
    assert not isinstance(e.value, _lib.HandoffTimeout)


def test_sampler_desc_struct_layout_matches_header():
    # 12 int32, uint64 seed, then the ABI v2 tail: 6 int32 + 2 reserved
    assert ctypes.sizeof(_lib.SeirSamplerDesc) == 12 * 4 + 8 + 8 * 4
    assert _lib.SeirSamplerDesc.seed.offset == 48 and _lib.SeirSamplerDesc.moves_mode.offset == 56


def test_desc_struct_layout_matches_header():
    # 4 int32, 6 pointers, double, pointer, 3 doubles
    assert ctypes.sizeof(_lib.SeirDesc) == 16 + 6 * 8 + 8 + 8 + 3 * 8
    # seir_sim_desc: 4 int32, uint64 seed, 7 pointers
    assert ctypes.sizeof(_lib.SeirSimDesc) == 4 * 4 + 8 + 7 * 8


def test_product_state_struct_layout_matches_header():
    # 16 int32 (group_L is three of them), 6 int64, 2 reserved words
    assert ctypes.sizeof(_lib.SeirProductState) == 16 * 4 + 6 * 8 + 2 * 8
    assert _lib.SeirProductState.group_L.offset == 32 and _lib.SeirProductState.fc_j.offset == 64
    # member for member the header's struct, in its order
    text = open(os.path.join(ROOT, "include", "seir_hip.h")).read()
    body = re.search(r"typedef struct seir_product_state \{(.*?)\} seir_product_state;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [(t, n, int(k or 1)) for t, n, k in re.findall(r"\b(u?int(?:32|64)_t)\s+(\w+)(?:\[(\d+)\])?;", body)]
    bound = [(f[0], f[1]) for f in _lib.SeirProductState._fields_]
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64}
    assert bound == [(n, ctype[t] * k if k > 1 else ctype[t]) for t, n, k in declared]


def test_product_state_refuses_null_pointers_without_touching_the_gpu(lib):
    out = _lib.SeirProductState()
    assert lib.seir_sampler_product_state(None, ctypes.byref(out)) == _lib.ERR_INVALID
    assert b"null sampler" in lib.seir_last_error()
    assert lib.seir_sampler_product_state(None, None) == _lib.ERR_INVALID


def test_sweep_plan_struct_layout_matches_header_and_the_planner(lib):
    # 27 int32 and 5 reserved: member for member the header's struct, and every one of them a member of SweepPlan
    assert ctypes.sizeof(_lib.SeirSweepPlan) == 32 * 4
    text = open(os.path.join(ROOT, "include", "seir_hip.h")).read()
    body = re.search(r"typedef struct seir_sweep_plan \{(.*?)\} seir_sweep_plan;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n.strip() for line in re.findall(r"\bint32_t\s+([^;]+);", body) for n in line.split(",")]
    bound = [f[0] for f in _lib.SeirSweepPlan._fields_]
    assert declared[:-1] == bound[:-1] and declared[-1] == "reserved[5]" and bound[-1] == "reserved"
    plan = open(os.path.join(ROOT, "covid19uk_amd", "csrc", "sweep_plan.h")).read()
    members = re.search(r"struct SweepPlan \{(.*?)\n\};", plan, flags=re.S).group(1)
    members = re.sub(r"//[^\n]*|enum \{[^}]*\};", "", members)
    planner = {n.strip() for line in re.findall(r"\b(?:int|bool)\s+([^;]+);", members) for n in line.split(",")}
    assert planner == set(bound[:-1]), planner ^ set(bound[:-1])
    # the enums by the names the binding gives them, in the planner's order
    for names, enum in ((_lib.PLAN_HMC, "FOLD, TAILFOLD, STAGE"), (_lib.PLAN_INNER, "SINGLE, LEAP, SE_CHUNK, SPLIT"),
                        (_lib.PLAN_MOVES, "PAIRS, PAIR, SPLIT_MOVES"), (_lib.PLAN_FPEND, "F_NONE, F_PAIRS, F_RECORD, F_APPLY")):
        assert f"enum {{ {enum} }};" in plan and len(names) == len(enum.split(","))
    # host code only: NULL is refused without touching the GPU
    out = _lib.SeirSweepPlan()
    assert lib.seir_sampler_sweep_plan(None, ctypes.byref(out)) == _lib.ERR_INVALID
    assert b"null sampler" in lib.seir_last_error()


def test_every_key_the_burst_table_sizes_from_is_a_member_of_the_product_state():
    """The sizes of the burst table come from `ChainSampler._state()` alone: a sampler that has nothing but a record with
    everything on sizes every row, reads only members of the record, and the class has no private default to read instead."""
    from covid19uk_amd import sampler as sm
    read = set()

    class Spy:
        def __getattr__(self, key):
            read.add(key)
            return dict(group_L=(5, 2, 2)).get(key, 2)

    class Bare(sm.ChainSampler):
        T = 5

        def _state(self):
            return Spy()
    on = Bare.__new__(Bare)._burst_products(dict({p.request: True for p in sm.BURST_PRODUCTS if p.request}))
    assert list(on) == [p.field for p in sm.BURST_PRODUCTS]
    assert read and read <= set(sm.ProductState._fields), read - set(sm.ProductState._fields)
    private = [k for k, v in vars(sm.ChainSampler).items() if k.startswith("_") and not k.startswith("__") and not callable(v)]
    assert private == ["_thin", "_s"], private


def test_create_rejects_bad_arguments_without_touching_the_gpu(lib):
    ctx = ctypes.c_void_p()
    desc = _lib.SeirDesc(M=0, T=5, max_chains=1)
    assert lib.seir_create(ctypes.byref(desc), ctypes.byref(ctx)) == -1
    assert b"must be >= 1" in lib.seir_last_error()
    assert not ctx


def test_missing_device_fails_loudly(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from covid19uk_amd.seir import SeirModel
    cov = synth.make_covariates("ni11")
    _, init, _ = synth.simulate_epidemic(cov)
    with pytest.raises(_lib.SeirError):
        SeirModel(cov, init)


@pytest.mark.parametrize("name", ["ni11", "uk380"])
def test_host_constants_match_oracle(name):
    cov = synth.make_covariates(name)
    _, init, _ = synth.simulate_epidemic(cov)
    k = ms.derive_constants(cov)
    o = so.make_constants(cov.C, cov.N, cov.W, cov.weekday, cov.area, cov.adjacency, init)
    assert np.array_equal(k.Cstar, o.Cstar)
    assert np.array_equal(k.weekday_c, o.weekday_c)
    assert np.allclose(k.log_area_c, o.log_area_c, rtol=0, atol=1e-15)
    assert np.array_equal(k.car_Q, o.Q)
    assert abs(k.car_half_logdet - o.half_logdet_Q) < 1e-10 * abs(o.half_logdet_Q)
    assert ms.num_params(cov.M, cov.T) == o.P


def test_workload_shapes():
    for name, (M, T) in synth.WORKLOADS.items():
        if name == "syn2048":
            continue
        cov = synth.make_covariates(name)
        assert (cov.M, cov.T) == (M, T)
        ev, init, _ = synth.simulate_epidemic(cov)
        st = ms.compute_state(init, ev)
        assert st.min() >= 0 and ev.min() >= 0
        assert np.all(ev[..., 0] <= st[..., 0]) and np.all(ev[..., 1] <= st[..., 1])
        assert np.all(ev[..., 2] <= st[..., 2])


def test_series_constants():
    """The small-rate series in csrc/device_math.h: literals equal the exact Taylor
    coefficients and the truncated series meet 3e-16 on (0, 1/8] (mpmath reference)."""
    import mpmath as mp
    text = open(os.path.join(ROOT, "covid19uk_amd", "csrc", "device_math.h")).read()
    lits = sorted(set(float(x) for x in re.findall(r"\d\.\d{10,}e-\d+", text)))
    exact = sorted([1 / 24, 1 / 2880, 1 / 181440, 1 / 9676800, 1 / 12, 1 / 720, 1 / 30240, 1 / 1209600,
                    1 / 12, 1 / 360, 1 / 1260, 1 / 1680, 1 / 3, 1 / 6, 1 / 7, 2.3190468138462996e-17] +
                   # Bernoulli terms 5..8 of l1me_inv_wide: |B_2n| / (2n (2n)!) and |B_2n| / (2n)!
                   [float(abs(mp.bernoulli(2 * n)) / (2 * n * mp.factorial(2 * n))) for n in range(5, 9)] +
                   [float(abs(mp.bernoulli(2 * n)) / mp.factorial(2 * n)) for n in range(5, 9)])
    for v in lits:
        assert min(abs(v - e) / e for e in exact) < 1e-15, v
    m = re.search(r"L1ME_SERIES_MAX = ([0-9.]+);", text)
    rmax = float(m.group(1))
    mp.mp.dps = 40
    for r in list(np.logspace(-12, np.log10(rmax), 60)) + [rmax]:
        r2 = r * r
        L = np.log(r) + r * (-0.5 + r * (1 / 24 - r2 * (1 / 2880 - r2 * (1 / 181440 - r2 / 9676800))))
        inv = 1 / r - 0.5 + r * (1 / 12 - r2 * (1 / 720 - r2 * (1 / 30240 - r2 / 1209600)))
        Lt = mp.log(1 - mp.e ** (-mp.mpf(r)))
        It = 1 / (mp.e ** mp.mpf(r) - 1)
        assert abs((mp.mpf(L) - Lt) / Lt) < 3e-16 and abs((mp.mpf(inv) - It) / It) < 3e-16

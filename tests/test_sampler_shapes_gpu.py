"""The sampler sweep's persistent launches at the shapes its plan turns on (covid19uk_amd/csrc/sweep_plan.h): every template
instance of k_leap, k_se_chunk and k_hmc_final that plan_sweep can choose on this chip, at the smallest shape that reaches
it and at the edges inside it -- a 24-row tile that is all padding, a last day chunk with one live day, M and T exactly on
a 64 boundary at 6 and 12 day chunks, 64 row tiles -- draw by draw against the oracle sampler with the C density, with
tests/test_sampler_gpu.py's comparison and tolerances.  Every run reads the plan the sampler is about to execute
(`ChainSampler.sweep_plan()`) and holds it to the row of tests/test_sweep_plan.py: a shape that silently fell back to
another form fails here, and so does a run that timed out and went down the fall-back ladder."""
import numpy as np
import pytest

from oracle import mcmc_oracle as mo
from tests import helpers as H
from tests.test_sampler_gpu import CFG_SMALL, _compare, _start
from tests.test_sweep_plan import SAMPLER_SHAPE_CASES, SHAPE_IDS, shape_of

pytestmark = pytest.mark.gpu

SEED, B, EPS = 51, 3, 1e-5
NO_XCD = "this GPU does not place block ids congruent mod 8 on one XCD: the persistent forms are not used"
# The last 64-row block of these holds one or two live rows and no update of these few sweeps proposes there (the oracle
# alone: highest proposed row 62, 123, 124, 185, 492, 553, 983 -- the draws are exact, so the sampler's are the same);
# the density still sums those rows.  Everywhere else the proposals must reach the last 64-row block; in every case they
# must reach the last day chunk.
ROWS_STOP_SHORT = ("slow_65x330", "slow_129x705", "slow_130x321", "slow_193x705", "slow_513x321", "slow_577x64",
                   "slow_1025x33")
# Step sizes per chain for the run that takes the reject branch inside the launch.  Chosen on the CPU, the oracle alone
# (seed 51, three chains, the sweeps of the case): HMC here is either stable or not -- at 1e-5 every proposal of these
# shapes is accepted and from a threshold on every one is rejected, in all three chains at once (slow_130x321: all nine
# accepted at 2e-5, 3e-5 and 5e-5, none at 1e-4; slow_129x705, slow_193x705, slow_513x321: none of six at 2e-5, 3e-5, 5e-5
# or 1e-4) -- so no ONE step size of {2e-5, 3e-5, 5e-5, 1e-4} both accepts and rejects.  One launch carries all chains,
# each with its own step size: the first chain keeps the largest size at which it accepts, the other two take the
# smallest at which they reject, and the accept and the reject branch run side by side in the same launch.
REJECT_EPS = {
    "slow_130x321": (5e-5, 1e-4, 1e-4),
    "slow_129x705": (1e-5, 2e-5, 2e-5),
    "slow_193x705": (1e-5, 2e-5, 2e-5),
    "slow_513x321": (1e-5, 2e-5, 2e-5),
}
_CASES, _ORACLES, _TRACES = {}, {}, {}


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as entry
    entry.build()
    from covid19uk_amd.seir import SeirModel
    from covid19uk_amd.sampler import ChainSampler
    return SeirModel, ChainSampler


def _case(name):
    """The epidemic of a shape and the start of its three chains, built once."""
    if name not in _CASES:
        case = H.build_case(name, SEED, alpha_t_sd=0.005)
        _CASES[name] = (case,) + _start(case, B, SEED, scale=0.01)
    return _CASES[name]


def _oracles(name, n, eps=(EPS,) * B):
    """Three oracle chains (ids 5, 6, 7) of a shape with the C restatement of the density, shared by every run of it."""
    from oracle import c_binding
    if (name, eps) not in _ORACLES:
        case, u, ev = _case(name)
        k = case["k"]
        out = []
        for b in range(B):
            ch = mo.OracleChain(k, CFG_SMALL, u[b], ev[b], seed=77, chain_id=5 + b,
                                log_prob_fn=lambda u_, e_: c_binding.evaluate(k, u_, e_, 1),
                                log_prob_grad_fn=lambda u_, e_: c_binding.evaluate(k, u_, e_, 1, want_grad=True))
            ch.eps = eps[b]
            out.append([ch.sweep_once() for _ in range(n)])
        _ORACLES[name, eps] = out
    return _ORACLES[name, eps]


def _run(api, name, rows, n, want, eps=EPS, skew=0, u=None, ev=None, **more):
    """n sweeps in the default launch forms; the plan in force is the one expected, and nothing timed out."""
    SeirModel, ChainSampler = api
    case, u3, ev3 = _case(name)
    u, ev = (u3, ev3) if u is None else (u, ev)
    nb = u.shape[0]
    with SeirModel(case["cov"], case["init"], max_chains=nb) as model:
        if skew:
            model.set_option(debug_skew=skew)
        with ChainSampler(model, CFG_SMALL, nb, seed=77, first_chain_id=5, trace_capacity=n, record_events=True,
                          leap_rows=rows) as s:
            if not s.xcd_local():
                pytest.skip(NO_XCD)
            plan = s.sweep_plan()
            want = dict(want, nbv=(nb + 7) // 8 * 8, **more)
            assert {k: plan[k] for k in want} == want, plan
            assert s.launch_form() == ("chunk", "paired")
            s.set_state(u, ev)
            s.set_kernel(step_size=eps)
            tr = s.sample(n)
            assert not s.recoveries and not s.pair_timeouts().any()
            assert s.sweep_plan() == plan
    return tr


def _plain(api, name, rows, n, want):
    if (name, rows) not in _TRACES:
        _TRACES[name, rows] = _run(api, name, rows, n, want)
    return _TRACES[name, rows]


def _arrays(tr):
    yield "theta", tr.theta
    yield "events", tr.events
    for k, v in tr.hmc.items():
        yield "hmc/" + k, v
    for mk, mv in tr.moves.items():
        for k, v in mv.items():
            yield mk + "/" + k, v


@pytest.mark.parametrize("name,rows,n,want", SAMPLER_SHAPE_CASES, ids=SHAPE_IDS)
def test_shape_matches_oracle_draw_by_draw(api, name, rows, n, want):
    M, T = shape_of(name)
    tr = _plain(api, name, rows, n, want)
    assert tr.events.dtype == np.int32
    _compare(tr, _oracles(name, n), n, B, CFG_SMALL)
    assert tr.hmc["is_accepted"].any()
    assert any(tr.moves[k]["is_accepted"].any() for k in tr.moves)
    days = np.concatenate([tr.moves[k]["proposed_delta"][..., 1, :].ravel() for k in tr.moves])
    assert (days >= (T - 1) // 64 * 64).any()
    if name not in ROWS_STOP_SHORT:
        rows_ = np.concatenate([tr.moves[k]["proposed_delta"][..., 0, :].ravel() for k in tr.moves])
        assert (rows_ >= (M - 1) // 64 * 64).any()
    # the data reaches the last day chunk and the last 64-row block in every case
    ev = _case(name)[0]["events"]
    assert ev[:, (T - 1) // 64 * 64:, :2].sum() > 0 and ev[(M - 1) // 64 * 64:, :, :2].sum() > 0


@pytest.mark.parametrize("name,rows,n,want", SAMPLER_SHAPE_CASES, ids=SHAPE_IDS)
def test_shape_does_not_depend_on_workgroup_timing(api, name, rows, n, want):
    """Every case is one persistent launch (fold) or a chain of launches with hand-offs inside them (tailfold): with the
    workgroups started out of step the trace is the same to the bit."""
    assert want["hmc"] in ("fold", "tailfold")
    ref = _plain(api, name, rows, n, want)
    got = _run(api, name, rows, n, want, skew=2)
    for (key, a), (_, b) in zip(_arrays(ref), _arrays(got)):
        assert a.dtype == b.dtype and np.array_equal(a, b), key


@pytest.mark.parametrize("name,rows,n,want", [c for c in SAMPLER_SHAPE_CASES if c[0] in REJECT_EPS and c[1] == 0],
                         ids=[i for i, c in zip(SHAPE_IDS, SAMPLER_SHAPE_CASES) if c[0] in REJECT_EPS and c[1] == 0])
def test_shape_takes_the_reject_branch_inside_the_launch(api, name, rows, n, want):
    """Accepted and rejected trajectories side by side in one launch (REJECT_EPS): draw by draw against the oracle, and a
    rejected sweep leaves theta as the previous draw has it, to the bit."""
    eps = REJECT_EPS[name]
    oracles = _oracles(name, n, eps)
    acc = np.array([[oracles[b][i]["hmc"]["is_accepted"] for b in range(B)] for i in range(n)])
    assert acc.any() and not acc.all(), "REJECT_EPS: the oracle alone must both accept and reject"
    assert not acc[1:].all(), "REJECT_EPS: a rejected sweep with a draw before it"
    tr = _run(api, name, rows, n, want, eps=np.array(eps))
    _compare(tr, oracles, n, B, CFG_SMALL)
    assert np.array_equal(tr.hmc["is_accepted"].astype(bool), acc)
    for i in range(1, n):
        for b in range(B):
            if not acc[i, b]:
                assert np.array_equal(tr.theta[i, b], tr.theta[i - 1, b]), (i, b)


def test_slow_129x705_x16_is_two_launches_of_8(api):
    """Sixteen chains of the 12-chunk instance do not fit the chip at once: two launches of eight, one after the other.
    Chains are keyed by their id, so chains 0-2 are the three of the other runs whatever else is in the batch."""
    name, rows, n, want = next(c for c in SAMPLER_SHAPE_CASES if c[0] == "slow_129x705")
    case, u3, ev3 = _case(name)
    u16, ev16 = _start(case, 16, SEED, scale=0.01)
    u16[:B], ev16[:B] = u3, ev3
    tr = _run(api, name, rows, n, want, u=u16, ev=ev16, leap_nbv=8, leap_launches=2)
    assert tr.theta.shape[1] == 16
    _compare(tr, _oracles(name, n), n, B, CFG_SMALL)
    assert tr.hmc["is_accepted"].any()
    # the other thirteen are chains of their own
    assert len({tr.theta[-1, b].tobytes() for b in range(16)}) == 16

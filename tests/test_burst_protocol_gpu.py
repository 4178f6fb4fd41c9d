"""The burst protocol on the device (covid19uk_amd/sampler.py, `BURST_PRODUCTS`): the blocking path and the overlapped
bursts run the same table, so two samplers started alike -- one advanced by `sample`, one by `sample_bursts` -- leave the
same bits in every field of the trace, with every product on."""
import numpy as np
import pytest

import __graft_entry__ as entry
from covid19uk_amd import synth
from covid19uk_amd.inference import inference as inf
from covid19uk_amd.posterior import groups as G
from covid19uk_amd.posterior import predict
from covid19uk_amd.sampler import Trace
from tests import helpers as H

pytestmark = pytest.mark.gpu

CFG = dict(dmax=8, nmax=6, m=2, occult_nmax=5, num_event_time_updates=3)
FIELDS = tuple(f for f in Trace.__dataclass_fields__ if f not in ("hmc", "moves"))   # theta, events and every product's field


def _copy(tr):
    out = {}
    for f in FIELDS:
        v = getattr(tr, f)
        assert v is not None, f                                # every product is on
        out[f] = {k: np.array(a) for k, a in v.items()} if isinstance(v, dict) else np.array(v)
    return out


def test_sample_and_sample_bursts_leave_the_same_bits_in_every_field():
    """M = 3, T = 5, B = 2: three calls of sample(4) against sample_bursts(3, 4), summaries, a forecast with random-walk
    steps, R_t, the check, within / between, the group sums of all three sources and both group curves on."""
    import torch
    assert torch.cuda.is_available()
    entry.build()
    from covid19uk_amd.sampler import ChainSampler
    from covid19uk_amd.seir import SeirModel
    M, T, B, nb, burst, Hn, K, D = 3, 5, 2, 3, 4, 2, 3, 4
    case = H.build_case(f"micro_{M}x{T}", 43, alpha_t_sd=0.005)
    cov, N = case["cov"], np.asarray(case["cov"].N, np.float64).reshape(-1)
    u = synth.jitter_params(case["u"], B, scale=0.01, seed=3, T=T)
    ev = np.stack([case["events"]] * B)
    tab = G.parse_groups({"all": [0, 1, 2], "ends": [0, 2], "middle": [1]}, M)
    kw = dict(summarize=True, forecast=inf.forecast_steps_fn(7, [0, 1], Hn), rt=True, check=True, within_between=True,
              groups=True)
    runs = []
    for overlapped in (False, True):
        with SeirModel(cov, case["init"], max_chains=B) as model, \
                ChainSampler(model, CFG, B, seed=13, trace_capacity=2 * burst, log=None) as s:
            s.set_state(u, ev)
            s.set_kernel(step_size=0.0004)
            s.set_groups(tab.offsets, tab.members)
            s.set_group_rt(G.rt_weights(tab, N))
            s.set_group_within_between(True)
            s.reset_forecast(Hn, *predict.forecast_calendar(cov, None, T, Hn), 5)
            s.reset_check(K, *predict.check_calendar(cov, None, T, K), 6)
            s.reset_rt(D, N / N.sum())
            s.reset_within_between(D)
            if overlapped:
                got = {}
                s.sample_bursts(nb, burst, lambda tr, i, got=got: got.__setitem__(i, _copy(tr)), **kw)
                runs.append([got[i] for i in range(nb)])
            else:
                runs.append([_copy(s.sample(burst, **kw)) for _ in range(nb)])
    for i, (a, b) in enumerate(zip(*runs)):
        for f in FIELDS:
            if isinstance(a[f], dict):
                assert list(a[f]) == list(b[f]), (i, f)
                for k in a[f]:
                    assert a[f][k].shape[:2] == (burst, 2) and np.array_equal(a[f][k], b[f][k]), (i, f, k)
            else:
                assert a[f].shape[:2] == (burst, 2) and np.array_equal(a[f], b[f]), (i, f)
    assert not np.array_equal(runs[0][0]["theta"], runs[0][1]["theta"])       # the chain moves

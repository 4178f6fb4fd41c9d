"""Developer timelines: what every stamp tool needs, once (the facility itself: covid19uk_amd/csrc/stamps.h).

    load_variant(tag)             the stamped library tools/dev/variants/libseirhip_<tag>.so (build_variant.sh <tag>) in place
                                  of the product library, with the two readers declared
    probe_sampler(...)            the UK-380 x 8 model and sampler every tool stamps (a context manager: model, sampler)
    read(handle, family, reset)   the family's region as named arrays, shaped by LAYOUT -- the Python copy of the header's table
"""
import contextlib
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# family -> B -> {name: (first word, shape)}, as stamps.h states it
LAYOUT = {
    "seir": lambda B: {"words": (0, (16,))},
    "pair": lambda B: {"steps": (0, (27, 12, 16))},                       # [slot][step][stamp]
    "leap": lambda B: {"chains": (0, (B, 16, 8)), "tiles": (B * 128, (2, 16, 8)), "roles": ((B + 2) * 128, (2, 16, 16)),
                       "all": ((B + 6) * 128, (1024, 4))},                # [..][step][stamp]; all: [tile][stamp]
    "tail": lambda B: {"chains": (0, (B, 8))},
    "eval": lambda B: {"words": (0, (7,))},
}
CTX_FAMILIES = ("se", "eval")                                             # read through the model, not the sampler
# named words (stamps.h: SW_ROLE, SW_DELTA)
SW_ROLE, SW_ROLE_PROPOSE, SW_DELTA = 8, 12, 12


def extent(family, B):
    return max(first + int(np.prod(shape)) for first, shape in LAYOUT[family](B).values())


def load_variant(tag):
    from covid19uk_amd import _lib
    _lib.LIB_PATH = os.path.join(ROOT, "tools", "dev", "variants", f"libseirhip_{tag}.so")
    lib = _lib.load()
    for fn in (lib.seir_stamps_read, lib.seir_stamps_read_ctx):
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int]
        fn.restype = ctypes.c_int
    return lib


@contextlib.contextmanager
def probe_sampler(B=8, workload="uk380", trace_capacity=50, step_size=1.2e-5, jitter_scale=0.002, cfg=None, **sampler_kw):
    """The tools' common set-up: `workload` x B chains around the simulated truth, event updates as in production
    (cfg overrides, e.g. num_event_time_updates), record_events off; sampler_kw: moves, leap_rows, num_leapfrog_steps ..."""
    from covid19uk_amd import synth
    from covid19uk_amd.sampler import ChainSampler
    from covid19uk_amd.seir import SeirModel
    full = dict(dmax=84, nmax=25, m=2, occult_nmax=15, num_event_time_updates=5)
    full.update(cfg or {})
    cov = synth.make_covariates(workload)
    events, init, truth = synth.simulate_epidemic(cov)
    u0 = synth.unconstrain(synth.pack_params(truth, cov.M, cov.T))
    u = synth.jitter_params(u0, B, scale=jitter_scale, seed=7, T=cov.T)
    ev = np.stack([events] * B)
    with SeirModel(cov, init, max_chains=B) as model:
        with ChainSampler(model, full, B, seed=1, trace_capacity=trace_capacity, record_events=False, **sampler_kw) as s:
            s.set_state(u, ev)
            s.set_kernel(step_size=step_size)
            yield model, s


def read(handle, family, reset=False, n_words=None):
    """The family's region after everything enqueued has finished; reset: rewritten afterwards by the table's pattern.
    handle: the ChainSampler (seir, pair, leap, tail) or the SeirModel (se: n_words tile-scalar words as [n / 4][4]; eval)."""
    from covid19uk_amd import _lib
    lib = _lib.load()
    if family in CTX_FAMILIES:
        n = n_words if family == "se" else extent(family, 0)
        out = np.zeros(n, dtype=np.uint64)
        rc = lib.seir_stamps_read_ctx(handle._ctx, out.ctypes.data, n, int(reset))
        if rc:
            raise _lib.SeirError(f"seir_stamps_read_ctx: {rc}")
        return {"tiles": out.reshape(-1, 4)} if family == "se" else {"words": out}
    B = handle.B
    out = np.zeros(extent(family, B), dtype=np.uint64)
    rc = lib.seir_stamps_read(handle._s, out.ctypes.data, out.size, int(reset))
    if rc:
        raise _lib.SeirError(f"seir_stamps_read: {rc}")
    return {name: out[first:first + int(np.prod(shape))].reshape(shape) for name, (first, shape) in LAYOUT[family](B).items()}

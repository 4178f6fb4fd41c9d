"""`SeirModel`: the device-resident counterpart of the reference's
`model = CovidUK(covariates, initial_state, initial_step=0, num_steps=T)`
together with the `joint_log_prob(unconstrained_params, events)` closure built
on it (covid19uk/inference/inference.py:518-557).

All arithmetic happens in libseirhip.so (HIP, gfx950) through the C-ABI of
include/seir_hip.h; this class only marshals arrays.  PyTorch is used purely as
a device-memory container for the `*_dev` methods.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from . import model_spec as ms


def _dptr(a: np.ndarray):
    return a.ctypes.data_as(_lib.c_double_p)


class SeirModel:
    def __init__(self, covariates: ms.Covariates, initial_state, max_chains: int = 1, device: int = 0,
                 constants: ms.DerivedConstants = None):
        """`constants`: pre-derived closure constants to use instead of `derive_constants(covariates)` -- a
        T-shard passes the slices of the FULL series' constants (the weekday is centred over all days,
        model_spec.py:224-225), see covid19uk_amd/tshard.py."""
        self._lib = _lib.load()
        self._ctx = ctypes.c_void_p()
        k = ms.derive_constants(covariates) if constants is None else constants
        self.M, self.T = covariates.M, covariates.T
        self.P = ms.num_params(self.M, self.T)
        self.max_chains = int(max_chains)
        self.device = int(device)
        init = np.ascontiguousarray(initial_state, dtype=np.float64)
        if init.shape != (self.M, 4):
            raise ValueError(f"initial_state must be [M,4]=({self.M},4), got {init.shape}")
        self.initial_state = init
        keep = dict(Cstar=np.ascontiguousarray(k.Cstar), N=np.ascontiguousarray(k.N),
                    W=np.ascontiguousarray(k.W), wd=np.ascontiguousarray(k.weekday_c),
                    la=np.ascontiguousarray(k.log_area_c), Q=np.ascontiguousarray(k.car_Q))
        desc = _lib.SeirDesc(
            M=self.M, T=self.T, max_chains=self.max_chains, device=self.device,
            Cstar=_dptr(keep["Cstar"]), N=_dptr(keep["N"]), W=_dptr(keep["W"]),
            weekday_c=_dptr(keep["wd"]), log_area_c=_dptr(keep["la"]), car_Q=_dptr(keep["Q"]),
            car_half_logdet=k.car_half_logdet, init_state=_dptr(init),
            nu=ms.NU, time_delta=ms.TIME_DELTA, rate_floor=ms.RATE_FLOOR)
        _lib.check(self._lib.seir_create(ctypes.byref(desc), ctypes.byref(self._ctx)))
        assert self._lib.seir_num_params(self._ctx) == self.P

    def set_initial_state(self, initial_state):
        """Replace S,E,I,R at the first day (seir_set_initial_state)."""
        init = np.ascontiguousarray(initial_state, dtype=np.float64)
        if init.shape != (self.M, 4):
            raise ValueError(f"initial_state must be [M,4]=({self.M},4), got {init.shape}")
        _lib.check(self._lib.seir_set_initial_state(self._ctx, _dptr(init)))
        self.initial_state = init

    # -- lifetime -----------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx:
            self._lib.seir_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- host-array entry points ---------------------------------------------
    def _batch(self, u, events):
        u = np.ascontiguousarray(u, dtype=np.float64)
        ev = np.ascontiguousarray(events, dtype=np.float64)
        single = u.ndim == 1
        if single:
            u, ev = u[None], ev[None]
        B = u.shape[0]
        if u.shape != (B, self.P):
            raise ValueError(f"u must be [B,{self.P}], got {u.shape}")
        if ev.shape != (B, self.M, self.T, 3):
            raise ValueError(f"events must be [B,{self.M},{self.T},3], got {ev.shape}")
        return u, ev, B, single

    def log_prob(self, u, events):
        """joint_log_prob(u, events) (inference.py:537-557); batched over a leading axis."""
        u, ev, B, single = self._batch(u, events)
        out = np.empty(B)
        _lib.check(self._lib.seir_log_prob(self._ctx, B, _dptr(u), _dptr(ev), _dptr(out)))
        return float(out[0]) if single else out

    def log_prob_grad(self, u, events):
        """Value and d/du (the reference differentiates joint_log_prob with TF autodiff)."""
        u, ev, B, single = self._batch(u, events)
        out, g = np.empty(B), np.empty((B, self.P))
        _lib.check(self._lib.seir_log_prob_grad(self._ctx, B, _dptr(u), _dptr(ev), _dptr(out), _dptr(g)))
        return (float(out[0]), g[0]) if single else (out, g)

    # -- device-tensor entry points (torch tensors on cuda:<device>, float64) --
    @staticmethod
    def _tptr(t, shape):
        import torch
        if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
            raise ValueError("expected a contiguous float64 CUDA tensor")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return ctypes.c_void_p(t.data_ptr())

    def _torch_ready(self):
        import torch
        torch.cuda.current_stream(self.device).synchronize()

    def log_prob_dev(self, u_t, events_t, logp_t, grad_t=None):
        """Asynchronous on the context stream; call sync() before reading outputs."""
        B = u_t.shape[0]
        self._torch_ready()
        _lib.check(self._lib.seir_log_prob_dev(
            self._ctx, B, self._tptr(u_t, (B, self.P)), self._tptr(events_t, (B, self.M, self.T, 3)),
            self._tptr(logp_t, (B,)), None if grad_t is None else self._tptr(grad_t, (B, self.P))))

    def prepare_events_dev(self, events_t):
        B = events_t.shape[0]
        self._torch_ready()
        _lib.check(self._lib.seir_prepare_events_dev(
            self._ctx, B, self._tptr(events_t, (B, self.M, self.T, 3))))

    def eval_prepared_dev(self, u_t, logp_t, grad_t=None):
        B = u_t.shape[0]
        _lib.check(self._lib.seir_eval_prepared_dev(
            self._ctx, B, self._tptr(u_t, (B, self.P)), self._tptr(logp_t, (B,)),
            None if grad_t is None else self._tptr(grad_t, (B, self.P))))

    def sync(self):
        _lib.check(self._lib.seir_sync(self._ctx))

    def set_option(self, debug_skew=None, xcd_affinity=None, gemm_f32=None, eval_form=None, rt_staging_kib=None,
                   generic_moves=None):
        """Launch options of the context (seir_set_option): the workgroup-timing test hook, the
        chain <-> XCD block mapping and the launch form of `log_prob_dev` ("fused" -- one launch for 8 or 16 chains where the GPU
        allows it, else three -- | "three-launch" | "four-launch"; none of
        them changes a result beyond summation order), and `gemm_f32`: the mobility contraction
        with fp32 operands on the fp32 matrix instruction (BASELINE config 5; ~1e-8 relative on the log-prob).
        `rt_staging_kib` (test hook): bound on the staging plane of a `ChainSampler.rt` batch, read by `reset_rt`.
        `generic_moves`: a sampler's event updates run the kernels that serve every m <= 4 (`_m4`) also where m <= 2 has
        instances of its own; same draws bit for bit (`ChainSampler.move_instance` tells which ones run)."""
        if generic_moves is not None:
            _lib.check(self._lib.seir_set_option(self._ctx, _lib.OPT_GENERIC_MOVES, int(bool(generic_moves))))
        if rt_staging_kib is not None:
            _lib.check(self._lib.seir_set_option(self._ctx, _lib.OPT_RT_STAGING_KIB, int(rt_staging_kib)))
        if eval_form is not None:
            form = {"fused": 0, "four-launch": 1, "three-launch": 2}[eval_form]
            _lib.check(self._lib.seir_set_option(self._ctx, _lib.OPT_EVAL_FORM, form))
        if gemm_f32 is not None:
            _lib.check(self._lib.seir_set_option(self._ctx, _lib.OPT_GEMM_F32, int(bool(gemm_f32))))
        if debug_skew is not None:
            _lib.check(self._lib.seir_set_option(self._ctx, _lib.OPT_DEBUG_SKEW, int(debug_skew)))
        if xcd_affinity is not None:
            _lib.check(self._lib.seir_set_option(self._ctx, _lib.OPT_XCD_AFFINITY, int(xcd_affinity)))

    # -- timing (HIP events on the context stream) ----------------------------
    def timer_start(self):
        _lib.check(self._lib.seir_timer_start(self._ctx))

    def timer_stop(self) -> float:
        ms_ = ctypes.c_float()
        _lib.check(self._lib.seir_timer_stop(self._ctx, ctypes.byref(ms_)))
        return float(ms_.value)

    KERNELS = {"scan": 0, "gemm": 1, "se_value": 2, "se_grad": 3, "finish": 4,
               "state": 5, "tiles_value": 6, "tiles_grad": 7, "finish_fused": 8}

    def time_kernel(self, which: str, B: int, iters: int = 50) -> float:
        """Mean launch duration (ms) of one kernel of the last evaluation."""
        ms_ = ctypes.c_float()
        _lib.check(self._lib.seir_time_kernel(self._ctx, self.KERNELS[which], B, iters, ctypes.byref(ms_)))
        return float(ms_.value)

    def selftest_math(self, x):
        """Device values of log(1-exp(-x)), 1/expm1(x), log Gamma(floor(x)+1) (csrc/device_math.h)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        L, inv, lf = np.empty_like(x), np.empty_like(x), np.empty_like(x)
        _lib.check(self._lib.seir_selftest_math(self._ctx, x.size, _dptr(x), _dptr(L), _dptr(inv), _dptr(lf)))
        return L, inv, lf

    def selftest_math_wide(self, x):
        """Device values of log(1-exp(-x)), 1/expm1(x) from the 8-term series (l1me_inv_wide)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        L, inv = np.empty_like(x), np.empty_like(x)
        _lib.check(self._lib.seir_selftest_math_wide(self._ctx, x.size, _dptr(x), _dptr(L), _dptr(inv)))
        return L, inv

    def selftest_fn(self, name, x, y=None):
        """One scalar function of csrc/device_math.h (a key of `_lib.SELFTEST_FN`) on each x[i] (and y[i]) as the kernels
        evaluate it: the values, or (values, second result) for a function that has two (include/seir_hip.h)."""
        op, two_in, two_out = _lib.SELFTEST_FN[name]
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        if two_in:
            y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
            if y.shape != x.shape:
                raise ValueError("x and y differ in length")
        out0 = np.empty_like(x)
        out1 = np.empty_like(x) if two_out else None
        _lib.check(self._lib.seir_selftest_fn(self._ctx, op, x.size, _dptr(x), _dptr(y) if two_in else None, _dptr(out0),
                                              _dptr(out1) if two_out else None))
        return (out0, out1) if two_out else out0

    def selftest_delta(self, which, S, I, K0, F, dF, ee, psiW, rate_floor, dt):
        """`band_delta` ("band") or the S->E piece of `own_rows_delta` ("own_ei", "own_se") per element
        (csrc/sampler_kernels.h; the arguments: include/seir_hip.h, seir_selftest_band_delta)."""
        arrs = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (S, I, K0, F, dF, ee, psiW)]
        n = arrs[0].size
        if any(a.size != n for a in arrs):
            raise ValueError("arguments differ in length")
        out = np.empty(n)
        _lib.check(self._lib.seir_selftest_band_delta(self._ctx, _lib.SELFTEST_DELTA[which], n, *[_dptr(a) for a in arrs],
                                                      float(rate_floor), float(dt), _dptr(out)))
        return out

    def selftest_wave(self, name, v):
        """A wave or block primitive of csrc/device_math.h (a key of `_lib.SELFTEST_WAVE`) fed v[block * 256 + tid] by
        256-thread blocks; v int32 or float64, a multiple of 256 long.  Returns (what each thread got back, the block total
        each thread was handed: zeros for the wave forms and block_sum_256)."""
        op, has_int = _lib.SELFTEST_WAVE[name]
        v = np.asarray(v)
        is_int = v.dtype == np.int32
        if not is_int:
            v = np.ascontiguousarray(v, dtype=np.float64)
        v = np.ascontiguousarray(v).reshape(-1)
        if v.size % 256 or (is_int and not has_int):
            raise ValueError("need whole 256-thread blocks, and int32 only where the primitive has that form")
        out, tot = np.empty_like(v), np.empty_like(v)
        _lib.check(self._lib.seir_selftest_wave(self._ctx, op, int(is_int), v.size // 256, v.ctypes.data, out.ctypes.data,
                                                tot.ctypes.data))
        return out, tot

    def within_between(self, psi, I_last, W):
        """(within, between) fractions [n,M] of the infection pressure of the last state
        (covid19uk/posterior/within_between.py:13-57).  psi [n], I_last [n,M], W scalar."""
        psi = np.ascontiguousarray(psi, dtype=np.float64).reshape(-1)
        I = np.ascontiguousarray(I_last, dtype=np.float64)
        n = psi.shape[0]
        if I.shape != (n, self.M):
            raise ValueError(f"need psi [n] and I_last [n,{self.M}]")
        wi, be = np.empty((n, self.M)), np.empty((n, self.M))
        _lib.check(self._lib.seir_within_between(self._ctx, n, _dptr(psi), _dptr(I), float(W), _dptr(wi), _dptr(be)))
        return wi, be

    def simulate(self, par, log_baseline, spatial, W, weekday_c, init_state, seed=0, first_draw_id=0):
        """Chain-binomial forward simulation of n draws (DiscreteTimeStateTransitionModel.sample as
        used by covid19uk/posterior/predict.py:50-70): events [n,M,S,3].

        par [n,5] = psi, sigma_space, beta_area, gamma0, gamma1; log_baseline [n,S] = a_t of each
        simulated day; spatial [n,M]; W, weekday_c [S]; init_state [n,M,4]."""
        par = np.ascontiguousarray(par, dtype=np.float64)
        ap = np.ascontiguousarray(log_baseline, dtype=np.float64)
        sp = np.ascontiguousarray(spatial, dtype=np.float64)
        W = np.ascontiguousarray(W, dtype=np.float64)
        wd = np.ascontiguousarray(weekday_c, dtype=np.float64)
        init = np.ascontiguousarray(init_state, dtype=np.float64)
        n = par.shape[0]
        S = ap.shape[1] if ap.ndim == 2 else -1
        if par.shape != (n, 5) or ap.shape != (n, S) or sp.shape != (n, self.M) or W.shape != (S,) \
                or wd.shape != (S,) or init.shape != (n, self.M, 4):
            raise ValueError(f"need par [n,5], log_baseline [n,S], spatial [n,{self.M}], W [S], weekday_c [S], "
                             f"init_state [n,{self.M},4]")
        out = np.empty((n, self.M, S, 3))
        desc = _lib.SeirSimDesc(num_draws=n, num_steps=S, first_draw_id=int(first_draw_id), reserved=0,
                                seed=int(seed) & 0xFFFFFFFFFFFFFFFF, par=_dptr(par), log_baseline=_dptr(ap),
                                spatial=_dptr(sp), W=_dptr(W), weekday_c=_dptr(wd), init_state=_dptr(init),
                                events=_dptr(out))
        _lib.check(self._lib.seir_simulate(self._ctx, ctypes.byref(desc)))
        return out

    def selftest_binomial(self, n, p, seed=0):
        """Device Binomial(n_i, p_i) variates from the simulator's sampler (csrc/sim_kernels.h)."""
        n = np.ascontiguousarray(n, dtype=np.int32)
        p = np.ascontiguousarray(p, dtype=np.float64)
        out = np.empty(n.size, dtype=np.int32)
        ip = ctypes.POINTER(ctypes.c_int32)
        _lib.check(self._lib.seir_selftest_binomial(self._ctx, n.size, n.ctypes.data_as(ip), _dptr(p),
                                                    int(seed) & 0xFFFFFFFFFFFFFFFF, out.ctypes.data_as(ip)))
        return out

    def order_stats(self, values, ranks, cells=1, segs=1, seg_len=None, seg_stride=None, cell_stride=None):
        """Exact order statistics on the device (csrc/order_stats_kernels.h; include/seir_hip.h, seir_order_stats):
        `values` is a flat int32 array holding `cells` cells, cell c starting at c x cell_stride, each of `segs` runs of
        seg_len contiguous values seg_stride apart.  Returns int32 [R, cells]: np.sort(cell)[ranks]."""
        v = np.ascontiguousarray(values, dtype=np.int32).reshape(-1)
        ranks = np.ascontiguousarray(ranks, dtype=np.int64).reshape(-1)
        cells, segs = int(cells), int(segs)
        if seg_len is None:
            seg_len = v.size // max(cells * segs, 1)
        seg_stride = int(seg_len) if seg_stride is None else int(seg_stride)
        cell_stride = segs * seg_stride if cell_stride is None else int(cell_stride)
        extent = (cells - 1) * cell_stride + (segs - 1) * seg_stride + int(seg_len)
        if cells < 1 or segs < 1 or int(seg_len) < 1 or min(seg_stride, cell_stride) < 0 or extent > v.size:
            raise ValueError(f"{cells} cell(s) of {segs} x {seg_len} values at strides {seg_stride}, {cell_stride} do not "
                             f"lie within the {v.size} values given")
        out = np.empty((len(ranks), cells), dtype=np.int32)
        ip = ctypes.POINTER(ctypes.c_int32)
        _lib.check(self._lib.seir_order_stats(self._ctx, v.ctypes.data_as(ip), cells, segs, int(seg_len), seg_stride,
                                              cell_stride, ranks.ctypes.data_as(_lib.c_int64_p), len(ranks),
                                              out.ctypes.data_as(ip)))
        return out

    def pair_abs_sums(self, values, cells=1, segs=1, seg_len=None, seg_stride=None, cell_stride=None):
        """The sum of pairwise absolute differences of every cell on the device (csrc/verify_kernels.h, k_pair_abs;
        include/seir_hip.h, seir_pair_abs_sums): the cell geometry of `order_stats`.  Returns int64 [cells], equal to
        `posterior.verify.pair_sum` of each cell; the library refuses more than `_lib.PAIR_ABS_MAX_N` values per cell."""
        v = np.ascontiguousarray(values, dtype=np.int32).reshape(-1)
        cells, segs = int(cells), int(segs)
        if seg_len is None:
            seg_len = v.size // max(cells * segs, 1)
        seg_stride = int(seg_len) if seg_stride is None else int(seg_stride)
        cell_stride = segs * seg_stride if cell_stride is None else int(cell_stride)
        extent = (cells - 1) * cell_stride + (segs - 1) * seg_stride + int(seg_len)
        if cells < 1 or segs < 1 or int(seg_len) < 1 or min(seg_stride, cell_stride) < 0 or extent > v.size:
            raise ValueError(f"{cells} cell(s) of {segs} x {seg_len} values at strides {seg_stride}, {cell_stride} do not "
                             f"lie within the {v.size} values given")
        out = np.empty(cells, dtype=np.int64)
        flag = ctypes.c_uint32(0)
        _lib.check(self._lib.seir_pair_abs_sums(self._ctx, v.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), cells, segs,
                                                int(seg_len), seg_stride, cell_stride, out.ctypes.data_as(_lib.c_int64_p),
                                                ctypes.byref(flag)))
        return out

    def group_sums(self, events, offsets, members):
        """Sums over groups of locations on the device (csrc/group_kernels.h; include/seir_hip.h, seir_group_sums): `events`
        int32 [n, M, L, 3] (M and L the array's own), the groups a CSR pair (`offsets` [G+1], `members` [nnz], ascending and
        unique within a group).  Returns int64 [n, G, L, 3]: events[:, members(g)].sum(1)."""
        ev = np.ascontiguousarray(events, dtype=np.int32)
        if ev.ndim != 4 or ev.shape[3] != 3:
            raise ValueError(f"events {ev.shape}: need [n, M, L, 3]")
        off = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
        mem = np.ascontiguousarray(members, dtype=np.int32).reshape(-1)
        G = off.size - 1
        if G >= 1 and mem.size < int(off.max()):            # what the library cannot check: it reads members up to the offsets
            raise ValueError(f"offsets reach {int(off.max())}, members holds {mem.size}")
        n, M, L, _ = ev.shape
        out = np.empty((n, max(G, 0), L, 3), dtype=np.int64)
        ip = ctypes.POINTER(ctypes.c_int32)
        mem_arg = mem if mem.size else np.zeros(1, np.int32)
        _lib.check(self._lib.seir_group_sums(self._ctx, ev.ctypes.data_as(ip), n, M, L, G, off.ctypes.data_as(ip),
                                             mem_arg.ctypes.data_as(ip), out.ctypes.data_as(_lib.c_int64_p)))
        return out

    def scenario_diffs(self, base_events, scenario_events, acc=None):
        """The fold of a scenario's paired differences on the device (csrc/scenario_kernels.h; include/seir_hip.h,
        seir_scenario_diffs): `base_events` and `scenario_events` int32 [n, B, M, H, 3], the simulated counts of n draws per
        chain of the baseline and of the scenario (B, M and H the arrays' own).  `acc`: what an earlier call returned, to fold
        these draws behind its own, or None.  Returns a dict: `count` (draws per chain folded), `ref` int32, `sum` int64, `sumsq`
        uint64, `lt`, `eq` uint32, each [B, M, H, 4] (cases, cum_cases, prevalence, cum_infections), and `overflow` -- the
        integers of `posterior.scenarios.fold_differences`."""
        fev = np.ascontiguousarray(base_events, dtype=np.int32)
        sev = np.ascontiguousarray(scenario_events, dtype=np.int32)
        if fev.ndim != 5 or fev.shape[4] != 3 or sev.shape != fev.shape:
            raise ValueError(f"events {fev.shape} and {sev.shape}: need two of [n, B, M, H, 3]")
        n, B, M, H, _ = fev.shape
        shape = (B, M, H, 4)
        if acc is None:
            folded = 0
            out = dict(ref=np.zeros(shape, np.int32), sum=np.zeros(shape, np.int64), sumsq=np.zeros(shape, np.uint64),
                       lt=np.zeros(shape, np.uint32), eq=np.zeros(shape, np.uint32))
            ovf = np.zeros(1, np.uint32)
        else:
            folded = int(acc["count"])
            out = {}
            for key, ty in (("ref", np.int32), ("sum", np.int64), ("sumsq", np.uint64), ("lt", np.uint32), ("eq", np.uint32)):
                out[key] = np.array(acc[key], dtype=ty, order="C")
                if out[key].shape != shape:
                    raise ValueError(f"acc[{key!r}] {out[key].shape}: these events need {shape}")
            ovf = np.array([1 if acc["overflow"] else 0], np.uint32)
        ip, up = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32)
        _lib.check(self._lib.seir_scenario_diffs(
            self._ctx, fev.ctypes.data_as(ip), sev.ctypes.data_as(ip), n, B, M, H, folded, out["ref"].ctypes.data_as(ip),
            out["sum"].ctypes.data_as(_lib.c_int64_p), out["sumsq"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            out["lt"].ctypes.data_as(up), out["eq"].ctypes.data_as(up), ovf.ctypes.data_as(up)))
        out["count"] = folded + n
        out["overflow"] = bool(ovf[0])
        return out

    def trigger_counts(self, masks, H, acc=None):
        """The fold of a triggered scenario's record on the device (csrc/scenario_trigger_kernels.h; include/seir_hip.h,
        seir_trigger_counts): `masks` uint64 [n, B, M, 2], bit s of a cell's 128 set iff the location is under the measure on
        day s in that draw; `H` the days counted.  `acc`: what an earlier call returned, to fold these draws behind its own, or
        None.  Returns a dict: `count` (draws per chain folded), `active_count` uint32 [B, M, H] and `active_by_day` int32
        [n, B, H] of this call's draws -- the integers of `posterior.scenarios.fold_triggers`."""
        mk = np.ascontiguousarray(masks, dtype=np.uint64)
        if mk.ndim != 4 or mk.shape[3] != 2:
            raise ValueError(f"masks {mk.shape}: need [n, B, M, 2]")
        n, B, M, _ = mk.shape
        H = int(H)
        if acc is None:
            folded, cnt = 0, np.zeros((B, M, max(H, 0)), np.uint32)
        else:
            folded, cnt = int(acc["count"]), np.array(acc["active_count"], dtype=np.uint32, order="C")
            if cnt.shape != (B, M, H):
                raise ValueError(f"acc['active_count'] {cnt.shape}: these masks need {(B, M, H)}")
        by_day = np.zeros((n, B, max(H, 0)), np.int32)
        _lib.check(self._lib.seir_trigger_counts(
            self._ctx, mk.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n, B, M, H, folded,
            cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), by_day.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return dict(count=folded + n, active_count=cnt, active_by_day=by_day)

    def group_wsums(self, v, offsets, members, weights=None):
        """Group sums of fp64 values on the device (csrc/group_curve_kernels.h; include/seir_hip.h, seir_group_wsums): `v`
        float64 [nd, L, M] (L and M the array's own), the groups a CSR pair as for `group_sums`, `weights` [nnz] aligned with
        `members` or None.  Returns float64 [nd, G, L]: the bits of `posterior.groups.weighted_sum_rows`."""
        x = np.ascontiguousarray(v, dtype=np.float64)
        if x.ndim != 3:
            raise ValueError(f"v {x.shape}: need [nd, L, M]")
        off = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
        mem = np.ascontiguousarray(members, dtype=np.int32).reshape(-1)
        G = off.size - 1
        if G >= 1 and mem.size < int(off.max()):            # what the library cannot check: it reads members up to the offsets
            raise ValueError(f"offsets reach {int(off.max())}, members holds {mem.size}")
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
            if w.size != mem.size:
                raise ValueError(f"weights [{w.size}] are not aligned with members [{mem.size}]")
        nd, L, M = x.shape
        out = np.empty((nd, max(G, 0), L), dtype=np.float64)
        ip = ctypes.POINTER(ctypes.c_int32)
        mem_arg = mem if mem.size else np.zeros(1, np.int32)
        _lib.check(self._lib.seir_group_wsums(self._ctx, x.ctypes.data_as(_lib.c_double_p), nd, L, M, G, off.ctypes.data_as(ip),
                                              mem_arg.ctypes.data_as(ip),
                                              None if w is None or not w.size else w.ctypes.data_as(_lib.c_double_p),
                                              out.ctypes.data_as(_lib.c_double_p)))
        return out

    def group_ngm_rows(self, theta, events, offsets, members, days=None):
        """The rows plane of the group next-generation matrix on the device (csrc/ngm_kernels.h; include/seir_hip.h,
        seir_group_ngm_rows): `theta` [n, P] constrained draws, `events` integer [n, M, T, 3] (the trace layout with one chain),
        the groups a CSR pair as for `group_sums`, `days` the window [T - days, T) (None: all T days).  Returns float64
        [n, G, days, M]: P[g][t][j], the expected infections in group g caused by one infective of location j on day t -- the
        bits of `posterior.groups.ngm_rows`; `posterior.groups.group_ngm` makes K of it."""
        th = np.ascontiguousarray(theta, dtype=np.float64)
        ev = np.ascontiguousarray(events)
        n = th.shape[0]
        if th.shape != (n, self.P) or ev.shape != (n, self.M, self.T, 3):
            raise ValueError(f"need theta [n,{self.P}] and events [n,{self.M},{self.T},3]")
        if ev.dtype.kind not in "iu":
            raise TypeError("events: integer counts (the trace layout), not " + str(ev.dtype))
        ev = np.ascontiguousarray(ev, dtype=np.int32)
        off = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
        mem = np.ascontiguousarray(members, dtype=np.int32).reshape(-1)
        G = off.size - 1
        if G >= 1 and mem.size < int(off.max()):            # what the library cannot check: it reads members up to the offsets
            raise ValueError(f"offsets reach {int(off.max())}, members holds {mem.size}")
        D = self.T if days is None else int(days)
        out = np.empty((n, max(G, 0), max(D, 0), self.M), dtype=np.float64)
        ip = ctypes.POINTER(ctypes.c_int32)
        mem_arg = mem if mem.size else np.zeros(1, np.int32)
        _lib.check(self._lib.seir_group_ngm_rows(self._ctx, n, _dptr(th), ev.ctypes.data_as(ip), D, G, off.ctypes.data_as(ip),
                                                 mem_arg.ctypes.data_as(ip), _dptr(out)))
        return out

    def order_stats_f64(self, values, ranks, cells=1, segs=1, seg_len=None, seg_stride=None, cell_stride=None):
        """`order_stats` for float64 (csrc/order_stats_kernels.h; include/seir_hip.h, seir_order_stats_f64): the same
        cell geometry, the order of IEEE-754 totalOrder on the bit patterns (np.sort's on values without NaN, except that
        -0.0 comes before +0.0).  Returns float64 [R, cells]."""
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        ranks = np.ascontiguousarray(ranks, dtype=np.int64).reshape(-1)
        cells, segs = int(cells), int(segs)
        if seg_len is None:
            seg_len = v.size // max(cells * segs, 1)
        seg_stride = int(seg_len) if seg_stride is None else int(seg_stride)
        cell_stride = segs * seg_stride if cell_stride is None else int(cell_stride)
        extent = (cells - 1) * cell_stride + (segs - 1) * seg_stride + int(seg_len)
        if cells < 1 or segs < 1 or int(seg_len) < 1 or min(seg_stride, cell_stride) < 0 or extent > v.size:
            raise ValueError(f"{cells} cell(s) of {segs} x {seg_len} values at strides {seg_stride}, {cell_stride} do not "
                             f"lie within the {v.size} values given")
        out = np.empty((len(ranks), cells), dtype=np.float64)
        _lib.check(self._lib.seir_order_stats_f64(self._ctx, _dptr(v), cells, segs, int(seg_len), seg_stride, cell_stride,
                                                  ranks.ctypes.data_as(_lib.c_int64_p), len(ranks), _dptr(out)))
        return out

    def reproduction_number(self, theta, events):
        """R_it [n,T,M] for n posterior draws: column sums of the next-generation matrix
        (covid19uk/posterior/reproduction_number.py:13-44, model_spec.py:302-368).
        theta [n,P] constrained draws, events [n,M,T,3]."""
        th = np.ascontiguousarray(theta, dtype=np.float64)
        ev = np.ascontiguousarray(events, dtype=np.float64)
        n = th.shape[0]
        if th.shape != (n, self.P) or ev.shape != (n, self.M, self.T, 3):
            raise ValueError(f"need theta [n,{self.P}] and events [n,{self.M},{self.T},3]")
        out = np.empty((n, self.T, self.M))
        _lib.check(self._lib.seir_reproduction_number(self._ctx, n, _dptr(th), _dptr(ev), _dptr(out)))
        return out

#!/usr/bin/env python3
"""Developer probe (GPU box): when every tile workgroup of the gradient kernel k_se starts and ends within a launch.
Build: bash tools/dev/build_variant.sh sest;  python tools/dev/se_timeline.py sest [chains]"""
import sys, numpy as np
import stamps
stamps.load_variant(sys.argv[1])
B = int(sys.argv[2]) if len(sys.argv) > 2 else 8
with stamps.probe_sampler(B, trace_capacity=10) as (model, s):
    s.run(2); model.sync()
    us = 1e3 * s.time_grad_kernel(50)
    ntile = 6 * 24
    raw = stamps.read(model, "se", n_words=B * ntile * 4)["tiles"].reshape(B, ntile, 4)
    t0 = (raw[..., 2] & np.uint64(0xffffffffffff)).astype(np.int64)
    t1 = (raw[..., 3] & np.uint64(0xffffffffffff)).astype(np.int64)
    xcc = (raw[..., 3] >> np.uint64(60)).astype(np.int64)
    cu = ((raw[..., 3] >> np.uint64(48)) & np.uint64(0xfff)).astype(np.int64)
    base = t0.min()
    st, en = (t0 - base) * 10, (t1 - base) * 10
    print(f"kernel {us:.2f} us by events; {B} chains x {ntile} tiles")
    print("start ns: min/median/p90/max", st.min(), int(np.median(st)), int(np.percentile(st, 90)), st.max())
    print("end   ns: min/median/p90/max", en.min(), int(np.median(en)), int(np.percentile(en, 90)), en.max())
    dur = en - st
    print("tile duration ns: min/median/p90/max", dur.min(), int(np.median(dur)), int(np.percentile(dur, 90)), dur.max())
    for b in range(min(B, 2)):
        order = np.argsort(st[b])
        print(f"chain {b}: xcc {sorted(set(xcc[b].tolist()))}, distinct CU ids {len(set(cu[b].tolist()))}; starts by order:",
              st[b][order][::12].tolist(), "ends:", en[b][order][::12].tolist())
    # workgroups per (xcc, cu)
    key = xcc * 4096 + cu
    uniq, cnt = np.unique(key, return_counts=True)
    print("workgroups per CU: ", dict(zip(*np.unique(cnt, return_counts=True))))

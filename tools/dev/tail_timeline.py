#!/usr/bin/env python3
"""Developer probe (GPU box): timeline of one k_se_chunk launch -- tiles, the hand-off, the chunk roles.
Build: bash tools/dev/build_variant.sh tailst;  python tools/dev/tail_timeline.py tailst [uk380|syn2048]"""
import sys, numpy as np
import stamps
stamps.load_variant(sys.argv[1])
wl = sys.argv[2] if len(sys.argv) > 2 else "uk380"
# (hmc="chunk-launch": the form whose inner steps are k_se_chunk launches -- the default plan runs them inside k_leap)
with stamps.probe_sampler(8, wl, step_size=1.2e-5 if wl == "uk380" else 2e-6, num_leapfrog_steps=3, hmc="chunk-launch") as (model, s):
    s.run(20); model.sync()
    rows = []
    for rep in range(5):
        stamps.read(s, "tail", reset=True)
        s.run(1); model.sync()
        st = stamps.read(s, "tail")["chains"].astype(np.int64)
        t0 = st[:, 0]
        rel = lambda k: (st[:, k] - t0) * 10
        rows.append(np.stack([rel(5), rel(1), rel(2), rel(3), rel(4)]))
    r = np.median(np.stack(rows), axis=0)
    print("ns after the chain's first tile started (median of 5 launches; min / median / max over the 8 chains)")
    for name, v in zip(["first role workgroup starts", "last tile has counted in", "first role past its wait",
                        "last role past its wait", "last role done (stores acknowledged)"], r):
        print(f"  {name:40s} {v.min():7.0f} {np.median(v):7.0f} {v.max():7.0f}")

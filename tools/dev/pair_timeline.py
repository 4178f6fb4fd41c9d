#!/usr/bin/env python3
"""Developer probe (GPU box): per-step timeline of the event-update launches from the stamps of chain 0's workgroups
(roles 1, 2, 0 in slots 0, 1, 2; band workgroups from slot 3) -- plain stores of s_memrealtime.
Build: bash tools/dev/build_variant.sh pairst
Run:   python tools/dev/pair_timeline.py pairst [paired|paired-launch]"""
import sys, numpy as np
import stamps
stamps.load_variant(sys.argv[1])
moves = sys.argv[2] if len(sys.argv) > 2 else "paired"
NR = int(sys.argv[3]) if len(sys.argv) > 3 else 3          # role slots of the launch (the early-draw experiment of round 4 had 4)
NS = NR + 24
with stamps.probe_sampler(8, moves=moves) as (model, s):
    s.run(20); model.sync()
    reps = []
    for rep in range(9):
        s.run(1); model.sync()
        reps.append(stamps.read(s, "pair")["steps"][:NS].astype(np.int64))
    st = np.stack(reps) * 10.0                             # [rep, slot, step, stamp] ns (100 MHz clock)
    R0 = NR - 1                                            # role 0 sits in the last role slot
    t0 = st[:, R0:R0 + 1, :, 0:1]                          # role 0's entry of the step
    rel = st - t0
    med = lambda a: np.median(a, axis=0)
    names = {0: "role 1", 1: "role 2", R0: "role 0", NR: "band 0", NR + 11: "band 11", NR + 23: "band 23"}
    if NR == 4:
        names[2] = "role 3"
    print(f"moves={moves}; ns after role 0 entered the step (median of 9 sweeps); stamps: 0 entry, roles: 6 entry loads issued, 12 back, 13 past the barrier, 14 uniforms drawn, 15 pending descriptors in LDS; 7 the band's words of the step before seen (their wait began at 6); 1..5 inside, 8 step done; roles: 10 drained, 11 the roles' barrier released, 9 L1 dropped; band: 10 partial sums published as words (F band applied), 9 own L1 dropped")
    for step in (0, 1, 4, 5, 8, 9):
        print(f"-- step {step}")
        for slot, name in names.items():
            row = med(rel[:, slot, step, :])
            print(f"   {name:8s} " + " ".join(f"{k}:{row[k]:.0f}" for k in (0, 4, 5, 7, 6, 12, 13, 14, 15, 1, 2, 3, 8, 10, 11, 9)))
    per = med(st[:, R0, 1:10, 0] - st[:, R0, 0:9, 0])
    print("step period (role 0 entry to entry):", per.round().tolist(), "mean %.0f ns" % per.mean())
    last = st[:, :, :10, 8].max(axis=1) - st[:, R0, :10, 0]
    who = st[:, :, :10, 8].argmax(axis=1)
    print("last workgroup done (ns after role 0's entry):", med(last).round().tolist())
    print("which slot is last (last sweep):", who[-1].tolist())
    roles = [0, 1, R0]
    print("roles' barrier: last role done -> released (ns):", med(st[:, roles, :10, 11].max(axis=1) - st[:, roles, :10, 8].max(axis=1)).round().tolist())
    if (st[:, R0, 1:10, 7] > 0).all():
        print("role 0: entry -> band's words of the step before seen (ns):", med(st[:, R0, 1:10, 7] - st[:, R0, 1:10, 0]).round().tolist())
        print("last band workgroup published -> role 0 entered the next step (ns; > 0: the words were waiting):",
              med(st[:, R0, 1:10, 0] - st[:, NR:, 0:9, 10].max(axis=1)).round().tolist())

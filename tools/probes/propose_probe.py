"""Developer probe (GPU box): phases of a speculative role's event-time-move proposal inside k_move_pair.
Build: bash tools/dev/build_variant.sh propst [-DSEIR_STAMP_SLOT=<1|3> -DSEIR_STAMP_ROLE=<1|2>];  python tools/probes/propose_probe.py propst"""
import os, sys, numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dev"))
import stamps
stamps.load_variant(sys.argv[1])
R = stamps.SW_ROLE_PROPOSE                                   # the role's own four phases; 4..9 are its mv_propose's
with stamps.probe_sampler(8, trace_capacity=10) as (model, s):
    s.reset_trace(); s.run(3); model.sync()
    st = stamps.read(s, "seir")["words"].astype(np.int64)
    d = lambda a, b: (st[b] - st[a]) * 10
    print("role: entry+pending", d(R, R + 1), "| tables", d(R + 1, 4), "| select rows", d(4, 5), "| stage rows", d(5, 6),
          "| select days", d(6, 7), "| bounds (mins)", d(7, 8), "| finish lanes", d(8, 9), "| compact+store", d(9, R + 2),
          "| own rows", d(R + 2, R + 3), "ns; total", d(R, R + 3))

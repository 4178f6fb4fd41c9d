"""Developer probe (GPU box): phases of the HMC stage kernel (NSCAN=0) or of an event update's kernels (NSCAN=5) of chain 0.
Build: bash tools/dev/build_variant.sh seirst [-DSEIR_STAMP_SLOT=<1|3> -DSEIR_STAMP_ROLE=<1|2> -DSEIR_STAMP_BLOCK=<n>]
Run:   NSCAN=5 python tools/probes/stamp_probe.py seirst   (STAMP_SLOT / STAMP_ROLE / STAMP_BLOCK: the labels to print)"""
import os, sys, numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dev"))
import stamps
from stamps import SW_ROLE as R, SW_DELTA as D
stamps.load_variant(sys.argv[1])
cfg = dict(num_event_time_updates=int(os.environ.get("NSCAN", "0")))
# (NSCAN=0 stamps k_hmc_step<SEIR_STAMP_STAGE>: hmc="chunk-stage" is the form that still closes a trajectory with that launch)
form = dict(hmc="chunk-stage") if cfg["num_event_time_updates"] == 0 else {}
with stamps.probe_sampler(8, trace_capacity=10, cfg=cfg, **form) as (model, s):
    s.reset_trace(); s.run(3); model.sync()
    st = stamps.read(s, "seir")["words"].astype(np.int64)
    if cfg["num_event_time_updates"] == 0:
        print("stamps (10ns ticks) deltas:", np.diff(st[:10]) * 10, "ns ; total", (st[9] - st[0]) * 10, "ns")
        print("phase 0 split: kernarg+scalars+L/Ppart", (st[10] - st[0]) * 10, "Kpart+T vectors", (st[11] - st[10]) * 10,
              "Rpart+M vectors", (st[12] - st[11]) * 10, "barrier", (st[1] - st[12]) * 10, "ns")
    else:
        print("k_move_pair block 0 (se slot", int(os.environ.get("STAMP_SLOT", "1")) & 2, "): entry+finalize", (st[1]-st[0])*10, "se tables", (st[2]-st[1])*10,
              "se propose", (st[3]-st[2])*10, "se delta", (st[4]-st[3])*10, "se accept/apply/trace", (st[5]-st[4])*10,
              "nx tables", (st[6]-st[5])*10, "nx propose+store", (st[7]-st[6])*10, "ns; total", (st[7]-st[0])*10)
        print("   speculative role", os.environ.get("STAMP_ROLE", "1"), ": entry+pending", (st[R+1]-st[R])*10, "tables+propose", (st[R+2]-st[R+1])*10,
              "store+own-rows", (st[R+3]-st[R+2])*10, "ns; total", (st[R+3]-st[R])*10)
        print("k_move_delta block", os.environ.get("STAMP_BLOCK", "0"), ": mv+ltab", (st[D+1]-st[D])*10, "band", (st[D+2]-st[D+1])*10,
              "own rows", (st[D+3]-st[D+2])*10, "ns")
    tr = s.read_trace(3, events=False)
    print("accepts", {k: v["is_accepted"][-1].astype(int).tolist() for k, v in tr.moves.items()})

"""Phase split of rq_merge_flat on C3 (diagnostic -DRQ_PHASE_CLOCK build loaded through
RQ_SO_PATH): s_memtime sums of thread 0 of every block.  RQ_FLAT_SLICES=0 gives the search
loop's split, the default the slice table's."""
import ctypes as C
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: F401
from redqueen_amd import _lib as L, engine, graphs
so = graphs.c3()
g = engine.Graph(so["src_id"], so["other_sources"], so["sink_ids"], so["edge_list"], so["end_time"])
lib = L.lib()
lib.rq_phase_clock.argtypes = [C.POINTER(C.c_ulonglong)]
os.environ["RQ_CLK_MERGE"] = "1"
R = 10000
names = {7: "pre-pass", 0: "run search", 1: "pre / sbase + barriers", 2: "item loads", 3: "hist + scan + scatter",
         6: "rank + write"}
for k in range(2):
    g.run("opt", q=so["q"], s=so["s"], n_rep=R, ctrl_seed=0, world_seed=0, randomize=True, check=False)
    torch.cuda.synchronize()
    out = (C.c_ulonglong * 8)()
    rc = lib.rq_phase_clock(out)
    tot = sum(out[q] for q in names)
    print(rc, "slices", os.environ.get("RQ_FLAT_SLICES", "default"),
          {n: round(out[q] / max(tot, 1), 3) for q, n in names.items()},
          "ticks/replica %.0f windows/replica %.2f retried/replica %.2f on the search loop %.4f" %
          (tot / R, out[4] / R, (out[5] & 0xFFFFFFFF) / R, (out[5] >> 32) / R), flush=True)

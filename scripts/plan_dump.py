"""Print the plan of a fixed list of (graph, batch) cases: the nine rq_plan_info_n values,
rq_workspace_size and rq_event_capacity, all at one fixed ws_budget, one line per case.

Two builds plan alike when their outputs are identical; run each in its own process:

    RQ_SO_PATH=/path/to/other/librq.so python scripts/plan_dump.py > a.txt
    python scripts/plan_dump.py > b.txt && cmp a.txt b.txt

The cases: every row of the tests/test_gpu_graphs.py instance table, C3, C4 and c5_small
from redqueen_amd/graphs.py, OptPWSignificance with 4 segments, and C3 under a budget small
enough to shrink its chunks.  Needs the GPU (the plan asks the runtime for occupancy).
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from redqueen_amd import _lib as L, engine, graphs  # noqa: E402
from tests import test_gpu_graphs as T  # noqa: E402

BUDGET = 8 << 30
_extra = {}


def _hook(lib):
    """rq_plan_info_n, and with the same (graph, batch): workspace size and event capacity."""
    inner = lib.rq_plan_info_n

    def plan_info_n(h, bref, info, n):
        rc = inner(h, bref, info, n)
        nbytes, cap = C.c_size_t(), C.c_int64()
        _extra["ws"] = (lib.rq_workspace_size(h, bref, C.byref(nbytes)), nbytes.value)
        _extra["ev"] = (lib.rq_event_capacity(h, bref, C.byref(cap)), cap.value)
        return rc
    lib.rq_plan_info_n = plan_info_n


def dump(name, so, ctrl="opt", budget=BUDGET, **kw):
    g = T._graph(engine, so)
    g._ws_budget = lambda *a, **k: budget
    try:
        plan = g.run(ctrl, plan_only=True, **kw)
        vals = " ".join(str(v) for v in plan.values())
    except L.RQError as e:
        vals = "error %d" % e.code
    print("%-58s %s | ws %s | evcap %s" % (name, vals, _extra.get("ws"), _extra.get("ev")))
    sys.stdout.flush()


def main():
    _hook(L.lib())
    rows = next(m for m in T.test_50k_sinks.pytestmark if m.name == "parametrize").args[1]
    for i, (Ks, kw, _) in enumerate(rows):
        kw = dict(kw)
        gk = kw.pop("graph", {})
        kw.pop("plan", None)
        so = T._wide(**gk)
        dump("wide[%02d] %s Ks=%s %s" % (i, gk, Ks, kw), so, q=so["q"], s=so["s"], n_rep=6, Ks=Ks, **kw)
    c3 = graphs.c3()
    for Ks in ((1,), (1, 2, 5)):
        dump("c3 n_rep=10000 Ks=%s" % (Ks,), c3, q=c3["q"], s=c3["s"], n_rep=10000, Ks=Ks)
    dump("c3 n_rep=10000 event_log", c3, q=c3["q"], s=c3["s"], n_rep=10000, event_log=True)
    dump("c3 n_rep=10000 budget=64MiB", c3, budget=64 << 20, q=c3["q"], s=c3["s"], n_rep=10000)
    rd = graphs.readme()
    grid = graphs.c4_grid()
    dump("c4 256 grid points x 1000", rd, q=np.array([q for q, _ in grid]),
         s=np.array([s for _, s in grid], dtype=np.float64), n_rep=1000, seed_mod=1000)
    c5s = graphs.c5_small()
    dump("c5_small n_rep=10000", c5s, q=c5s["q"], s=c5s["s"], n_rep=10000)
    for nm, so in (("readme", rd), ("c3", c3)):
        gtmp = T._graph(engine, so)
        spw = np.tile(np.array([1.0, 0.5, 2.0, 1.5]), (gtmp.n_followers, 1))
        dump("optpw 4 segments %s" % nm, so, ctrl="sig", q=1.0, s_pw=spw, period=so["end_time"],
             n_rep=1000, Ks=(1, 2))


if __name__ == "__main__":
    main()

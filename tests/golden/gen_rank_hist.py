#!/usr/bin/env python
"""Generate tests/golden/rank_hist.npz from the REFERENCE (build container only; the
reference never travels to the GPU box):

    MPLBACKEND=Agg python tests/golden/gen_rank_hist.py

The four reference runs of gen_timeline.py (MPI-SWS/RedQueen imported as it does; the
same worlds, seeds and two edge sets each; the event lists are asserted equal to
timeline.npz's).  Per run the fixture holds the world (sink ids, edge list, controlled
id, other source ids, end_time), the event list (t, src_id) of the reference's
dataframe, S (the pivot's columns), the number of pivot rows and the table's maximum
(``<run>_rows`` = [rows, S, max rank]), the two edge sets (``<run>_bins<k>``) and, for
n_ranks in RANKS = 1, 3, 64, 255, ``<run>_hist<k>_<n_ranks>`` [n_bins][n_ranks + 1]:
the reference's OWN rank_of_src_in_df table through tests/rank_hist_ref.bin_table --
per bin and rank cell the exactly rounded (math.fsum) sum of count(row == rho) x
overlap, the last cell counting row >= n_ranks, divided by S.

  readme_opt    README world, create_manager_with_opt(seed=101)
  readme_pois   README world, create_manager_with_poisson(seed=7, capacity=400)
  rd_ties       an all-RealData world: two wall sources post at one time on disjoint
                sinks, and the controlled source posts at a wall source's time on
                disjoint sinks
  late_sink     a sink whose only source first posts after the second bin

Asserted here: the tail is positive at n_ranks 1 and 3 in every run; it is exactly 0 at
n_ranks 255 in every run whose table stays below 255 (rd_ties, late_sink).  In the README
world sink 2 follows source 2 only -- the controlled source has no edge to it -- so its
rank counts source 2's ~1000 posts whatever the seed: the two README runs instead pin a
positive tail at 255 under a maximum rank far above it.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "_shim"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
warnings.filterwarnings("ignore")
os.environ.setdefault("MPLBACKEND", "Agg")

from redqueen.opt_model import SimOpts  # noqa: E402
import redqueen.utils as U  # noqa: E402
import rank_hist_ref as RH  # noqa: E402
from gen_timeline import LATE, RD_TIES, RD_TIES_OWN, README  # noqa: E402

RANKS = [1, 3, 64, 255]
SMALL = ("rd_ties", "late_sink")   # the runs whose ranks stay below 255


def record(rec, old, name, so_kw, manager):
    so = SimOpts(**so_kw)
    m = manager(so)
    m.run_dynamic()
    df = m.state.get_dataframe()
    ev = df.groupby("event_id", sort=True).first()
    T = float(so_kw["end_time"])
    rec[name + "_sinks"] = np.asarray(so_kw["sink_ids"], dtype=np.int64)
    rec[name + "_edges"] = np.asarray(so_kw["edge_list"], dtype=np.int64)
    rec[name + "_srcs"] = np.asarray([kw["src_id"] for _n, kw in so_kw["other_sources"]], dtype=np.int64)
    rec[name + "_world"] = np.asarray([so_kw["src_id"], T], dtype=np.float64)
    rec[name + "_t"] = ev.t.values.astype(np.float64)
    rec[name + "_src"] = ev.src_id.values.astype(np.int64)
    assert np.array_equal(rec[name + "_t"], old[name + "_t"]) and np.array_equal(rec[name + "_src"], old[name + "_src"])
    ranks = U.rank_of_src_in_df(df, so.src_id)
    top = int(np.nanmax(ranks.values))
    rec[name + "_rows"] = np.asarray([ranks.shape[0], ranks.shape[1], top], dtype=np.int64)
    assert (top < 255) == (name in SMALL), (name, top)
    for k in (0, 1):
        edges = old["%s_bins%d" % (name, k)]
        rec["%s_bins%d" % (name, k)] = edges
        for nr in RANKS:
            h = RH.bin_table(ranks.values, ranks.index.values, T, edges, nr)
            rec["%s_hist%d_%d" % (name, k, nr)] = h
            tail = h[:, nr].sum()
            if nr in (1, 3):
                assert tail > 0, (name, k, nr)
            if nr == 255:
                assert (h[:, nr] == 0.0).all() if name in SMALL else tail > 0, (name, k)


def main():
    old = np.load(os.path.join(HERE, "timeline.npz"))
    rec = {"ranks": np.asarray(RANKS, dtype=np.int32),
           "names": np.asarray(["readme_opt", "readme_pois", "rd_ties", "late_sink"])}
    record(rec, old, "readme_opt", README, lambda so: so.create_manager_with_opt(seed=101))
    record(rec, old, "readme_pois", README, lambda so: so.create_manager_with_poisson(seed=7, capacity=400))
    record(rec, old, "rd_ties", RD_TIES, lambda so: so.create_manager_with_times(RD_TIES_OWN))
    record(rec, old, "late_sink", LATE, lambda so: so.create_manager_with_opt(seed=3))
    out = os.path.join(HERE, "rank_hist.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

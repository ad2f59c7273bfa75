#!/usr/bin/env python
"""Generate tests/golden/timeline.npz from the REFERENCE (build container only; the
reference never travels to the GPU box):

    MPLBACKEND=Agg python tests/golden/gen_timeline.py

Four reference runs (MPI-SWS/RedQueen imported as gen_golden.py does).  Per run the
fixture holds the world (sink ids, edge list, controlled id, other source ids,
end_time), the event list (t, src_id) of the reference's dataframe, two edge sets, and
for each the per-bin values obtained by feeding the reference's OWN
rank_of_src_in_df table through tests/timeline_ref.bin_table, plus the per-bin post
counts of the reference's dataframe.

  readme_opt    README world, create_manager_with_opt(seed=101)
  readme_pois   README world, create_manager_with_poisson(seed=7, capacity=400)
  rd_ties       an all-RealData world: two wall sources post at one time on disjoint
                sinks, and the controlled source posts at a wall source's time on
                disjoint sinks
  late_sink     a sink whose only source first posts after the second bin
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "_shim"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
warnings.filterwarnings("ignore")
os.environ.setdefault("MPLBACKEND", "Agg")

from redqueen.opt_model import SimOpts  # noqa: E402
import redqueen.utils as U  # noqa: E402
import timeline_ref as TR  # noqa: E402

KS = [1, 2, 5]

README = dict(src_id=1, end_time=100.0, s={1: 1.0, 3: 1.0}, q=1.0, sink_ids=[1, 2, 3],
              other_sources=[("Poisson2", {"src_id": 2, "seed": 42, "rate": 10}),
                             ("Hawkes", {"src_id": 3, "seed": 43, "l_0": 10, "alpha": 1.0,
                                         "beta": 10.0})],
              edge_list=[(1, 1), (1, 3), (2, 1), (2, 2), (2, 3), (3, 3)])

RD_TIES = dict(src_id=1, end_time=20.0, s=1.0, q=1.0, sink_ids=[10, 11, 12, 13],
               other_sources=[("RealData", {"src_id": 2, "times": [1.0, 2.0, 4.5, 9.0, 9.0 + 2 ** -40, 15.0]}),
                              ("RealData", {"src_id": 3, "times": [0.5, 2.0, 7.0, 15.0, 19.5]}),
                              ("RealData", {"src_id": 4, "times": [3.5, 6.0, 12.25]})],
               edge_list=[(1, 10), (1, 12), (2, 10), (2, 11), (3, 12), (4, 13)])
RD_TIES_OWN = [3.5, 5.0, 12.25, 16.0]

LATE = dict(src_id=1, end_time=50.0, s=1.0, q=0.5, sink_ids=[1, 2],
            other_sources=[("Poisson2", {"src_id": 2, "seed": 5, "rate": 2.0}),
                           ("RealData", {"src_id": 3, "times": [31.0, 33.5, 47.0]})],
            edge_list=[(1, 1), (2, 1), (3, 2)])


def record(rec, name, so_kw, manager, inner):
    """One reference run; edge sets: 10 equal bins over the horizon, and inner(event
    times) -- uneven bins inside the horizon."""
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
    ranks = U.rank_of_src_in_df(df, so.src_id)
    rec[name + "_rows"] = np.asarray([ranks.shape[0], ranks.shape[1]], dtype=np.int64)
    edge_sets = [[T * k / 10 for k in range(10)] + [T], inner(ev.t.values)]
    for k, edges in enumerate(edge_sets):
        edges = np.asarray(edges, dtype=np.float64)
        assert np.all(np.diff(edges) > 0)
        rec["%s_bins%d" % (name, k)] = edges
        rec["%s_met%d" % (name, k)] = TR.bin_table(ranks.values, ranks.index.values, T, edges, KS)
        rec["%s_posts%d" % (name, k)] = TR.posts(df.t.values, df.src_id.values, so.src_id, edges,
                                                 event_id=df.event_id.values)
        rec["%s_wall%d" % (name, k)] = TR.wall_posts(df.t.values, df.src_id.values, df.sink_id.values,
                                                     so.src_id, edges, so_kw["sink_ids"])


def main():
    rec = {"Ks": np.asarray(KS, dtype=np.int32),
           "names": np.asarray(["readme_opt", "readme_pois", "rd_ties", "late_sink"])}
    # the inner sets are uneven and have one edge exactly on an event time
    record(rec, "readme_opt", README, lambda so: so.create_manager_with_opt(seed=101),
           lambda t: [3.0, 7.5, float(t[len(t) // 3]), 55.0, 55.5, 91.0])
    record(rec, "readme_pois", README,
           lambda so: so.create_manager_with_poisson(seed=7, capacity=400),
           lambda t: [0.25, float(t[200]), 20.0, 20.125, 64.0, 99.0])
    record(rec, "rd_ties", RD_TIES, lambda so: so.create_manager_with_times(RD_TIES_OWN),
           lambda t: [0.5, 2.0, 3.5, 9.0, 12.25, 19.0])
    record(rec, "late_sink", LATE, lambda so: so.create_manager_with_opt(seed=3),
           lambda t: [4.0, 30.0, 31.0, 33.0, 49.5])
    out = os.path.join(HERE, "timeline.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

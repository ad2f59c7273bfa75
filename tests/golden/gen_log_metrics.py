#!/usr/bin/env python
"""Generate tests/golden/log_metrics.npz from the REFERENCE (build container only; the
reference never travels to the GPU box):

    MPLBACKEND=Agg python tests/golden/gen_log_metrics.py

Reference runs (MPI-SWS/RedQueen imported as gen_golden.py does) of small worlds whose
dataframes have several rows per (t, sink).  Per world the fixture holds the world (sink
ids, edge list, controlled id, end_time), the event list (t, src_id) of the reference's
dataframe and the reference's OWN values: time_in_top_k for K = 1, 2, 3, average_rank,
int_r_2, num_tweets_of and the number of distinct event ids of the other sources.

  game5     5 Opts on 4 sinks (small_world(5) of tests/test_gpu_game.py,
            create_manager_for_wall): Opts 20, 23 and 24 tie three ways on sink 1 at start
  thirds    14 sinks, all RealData.  Sources 2, 3 (controlled) and 4 repeat one time on
            the shared sinks 101..109, which source 5 never touches: their cells are
            thirds over source 5's many rows.  Sink 100, the lowest id, is followed only
            by source 9, which has no event: it is no pivot column
  wide      140 seen sinks, thirds live on the first 100 while 40 others get rows
  places    tie groups with the controlled source's post first, in the middle and last
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
import log_metrics_ref as LR  # noqa: E402

KS = [1, 2, 3]


def rd(src_id, times):
    return ("RealData", {"src_id": src_id, "times": [float(x) for x in times]})


def game5():
    others = [("Poisson", {"src_id": 10, "seed": 1, "rate": 10.0}),
              ("Poisson2", {"src_id": 11, "seed": 2, "rate": 10.0}),
              ("Hawkes", {"src_id": 12, "seed": 3, "l_0": 2.0, "alpha": 1.0, "beta": 4.0})]
    edges = [(10, 1), (10, 2), (11, 3), (11, 2), (12, 3), (12, 4)]
    for k in range(5):
        others.append(("Opt", {"src_id": 20 + k, "seed": 100 + k, "q": 1.0, "s": [1.0, 0.5]}))
        edges += [(20 + k, 1 + k % 4), (20 + k, 1 + (k + 1) % 4)]
    return dict(src_id=1, q=1.0, s=[], end_time=10.0, sink_ids=[1, 2, 3, 4], other_sources=others,
                edge_list=edges)


def thirds():
    sinks = list(range(100, 114))
    shared = sinks[1:10]
    tie_t = [1.0, 6.0, 6.5, 11.0, 15.0]
    edges = [(9, 100)] + [(k, x) for k in (2, 3, 4) for x in shared] + [(5, x) for x in sinks[10:]]
    edges += [(6, x) for x in shared[1::2]] + [(7, x) for x in shared[2::3]] + [(7, 108)]
    five = [0.3 + 0.37 * k for k in range(50)]
    others = [rd(2, tie_t + [8.25]), rd(4, tie_t + [13.5]), rd(5, five), rd(6, [0.5, 5.0, 10.5]),
              rd(7, [0.75, 0.875, 5.5, 14.0]), rd(9, [])]
    return dict(src_id=3, q=1.0, s=1.0, end_time=20.0, sink_ids=sinks, other_sources=others,
                edge_list=edges), tie_t + [3.0]


def wide():
    sinks = list(range(1000, 1140))
    tied = sinks[:100]
    tie_t = [1.0, 4.0, 4.25, 7.0]
    edges = [(k, x) for k in (2, 3, 4) for x in tied] + [(5, x) for x in sinks[100:]]
    edges += [(6, x) for x in tied[::2]] + [(7, x) for x in tied[::3]]
    others = [rd(2, tie_t), rd(4, tie_t + [5.5]), rd(5, [0.2 + 0.31 * k for k in range(30)]),
              rd(6, [0.5, 3.0]), rd(7, [0.75, 0.8, 3.5, 6.0])]
    return dict(src_id=3, q=1.0, s=1.0, end_time=10.0, sink_ids=sinks, other_sources=others,
                edge_list=edges), tie_t


def places():
    sinks = [1, 2, 3]
    edges = [(k, x) for k in (2, 3, 4) for x in sinks]
    others = [rd(2, [0.5, 2.0, 3.0, 4.5]), rd(4, [1.0, 2.0, 3.75])]
    return dict(src_id=3, q=1.0, s=1.0, end_time=6.0, sink_ids=sinks, other_sources=others,
                edge_list=edges), [1.0, 2.0, 3.0, 5.0]


def record(rec, name, so_kw, manager):
    so = SimOpts(**so_kw)
    m = manager(so)
    m.run_dynamic()
    df = m.state.get_dataframe()
    ev = df.groupby("event_id", sort=True).first()
    assert len(set(so_kw["edge_list"])) == len(so_kw["edge_list"]), "no duplicate edges"
    rec[name + "_sinks"] = np.asarray(so_kw["sink_ids"], dtype=np.int64)
    rec[name + "_edges"] = np.asarray(so_kw["edge_list"], dtype=np.int64)
    rec[name + "_world"] = np.asarray([so_kw["src_id"], so_kw["end_time"]], dtype=np.float64)
    rec[name + "_t"] = ev.t.values.astype(np.float64)
    rec[name + "_src"] = ev.src_id.values.astype(np.int64)
    vals = [U.time_in_top_k(df=df, K=K, sim_opts=so) for K in KS]
    vals += [U.average_rank(df, sim_opts=so), U.int_r_2(df, so)]
    rec[name + "_metrics"] = np.asarray(vals, dtype=np.float64)
    other = int(df.event_id[df.src_id != so.src_id].nunique())
    rec[name + "_posts"] = np.asarray([int(U.num_tweets_of(df, sim_opts=so)), other], dtype=np.int64)
    # what the fixture is for, by the checker: ties, live fractions, and (thirds) a world on
    # which a zero column in front of the pivot columns changes the bits
    got = LR.play(rec[name + "_t"], rec[name + "_src"], so_kw["edge_list"], so_kw["src_id"],
                  so_kw["end_time"], KS)
    shifted = LR.play(rec[name + "_t"], rec[name + "_src"], so_kw["edge_list"], so_kw["src_id"],
                      so_kw["end_time"], KS, lead_zeros=1)
    print(name, "events", len(ev), "rows", got["counts"][2], "cols", got["counts"][3], "status", got["status"],
          "frac rows", got["frac_rows"], "dens", sorted(got["dens"]),
          "checker == reference:", LR.same_bits(got["metrics"], rec[name + "_metrics"]),
          "zero column changes bits:", not LR.same_bits(shifted["metrics"], got["metrics"]))
    return got, shifted


def main():
    rec = {"Ks": np.asarray(KS, dtype=np.int32), "names": np.asarray(["game5", "thirds", "wide", "places"])}
    record(rec, "game5", game5(), lambda so: so.create_manager_for_wall())
    for name, make in (("thirds", thirds), ("wide", wide), ("places", places)):
        kw, own = make()
        got, shifted = record(rec, name, kw, lambda so: so.create_manager_with_times(own))
        if name != "places":
            assert 3 in got["dens"] and got["frac_rows"] >= 20, name
        if name == "thirds":
            assert not LR.same_bits(shifted["metrics"], got["metrics"])
    out = os.path.join(HERE, "log_metrics.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

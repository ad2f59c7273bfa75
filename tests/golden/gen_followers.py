#!/usr/bin/env python
"""Generate tests/golden/followers.npz from the REFERENCE (build container only; the
reference never travels to the GPU box):

    MPLBACKEND=Agg python tests/golden/gen_followers.py

Six reference runs (MPI-SWS/RedQueen imported as gen_timeline.py does).  Per run the
fixture holds the world (sink ids, edge list, controlled id, other source ids, end_time,
q), the event list (t, src_id) of the reference's dataframe, and, for every sink column
of the reference's OWN rank_of_src_in_df table, the exactly rounded (math.fsum) sums of
f(r) * dt over the column's non-NaN rows (tests/followers_ref.column_sums), the column's
first non-NaN index and its own / wall row counts from the dataframe; plus what the
reference returns for int_r_2_true, calc_loss_opt and calc_loss_poisson (with an s vector
over all sinks and u_const = U_CONST; a world in which a sink never gets a row has no
losses: the reference raises KeyError there).

  readme_opt    README world, create_manager_with_opt(seed=101)
  readme_pois   README world, create_manager_with_poisson(seed=7, capacity=400)
  rd_ties       an all-RealData world: equal times on disjoint sinks
  late_sink     a sink whose only source first posts late
  wide          130 sinks: one wall source to all 130, one to 65, the controlled source
                to 129; a short horizon -- CSR rows of 1, 2 and 3 rounds, the last partial
  lonely        a sink nobody posts to
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
import followers_ref as FR  # noqa: E402
from gen_timeline import LATE, RD_TIES, RD_TIES_OWN, README  # noqa: E402

KS = [1, 2, 5]
U_CONST = 2.5

W_SINKS = list(range(2000, 2130))
WIDE = dict(src_id=1, end_time=4.0, s=1.0, q=50.0, sink_ids=W_SINKS,
            other_sources=[("Poisson2", {"src_id": 2, "seed": 11, "rate": 6.0}),
                           ("Poisson2", {"src_id": 3, "seed": 12, "rate": 9.0})],
            edge_list=[(2, x) for x in W_SINKS] + [(3, x) for x in W_SINKS[40:105]] +
                      [(1, x) for x in W_SINKS[1:]])

LONELY = dict(src_id=1, end_time=30.0, s=1.0, q=2.0, sink_ids=[5, 6, 7, 8],
              other_sources=[("Poisson2", {"src_id": 2, "seed": 21, "rate": 1.5}),
                             ("Hawkes", {"src_id": 3, "seed": 22, "l_0": 1.0, "alpha": 1.0, "beta": 4.0})],
              edge_list=[(1, 5), (1, 8), (2, 5), (2, 6), (3, 8)])


def record(rec, name, so_kw, manager):
    so = SimOpts(**so_kw)
    m = manager(so)
    m.run_dynamic()
    df = m.state.get_dataframe()
    ev = df.groupby("event_id", sort=True).first()
    T = float(so_kw["end_time"])
    sinks = sorted(so_kw["sink_ids"])
    rec[name + "_sinks"] = np.asarray(so_kw["sink_ids"], dtype=np.int64)
    rec[name + "_edges"] = np.asarray(so_kw["edge_list"], dtype=np.int64)
    rec[name + "_srcs"] = np.asarray([kw["src_id"] for _n, kw in so_kw["other_sources"]], dtype=np.int64)
    rec[name + "_world"] = np.asarray([so_kw["src_id"], T, so_kw["q"]], dtype=np.float64)
    rec[name + "_t"] = ev.t.values.astype(np.float64)
    rec[name + "_src"] = ev.src_id.values.astype(np.int64)
    ranks = U.rank_of_src_in_df(df, so.src_id)
    rec[name + "_rows"] = np.asarray([ranks.shape[0], ranks.shape[1]], dtype=np.int64)
    cols = np.asarray(ranks.columns.values, dtype=np.int64)
    vals, first = FR.column_sums(ranks.values, ranks.index.values, T, KS)
    rec[name + "_cols"] = cols
    rec[name + "_vals"] = vals
    rec[name + "_first"] = first
    own = df.src_id.values == so.src_id
    rec[name + "_cnt"] = np.asarray([[int(np.sum((df.sink_id.values == c) & own)),
                                      int(np.sum((df.sink_id.values == c) & ~own))] for c in cols],
                                    dtype=np.int32)
    rec[name + "_r2true"] = np.float64(U.int_r_2_true(df, so))
    # the losses: an s vector over all sinks, in ascending sink order
    s_vec = 0.25 + 0.5 * np.arange(len(sinks), dtype=np.float64) / len(sinks)
    so2 = SimOpts(**dict(so_kw, sink_ids=sinks, s=s_vec))
    rec[name + "_svec"] = s_vec
    try:
        lo = U.calc_loss_opt(df, so2)
        lp = U.calc_loss_poisson(df, U_CONST, sim_opts=so2)
        assert np.array_equal(lo.index.values, ranks.index.values)
        assert np.array_equal(lp.index.values, ranks.index.values)
        rec[name + "_index"] = lo.index.values.astype(np.float64)
        rec[name + "_loss_opt"] = lo.values.astype(np.float64)
        rec[name + "_loss_pois"] = lp.values.astype(np.float64)
    except KeyError:
        assert len(cols) < len(sinks), name
    print(name, "events", len(ev), "pivot rows", ranks.shape, "losses", (name + "_loss_opt") in rec)


def main():
    names = ["readme_opt", "readme_pois", "rd_ties", "late_sink", "wide", "lonely"]
    rec = {"Ks": np.asarray(KS, dtype=np.int32), "names": np.asarray(names),
           "u_const": np.float64(U_CONST)}
    record(rec, "readme_opt", README, lambda so: so.create_manager_with_opt(seed=101))
    record(rec, "readme_pois", README, lambda so: so.create_manager_with_poisson(seed=7, capacity=400))
    record(rec, "rd_ties", RD_TIES, lambda so: so.create_manager_with_times(RD_TIES_OWN))
    record(rec, "late_sink", LATE, lambda so: so.create_manager_with_opt(seed=3))
    record(rec, "wide", WIDE, lambda so: so.create_manager_with_opt(seed=9))
    record(rec, "lonely", LONELY, lambda so: so.create_manager_with_opt(seed=4))
    out = os.path.join(HERE, "followers.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

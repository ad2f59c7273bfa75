#!/usr/bin/env python
"""Time rq_log_rank_hist against rq_log_timeline on the C3 network (graphs.c3, as bench.py
builds it): R replicas with their event logs, n time bins.

  (a) rq_log_rank_hist, 64 ranks (2 cells per lane); also 255 ranks (4) and 1 rank (1)
  (b) one rq_log_timeline call, the same bins, nK = 4: the sibling kernel on the same
      walk -- the floor
  (c) the sixteen nK = 4 rq_log_timeline calls that give the same 64 top-K curves: the
      only route to them without rq_log_rank_hist

Each is timed with HIP events around the calls on one stream, after warm-up rounds of
the same shapes; the routes alternate within every repeat, and the median and the range
of the repeats are reported.  The outputs are compared before anything is timed: the sum
of (a)'s first K cells must be (c)'s top_K for every K (rounding apart).

    python scripts/bench_rank_hist.py [--replicas 1024] [--bins 24] [--reps 7] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=1024)
    ap.add_argument("--bins", type=int, default=24)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_hist_c3.json"))
    a = ap.parse_args()
    import torch
    from redqueen_amd import _lib, engine, graphs
    assert torch.cuda.is_available(), "bench_rank_hist.py needs the GPU"
    so = graphs.c3()
    g = engine.Graph(so["src_id"], so["other_sources"], so["sink_ids"], so["edge_list"], so["end_time"])
    R = a.replicas
    res = g.run("opt", q=so["q"], s=so["s"], n_rep=R, ctrl_seed=0, world_seed=0, randomize=True,
                Ks=(1,), event_log=True)
    counts = res.counts.cpu().numpy()
    events = int(counts[:, 2].sum())
    k_sets = [tuple(range(4 * j + 1, 4 * j + 5)) for j in range(16)]

    def route_a(ranks):
        return lambda: res.rank_hist(ranks=ranks, bins=a.bins)

    def route_b():
        return res.timeline(bins=a.bins, Ks=k_sets[0])

    def route_c():
        return [res.timeline(bins=a.bins, Ks=ks) for ks in k_sets]

    # same results first
    rh = route_a(64)()
    assert (rh.status == 0).all()
    top = torch.cat([tl.metrics[:, :, :4] for tl in route_c()], dim=2)   # [R, bins, 64]
    cum = rh.hist[:, :, :64].cumsum(-1)
    rel = float(((cum - top).abs() / top.abs().clamp_min(1e-300)).max())
    assert rel < 1e-11, rel
    max_rank = int(rh.max_rank.max())
    tail64 = float(rh.tail.sum() / rh.hist.sum())
    del rh, top, cum

    routes = {"a_rank_hist_64": route_a(64), "a_rank_hist_255": route_a(255), "a_rank_hist_1": route_a(1),
              "b_timeline_nK4": route_b, "c_timeline_x16": route_c}
    ms = {k: [] for k in routes}
    for it in range(a.warmup + a.reps):
        for k, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            del out
            if it >= a.warmup:
                ms[k].append(e0.elapsed_time(e1))
    rec = {"network": "C3 (graphs.c3)", "replicas": R, "bins": a.bins, "events": events,
           "sinks": g.n_sinks, "reps": a.reps, "warmup": a.warmup, "count_update": "plain LDS atomics",
           "cum_hist_vs_top_k_max_rel": rel, "max_rank": max_rank, "tail_share_at_64_ranks": tail64,
           "build": _lib.build_stamp()}
    for k, v in ms.items():
        rec[k + "_ms"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)),
                          "all": [float(x) for x in v]}
    med = {k: rec[k + "_ms"]["median"] for k in routes}
    rec["a64_over_b"] = med["a_rank_hist_64"] / med["b_timeline_nK4"]
    rec["a64_over_c"] = med["a_rank_hist_64"] / med["c_timeline_x16"]
    rec["a64_c_ranges_overlap"] = bool(rec["a_rank_hist_64_ms"]["max"] >= rec["c_timeline_x16_ms"]["min"])
    rec["a64_events_per_s"] = events / (med["a_rank_hist_64"] * 1e-3)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

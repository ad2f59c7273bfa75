#!/usr/bin/env python
"""Time rq_log_timeline against the dataframe route on the C3 network (graphs.c3, as
bench.py builds it): R replicas with their event logs, n time bins.

  (a) rq_log_timeline, wall_posts = NULL           reads ~12 B per event
  (b) rq_log_timeline with wall_posts
  (c) the route from the same logs to whole-horizon metrics without it:
      rq_log_rows + rq_log_expand + rq_metrics_replay_batch (40 B written per
      (event, sink) row, 24 B of it read back)

Each is timed with HIP events around the calls on one stream, after warm-up calls of the
same shapes; the three alternate within every repeat, and the median and the fastest of
the repeats are reported.  The outputs are compared before anything is timed: (a)'s bins
must sum to the run's metrics (rounding apart), (c) must reproduce them.

    python scripts/bench_timeline.py [--replicas 1024] [--bins 24] [--reps 7] [--out FILE]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timeline_c3.json"))
    a = ap.parse_args()
    import torch
    from redqueen_amd import _lib, engine, graphs, utils
    assert torch.cuda.is_available(), "bench_timeline.py needs the GPU"
    so = graphs.c3()
    g = engine.Graph(so["src_id"], so["other_sources"], so["sink_ids"], so["edge_list"], so["end_time"])
    R = a.replicas
    res = g.run("opt", q=so["q"], s=so["s"], n_rep=R, ctrl_seed=0, world_seed=0, randomize=True,
                Ks=(1,), event_log=True)
    counts = res.counts.cpu().numpy()
    events = int(counts[:, 2].sum())

    def route_a():
        return res.timeline(bins=a.bins)

    def route_b():
        return res.timeline(bins=a.bins, wall=True)

    def route_c():
        ro, cols = res.log_columns()
        off = torch.from_numpy(ro).cuda()
        m, c = utils.replay_columns(cols["t"], cols["src_id"], cols["sink_id"], None, off, so["src_id"],
                                    so["end_time"], (1,))
        return m, int(ro[-1])

    # same results first
    tl = route_a()
    whole = res.metrics.cpu().numpy()
    tot = tl.metrics.sum(1).cpu().numpy()
    assert (tl.status == 0).all()
    rel = float(np.max(np.abs(tot - whole) / np.abs(whole)))
    assert rel < 1e-11, rel
    assert np.array_equal(tl.posts.sum(1).cpu().numpy(), counts[:, :2])
    tb = route_b()
    assert torch.equal(tb.metrics, tl.metrics)
    m, rows = route_c()
    assert torch.equal(m, res.metrics)
    del tl, tb, m

    routes = {"a_timeline": route_a, "b_timeline_wall": route_b, "c_rows_expand_replay": route_c}
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
    rec = {"network": "C3 (graphs.c3)", "replicas": R, "bins": a.bins, "events": events, "rows": rows,
           "sinks": g.n_sinks, "reps": a.reps, "warmup": a.warmup,
           "bins_sum_vs_metrics_max_rel": rel, "build": _lib.build_stamp()}
    for k, v in ms.items():
        rec[k + "_ms"] = {"median": float(np.median(v)), "min": float(np.min(v)), "all": [float(x) for x in v]}
    rec["a_replicas_per_s"] = R / (rec["a_timeline_ms"]["median"] * 1e-3)
    rec["a_event_bytes_per_s"] = 12.0 * events / (rec["a_timeline_ms"]["median"] * 1e-3)
    rec["a_over_c"] = rec["a_timeline_ms"]["median"] / rec["c_rows_expand_replay_ms"]["median"]
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

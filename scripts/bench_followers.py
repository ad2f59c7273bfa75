#!/usr/bin/env python
"""Time rq_log_followers on the C3 network (graphs.c3, as bench.py builds it): R replicas
with their event logs, nK = 1 (--nk N: Ks = 1..N).  Beside it, on the same logs:

  (a) rq_log_followers, rows = NULL (--rows: with the own / wall row counts)
  (b) rq_log_timeline with one bin: the sibling kernel that makes the same walk
  (c) the route (a) replaces: log_columns() (rq_log_rows + rq_log_expand, 40 B per
      (event, sink) row), the pivot's column index and unique-time count of every
      replica (torch, batched), and one rq_rank_table per replica into a reused table.
      rq_rank_table walks a replica's ~0.7 M rows with one wave per 64 sink columns, so
      1,024 calls take tens of seconds: the calls are timed on a sample of --sample
      replicas (evenly spaced over the batch, their host loop included) and the record
      says so; c_full_batch_estimate_ms = preparation + sample time x replicas / sample.

Each is timed with HIP events around the calls on one stream, after warm-up rounds of the
same shapes; the routes alternate within every repeat, and the median, the fastest, the
slowest and all repeats are reported.  Before anything is timed (a) is compared with the
run's own metrics (the mean over the seen sinks of the per-sink top-1 integrals is the
sweep's top_1) and (c)'s unique-time counts with the run's pivot rows.

    python scripts/bench_followers.py [--replicas 1024] [--reps 7] [--sample 32] [--nk 1] [--rows]
                                      [--out FILE]
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sample", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nk", type=int, default=1, help="route (a) with Ks = 1..nk")
    ap.add_argument("--rows", action="store_true", help="route (a) with the row counts")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "followers_c3.json"))
    a = ap.parse_args()
    import torch
    from redqueen_amd import _lib as L
    from redqueen_amd import engine, graphs
    assert torch.cuda.is_available(), "bench_followers.py needs the GPU"
    so = graphs.c3()
    g = engine.Graph(so["src_id"], so["other_sources"], so["sink_ids"], so["edge_list"], so["end_time"])
    R = a.replicas
    res = g.run("opt", q=so["q"], s=so["s"], n_rep=R, ctrl_seed=0, world_seed=0, randomize=True,
                Ks=(1,), event_log=True)
    counts = res.counts.cpu().numpy()
    events = int(counts[:, 2].sum())
    dev = res.ev_t.device
    lib = L.lib()
    sink_sorted = torch.from_numpy(np.sort(np.asarray(g.sink_ids, dtype=np.int64))).to(dev)
    n_t_max = int(counts[:, 3].max())
    table = torch.empty((n_t_max, g.n_sinks), dtype=torch.float64, device=dev)
    index = torch.empty(n_t_max, dtype=torch.float64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)

    Ks = tuple(range(1, a.nk + 1))

    def route_a():
        return res.followers(Ks=Ks, rows=a.rows)

    def route_b():
        return res.timeline(bins=1)

    def say(msg):
        print("# " + msg, file=sys.stderr, flush=True)

    def prep_c():
        """Rows of every replica, their pivot column and every replica's unique times."""
        ro, cols = res.log_columns()
        col = torch.searchsorted(sink_sorted, cols["sink_id"]).to(torch.int32)
        t = cols["t"]
        new = torch.ones(t.numel(), dtype=torch.int64, device=dev)
        new[1:] = (t[1:] != t[:-1]).to(torch.int64)
        off = torch.from_numpy(ro).to(dev)
        new[off[:-1][off[:-1] < t.numel()]] = 1          # a replica's first row starts a time
        cs = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(new, 0)])
        n_t = (cs[off[1:]] - cs[off[:-1]]).cpu().numpy()
        return ro, cols, col, n_t

    sample = np.unique(np.linspace(0, R - 1, min(a.sample, R)).astype(np.int64))

    def tables_c(p):
        ro, cols, col, n_t = p
        st = torch.cuda.current_stream().cuda_stream
        for i in sample:
            lo, n = int(ro[i]), int(ro[i + 1] - ro[i])
            if n == 0:
                continue
            L.check("rq_rank_table", lib.rq_rank_table(
                cols["t"].data_ptr() + 8 * lo, cols["src_id"].data_ptr() + 8 * lo, col.data_ptr() + 4 * lo,
                n, g.n_sinks, int(so["src_id"]), 1, int(n_t[i]), table.data_ptr(), index.data_ptr(),
                err.data_ptr(), st))
        return None

    # same results first
    fl = route_a()
    assert (fl.status == 0).all()
    S = (~torch.isnan(fl.first_t)).sum(1).to(torch.float64)
    top1 = (fl.top_k(1).sum(1) / S).cpu().numpy()
    whole = res.metrics[:, 0].cpu().numpy()
    rel = float(np.max(np.abs(top1 - whole) / np.abs(whole)))
    assert rel < 1e-11, rel
    say("followers checked against the run's metrics")
    p = prep_c()
    rows = int(p[0][-1])
    assert np.array_equal(p[3], counts[:, 3])
    tables_c(p)
    assert int(err.item()) == 0
    del fl, p
    say("rank tables of %d sample replicas checked" % len(sample))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    ms = {"a_followers": [], "b_timeline_one_bin": [], "c_prepare_all_replicas": [],
          "c_rank_tables_sample": []}
    for it in range(a.warmup + a.reps):
        ta, out = timed(route_a)
        del out
        tb, out = timed(route_b)
        del out
        tp, p = timed(prep_c)
        tt, _ = timed(lambda: tables_c(p))
        del p
        say("round %d: a %.3f ms, b %.3f ms, c prepare %.1f ms + %d tables %.1f ms" % (it, ta, tb, tp, len(sample), tt))
        if it >= a.warmup:
            for k, v in zip(ms, (ta, tb, tp, tt)):
                ms[k].append(v)
    lds = g.n_sinks * (12 + 8 * (a.nk + 2) + (8 if a.rows else 0))
    rec = {"network": "C3 (graphs.c3)", "replicas": R, "nK": a.nk, "row_counts": a.rows, "events": events,
           "rows": rows,
           "sinks": g.n_sinks, "reps": a.reps, "warmup": a.warmup,
           "c_sample_replicas": int(len(sample)),
           "top1_vs_metrics_max_rel": rel, "lds_bytes_per_block": lds,
           "resident_blocks_per_cu_by_lds": (160 * 1024) // lds, "build": L.build_stamp()}
    for k, v in ms.items():
        rec[k + "_ms"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)),
                          "all": [float(x) for x in v]}
    rec["c_full_batch_estimate_ms"] = (rec["c_prepare_all_replicas_ms"]["median"] +
                                       rec["c_rank_tables_sample_ms"]["median"] * R / len(sample))
    rec["a_events_per_s"] = events / (rec["a_followers_ms"]["median"] * 1e-3)
    rec["a_replicas_per_s"] = R / (rec["a_followers_ms"]["median"] * 1e-3)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

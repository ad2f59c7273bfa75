#!/usr/bin/env python
"""Time rq_log_followers_tiled (BatchResult.followers(tiled=True)): nK = 1, no row counts.

  --net c5   graphs.c5() (10,000 followers: past rq_log_followers' limit), R replicas with
             their event logs.  The tiled call, and with --route-c N the only route that
             existed for this world: log_columns() (rq_log_rows + rq_log_expand, 40 B per
             (event, sink) row), every replica's pivot column and unique-time count (torch)
             and one rq_rank_table per replica -- on a batch of its own of N replicas (a C5
             replica expands to ~2 GB of rows and a rank table of tens of GB), timed once,
             no repeat.
  --net c3   graphs.c3() (1,000 followers: one tile), R replicas: the tiled entry (one tile
             plus the r2 pass) beside rq_log_followers of the same build, alternating within
             every repeat, and their ratio.

Each call is timed with HIP events on one stream after warm-up rounds of the same shapes;
the median, the fastest, the slowest and all repeats are reported.  Before anything is timed
the tiled result is checked: on C3 bit for bit against rq_log_followers, on C5 against the
run's own metrics (the mean over the seen sinks of the per-sink top-1 integrals is the
sweep's top_1).  The record goes into --out under the key "<net>_ts<TS>" (TS: the loaded
library's rq_log_followers_tile_sinks; RQ_SO_PATH selects a library built with
EXTRA=-DRQ_FOLLOWERS_TILE_SINKS=...), beside what the file already holds.

    python scripts/bench_followers_tiled.py --net c5 [--replicas 256] [--reps 3] [--route-c 1]
    python scripts/bench_followers_tiled.py --net c3 [--replicas 1024] [--reps 7]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def say(msg):
    print("# " + msg, file=sys.stderr, flush=True)


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)),
            "all": [float(x) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", choices=("c5", "c3"), required=True)
    ap.add_argument("--replicas", type=int, default=0)
    ap.add_argument("--reps", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--route-c", type=int, default=0, help="c5: replicas of the dataframe route (0: skip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "followers_tiled.json"))
    a = ap.parse_args()
    import torch
    from redqueen_amd import _lib as L
    from redqueen_amd import engine, graphs
    assert torch.cuda.is_available(), "bench_followers_tiled.py needs the GPU"
    lib = L.lib()
    TS = int(lib.rq_log_followers_tile_sinks())
    c5 = a.net == "c5"
    so = graphs.c5() if c5 else graphs.c3()
    R = a.replicas or (256 if c5 else 1024)
    reps = a.reps or (3 if c5 else 7)
    g = engine.Graph(so["src_id"], so["other_sources"], so["sink_ids"], so["edge_list"], so["end_time"])
    kw = dict(q=so["q"], s=so["s"], ctrl_seed=0, world_seed=0, randomize=True, Ks=(1,), event_log=True)
    res = g.run("opt", n_rep=R, **kw)
    counts = res.counts.cpu().numpy()
    events = int(counts[:, 2].sum())
    n_tiles = -(-g.n_sinks // TS)
    say("%s: %d replicas, %d events, %d sinks, TS %d (%d tiles)" % (a.net, R, events, g.n_sinks, TS, n_tiles))

    def tiled():
        return res.followers(tiled=True)

    def plain():
        return res.followers(tiled=False)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    # same results first
    fl = tiled()
    ok = fl.status == 0
    assert bool(ok.all()), "flagged replicas: pick other seeds"
    S = (~torch.isnan(fl.first_t)).sum(1).to(torch.float64)
    top1 = (fl.top_k(1).sum(1) / S).cpu().numpy()
    whole = res.metrics[:, 0].cpu().numpy()
    rel = float(np.max(np.abs(top1 - whole) / np.abs(whole)))
    # another summation order of <= n terms: (n + 8) ulp, n the pivot rows (tests/followers_ref.py)
    assert rel <= (int(counts[:, 3].max()) + 8) * 2.0 ** -52, rel
    say("tiled top_1 against the run's metrics: max rel %.3g" % rel)
    if not c5:
        fo = plain()
        for x, y in ((fl.vals, fo.vals), (fl.first_t, fo.first_t), (fl.r_2_true, fo.r_2_true)):
            assert torch.equal(torch.isnan(x), torch.isnan(y))
            assert torch.equal(torch.nan_to_num(x).view(torch.int64), torch.nan_to_num(y).view(torch.int64))
        assert torch.equal(fl.status, fo.status)
        say("tiled equals rq_log_followers bit for bit")
        del fo
    del fl

    routes = {"tiled": tiled} if c5 else {"tiled": tiled, "plain": plain}
    ms = {k: [] for k in routes}
    for it in range(a.warmup + reps):
        line = []
        for k, fn in routes.items():
            t, out = timed(fn)
            del out
            line.append("%s %.3f ms" % (k, t))
            if it >= a.warmup:
                ms[k].append(t)
        say("round %d: %s" % (it, ", ".join(line)))
    lds = min(TS, g.n_sinks) * (12 + 8 * 3)
    rec = {"network": "C5 (graphs.c5)" if c5 else "C3 (graphs.c3)", "replicas": R, "nK": 1, "rows": False,
           "events": events, "sinks": g.n_sinks, "tile_sinks": TS, "tiles": n_tiles, "reps": reps,
           "warmup": a.warmup, "top1_vs_metrics_max_rel": rel, "tile_lds_bytes_per_block": lds,
           "tile_blocks_per_cu_by_lds": (160 * 1024) // lds, "r2_lds_bytes_per_block": 4 * g.n_sinks,
           "build": L.build_stamp()}
    for k, v in ms.items():
        rec[k + "_ms"] = stats(v)
    med = rec["tiled_ms"]["median"]
    rec["tiled_events_per_s"] = events / (med * 1e-3)
    rec["tiled_ms_per_replica"] = med / R
    if not c5:
        rec["tiled_over_plain"] = med / rec["plain_ms"]["median"]

    if c5 and a.route_c > 0:
        del res
        torch.cuda.empty_cache()
        n = a.route_c
        sub = g.run("opt", n_rep=n, **kw)
        sc = sub.counts.cpu().numpy()
        dev = sub.ev_t.device
        sink_sorted = torch.from_numpy(np.sort(np.asarray(g.sink_ids, dtype=np.int64))).to(dev)
        n_t_max = int(sc[:, 3].max())
        need = 8.0 * n_t_max * g.n_sinks
        free = torch.cuda.mem_get_info()[0]
        rec["c_replicas"] = n
        rec["c_rank_table_bytes"] = need
        # ~60 B per expanded (event, sink) row: the five columns, the pivot column, the time marks
        rows_est = float(sc[:, 2].sum()) * len(so["edge_list"]) / (len(so["other_sources"]) + 1)
        if need + 60.0 * rows_est > 0.8 * free:
            rec["c_not_measured"] = "a replica's rank table (%.1f GB) does not fit the free memory" % (need / 1e9)
        else:
            table = torch.empty((n_t_max, g.n_sinks), dtype=torch.float64, device=dev)
            index = torch.empty(n_t_max, dtype=torch.float64, device=dev)
            err = torch.zeros(1, dtype=torch.int32, device=dev)

            def prep_c():
                ro, cols = sub.log_columns()
                col = torch.searchsorted(sink_sorted, cols["sink_id"]).to(torch.int32)
                t = cols["t"]
                new = torch.ones(t.numel(), dtype=torch.int64, device=dev)
                new[1:] = (t[1:] != t[:-1]).to(torch.int64)
                off = torch.from_numpy(ro).to(dev)
                new[off[:-1][off[:-1] < t.numel()]] = 1
                cs = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(new, 0)])
                n_t = (cs[off[1:]] - cs[off[:-1]]).cpu().numpy()
                return ro, cols, col, n_t

            def tables_c(p):
                ro, cols, col, n_t = p
                st = torch.cuda.current_stream().cuda_stream
                for i in range(n):
                    lo, m = int(ro[i]), int(ro[i + 1] - ro[i])
                    if m:
                        L.check("rq_rank_table", lib.rq_rank_table(
                            cols["t"].data_ptr() + 8 * lo, cols["src_id"].data_ptr() + 8 * lo,
                            col.data_ptr() + 4 * lo, m, g.n_sinks, int(so["src_id"]), 1, int(n_t[i]),
                            table.data_ptr(), index.data_ptr(), err.data_ptr(), st))

            tp, p = timed(prep_c)
            assert np.array_equal(p[3], sc[:, 3])
            tt, _ = timed(lambda: tables_c(p))
            assert int(err.item()) == 0
            say("route c: prepare %.1f ms, %d rank tables %.1f ms" % (tp, n, tt))
            rec["c_rows"] = int(p[0][-1])
            rec["c_prepare_ms"] = tp
            rec["c_rank_tables_ms"] = tt
            rec["c_ms_per_replica"] = (tp + tt) / n
            rec["c_timed_once_no_warmup"] = True
            rec["c_over_tiled_per_replica"] = rec["c_ms_per_replica"] / rec["tiled_ms_per_replica"]

    print(json.dumps(rec))
    if a.out:
        allrec = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                allrec = json.load(f)
        allrec["%s_ts%d" % (a.net, TS)] = rec
        with open(a.out, "w") as f:
            json.dump(allrec, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Time the metrics of every player of a game from its completed event logs
(rq_log_metrics_of) on bench_game.py's C3 game: k = 16 of C3's 50 wall sources as Opt
broadcasters plus the controlled RedQueen, 17 players, R replicas after a warm-up batch.

Per process: the game runs once with its event log; then, --runs times and interleaved, the
device milliseconds (HIP events on the stream, the call already warm at this shape) of
  lm      rq_log_metrics on the completed logs (BatchResult.log_metrics), the controlled
          source alone -- the figure the shared kernel body must not have changed
  of_df   one rq_log_metrics_of call for the 17 players, scope "df"
  of_own  the same, scope "own"
The second and third are skipped on a library from before the entry (RQ_SO_PATH points at
such a build for the A/B: --label parent).  Every process appends its record to --out;
with records of both labels in the file the summary holds t1 = the parent's median, the
ratio of this build's lm to it (bound 1.10), of_df against its bound 17 x t1 x 1.1 and
of_own / of_df.  Alternate the labels in one session on one device:

    RQ_SO_PATH=<parent librq.so> python scripts/bench_log_sources.py --label parent
    python scripts/bench_log_sources.py --label after
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def summary(rec):
    by = {}
    for m in rec["measurements"]:
        for what, ms in m["ms"].items():
            by.setdefault((m["label"], what), []).extend(ms)
    med = {k: float(np.median(v)) for k, v in by.items()}
    s = {"median_ms": {"%s/%s" % k: v for k, v in sorted(med.items())},
         "range_ms": {"%s/%s" % k: [float(min(v)), float(max(v))] for k, v in sorted(by.items())}}
    t1 = med.get(("parent", "lm"))
    if t1 is not None and ("after", "lm") in med:
        s["t1_parent_lm_ms"] = t1
        s["after_lm_over_t1"] = med[("after", "lm")] / t1
        s["after_lm_within_10_percent"] = bool(med[("after", "lm")] <= 1.1 * t1)
        if ("after", "of_df") in med:
            P = rec["players"]
            s["of_df_bound_ms"] = P * t1 * 1.1
            s["of_df_within_bound"] = bool(med[("after", "of_df")] <= P * t1 * 1.1)
            s["of_df_over_players_x_t1"] = med[("after", "of_df")] / (P * t1)
            s["of_own_over_of_df"] = med[("after", "of_own")] / med[("after", "of_df")]
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=10000)
    ap.add_argument("--warmup-replicas", type=int, default=256)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--label", default="after", help='"parent", "after", or the name of another A/B build')
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "log_sources_c3.json"))
    a = ap.parse_args()
    import torch
    from bench_game import world
    from redqueen_amd import _lib, engine, graphs
    assert torch.cuda.is_available(), "bench_log_sources.py needs the GPU"
    w = world(graphs.c3(), a.k)
    g = engine.Graph(w["src_id"], w["other_sources"], w["sink_ids"], w["edge_list"], w["end_time"])
    kw = dict(q=w["q"], s=w["s"], randomize=True, Ks=(1,), event_log=True)
    have_of = all(_lib.has(fn) for fn in _lib.OPTIONAL) and hasattr(engine.BatchResult, "source_metrics")
    calls = {"lm": lambda r: r.log_metrics()}
    if have_of:
        calls["of_df"] = lambda r: r.player_metrics("df")
        calls["of_own"] = lambda r: r.player_metrics("own")
    warm = g.run("opt", n_rep=a.warmup_replicas, ctrl_seed=1, world_seed=1, **kw)
    for fn in calls.values():
        fn(warm)
    del warm
    res = g.run("opt", n_rep=a.replicas, ctrl_seed=7, world_seed=7, **kw)
    first = {what: fn(res) for what, fn in calls.items()}   # warm at the timed shape
    torch.cuda.synchronize()
    ms = {what: [] for what in calls}
    for _i in range(a.runs):
        for what, fn in calls.items():
            t, out = timed(torch, lambda: fn(res))
            ms[what].append(t)
            same = (np.array_equal(out.metrics.cpu().numpy().view(np.int64),
                                   first[what].metrics.cpu().numpy().view(np.int64)) and
                    bool((out.counts == first[what].counts).all()))
            assert same, what   # run to run: the same bits
    events = res.counts[:, 2].double()
    m = {"label": a.label, "build": _lib.build_stamp(), "ms": ms,
         "events_per_replica": float(events.mean()), "log_capacity": int(res.ev_t.shape[1]),
         "lm_equals_run_metrics": bool(np.array_equal(first["lm"].metrics.cpu().numpy().view(np.int64),
                                                      res.metrics.cpu().numpy().view(np.int64)))}
    if have_of:
        c = res.player_ids.index(g.src_id)
        lm = first["lm"].metrics.cpu().numpy().view(np.int64)
        m["of_df_ctrl_equals_lm"] = bool(np.array_equal(first["of_df"].metrics[:, c].cpu().numpy().view(np.int64), lm))
        m["of_own_ctrl_equals_lm"] = bool(np.array_equal(first["of_own"].metrics[:, c].cpu().numpy().view(np.int64), lm))
        own, df = first["of_own"], first["of_df"]
        m["events_own_over_df"] = float(own.counts[:, :, :2].sum().item()) / float(df.counts[:, :, :2].sum().item())
        m["columns_own_over_df"] = float(own.counts[:, :, 3].sum().item()) / float(df.counts[:, :, 3].sum().item())
        m["players_mean"] = {str(s): {"posts": float(own.counts[:, k, 0].double().mean()),
                                      "top_1_own": float(own.top_k(1)[:, k].mean()),
                                      "avg_rank_own": float(own.avg_rank[:, k].mean()),
                                      "avg_rank_df": float(df.avg_rank[:, k].mean())}
                             for k, s in enumerate(own.src_ids)}
    print(json.dumps(m), flush=True)
    rec = {"network": "C3 (graphs.c3), k = %d wall sources as Opt broadcasters" % a.k, "players": a.k + 1,
           "replicas": a.replicas, "warmup_replicas": a.warmup_replicas, "runs_per_process": a.runs,
           "measurements": []}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        if all(old.get(key) == rec[key] for key in ("network", "replicas", "warmup_replicas")):
            rec["measurements"] = old["measurements"]
    rec["measurements"].append(m)
    rec["summary"] = summary(rec)
    print(json.dumps(rec["summary"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

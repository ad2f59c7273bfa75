#!/usr/bin/env python
"""Time stage 3 of a game -- the metrics of the completed logs -- on the 8-byte pivot cells
(rq_log_metrics_slim) against what it replaces, on one build, after a warm-up of each
variant, --runs runs per variant interleaved, HIP events around the stage:

  c3    bench_game.py's C3 game (k = 1, 4, 16 wall sources as Opt broadcasters, R replicas,
        the controlled RedQueen one more player), played once per k with its event log;
        then the call stage 3 makes on those logs, BatchResult.log_metrics, with the
        16-byte entry (slim=False, the default for this graph) and with the slim entry
        forced (slim=True).  Recorded only: the default below 9,801 sinks stays.
  c5    a C5-shaped game: graphs.c5() (10,000 followers, 500 Hawkes sources) with k sources
        as Opt broadcasters and end_time cut down so that the replay route's dataframe rows
        fit its chunks; Graph.run per route ("replay": rq_log_expand +
        rq_metrics_replay_batch, what a graph of more than 9,800 sinks took before; "log":
        here rq_log_metrics_slim), stage 3 from Graph.game_ms.  ``adopt``: the game's "log"
        takes the slim entry past 9,800 sinks only if its slowest run beats the replay
        route's fastest.
  full  one ordinary C5 run at its full end_time with a few replicas and its event log,
        then log_metrics(slim=True): the log capacity, the workspace of one block, the
        replicas a LOG_METRICS_WS_BYTES chunk holds, the time.

Every pair of variants is compared bit for bit (metrics, counts, status).

    python scripts/bench_log_metrics_slim.py [--parts c3 c5 full] [--replicas 10000] [--k 1 4 16]
        [--c5-replicas 64] [--c5-end 10] [--c5-k 4] [--full-replicas 4] [--runs 3] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def timed(torch, fn):
    """(device ms, result) of fn on the current stream."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return float(e0.elapsed_time(e1)), out


def bits(x):
    return (x.metrics.cpu().numpy().view(np.int64), x.counts.cpu().numpy(), x.status.cpu().numpy())


def same(a, b):
    return bool(all(np.array_equal(u, v) for u, v in zip(a, b)))


def part_c3(a, torch, engine, graphs, rec):
    from bench_game import world
    so = graphs.c3()
    for k in a.k:
        w = world(so, k)
        g = engine.Graph(w["src_id"], w["other_sources"], w["sink_ids"], w["edge_list"], w["end_time"])
        res = g.run("opt", q=w["q"], s=w["s"], randomize=True, Ks=(1,), n_rep=a.replicas, ctrl_seed=7,
                    world_seed=7, event_log=True)
        torch.cuda.synchronize()
        variants = {"cells16": False, "slim": True}
        first = {}
        for name, slim in variants.items():   # warm-up: the allocator's blocks, the code objects
            first[name] = bits(res.log_metrics(slim=slim))
        ms = {name: [] for name in variants}
        for _i in range(a.runs):
            for name, slim in variants.items():
                t, _lm = timed(torch, lambda: res.log_metrics(slim=slim))
                ms[name].append(t)
        events = res.counts[:, 2].double()
        row = {"k": k, "players": len(res.player_ids), "replicas": a.replicas, "ev_cap": int(res.ev_t.shape[1]),
               "events_per_replica": float(events.mean()), "n_sinks": g.n_sinks, "ms": ms,
               "same_bits": same(first["cells16"], first["slim"]),
               "ties": int((first["slim"][2] & 4 != 0).sum()),
               "slim_median_over_cells16_median": float(np.median(ms["slim"]) / np.median(ms["cells16"]))}
        rec["c3"].append(row)
        print(json.dumps(row), flush=True)
        del res, g
        torch.cuda.empty_cache()


def part_c5(a, torch, engine, graphs, rec):
    from bench_game import world
    so = dict(graphs.c5(), end_time=float(a.c5_end))
    w = world(so, a.c5_k)
    g = engine.Graph(w["src_id"], w["other_sources"], w["sink_ids"], w["edge_list"], w["end_time"])
    kw = dict(q=w["q"], s=w["s"], randomize=True, Ks=(1,), n_rep=a.c5_replicas, ctrl_seed=7, world_seed=7)
    g.GAME_METRICS_SLIM = True   # the variant under test, whatever the adopted default
    routes = ("replay", "log")
    for route in routes:
        g.GAME_METRICS = route
        g.run("opt", **kw)
    torch.cuda.synchronize()
    g.game_timing = True
    ms = {r: [] for r in routes}
    taken, first, info = {}, {}, {}
    for i in range(a.runs):
        for route in routes:
            g.GAME_METRICS = route
            res = g.run("opt", event_log=(i == 0 and route == "log"), **kw)
            torch.cuda.synchronize()
            ms[route].append(float(g.game_ms["replay"]))
            taken[route] = g.game_metrics_route
            if i == 0:
                first[route] = (res.metrics.cpu().numpy().view(np.int64), res.counts.cpu().numpy(),
                                res.status.cpu().numpy())
                if route == "log":
                    info = {"ev_cap": int(res.ev_t.shape[1]),
                            "events_per_replica": float(res.counts[:, 2].double().mean()),
                            "pivot_rows_per_replica": float(res.counts[:, 3].double().mean()),
                            "players": len(res.player_ids)}
            del res
    row = {"network": "graphs.c5() with end_time = %g, %d sources as Opt broadcasters" % (a.c5_end, a.c5_k),
           "n_sinks": g.n_sinks, "replicas": a.c5_replicas, "routes_taken": taken, "ms": ms,
           "same_bits": same(first["replay"], first["log"]),
           "slim_slowest_beats_replay_fastest": bool(max(ms["log"]) < min(ms["replay"])),
           "replay_median_over_slim_median": float(np.median(ms["replay"]) / np.median(ms["log"]))}
    row.update(info)
    row["adopt"] = bool(row["slim_slowest_beats_replay_fastest"] and row["same_bits"] and
                        taken["log"] == "log-slim")
    rec["c5"] = row
    print(json.dumps(row), flush=True)
    del g
    torch.cuda.empty_cache()


def part_full(a, torch, engine, graphs, L, rec):
    so = graphs.c5()
    g = engine.Graph(so["src_id"], so["other_sources"], so["sink_ids"], so["edge_list"], so["end_time"])
    res = g.run("opt", q=so["q"], s=so["s"], randomize=True, Ks=(1,), n_rep=a.full_replicas, ctrl_seed=7,
                world_seed=7, event_log=True)
    torch.cuda.synchronize()
    cap = int(res.ev_t.shape[1])
    row = {"network": "graphs.c5(), end_time = %g" % so["end_time"], "n_sinks": g.n_sinks,
           "replicas": a.full_replicas, "ev_cap": cap,
           "events_per_replica": float(res.counts[:, 2].double().mean())}
    nb = C.c_size_t()
    rc = L.lib().rq_log_metrics_slim_workspace(g._h, 1, cap, 1, C.byref(nb))
    row["workspace_query_status"] = int(rc)
    if rc == 0:
        row["workspace_bytes_per_block"] = int(nb.value)
        row["ws_budget_bytes"] = int(res.LOG_METRICS_WS_BYTES)
        row["replicas_per_chunk"] = int(max(1, res.LOG_METRICS_WS_BYTES // nb.value))
        first = bits(res.log_metrics(slim=True))
        ms = [timed(torch, lambda: res.log_metrics(slim=True))[0] for _i in range(a.runs)]
        row["ms"] = ms
        row["same_bits_as_the_run"] = bool(np.array_equal(first[0], res.metrics.cpu().numpy().view(np.int64)))
        row["ties"] = int((first[2] & 4 != 0).sum())
    rec["full"] = row
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["c3", "c5", "full"], choices=["c3", "c5", "full"])
    ap.add_argument("--replicas", type=int, default=10000)
    ap.add_argument("--k", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--c5-replicas", type=int, default=64)
    ap.add_argument("--c5-end", type=float, default=10.0)
    ap.add_argument("--c5-k", type=int, default=4)
    ap.add_argument("--full-replicas", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "log_metrics_slim.json"))
    a = ap.parse_args()
    import torch
    from redqueen_amd import _lib as L
    from redqueen_amd import engine, graphs
    assert torch.cuda.is_available(), "bench_log_metrics_slim.py needs the GPU"
    rec = {"build": L.build_stamp(), "runs_per_variant": a.runs, "c3": [], "c5": None, "full": None}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rec, f, indent=1)
                f.write("\n")
    if "c3" in a.parts:
        part_c3(a, torch, engine, graphs, rec)
        save()
    if "c5" in a.parts:
        part_c5(a, torch, engine, graphs, rec)
        save()
    if "full" in a.parts:
        part_full(a, torch, engine, graphs, L, rec)
        save()


if __name__ == "__main__":
    main()

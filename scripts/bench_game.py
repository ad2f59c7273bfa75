#!/usr/bin/env python
"""Time a game of competing RedQueen broadcasters (rq_log_game) on the C3 network
(graphs.c3, as bench.py builds it) with k of its 50 wall sources turned into Opt
broadcasters (every 50 / k-th source, on its own followers, s = 1, C3's q), the controlled
RedQueen included as one more player: R replicas, k = 1, 4, 16.

Per k, after a warm-up batch of the same graph on each route: the device milliseconds of
the three stages of Graph.run -- the exogenous pass (the ordinary engine with its event
log), the game kernel (with any overflow rerun) and the metrics of the completed logs --
from HIP events around each stage (Graph.game_timing), and the posts per player.  The third
stage is timed on both of its routes (Graph.GAME_METRICS): "replay", rq_log_expand +
rq_metrics_replay_batch, and "log", rq_log_metrics; --runs runs per route, interleaved, on
one build, and the routes' metrics and counts are compared bit for bit.  ``stage3`` sums it
up per k, with the rule the default route is chosen by: "log" only if its slowest run beats
the replay route's fastest at every k.

    python scripts/bench_game.py [--replicas 10000] [--k 1 4 16] [--routes replay log] [--runs 3]
                                 [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def world(so, k):
    n = len(so["other_sources"])
    pick = {i * n // k for i in range(k)}
    others = [("Opt", {"src_id": kw["src_id"], "seed": kw["seed"], "q": so["q"], "s": 1.0}) if i in pick
              else (kind, kw) for i, (kind, kw) in enumerate(so["other_sources"])]
    return dict(so, other_sources=others)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=10000)
    ap.add_argument("--warmup-replicas", type=int, default=256)
    ap.add_argument("--k", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--routes", nargs="+", default=["replay", "log"], choices=["replay", "log"])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "game_c3_logmetrics.json"))
    a = ap.parse_args()
    import torch
    from redqueen_amd import _lib, engine, graphs
    assert torch.cuda.is_available(), "bench_game.py needs the GPU"
    so = graphs.c3()
    R = a.replicas
    rec = {"network": "C3 (graphs.c3), k wall sources as Opt broadcasters", "replicas": R,
           "warmup_replicas": a.warmup_replicas, "build": _lib.build_stamp(), "routes": a.routes,
           "runs_per_route": a.runs, "runs": [], "stage3": []}
    for k in a.k:
        w = world(so, k)
        g = engine.Graph(w["src_id"], w["other_sources"], w["sink_ids"], w["edge_list"], w["end_time"])
        kw = dict(q=w["q"], s=w["s"], randomize=True, Ks=(1,))
        for route in a.routes:
            g.GAME_METRICS = route
            g.run("opt", n_rep=a.warmup_replicas, ctrl_seed=1, world_seed=1, **kw)
        torch.cuda.synchronize()
        g.game_timing = True
        ms3 = {route: [] for route in a.routes}
        first = {}
        for i in range(a.runs):
            for route in a.routes:
                g.GAME_METRICS = route
                t0 = time.perf_counter()
                res = g.run("opt", n_rep=R, ctrl_seed=7, world_seed=7, **kw)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                posts = res.player_posts.double().mean(0).cpu().numpy()
                events = res.counts[:, 2].double()
                run = {"k": k, "route": route, "run": i, "players": len(res.player_ids), "streams": g.n_streams,
                       "table_in_lds": int(_lib.lib().rq_log_game_table_in_lds(g._h, len(res.player_ids))),
                       "ms": {s: float(v) for s, v in g.game_ms.items()}, "wall_s": wall, "reruns": int(g.reruns),
                       "events_per_replica": float(events.mean()), "events": float(events.sum()),
                       "game_events_per_s": float(events.sum()) / (g.game_ms["game"] * 1e-3),
                       "posts_per_player": {str(i): float(p) for i, p in zip(res.player_ids, posts)},
                       "status_or": int(np.bitwise_or.reduce(res.status.cpu().numpy()))}
                ms3[route].append(run["ms"]["replay"])
                if i == 0:   # every route gives the same bits
                    first[route] = (res.metrics.cpu().numpy().view(np.int64), res.counts.cpu().numpy())
                rec["runs"].append(run)
                print(json.dumps(run), flush=True)
                del res
        s3 = {"k": k, "ms": ms3}
        if len(first) == 2:
            (m0, c0), (m1, c1) = first.values()
            s3["same_bits"] = bool(np.array_equal(m0, m1) and np.array_equal(c0, c1))
            s3["log_slowest_beats_replay_fastest"] = bool(max(ms3["log"]) < min(ms3["replay"]))
            s3["replay_median_over_log_median"] = float(np.median(ms3["replay"]) / np.median(ms3["log"]))
        rec["stage3"].append(s3)
        print(json.dumps(s3), flush=True)
        del g
        torch.cuda.empty_cache()
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rec, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()

"""Batched replica grids: the multiprocessing drivers of the reference as GPU batches.

The reference runs one (seed, q, s) replica per process through mp.Pool /
mp.Queue (utils.calc_q_capacity_iter :447-470, opt_runs.worker_opt /
worker_poisson :51-126, opt_runs.run_inference_queue :560-646) and collects
``perf_opts.performance_fields`` (opt_runs.py:33-38) via add_perf (:41-48).
Here a whole grid is one launch sequence of the engine; the result is a
DataFrame with the same fields (seed, q, type, top_K..., avg_rank, r_2,
num_events, world_events, capacity).
"""
import collections
import hashlib

import numpy as np
import pandas as pd
import torch

from .engine import Graph

_CACHE = collections.OrderedDict()


def _val_key(v):
    # arrays (RealData times, PiecewiseConst tables) by dtype, shape and a content
    # hash: numpy's repr elides the middle of arrays longer than 1000 elements
    if isinstance(v, (np.ndarray, list, tuple)):
        a = np.ascontiguousarray(np.asarray(v))
        if a.dtype != object:
            return (str(a.dtype), a.shape, hashlib.sha1(a.tobytes()).hexdigest())
    if isinstance(v, dict):   # an Opt's s by sink id: whatever the insertion order
        return tuple(sorted((repr(k), _val_key(x)) for k, x in v.items()))
    return repr(v)


def _key(so):
    return (so.src_id, float(so.end_time), tuple(map(tuple, so.edge_list)),
            tuple(so.sink_ids), repr([(n if isinstance(n, str) else n.__name__,
                                       sorted((k, _val_key(v)) for k, v in kw.items()))
                                      for n, kw in so.other_sources]))


def compiled_graph(sim_opts):
    """Device-resident graph for a SimOpts (cached on its contents)."""
    k = _key(sim_opts)
    g = _CACHE.get(k)
    if g is None:
        g = Graph(sim_opts.src_id, sim_opts.other_sources, sim_opts.sink_ids, sim_opts.edge_list,
                  sim_opts.end_time)
        _CACHE[k] = g
        while len(_CACHE) > 8:
            _CACHE.popitem(last=False)
    return g


def _frame(res, seeds, qs, kind, Ks):
    m = res.metrics.cpu().numpy()
    c = res.counts.cpu().numpy()
    st = res.status.cpu().numpy()
    d = {"seed": seeds, "q": qs, "type": kind}
    for i, k in enumerate(Ks):
        d["top_" + str(k)] = m[:, i]
    d["avg_rank"] = m[:, len(Ks)]
    d["r_2"] = m[:, len(Ks) + 1]
    d["num_events"] = c[:, 0]
    d["world_events"] = c[:, 1]
    d["capacity"] = c[:, 0].astype(np.float64)
    d["events"] = c[:, 2]
    d["status"] = st
    return pd.DataFrame(d)


def run_grid(sim_opts, qs=None, ss=None, seeds=range(10), randomize=True, Ks=(1,),
             max_events=None, chunk=0):
    """RedQueen over the grid qs x ss x seeds.

    qs: iterable of q (default [sim_opts.q]); ss: iterable of s (scalar, vector over
    the sorted followers or dict), default [sim_opts.s]; seeds: replica seeds u --
    the RedQueen seed is u and, with randomize, the world is
    sim_opts.randomize_other_sources(u) (the C2 protocol); every grid point sees
    the same seeds (common random numbers, as calc_q_capacity_iter does)."""
    g = compiled_graph(sim_opts)
    qs = [sim_opts.q] if qs is None else list(qs)
    ss = [sim_opts.s] if ss is None else list(ss)
    seeds = np.asarray(list(seeds), dtype=np.int64)
    grid_q, grid_s = [], []
    for s in ss:
        for q in qs:
            grid_q.append(float(q))
            grid_s.append(g.s_matrix(s, 1)[0])
    qv = np.asarray(grid_q)
    sm = np.ascontiguousarray(np.stack(grid_s)) if grid_s and g.n_followers else \
        np.zeros((len(grid_q), g.n_followers))
    R = len(seeds)
    seed_t = torch.as_tensor(np.tile(seeds, len(grid_q)))
    res = g.run("opt", q=qv, s=sm, n_rep=R, ctrl_seed=seed_t, world_seed=seed_t,
                randomize=randomize, Ks=Ks, max_events=max_events, chunk=chunk)
    df = _frame(res, np.tile(seeds, len(grid_q)), np.repeat(qv, R), "Opt", Ks)
    df["s_idx"] = np.repeat(np.arange(len(grid_q)) // max(1, len(qs)), R)
    return df


def run_opt_vs_poisson(sim_opts, seeds=range(10), randomize=True, Ks=(1,), max_events=None,
                       poisson_seed_offset=0):
    """worker_opt then worker_poisson (opt_runs.py:51-126) for every seed: the
    Poisson broadcaster gets the RedQueen replica's capacity (posts) as
    rate = capacity / end_time on the same world; its seed is seed +
    poisson_seed_offset (0 = the reference's worker_poisson)."""
    g = compiled_graph(sim_opts)
    seeds = np.asarray(list(seeds), dtype=np.int64)
    st = torch.as_tensor(seeds)
    ro = g.run("opt", q=float(sim_opts.q), s=sim_opts.s, n_rep=len(seeds), ctrl_seed=st,
               world_seed=st, randomize=randomize, Ks=Ks, max_events=max_events)
    # capacity / end_time with IEEE division on the host (create_manager_with_poisson,
    # opt_model.py:829): torch's tensor / scalar multiplies by the reciprocal, which is
    # an ulp off for most capacities -- and every Poisson time with it
    rate = torch.as_tensor(ro.num_events.cpu().numpy().astype(np.float64) / float(sim_opts.end_time))
    rp = g.run("poisson", n_rep=len(seeds), ctrl_seed=st + int(poisson_seed_offset),
               world_seed=st, randomize=randomize, ctrl_rate=rate, Ks=Ks, max_events=max_events)
    a = _frame(ro, seeds, np.full(len(seeds), float(sim_opts.q)), "Opt", Ks)
    b = _frame(rp, seeds, np.full(len(seeds), float(sim_opts.q)), "Poisson", Ks)
    b["capacity"] = a["capacity"].values
    return pd.concat([a, b], ignore_index=True)


def run_significance(sim_opts, significance, time_period, seeds=range(10), randomize=True,
                     Ks=(1,), max_events=None, qs=None):
    """OptPWSignificance (create_manager_with_significance, opt_model.py:850-884) for
    every seed (x every q in qs): significance [sinks x segments] (or one row of
    segments for all followers); seed u runs world randomize_other_sources(u)."""
    from .opt_model import OptPWSignificance
    g = compiled_graph(sim_opts)
    qs = [sim_opts.q] if qs is None else list(qs)
    seeds = np.asarray(list(seeds), dtype=np.int64)
    spw = OptPWSignificance(sim_opts.src_id, 0, significance, time_period)._s_pw_for(g.n_followers)
    qv = np.asarray(qs, dtype=np.float64)
    # the reference raises (take_one_sample's int(nan)) in a run in which a source that
    # reaches no follower with positive significance actually posts: when such sources
    # exist, the batch keeps its event logs and every replica's log is checked
    from .opt_model import _sig_bad_sources, _sig_reach_check
    bad = set()
    for q in qv:
        bad |= _sig_bad_sources(g, sim_opts.edge_list, spw, float(q))
    R = len(seeds)
    seed_t = torch.as_tensor(np.tile(seeds, len(qv)))
    res = g.run("sig", q=qv, s_pw=spw, period=float(time_period), n_rep=R, ctrl_seed=seed_t,
                world_seed=seed_t, randomize=randomize, Ks=Ks, max_events=max_events,
                event_log=bool(bad))
    if bad:
        n = res.counts[:, 2].cpu().numpy()
        src = res.ev_src.cpu().numpy()
        ids = g.stream_src_ids
        for i in range(src.shape[0]):
            _sig_reach_check(g, sim_opts.edge_list, spw, 1.0, ids[src[i, :n[i]]], bad=bad,
                             max_events=max_events)
    return _frame(res, np.tile(seeds, len(qv)), np.repeat(qv, R), "OptPW", Ks)


def _seed_chunks(sim_opts, seeds, Ks, ctrl, randomize, chunk_replicas, run_kw, what):
    """The seed chunks of run_timeline / run_followers / run_rank_hist: yields the
    event-logged BatchResult of every chunk of ``chunk_replicas`` seeds (default: what a
    quarter of the free device memory holds of event logs), in seed order."""
    g = compiled_graph(sim_opts)
    seeds = np.asarray(list(seeds), dtype=np.int64)
    R = len(seeds)
    if R < 1:
        raise ValueError(what + ": no seeds")
    kw = dict(run_kw)
    if ctrl == "opt":
        kw.setdefault("q", float(sim_opts.q))
        kw.setdefault("s", sim_opts.s)
    rate = kw.pop("ctrl_rate", None)
    if rate is not None:
        rate = np.broadcast_to(np.asarray(rate, dtype=np.float64), (R,))
    if chunk_replicas is None:
        free, _total = torch.cuda.mem_get_info()
        probe = g.run(ctrl, n_rep=1, ctrl_seed=int(seeds[0]), world_seed=int(seeds[0]),
                      randomize=randomize, Ks=Ks, event_log=True,
                      **(dict(kw, ctrl_rate=rate[:1]) if rate is not None else kw))
        per = 12 * probe.ev_t.shape[1] * 2   # capacities double on overflow reruns
        chunk_replicas = max(1, min(R, int(free // 4 // max(1, per))))
    chunk_replicas = max(1, int(chunk_replicas))
    for a in range(0, R, chunk_replicas):
        sd = torch.as_tensor(seeds[a:a + chunk_replicas])
        ck = dict(kw, ctrl_rate=rate[a:a + chunk_replicas]) if rate is not None else kw
        yield g.run(ctrl, n_rep=len(sd), ctrl_seed=sd, world_seed=sd, randomize=randomize, Ks=Ks,
                    event_log=True, **ck)


def _mean_sem(v):
    """Mean and standard error (sample standard deviation / sqrt(n)) over the n leading
    entries of ``v`` [n, ...], summed in their order; NaN without entries, ``sem`` NaN for
    one."""
    n = v.shape[0]
    mean = np.full(v.shape[1:], np.nan)
    sem = np.full(v.shape[1:], np.nan)
    if n:
        tot = np.zeros(v.shape[1:])
        for r in range(n):          # fixed replica order
            tot = tot + v[r]
        mean = tot / n
        if n > 1:
            sq = np.zeros(v.shape[1:])
            for r in range(n):
                sq = sq + (v[r] - mean) ** 2
            sem = np.sqrt(sq / (n - 1)) / np.sqrt(n)
    return mean, sem


def run_timeline(sim_opts, seeds=range(10), bins=None, edges=None, Ks=(1,), ctrl="opt",
                 randomize=True, chunk_replicas=None, **run_kw):
    """The ensemble's metrics over time: one row per bin with ``t_lo``, ``t_hi`` and, for
    every metric (top_K..., avg_rank, r_2) and for own / other posts, the mean and the
    standard error over the replicas, plus ``n`` (replicas averaged) and ``n_flagged``
    (TIE / EMPTY replicas, left out).  Seed u runs as in run_grid: controller seed u and,
    with ``randomize``, the world randomize_other_sources(u).  The seeds run in chunks of
    ``chunk_replicas`` replicas (default: what a quarter of the free device memory holds
    of event logs); every chunk's per-bin values are gathered on the host and reduced in
    seed order, so the frame does not depend on the chunking.  ``run_kw`` goes to
    Graph.run (``ctrl_rate`` for ctrl="poisson", ``q`` / ``s`` override sim_opts')."""
    met, pst, sts = [], [], []
    tl = None
    for res in _seed_chunks(sim_opts, seeds, Ks, ctrl, randomize, chunk_replicas, run_kw, "run_timeline"):
        tl = res.timeline(edges=edges, bins=bins, Ks=Ks)
        met.append(tl.metrics.cpu().numpy())
        pst.append(tl.posts.cpu().numpy())
        sts.append(tl.status.cpu().numpy())
        del res
    return timeline_frame(tl.edges, tl.Ks, np.concatenate(met), np.concatenate(pst),
                          np.concatenate(sts))


def timeline_frame(edges, Ks, metrics, posts, status):
    """run_timeline's frame from per-replica values ([R, n_bins, nK + 2], [R, n_bins, 2],
    [R]): means and standard errors (sample standard deviation / sqrt(n)) over the
    replicas with status 0, summed in replica order."""
    ok = np.asarray(status) == 0
    n = int(ok.sum())
    names = ["top_" + str(k) for k in Ks] + ["avg_rank", "r_2", "own_posts", "other_posts"]
    vals = np.concatenate([np.asarray(metrics, dtype=np.float64)[ok],
                           np.asarray(posts)[ok].astype(np.float64)], axis=2)
    d = {"t_lo": np.asarray(edges[:-1]), "t_hi": np.asarray(edges[1:])}
    nb = len(edges) - 1
    mean, sem = _mean_sem(vals)
    for i, nm in enumerate(names):
        d[nm] = mean[:, i]
        d[nm + "_se"] = sem[:, i]
    d["n"] = np.full(nb, n, dtype=np.int64)
    d["n_flagged"] = np.full(nb, len(ok) - n, dtype=np.int64)
    return pd.DataFrame(d)


def run_followers(sim_opts, seeds=range(10), Ks=(1,), ctrl="opt", randomize=True,
                  chunk_replicas=None, tiled=None, **run_kw):
    """The ensemble's metrics per follower: one row per sink with ``sink_id`` and, for every
    metric (top_K..., rank_int, rank_sq_int: the integrals over the sink's seen span) and
    for its own / wall rows, the mean and the standard error over the replicas, plus ``n``
    (replicas averaged) and ``n_flagged`` (TIE / EMPTY replicas, left out).  Seeds, chunks
    and ``run_kw`` as in run_timeline: every chunk's per-sink values are gathered on the
    host and reduced in seed order, so the frame does not depend on the chunking.  ``tiled``
    goes to BatchResult.followers (None: the sink-tiled kernel past the plain one's limit)."""
    val, rws, sts = [], [], []
    fl = None
    for res in _seed_chunks(sim_opts, seeds, Ks, ctrl, randomize, chunk_replicas, run_kw, "run_followers"):
        fl = res.followers(Ks=Ks, rows=True, tiled=tiled)
        val.append(fl.vals.cpu().numpy())
        rws.append(fl.rows.cpu().numpy())
        sts.append(fl.status.cpu().numpy())
        del res
    return followers_frame(fl.sink_ids, fl.Ks, np.concatenate(val), np.concatenate(rws),
                           np.concatenate(sts))


def followers_frame(sink_ids, Ks, vals, rows, status):
    """run_followers' frame from per-replica values ([R, n_sinks, nK + 2], [R, n_sinks, 2],
    [R]): means and standard errors (sample standard deviation / sqrt(n)) over the
    replicas with status 0, summed in replica order."""
    ok = np.asarray(status) == 0
    n = int(ok.sum())
    names = ["top_" + str(k) for k in Ks] + ["rank_int", "rank_sq_int", "own_rows", "wall_rows"]
    v = np.concatenate([np.asarray(vals, dtype=np.float64)[ok],
                        np.asarray(rows)[ok].astype(np.float64)], axis=2)
    ns = len(sink_ids)
    d = {"sink_id": np.asarray(sink_ids, dtype=np.int64)}
    mean, sem = _mean_sem(v)
    for i, nm in enumerate(names):
        d[nm] = mean[:, i]
        d[nm + "_se"] = sem[:, i]
    d["n"] = np.full(ns, n, dtype=np.int64)
    d["n_flagged"] = np.full(ns, len(ok) - n, dtype=np.int64)
    return pd.DataFrame(d)


def run_sources(sim_opts, seeds=range(10), src_ids=None, scope="own", Ks=(1,), ctrl="opt", randomize=True,
                chunk_replicas=None, **run_kw):
    """The ensemble's metrics per source (BatchResult.source_metrics): returns
    (``frame``, ``summary``).  ``frame`` is long-form, one row per (replica, src_id), with
    ``replica`` (the seed's position), ``src_id``, the metrics (top_K..., avg_rank, r_2),
    ``num_events`` (the source's events with a row), ``other_events`` and ``status``;
    ``summary`` has one row per source with every metric's and count's mean and standard
    error over the replicas whose status is not ST_EMPTY, plus ``n`` and ``n_empty`` (ties
    are exact here, so ST_TIE replicas are averaged).  ``src_ids``: default the game's
    players, else every source of the graph; ``scope`` "own" (the source's followers' feeds)
    or "df".  Seeds, chunks and ``run_kw`` as in run_timeline: every chunk's values are
    gathered on the host and reduced in seed order."""
    met, cnt, sts = [], [], []
    sm = None
    for res in _seed_chunks(sim_opts, seeds, Ks, ctrl, randomize, chunk_replicas, run_kw, "run_sources"):
        sm = res.source_metrics(src_ids, scope=scope, Ks=Ks)
        met.append(sm.metrics.cpu().numpy())
        cnt.append(sm.counts.cpu().numpy())
        sts.append(sm.status.cpu().numpy())
        del res
    return sources_frame(sm.src_ids, sm.Ks, np.concatenate(met), np.concatenate(cnt), np.concatenate(sts))


def sources_frame(src_ids, Ks, metrics, counts, status):
    """run_sources' frames from per-replica values ([R, P, nK + 2], [R, P, 4], [R, P]):
    the long-form frame, and per source the means and standard errors (sample standard
    deviation / sqrt(n)) over the replicas that are not ST_EMPTY, summed in replica order."""
    from ._lib import ST_EMPTY
    metrics = np.asarray(metrics, dtype=np.float64)
    counts, status = np.asarray(counts), np.asarray(status)
    R, P = status.shape
    names = ["top_" + str(k) for k in Ks] + ["avg_rank", "r_2"]
    d = {"replica": np.repeat(np.arange(R, dtype=np.int64), P),
         "src_id": np.tile(np.asarray(src_ids, dtype=np.int64), R)}
    for i, nm in enumerate(names):
        d[nm] = metrics[:, :, i].reshape(-1)
    d["num_events"] = counts[:, :, 0].reshape(-1).astype(np.int64)
    d["other_events"] = counts[:, :, 1].reshape(-1).astype(np.int64)
    d["status"] = status.reshape(-1).astype(np.int64)
    frame = pd.DataFrame(d)
    v = np.concatenate([metrics, counts[:, :, :2].astype(np.float64)], axis=2)
    cols = names + ["num_events", "other_events"]
    s = {"src_id": np.asarray(src_ids, dtype=np.int64)}
    mean, sem = np.full((P, len(cols)), np.nan), np.full((P, len(cols)), np.nan)
    n = np.zeros(P, dtype=np.int64)
    for p in range(P):
        ok = (status[:, p] & ST_EMPTY) == 0
        n[p] = int(ok.sum())
        mean[p], sem[p] = _mean_sem(v[ok, p])
    for i, nm in enumerate(cols):
        s[nm] = mean[:, i]
        s[nm + "_se"] = sem[:, i]
    s["n"] = n
    s["n_empty"] = R - n
    return frame, pd.DataFrame(s)


def run_rank_hist(sim_opts, seeds=range(10), ranks=64, bins=None, edges=None, ctrl="opt",
                  randomize=True, chunk_replicas=None, **run_kw):
    """The ensemble's rank distribution over time: one row per (time bin, rank cell) with
    ``t_lo``, ``t_hi``, ``rank``, ``tail`` (the last cell: rank >= ``ranks``), the mean
    ``share`` of the seen sink-time and its standard error over the replicas, plus ``n``
    (replicas averaged) and ``n_flagged`` (TIE / EMPTY replicas, left out).  Seeds, chunks
    and ``run_kw`` as in run_timeline; ``bins`` / ``edges`` as in BatchResult.rank_hist
    (neither: one bin over the horizon).  Every chunk's histogram is gathered on the host
    and reduced in seed order, so the frame does not depend on the chunking."""
    hst, sts = [], []
    rh = None
    for res in _seed_chunks(sim_opts, seeds, (1,), ctrl, randomize, chunk_replicas, run_kw, "run_rank_hist"):
        rh = res.rank_hist(ranks=ranks, edges=edges, bins=bins)
        hst.append(rh.hist.cpu().numpy())
        sts.append(rh.status.cpu().numpy())
        del res
    return rank_hist_frame(rh.edges, rh.ranks, np.concatenate(hst), np.concatenate(sts))


def rank_hist_frame(edges, ranks, hist, status):
    """run_rank_hist's frame from per-replica values ([R, n_bins, ranks + 1], [R]): the
    mean and standard error (sample standard deviation / sqrt(n)) of every cell over the
    replicas with status 0, summed in replica order.  Rows: time bins outermost, the
    rank cells 0 .. ranks within (``tail`` marks the last)."""
    ok = np.asarray(status) == 0
    n = int(ok.sum())
    ranks = int(ranks)
    nb, nc = len(edges) - 1, ranks + 1
    v = np.asarray(hist, dtype=np.float64).reshape(-1, nb, nc)[ok]
    mean, sem = _mean_sem(v)
    cell = np.tile(np.arange(nc, dtype=np.int64), nb)
    return pd.DataFrame({"t_lo": np.repeat(np.asarray(edges[:-1], dtype=np.float64), nc),
                         "t_hi": np.repeat(np.asarray(edges[1:], dtype=np.float64), nc),
                         "rank": cell, "tail": cell == ranks,
                         "share": mean.reshape(-1), "share_se": sem.reshape(-1),
                         "n": np.full(nb * nc, n, dtype=np.int64),
                         "n_flagged": np.full(nb * nc, len(ok) - n, dtype=np.int64)})

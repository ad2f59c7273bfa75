"""The flat-window merge of <= 64 streams (rq_merge_flat, the default for 9-64 streams)
against the bucket rounds it replaces (RQ_MERGE_FLAT=0: rq_merge_streams<64>), the sweep
merging the per-source streams itself (sweep_mode 6) and the engine oracle.

Bar: bit-exact status, counts, metrics (NaN pattern included) and event logs.  The cases
sit at the kernel's own edges: stream counts around its 64 stream slots, stream lengths
around the run search's steps, window totals around its capacity, equal times below and
above that capacity, times at both ends of the horizon, the merged-capacity overflow.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 1024   # arrivals a window of rq_merge_flat holds (FCAP of the instance rq_launch_merge picks)


def _ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from redqueen_amd import engine, graphs
    from oracle import oracle as O
    return torch, engine, graphs, O


def _graph(engine, so):
    return engine.Graph(so["src_id"], so["other_sources"], so["sink_ids"], so["edge_list"],
                        so["end_time"])


def _same(torch, a, b, events=True):
    assert torch.equal(a.status, b.status)
    assert torch.equal(a.counts, b.counts)
    assert torch.equal(a.metrics.isnan(), b.metrics.isnan())
    assert torch.equal(a.metrics.nan_to_num(), b.metrics.nan_to_num())
    if events and a.ev_t is not None:
        for i in range(a.counts.shape[0]):
            ta, sa = a.events(i)
            tb, sb = b.events(i)
            assert np.array_equal(ta, tb) and np.array_equal(sa, sb), i


def _world(graphs, n_str, rd=(), end_time=10.0, rate=1.0, n_fol=12, seed=3, alpha=1.0, beta=10.0,
           n_base=None):
    """A followers_graph world (Poisson2 + Hawkes walls) brought to exactly n_str streams:
    the RealData sources `rd` (lists of times) and then silent Poisson sources (no arrival
    in any replica) are added, each followed by one of the followers."""
    n_base = n_str - len(rd) if n_base is None else n_base
    so = graphs.followers_graph(num_followers=n_fol, num_sources=n_base, degree=3, end_time=end_time,
                                kinds=("Poisson2", "Hawkes"), world_rate=rate, alpha=alpha, beta=beta,
                                seed=seed, network_seed=seed + 1)
    others, edges, sinks = list(so["other_sources"]), list(so["edge_list"]), so["sink_ids"]
    sid = 9000
    for times in rd:
        others.append(("RealData", {"src_id": sid, "times": [float(t) for t in times]}))
        edges.append((sid, sinks[sid % len(sinks)]))
        sid += 1
    while len(others) < n_str:
        others.append(("Poisson", {"src_id": sid, "seed": sid, "rate": 1e-9}))
        edges.append((sid, sinks[sid % len(sinks)]))
        sid += 1
    assert len(others) == n_str, (len(others), n_str)
    so.update(other_sources=others, edge_list=edges)
    return so


def _flat_off(monkeypatch, f):
    monkeypatch.setenv("RQ_MERGE_FLAT", "0")
    try:
        return f()
    finally:
        monkeypatch.delenv("RQ_MERGE_FLAT")


def _oracle_reps(O, so, res, reps, seed, Ks):
    from tests.test_gpu_engine import _world_with_seeds
    for r in reps:
        u = seed + r
        met, (t_o, _, s_o) = O.engine_metrics(O.Scenario(_world_with_seeds(so, u), ("opt", u)), Ks)
        t, s = res.events(r)
        assert np.array_equal(t, t_o) and np.array_equal(s, s_o), r
        top, avg, r2, _ = met
        assert np.array_equal(res.metrics[r].cpu().numpy(), np.asarray(list(top) + [avg, r2])), r


def _four_way(torch, monkeypatch, O, engine, so, n_rep, oracle_reps=(), seed=77, Ks=(1, 2), events=True):
    """default (flat) == RQ_MERGE_FLAT=0 (bucket rounds) == sweep_mode 6, with and without
    the event log, and == the engine oracle on oracle_reps."""
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=n_rep, ctrl_seed=seed, world_seed=seed, randomize=True, Ks=Ks)
    assert g.run("opt", plan_only=True, **kw)["sources_per_lane"] == 0   # merged streams
    a = g.run("opt", **kw)
    _same(torch, a, _flat_off(monkeypatch, lambda: g.run("opt", **kw)))
    _same(torch, a, g.run("opt", sweep_mode=6, **kw))
    if events:
        a = g.run("opt", event_log=True, **kw)
        _same(torch, a, _flat_off(monkeypatch, lambda: g.run("opt", event_log=True, **kw)))
        _same(torch, a, g.run("opt", event_log=True, sweep_mode=6, **kw))
        _oracle_reps(O, so, a, oracle_reps, seed, Ks)
    return a


@pytest.mark.parametrize("n_str", [9, 33, 51, 64])
def test_stream_counts(n_str, monkeypatch):
    """9, 33, 51 and 64 streams: some with no arrival in any replica (the silent ones, and
    at rate 0.3 over T = 10 many of the others in a given replica), one with exactly one."""
    torch, engine, graphs, O = _ctx()
    so = _world(graphs, n_str, rd=[[4.375]], rate=0.3, n_base=min(n_str - 3, 48))
    a = _four_way(torch, monkeypatch, O, engine, so, 96, oracle_reps=(0, 95))
    assert int(a.status.max().item()) == 0


def test_all_streams_empty(monkeypatch):
    """Replicas whose streams are all empty (out_len 0), next to replicas with one or two
    arrivals: 9 streams of rate 0.02 over T = 2."""
    torch, engine, graphs, O = _ctx()
    so = _world(graphs, 9, rate=0.02, end_time=2.0, n_base=7)
    a = _four_way(torch, monkeypatch, O, engine, so, 64, oracle_reps=(0, 1, 63))
    n_ev = [len(a.events(i)[0]) for i in range(64)]   # the controller's own post at 0.0 is always there
    assert min(n_ev) == 1 and max(n_ev) > 1   # nothing to merge in some replicas, something in others


@pytest.mark.parametrize("n", [15, 16, 17, 63, 64, 65, 129])
def test_stream_lengths(n, monkeypatch):
    """One replayed stream of 15 ... 129 arrivals (the run search's steps, the 64 lanes of a
    pass) among 32 generated ones."""
    torch, engine, graphs, O = _ctx()
    so = _world(graphs, 33, rd=[np.linspace(0.25, 9.75, n)], rate=0.5)
    _four_way(torch, monkeypatch, O, engine, so, 8, oracle_reps=(0,))


def _replayed(n_total, lo, hi, end_time=10.0, n_str=9, extra=()):
    """n_total distinct times in [lo, hi] dealt unevenly to n_str RealData streams."""
    t = np.linspace(lo, hi, n_total)
    own = np.random.RandomState(n_total).randint(0, n_str + 3, n_total) % n_str   # streams 0-2 heavier
    rd = [t[own == j] for j in range(n_str)]
    return dict(src_id=1, end_time=end_time, s=np.asarray([1.0, 2.0, 0.5]), q=0.7, sink_ids=[10, 11, 12],
                other_sources=[("RealData", {"src_id": 100 + j, "times": list(map(float, rd[j])) + list(extra)})
                               for j in range(n_str)],
                edge_list=[(1, 10), (1, 11), (1, 12)] + [(100 + j, 10 + j % 3) for j in range(n_str)])


def _fixed_world_check(torch, monkeypatch, O, engine, so, Ks=(1, 2)):
    """A world of replayed streams only (every replica merges the same sequence): flat ==
    bucket rounds == sweep_mode 6 == the oracle."""
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=2, ctrl_seed=4, Ks=Ks, event_log=True)
    assert g.run("opt", plan_only=True, **kw)["sources_per_lane"] == 0
    a = g.run("opt", **kw)
    _same(torch, a, _flat_off(monkeypatch, lambda: g.run("opt", **kw)))
    _same(torch, a, g.run("opt", sweep_mode=6, **kw))
    assert int(a.status.max().item()) == 0
    met, (t_o, _, s_o) = O.engine_metrics(O.Scenario(so, ("opt", 4)), Ks)
    t, s = a.events(0)
    assert np.array_equal(t, t_o) and np.array_equal(s, s_o)
    top, avg, r2, _ = met
    assert np.array_equal(a.metrics[0].cpu().numpy(), np.asarray(list(top) + [avg, r2]))
    return a


@pytest.mark.parametrize("total", [CAP - 1, CAP, CAP + 1, 2 * CAP + 500])
def test_window_capacity(total, monkeypatch):
    """Replica totals of CAP - 1, CAP, CAP + 1 and above 2 CAP, all inside [1, 1.001] of a
    T = 10 horizon: the first cut (aimed at the replica's mean rate) takes them all, so the
    window holds one short of the capacity, exactly the capacity, or is retried with halved
    spans; the largest total takes several windows."""
    torch, engine, graphs, O = _ctx()
    _fixed_world_check(torch, monkeypatch, O, engine, _replayed(total, 1.0, 1.001))


def test_bursty_retried_window(monkeypatch):
    """A bursty Hawkes world (alpha 1.5, beta 2.5) of ~7000 arrivals per replica with a
    replayed burst of 3000 arrivals in [20, 20.5]: the window that runs into the burst
    holds more than the capacity and is retried with a halved span."""
    torch, engine, graphs, O = _ctx()
    so = _world(graphs, 12, rd=[np.linspace(20.0, 20.5, 3000)], end_time=40.0, rate=6.0, alpha=1.5, beta=2.5,
                seed=5, n_base=10)
    _four_way(torch, monkeypatch, O, engine, so, 6, oracle_reps=(0,), Ks=(1, 3))


def _tie_streams(n_each, at, end_time=20.0, n_str=9):
    """n_str replayed streams with n_each entries at `at` each, among distinct others."""
    so = _replayed(330, 0.5, 19.5, end_time=end_time, n_str=n_str, extra=[float(at)] * n_each)
    return so


def _events_equal(a, b, n):
    for i in range(n):
        ta, sa = a.events(i)
        tb, sb = b.events(i)
        assert np.array_equal(ta, tb) and np.array_equal(sa, sb), i


@pytest.mark.parametrize("at", [0.0, 5.0, 20.0])
def test_equal_times_below_capacity(at, monkeypatch):
    """9 replayed streams with 40 entries at one time each (360 < CAP; at 0.0, inside, and at
    end_time, where the window is one ulp wide): the merge orders them exactly -- stream,
    then position -- so the merged sweeps (modes 5 and 1) play the events of the exact
    sequential sweep (mode 2).  The bucket rounds (256 per round) cannot, and flag it.
    (RQ_ST_TIE itself is no evidence here: the fast sweeps flag any equal times.)"""
    torch, engine, graphs, O = _ctx()
    so = _tie_streams(40, at)
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=3, ctrl_seed=2, Ks=(1, 3), event_log=True, check=False)
    a = g.run("opt", sweep_mode=5, **kw)
    _events_equal(a, g.run("opt", sweep_mode=2, **kw), 3)
    b = g.run("opt", sweep_mode=1, **kw)
    _events_equal(a, b, 3)
    assert torch.equal(a.counts, b.counts) and torch.equal(a.metrics, b.metrics)


@pytest.mark.parametrize("at", [0.0, 5.0])
def test_more_than_capacity_at_one_time(at, monkeypatch):
    """9 replayed streams of 400 equal times each (3600 > 3 CAP; at 0.0 the window is the one
    ulp above t_lo = 0, whose bucket scale is not finite): emitted CAP at a time and flagged
    RQ_ST_TIE; with check=True the engine reruns on the exact sequential sweep, so the
    result equals sweep_mode 2 and the oracle."""
    torch, engine, graphs, O = _ctx()
    so = _tie_streams(400, at)
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=2, ctrl_seed=4, Ks=(1, 2), sweep_mode=5)
    a = g.run("opt", check=False, **kw)
    assert int(a.status[0].item()) & 4 and int(a.status[1].item()) & 4
    assert int(a.counts[0].sum().item()) > 0
    b = g.run("opt", **kw)
    c = g.run("opt", **dict(kw, sweep_mode=2))
    _same(torch, b, c, events=False)
    met, _ = O.engine_metrics(O.Scenario(so, ("opt", 4)), (1, 2))
    top, avg, r2, _ = met
    assert np.array_equal(b.metrics[0].cpu().numpy(), np.asarray(list(top) + [avg, r2]))


def test_times_at_the_ends_of_the_horizon(monkeypatch):
    """Arrivals at 0.0 and exactly at end_time (distinct streams' single entries there, so
    the default plan stays on the fast merged sweep), and a world whose only arrivals are
    at end_time (t_lo = end: the window is one ulp wide)."""
    torch, engine, graphs, O = _ctx()
    so = _world(graphs, 33, rd=[[0.0, 2.5, 7.5], [1.25, 10.0]], rate=0.5)
    _four_way(torch, monkeypatch, O, engine, so, 8, oracle_reps=(0, 7))
    so = _replayed(40, 1.0, 9.0, n_str=9)
    so["other_sources"] = [("RealData", {"src_id": 100 + j, "times": [10.0]}) if j == 4 else
                           ("Poisson", {"src_id": 100 + j, "seed": 50 + j, "rate": 1e-9}) for j in range(9)]
    _fixed_world_check(torch, monkeypatch, O, engine, so)


def test_merged_capacity_overflow(monkeypatch):
    """Undersized merged capacity (RQ_CAP_SQUEEZE): the merge flags RQ_ST_STREAM_OVERFLOW and
    stops; the engine's rerun at doubled capacity gives the unsqueezed result."""
    torch, engine, graphs, O = _ctx()
    from redqueen_amd import _lib as L
    so = _world(graphs, 33, rate=2.0, n_base=33)
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=200, ctrl_seed=11, world_seed=11, randomize=True, Ks=(1, 2))
    want = g.run("opt", **kw)
    assert int(want.status.max().item()) == 0
    monkeypatch.setenv("RQ_CAP_SQUEEZE", "0.45")
    raw = g.run("opt", check=False, **kw)
    assert int(((raw.status & L.ST_STREAM_OVERFLOW) != 0).sum().item()) > 0
    got = g.run("opt", **kw)
    monkeypatch.delenv("RQ_CAP_SQUEEZE")
    _same(torch, got, want)


def test_poisson_controlled(monkeypatch):
    """A Poisson2-controlled run: the controlled stream is one of the merged streams."""
    torch, engine, graphs, O = _ctx()
    so = _world(graphs, 33, rd=[np.linspace(0.5, 9.5, 40)], rate=1.0)
    g = _graph(engine, so)
    rates = torch.linspace(0.0, 6.0, 64, dtype=torch.float64)
    kw = dict(n_rep=64, ctrl_seed=3, world_seed=3, randomize=True, ctrl_rate=rates, Ks=(1, 3))
    assert g.run("poisson", plan_only=True, **kw)["sources_per_lane"] == 0
    for ev in (False, True):
        a = g.run("poisson", event_log=ev, **kw)
        _same(torch, a, _flat_off(monkeypatch, lambda: g.run("poisson", event_log=ev, **kw)))
        _same(torch, a, g.run("poisson", event_log=ev, sweep_mode=6, **kw))


_BATCH = {}


def _batch_world(torch, engine, graphs):
    """The 51-stream, T = 10 world of the batch-shape cases and its 3000-replica result,
    computed once (nobody writes it)."""
    if not _BATCH:
        so = _world(graphs, 51, rd=[np.linspace(0.1, 9.9, 70)], rate=1.0, n_fol=20, n_base=50)
        g = _graph(engine, so)
        kw = dict(q=so["q"], s=so["s"], n_rep=3000, ctrl_seed=77, world_seed=77, randomize=True, Ks=(1,))
        _BATCH.update(so=so, g=g, kw=kw, full=g.run("opt", chunk=3000, **kw))
    return _BATCH["so"], _BATCH["g"], _BATCH["kw"], _BATCH["full"]


def test_batch_one_replica(monkeypatch):
    torch, engine, graphs, O = _ctx()
    so, g, kw, full = _batch_world(torch, engine, graphs)
    _four_way(torch, monkeypatch, O, engine, so, 1, oracle_reps=(0,), Ks=(1,))


def test_batch_more_replicas_than_resident_blocks(monkeypatch):
    """3,000 replicas in one chunk: more blocks than the chip holds at once."""
    torch, engine, graphs, O = _ctx()
    so, g, kw, full = _batch_world(torch, engine, graphs)
    assert g.run("opt", chunk=3000, plan_only=True, **kw)["sources_per_lane"] == 0
    assert int(full.status.max().item()) == 0
    _same(torch, full, _flat_off(monkeypatch, lambda: g.run("opt", chunk=3000, **kw)))
    _same(torch, full, g.run("opt", chunk=3000, sweep_mode=6, **kw))


def test_batch_chunks_and_replica_list(monkeypatch):
    """chunk=700 against one chunk, and a rep_idx list against those rows of the batch."""
    torch, engine, graphs, O = _ctx()
    so, g, kw, full = _batch_world(torch, engine, graphs)
    _same(torch, full, g.run("opt", chunk=700, **kw))
    pick = [2999, 0, 1500, 701, 700, 64]
    sub = g.run("opt", rep_idx=pick, **kw)
    at = torch.tensor(pick, device=full.counts.device)
    assert torch.equal(sub.status, full.status[at]) and torch.equal(sub.counts, full.counts[at])
    assert torch.equal(sub.metrics.isnan(), full.metrics[at].isnan())
    assert torch.equal(sub.metrics.nan_to_num(), full.metrics[at].nan_to_num())

"""The generator's kernels per class of source kinds (rq_gen_hawkes, rq_gen_poisson and
rq_gen_streams for the rest: RQ_GEN_SPLIT=1, the default) against the one kernel for every
stream (RQ_GEN_SPLIT=0) and the engine oracle.

Bar: bit-exact status, counts, metrics (NaN pattern included) and event logs.  The event log
of a merged-stream run holds every arrival of every stream, so stream j of replica i is the
log's events of source j: its length is the stream's slen, its times the stream's arrivals.

The cases sit at the kernels' own edges: stream lengths around the 16-slot chunks of the
Poisson kernel and the staging window of the Hawkes kernel (worlds found with the CPU oracle,
which asserts them here), streams that are done before their first draw, batch sizes around
the 64-lane wave and the 256-lane block, graphs of one, two and three classes with the class
lists interleaved in stream order, the controlled stream as a Poisson broadcaster, the ways a
replica gets its seeds, streams and merged sequences at their capacity.
"""
import numpy as np
import pytest

from tests.test_gpu_engine import _world_with_seeds
from tests.test_gpu_merge_flat import _ctx, _graph, _oracle_reps, _same, _world

pytestmark = pytest.mark.gpu

ST_STREAM_OVERFLOW = 2


def _both(torch, monkeypatch, run, events=True):
    """RQ_GEN_SPLIT=1 == RQ_GEN_SPLIT=0 for one way of running; the split result."""
    monkeypatch.setenv("RQ_GEN_SPLIT", "1")
    try:
        a = run()
        monkeypatch.setenv("RQ_GEN_SPLIT", "0")
        b = run()
    finally:
        monkeypatch.delenv("RQ_GEN_SPLIT")
    _same(torch, a, b, events)
    return a


def _merged(g, ctrl="opt", **kw):
    p = g.run(ctrl, plan_only=True, **kw)
    # streams from the generator: the fused sweep on merged streams, or the general sweep on them
    assert p["variant"] >= 20 or p["sources_per_lane"] == 0, p


def _check(torch, monkeypatch, O, engine, so, n_rep, oracle_reps, seed=77, Ks=(1, 2), randomize=True, **extra):
    """Both knob values with and without the event log, and the oracle on oracle_reps."""
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=n_rep, ctrl_seed=seed, world_seed=seed, randomize=randomize, Ks=Ks, **extra)
    _merged(g, **kw)
    _both(torch, monkeypatch, lambda: g.run("opt", **kw), events=False)
    a = _both(torch, monkeypatch, lambda: g.run("opt", event_log=True, **kw))
    if randomize:
        _oracle_reps(O, so, a, oracle_reps, seed, Ks)
    else:
        for r in oracle_reps:
            met, (t_o, _, s_o) = O.engine_metrics(O.Scenario(so, ("opt", seed + r)), Ks)
            t, s = a.events(r)
            assert np.array_equal(t, t_o) and np.array_equal(s, s_o), r
            top, avg, r2, _ = met
            assert np.array_equal(a.metrics[r].cpu().numpy(), np.asarray(list(top) + [avg, r2])), r
    return a


# ---- staging edges ----

def _edges_world(T):
    """A Poisson and a Hawkes source of about one arrival per time unit, and one of each that
    is done at init (rate 0, l_0 = 0)."""
    return dict(src_id=1, end_time=T, s=np.asarray([1.0, 1.0]), q=1.0, sink_ids=[10, 11],
                other_sources=[("Poisson", {"src_id": 2, "seed": 1, "rate": 1.0}),
                               ("Hawkes", {"src_id": 3, "seed": 2, "l_0": 0.9, "alpha": 1.0, "beta": 10.0}),
                               ("Poisson2", {"src_id": 4, "seed": 3, "rate": 0.0}),
                               ("Hawkes", {"src_id": 5, "seed": 4, "l_0": 0.0, "alpha": 1.0, "beta": 10.0})],
                edge_list=[(1, 10), (1, 11), (2, 10), (3, 11), (4, 10), (5, 11)])


# horizon -> the stream lengths both live sources must show among 256 replicas from seed 5
EDGE_LENGTHS = {0.75: (0, 1), 8.0: (7, 8, 9), 16.0: (15, 16, 17), 32.0: (31, 32, 33), 100.0: ()}


@pytest.mark.parametrize("T", sorted(EDGE_LENGTHS))
def test_staging_edges(T, monkeypatch):
    """Stream lengths 0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33 and about 100 (16 and 32: the
    horizon ends the stream right after a full chunk) of a Poisson and a Hawkes source, beside
    a Poisson source of rate 0 and a Hawkes source of l_0 = 0; every replica against the oracle."""
    torch, engine, graphs, O = _ctx()
    so, R, seed0 = _edges_world(T), 256, 5
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=R, ctrl_seed=seed0, world_seed=seed0, randomize=True, Ks=(1,))
    _merged(g, **kw)
    fast = _both(torch, monkeypatch, lambda: g.run("opt", **kw), events=False)
    log = _both(torch, monkeypatch, lambda: g.run("opt", event_log=True, **kw))
    assert int(log.status.max().item()) == 0 and int(fast.status.max().item()) == 0
    assert torch.equal(fast.counts, log.counts)
    lens = np.zeros((R, 4), dtype=np.int64)
    for i in range(R):
        u = seed0 + i
        t_o, _, s_o = O.engine_run(O.Scenario(_world_with_seeds(so, u), ("opt", u)), cap=1 << 14)
        t, s = log.events(i)
        assert np.array_equal(s, s_o) and np.array_equal(t, t_o), i
        lens[i] = [int((s == sid).sum()) for sid in (2, 3, 4, 5)]
    for k in (0, 1):
        for n in EDGE_LENGTHS[T]:
            assert (lens[:, k] == n).any(), (k, n)
        if T == 100.0:
            assert ((lens[:, k] >= 95) & (lens[:, k] <= 105)).any(), k
    assert not lens[:, 2:].any()   # done at init
    for i in (0, R - 1, int(np.argmax(lens[:, 0])), int(np.argmin(lens[:, 1]))):
        u = seed0 + i
        (top, avg, r2, _), _ = O.engine_metrics(O.Scenario(_world_with_seeds(so, u), ("opt", u)), (1,))
        assert np.array_equal(fast.metrics[i].cpu().numpy(), np.asarray(list(top) + [avg, r2])), i


# ---- block and wave edges ----

def _c3_cut(graphs):
    """A 4-source cut of C3: two Poisson2 and two Hawkes broadcasters, 12 followers."""
    so = graphs.followers_graph(num_followers=12, num_sources=4, degree=3, end_time=20.0)
    assert sorted(k for k, _ in so["other_sources"]) == ["Hawkes", "Hawkes", "Poisson2", "Poisson2"]
    return so


@pytest.mark.parametrize("n_rep", [1, 63, 64, 65, 255, 256, 257, 513])
def test_block_and_wave_edges(n_rep, monkeypatch):
    torch, engine, graphs, O = _ctx()
    a = _check(torch, monkeypatch, O, engine, _c3_cut(graphs), n_rep, sorted({0, n_rep // 2, n_rep - 1}))
    assert int(a.status.max().item()) == 0


# ---- classes ----

def _interleaved():
    """Every source kind, ordered so that no class is contiguous in stream order (dynamic
    sources by src_id, then the static ones): H P H | G G P ctrl."""
    return dict(src_id=1, end_time=40.0, s=np.asarray([1.0, 2.0, 0.5]), q=2.0, sink_ids=[10, 11, 12, 13],
                other_sources=[("PiecewiseConst", {"src_id": 4, "seed": 9, "change_times": [0.0, 10.0, 30.0],
                                                   "rates": [2.0, 8.0, 1.0]}),
                               ("Poisson", {"src_id": 5, "seed": 10, "rate": 3.0}),
                               ("RealData", {"src_id": 6, "times": [0.5, 7.25, 7.5, 33.0, 39.0, 60.0]}),
                               ("Hawkes", {"src_id": 7, "seed": 11, "l_0": 1.5, "alpha": 0.5, "beta": 2.0}),
                               ("Hawkes", {"src_id": 3, "seed": 12, "l_0": 0.5, "alpha": 1.0, "beta": 4.0}),
                               ("Poisson2", {"src_id": 8, "seed": 13, "rate": 1.5})],
                edge_list=[(1, 10), (1, 11), (1, 12), (4, 10), (4, 13), (5, 11), (5, 12), (6, 10), (6, 11),
                           (6, 12), (6, 13), (7, 12), (7, 13), (3, 10), (8, 11), (8, 13)])


def _world_of(graphs, name):
    if name == "poisson_only":
        return graphs.kat_two_walls((0.5, 1.5))
    if name == "readme":
        return graphs.readme()
    if name == "hawkes_only":
        return graphs.followers_graph(num_followers=8, num_sources=4, degree=2, end_time=30.0, kinds=("Hawkes",),
                                      world_rate=0.5, alpha=1.0, beta=2.0)
    if name == "all_kinds_interleaved":
        return _interleaved()
    if name == "c5_small":
        return graphs.c5_small()
    return graphs.g120()   # more than 64 sources: the general sweep


@pytest.mark.parametrize("name", ["poisson_only", "readme", "hawkes_only", "all_kinds_interleaved", "c5_small", "g120"])
@pytest.mark.parametrize("randomize", [False, True])
def test_classes(name, randomize, monkeypatch):
    """Graphs of one class (an empty class launches nothing), two and all three; the fixed
    seeds of the sources and the randomized ones."""
    torch, engine, graphs, O = _ctx()
    so = _world_of(graphs, name)
    kinds = {k for k, _ in so["other_sources"]}
    if name == "poisson_only":
        assert kinds <= {"Poisson", "Poisson2"}
    if name in ("hawkes_only", "c5_small"):
        assert kinds == {"Hawkes"}
    if name == "g120":
        assert len(so["other_sources"]) > 64
    a = _check(torch, monkeypatch, O, engine, so, 70, (0, 69), seed=31, randomize=randomize)
    assert int(a.status.max().item()) == 0


def test_controlled_poisson_broadcaster(monkeypatch):
    """The controlled stream in class P: a Poisson broadcaster with per-replica rates (0 among
    them), beside a P and an H wall stream and alone in its class (a Hawkes-only wall)."""
    torch, engine, graphs, O = _ctx()
    rates = torch.tensor([4.0, 0.0, 9.5, 1.25, 0.16, 1.0, 30.0], dtype=torch.float64)
    for so in (graphs.readme(), _world_of(graphs, "hawkes_only")):
        g = _graph(engine, so)
        kw = dict(n_rep=len(rates), ctrl_seed=7, ctrl_rate=rates, Ks=(1,))
        _merged(g, "poisson", **kw)
        _both(torch, monkeypatch, lambda: g.run("poisson", **kw), events=False)
        a = _both(torch, monkeypatch, lambda: g.run("poisson", event_log=True, **kw))
        assert int(a.status.max().item()) == 0
        for r in range(len(rates)):
            met, (t_o, _, s_o) = O.engine_metrics(O.Scenario(so, ("poisson", 7 + r, float(rates[r]))), (1,))
            t, s = a.events(r)
            assert np.array_equal(t, t_o) and np.array_equal(s, s_o), r
            top, avg, r2, _ = met
            assert np.array_equal(a.metrics[r].cpu().numpy(), np.asarray(list(top) + [avg, r2])), r


# ---- seeds ----

def test_seed_mod_grid_and_replica_list(monkeypatch):
    """A q grid over the README graph with seed_mod = n_rep (replica r of every grid point runs
    seed r, as C4's grid does), and a rep_idx list against those rows of the batch."""
    torch, engine, graphs, O = _ctx()
    so = graphs.readme()
    g = _graph(engine, so)
    qs = np.asarray([0.01, 1.0, 30.0])
    sm = np.asarray([[1.0, 1.0], [0.5, 1.5], [1.5, 0.25]])
    kw = dict(q=qs, s=sm, n_rep=5, ctrl_seed=40, world_seed=40, randomize=True, seed_mod=5, Ks=(1, 2))
    _merged(g, **kw)
    _both(torch, monkeypatch, lambda: g.run("opt", **kw), events=False)
    full = _both(torch, monkeypatch, lambda: g.run("opt", event_log=True, **kw))
    for gi in range(3):
        for r in (0, 4):
            u = 40 + r
            sog = _world_with_seeds(dict(so, q=float(qs[gi]), s=sm[gi]), u)
            met, (t_o, _, s_o) = O.engine_metrics(O.Scenario(sog, ("opt", u)), (1, 2))
            t, s = full.events(gi * 5 + r)
            assert np.array_equal(t, t_o) and np.array_equal(s, s_o), (gi, r)
            top, avg, r2, _ = met
            assert np.array_equal(full.metrics[gi * 5 + r].cpu().numpy(), np.asarray(list(top) + [avg, r2])), (gi, r)
    pick = [14, 0, 7, 5, 9]
    sub = _both(torch, monkeypatch, lambda: g.run("opt", rep_idx=pick, **kw), events=False)
    at = torch.tensor(pick, device=full.counts.device)
    assert torch.equal(sub.status, full.status[at]) and torch.equal(sub.counts, full.counts[at])
    assert torch.equal(sub.metrics.isnan(), full.metrics[at].isnan())
    assert torch.equal(sub.metrics.nan_to_num(), full.metrics[at].nan_to_num())


# ---- overflow ----

def test_merged_capacity_overflow(monkeypatch):
    """Undersized capacities (RQ_CAP_SQUEEZE): some replicas of the batch pass them.  The
    unchecked results, RQ_ST_STREAM_OVERFLOW bits included, are equal under both knob values,
    and the checked rerun gives the unsqueezed result under both."""
    torch, engine, graphs, O = _ctx()
    so = _world(graphs, 33, rate=2.0, n_base=33)
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=200, ctrl_seed=11, world_seed=11, randomize=True, Ks=(1, 2))
    want = g.run("opt", **kw)
    assert int(want.status.max().item()) == 0
    monkeypatch.setenv("RQ_CAP_SQUEEZE", "0.45")
    for ev in (False, True):
        raw = _both(torch, monkeypatch, lambda: g.run("opt", check=False, event_log=ev, **kw))
        assert int(((raw.status & ST_STREAM_OVERFLOW) != 0).sum().item()) > 0
    got = _both(torch, monkeypatch, lambda: g.run("opt", **kw), events=False)
    monkeypatch.delenv("RQ_CAP_SQUEEZE")
    _same(torch, got, want)
    _oracle_reps(O, so, g.run("opt", event_log=True, **kw), (0, 199), 11, (1, 2))


def test_stream_capacity_overflow(monkeypatch):
    """A supercritical Hawkes source whose stream passes its own capacity in some replicas
    (the generator's overflow: the stream is cut at the capacity, the replica flagged) beside
    a Poisson source: the same flags, prefixes and results under both knob values; the
    replicas that fit are the oracle's."""
    torch, engine, graphs, O = _ctx()
    so = dict(src_id=1, end_time=4.0, s=np.asarray([1.0]), q=100.0, sink_ids=[10],
              other_sources=[("Hawkes", {"src_id": 2, "seed": 1, "l_0": 2.0, "alpha": 3.5, "beta": 1.0}),
                             ("Poisson", {"src_id": 3, "seed": 2, "rate": 1.0})],
              edge_list=[(1, 10), (2, 10), (3, 10)])
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=64, ctrl_seed=5, world_seed=5, randomize=True, Ks=(1,))
    _merged(g, **kw)
    _both(torch, monkeypatch, lambda: g.run("opt", check=False, **kw), events=False)
    log = _both(torch, monkeypatch, lambda: g.run("opt", check=False, event_log=True, **kw))
    over = (log.status.cpu().numpy() & ST_STREAM_OVERFLOW) != 0
    assert over.sum() >= 8 and (~over).sum() >= 8
    _oracle_reps(O, so, log, [int(i) for i in np.flatnonzero(log.status.cpu().numpy() == 0)[:6]], 5, (1,))


# ---- the fused sweep's own generation ----

def test_fused_sweep_generates_the_same_streams(monkeypatch):
    """sweep_mode 7 (the fused sweep calls SrcGen::step itself, untouched by the knob) equals
    the merged path fed by the class kernels, and the oracle."""
    torch, engine, graphs, O = _ctx()
    so = _c3_cut(graphs)
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=70, ctrl_seed=9, world_seed=9, randomize=True, Ks=(1, 2), event_log=True)
    a = _both(torch, monkeypatch, lambda: g.run("opt", **kw))
    _same(torch, a, _both(torch, monkeypatch, lambda: g.run("opt", sweep_mode=7, **kw)))
    _oracle_reps(O, so, a, (0, 69), 9, (1, 2))

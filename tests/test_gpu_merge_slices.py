"""The flat merge's slice table (rq_merge_flat with windows cut from per-slice counts, the
default for 9-64 streams) against its own search loop (RQ_FLAT_SLICES=0), the bucket rounds
(RQ_MERGE_FLAT=0), the sweep merging the streams itself (sweep_mode 6) and the engine oracle.

Bar: bit-exact status, counts, metrics (NaN pattern included) and event logs.  The cases sit
at the table's own edges: the first time of a slice, the times one ulp below and above it
(found with the kernel's own slice expression), slice and window totals around the window's capacity,
the replicas that must leave the table for the search loop (a slice over the capacity, equal
times), both kinds of replica in one launch, the merged-capacity overflow, the batch shapes.
"""
import numpy as np
import pytest

from tests.test_gpu_merge_flat import (CAP, _ctx, _events_equal, _graph, _oracle_reps, _replayed, _same,
                                       _tie_streams, _world)

pytestmark = pytest.mark.gpu

NB = 16   # slices of the table (RQ_FLAT_NB of the instance rq_launch_merge picks)


def _slice_of(t, t_min, end):
    """The slice of [t_min, end] a time falls in: the kernel's expression, in f64 (products
    and differences rounded one by one)."""
    t = np.asarray(t, dtype=np.float64)
    inv = np.float64(NB) / (np.float64(end) - np.float64(t_min))
    return np.minimum(((t - np.float64(t_min)) * inv).astype(np.int64), NB - 1)


def _bnd(t_min, end, b):
    """The first f64 time of slice b (1 <= b < NB): the boundary as the kernel draws it."""
    t = np.float64(t_min + (end - t_min) * (float(b) / float(NB)))
    while _slice_of(t, t_min, end) >= b:
        t = np.nextafter(t, -np.inf)
    while _slice_of(t, t_min, end) < b:
        t = np.nextafter(t, np.inf)
    return float(t)


def _with_env(monkeypatch, name, f):
    monkeypatch.setenv(name, "0")
    try:
        return f()
    finally:
        monkeypatch.delenv(name)


def _legs(torch, monkeypatch, run, events=True):
    """default == RQ_FLAT_SLICES=0 == RQ_MERGE_FLAT=0 == sweep_mode 6 for one way of running."""
    a = run()
    _same(torch, a, _with_env(monkeypatch, "RQ_FLAT_SLICES", run), events)
    _same(torch, a, _with_env(monkeypatch, "RQ_MERGE_FLAT", run), events)
    _same(torch, a, run(sweep_mode=6), events)
    return a


def _five_way(torch, monkeypatch, O, engine, so, n_rep, oracle_reps=(), seed=77, Ks=(1, 2)):
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=n_rep, ctrl_seed=seed, world_seed=seed, randomize=True, Ks=Ks)
    assert g.run("opt", plan_only=True, **kw)["sources_per_lane"] == 0   # merged streams
    _legs(torch, monkeypatch, lambda **k: g.run("opt", **dict(kw, **k)), events=False)
    a = _legs(torch, monkeypatch, lambda **k: g.run("opt", event_log=True, **dict(kw, **k)))
    _oracle_reps(O, so, a, oracle_reps, seed, Ks)
    return a


def _fixed_world(torch, monkeypatch, O, engine, so, Ks=(1, 2)):
    """A world of replayed streams only (every replica merges the same sequence): the four
    legs and the oracle."""
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=2, ctrl_seed=4, Ks=Ks, event_log=True)
    assert g.run("opt", plan_only=True, **kw)["sources_per_lane"] == 0
    a = _legs(torch, monkeypatch, lambda **k: g.run("opt", **dict(kw, **k)))
    assert int(a.status.max().item()) == 0
    met, (t_o, _, s_o) = O.engine_metrics(O.Scenario(so, ("opt", 4)), Ks)
    t, s = a.events(0)
    assert np.array_equal(t, t_o) and np.array_equal(s, s_o)
    top, avg, r2, _ = met
    assert np.array_equal(a.metrics[0].cpu().numpy(), np.asarray(list(top) + [avg, r2]))
    return a


def _rd_world(streams, end_time=10.0):
    """One RealData stream per entry of `streams` (sorted times); an empty entry is a silent
    Poisson source."""
    n = len(streams)
    others = [("RealData", {"src_id": 100 + j, "times": [float(t) for t in streams[j]]}) if len(streams[j]) else
              ("Poisson", {"src_id": 100 + j, "seed": 50 + j, "rate": 1e-9}) for j in range(n)]
    return dict(src_id=1, end_time=end_time, s=np.asarray([1.0, 2.0, 0.5]), q=0.7, sink_ids=[10, 11, 12],
                other_sources=others, edge_list=[(1, 10), (1, 11), (1, 12)] + [(100 + j, 10 + j % 3) for j in range(n)])


def _deal(times, n_str):
    """Distinct sorted times dealt to n_str streams, unevenly."""
    t = np.sort(np.asarray(times, dtype=np.float64))
    assert len(np.unique(t)) == len(t)
    own = np.random.RandomState(len(t)).randint(0, n_str + 3, len(t)) % n_str
    return [t[own == j] for j in range(n_str)]


def _slice_counts(times, end_time):
    """Arrivals per slice as the kernel counts them (t_min is the replica's earliest arrival,
    the last slice is closed at end_time)."""
    t = np.asarray(times, dtype=np.float64)
    return np.bincount(_slice_of(t, float(t.min()), end_time), minlength=NB)


@pytest.mark.parametrize("n_str", [9, 33, 64])
def test_stream_counts(n_str, monkeypatch):
    """9, 33 and 64 streams, some silent in every replica, many silent in a given one (rate 0.3
    over T = 10), one with exactly one arrival."""
    torch, engine, graphs, O = _ctx()
    so = _world(graphs, n_str, rd=[[4.375]], rate=0.3, n_base=min(n_str - 3, 48))
    a = _five_way(torch, monkeypatch, O, engine, so, 96, oracle_reps=(0, 95))
    assert int(a.status.max().item()) == 0


def test_nothing_to_merge(monkeypatch):
    """Replicas whose streams are all empty next to replicas with one or two arrivals."""
    torch, engine, graphs, O = _ctx()
    so = _world(graphs, 9, rate=0.02, end_time=2.0, n_base=7)
    a = _five_way(torch, monkeypatch, O, engine, so, 64, oracle_reps=(0, 1, 63))
    n_ev = [len(a.events(i)[0]) for i in range(64)]   # the controller's own post at 0.0 is always there
    assert min(n_ev) == 1 and max(n_ev) > 1


def test_one_stream_holds_everything(monkeypatch):
    """700 arrivals in one replayed stream, eight silent streams beside it (one lane pair's
    pre-pass and cum hold the whole replica)."""
    torch, engine, graphs, O = _ctx()
    streams = [[] for _ in range(9)]
    streams[5] = np.linspace(0.5, 9.5, 700)
    _fixed_world(torch, monkeypatch, O, engine, _rd_world(streams))


def test_times_on_and_beside_boundaries(monkeypatch):
    """Arrivals exactly on one boundary (the first time of a slice), on several, one ulp below
    and one ulp above a boundary, at t_min and at end_time, among 300 others."""
    torch, engine, graphs, O = _ctx()
    t_min, end = 0.625, 10.0
    edge = [t_min, end] + [_bnd(t_min, end, b) for b in (1, 5, 9, 13, 15)]
    edge += [np.nextafter(_bnd(t_min, end, 12), -np.inf), np.nextafter(_bnd(t_min, end, 12), np.inf),
             np.nextafter(_bnd(t_min, end, 7), -np.inf), np.nextafter(_bnd(t_min, end, 8), np.inf),
             np.nextafter(end, -np.inf), np.nextafter(t_min, np.inf)]
    fill = np.linspace(0.7, 9.9, 300) + 1e-3 / 7.0   # off the boundaries
    streams = _deal(list(edge) + list(fill), 9)
    allt = np.concatenate(streams)
    assert allt.min() == t_min and allt.max() == end
    sl = _slice_of(np.sort(allt), t_min, end)
    assert sl[0] == 0 and sl[-1] == NB - 1 and (np.diff(sl) >= 0).all()
    for b in (1, 5, 9, 13, 15):   # on the boundary is inside slice b, one ulp below is not
        assert _slice_of(_bnd(t_min, end, b), t_min, end) == b
        assert _slice_of(np.nextafter(_bnd(t_min, end, b), -np.inf), t_min, end) == b - 1
    _fixed_world(torch, monkeypatch, O, engine, _rd_world(streams, end))


def test_stream_past_the_16_bit_counts(monkeypatch):
    """65,536 arrivals of one stream inside slice 0: one more than a 16-bit slice count holds
    (a count that wrapped would leave slice 0 empty and carry into slice 1).  The replica must
    take the search loop; the legs and the oracle see all of them in order."""
    torch, engine, graphs, O = _ctx()
    streams = [[] for _ in range(9)]
    streams[0] = np.linspace(1.0, 1.25, 65536)
    streams[3] = [2.5, 9.0]
    assert _slice_counts(np.concatenate([streams[0], streams[3]]), 10.0)[0] == 65536
    _fixed_world(torch, monkeypatch, O, engine, _rd_world(streams), Ks=(1,))


def test_all_arrivals_in_one_slice(monkeypatch):
    """300 arrivals in [1, 1.001] of a T = 10 horizon: slice 0 holds everything, one window."""
    torch, engine, graphs, O = _ctx()
    so = _replayed(300, 1.0, 1.001)
    allt = np.concatenate([np.asarray(k[1]["times"]) for k in so["other_sources"]])
    assert _slice_counts(allt, 10.0)[0] == 300
    _fixed_world(torch, monkeypatch, O, engine, so)


@pytest.mark.parametrize("total", [CAP - 1, CAP, CAP + 1, 2 * CAP + 500])
def test_slice_total_around_capacity(total, monkeypatch):
    """One slice holding CAP - 1, CAP, CAP + 1 and 2 CAP + 500 arrivals (all inside [1, 1.001]):
    the first two are one window of the table, the others send the replica to the search loop."""
    torch, engine, graphs, O = _ctx()
    so = _replayed(total, 1.0, 1.001)
    allt = np.concatenate([np.asarray(k[1]["times"]) for k in so["other_sources"]])
    assert _slice_counts(allt, 10.0)[0] == total
    _fixed_world(torch, monkeypatch, O, engine, so)


@pytest.mark.parametrize("second", [CAP - 600, CAP - 600 + 1])
def test_consecutive_slices_around_capacity(second, monkeypatch):
    """Slices 0 and 1 hold 600 and CAP - 600 arrivals (one window of exactly CAP) or one more
    (the window must end after slice 0); 100 more arrivals follow in slice 2 and 50 later."""
    torch, engine, graphs, O = _ctx()
    t_min, end = 1.0, 10.0
    b1, b2, b3 = (_bnd(t_min, end, b) for b in (1, 2, 3))
    times = np.concatenate([np.linspace(t_min, np.nextafter(b1, -np.inf), 600),
                            np.linspace(b1, np.nextafter(b2, -np.inf), second),
                            np.linspace(b2, np.nextafter(b3, -np.inf), 100),
                            np.linspace(5.0, 9.5, 50)])
    c = _slice_counts(times, end)
    assert c[0] == 600 and c[1] == second and c[2] == 100 and c.max() <= CAP
    _fixed_world(torch, monkeypatch, O, engine, _rd_world(_deal(times, 9), end))


def test_equal_times_below_capacity(monkeypatch):
    """9 replayed streams with 40 entries at 5.0 each (360 < CAP): the merge orders them exactly
    -- stream, then position -- so the merged sweep plays the events of the exact sequential
    sweep (mode 2), from the table and from the search loop."""
    torch, engine, graphs, O = _ctx()
    so = _tie_streams(40, 5.0)
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=3, ctrl_seed=2, Ks=(1, 3), event_log=True, check=False)
    exact = g.run("opt", sweep_mode=2, **kw)
    a = g.run("opt", sweep_mode=5, **kw)
    _events_equal(a, exact, 3)
    b = _with_env(monkeypatch, "RQ_FLAT_SLICES", lambda: g.run("opt", sweep_mode=5, **kw))
    _events_equal(b, exact, 3)
    assert torch.equal(a.counts, b.counts) and torch.equal(a.metrics, b.metrics) and torch.equal(a.status, b.status)


@pytest.mark.parametrize("at", [0.0, 5.0])
def test_more_than_capacity_at_one_time(at, monkeypatch):
    """9 replayed streams of 400 equal times each (3600 > 3 CAP), at 0.0 and inside the horizon:
    a slice over the capacity, so the search loop emits them CAP at a time and flags RQ_ST_TIE
    exactly as with RQ_FLAT_SLICES=0; with check=True the engine reruns on the exact sweep."""
    torch, engine, graphs, O = _ctx()
    so = _tie_streams(400, at)
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=2, ctrl_seed=4, Ks=(1, 2), sweep_mode=5)
    a = g.run("opt", check=False, **kw)
    assert int(a.status[0].item()) & 4 and int(a.status[1].item()) & 4
    _same(torch, a, _with_env(monkeypatch, "RQ_FLAT_SLICES", lambda: g.run("opt", check=False, **kw)), events=False)
    b = g.run("opt", **kw)
    _same(torch, b, g.run("opt", **dict(kw, sweep_mode=2)), events=False)
    _same(torch, b, _with_env(monkeypatch, "RQ_FLAT_SLICES", lambda: g.run("opt", **kw)), events=False)
    met, _ = O.engine_metrics(O.Scenario(so, ("opt", 4)), (1, 2))
    top, avg, r2, _ = met
    assert np.array_equal(b.metrics[0].cpu().numpy(), np.asarray(list(top) + [avg, r2]))


def test_bursty_world_takes_both_paths(monkeypatch):
    """A near-critical Hawkes world (alpha 2.3, beta 2.5): in one launch some replicas have a
    slice of more than CAP arrivals (the search loop) and some have none (the table).  Both
    kinds are counted from the replicas' own wall events."""
    torch, engine, graphs, O = _ctx()
    so = _world(graphs, 12, end_time=40.0, rate=3.0, alpha=2.3, beta=2.5, seed=5, n_base=12)
    a = _five_way(torch, monkeypatch, O, engine, so, 24, oracle_reps=(0,), Ks=(1, 3))
    over = []
    for i in range(24):
        t, s = a.events(i)
        walls = np.asarray(t)[np.asarray(s) != so["src_id"]]
        over.append(bool(_slice_counts(walls, so["end_time"]).max() > CAP))
    print("replicas on the search loop:", sum(over), "of", len(over))
    assert 0 < sum(over) < len(over)


def test_merged_capacity_overflow(monkeypatch):
    """Undersized merged capacity (RQ_CAP_SQUEEZE): some replicas of the launch pass it and some
    do not.  The unchecked result -- status, counts, metrics and the event log, so out_len and
    the emitted prefix of the flagged replicas too -- is the search loop's bit for bit, and the
    rerun gives the unsqueezed result on both."""
    torch, engine, graphs, O = _ctx()
    from redqueen_amd import _lib as L
    so = _world(graphs, 33, rate=2.0, n_base=33)
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=200, ctrl_seed=11, world_seed=11, randomize=True, Ks=(1, 2))
    want = g.run("opt", **kw)
    assert int(want.status.max().item()) == 0
    monkeypatch.setenv("RQ_CAP_SQUEEZE", "0.45")
    for ev in (False, True):
        raw = g.run("opt", check=False, event_log=ev, **kw)
        n_over = int(((raw.status & L.ST_STREAM_OVERFLOW) != 0).sum().item())
        assert n_over > 0
        _same(torch, raw, _with_env(monkeypatch, "RQ_FLAT_SLICES",
                                    lambda: g.run("opt", check=False, event_log=ev, **kw)))
    got = g.run("opt", **kw)
    got0 = _with_env(monkeypatch, "RQ_FLAT_SLICES", lambda: g.run("opt", **kw))
    monkeypatch.delenv("RQ_CAP_SQUEEZE")
    _same(torch, got, want)
    _same(torch, got0, want)


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
    _five_way(torch, monkeypatch, O, engine, so, 1, oracle_reps=(0,), Ks=(1,))


def test_batch_more_replicas_than_resident_blocks(monkeypatch):
    """3,000 replicas in one chunk: more blocks than the chip holds at once."""
    torch, engine, graphs, O = _ctx()
    so, g, kw, full = _batch_world(torch, engine, graphs)
    assert g.run("opt", chunk=3000, plan_only=True, **kw)["sources_per_lane"] == 0
    assert int(full.status.max().item()) == 0
    _same(torch, full, _with_env(monkeypatch, "RQ_FLAT_SLICES", lambda: g.run("opt", chunk=3000, **kw)))
    _same(torch, full, _with_env(monkeypatch, "RQ_MERGE_FLAT", lambda: g.run("opt", chunk=3000, **kw)))
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

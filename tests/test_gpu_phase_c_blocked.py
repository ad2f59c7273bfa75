"""Phase C of the merged K = 1 sink-bit sweep with a tile's events blocked four to a lane
(the default from 13 sink words on: lane 16 b + g scans events 4g .. 4g + 3 over the words of
column block b) against the word loop it replaces (RQ_PHASEC_BLK=0: one event per lane, a
six-level segmented scan per word) and the engine oracle.

Both forms count the same integer sets, so the bar is bit-exact status, counts and metrics
(NaN pattern included, event logs where kept): blocked == word loop == oracle, and the plan
reports which form runs (sweep_blk).

The blocked form takes over once every sink has a row, so a replica's first tile always runs
the word loop and every later one the blocked loop (the controller of the graphs below posts
or arrives inside the first tile).  What can go wrong sits at the segment heads (posts, or
the controlled stream's own arrivals) relative to the groups of four, the DPP rows and the
tile's ends, at the tile's last event, in the pad words of a column block, and where the
wave hands the top-1 words from one form to the other.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THRESH_NW = 13  # sink words from which the planner picks the blocked form


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


def _same(torch, a, b):
    assert torch.equal(a.status, b.status)
    assert torch.equal(a.counts, b.counts)
    assert torch.equal(a.metrics.isnan(), b.metrics.isnan())
    assert torch.equal(a.metrics.nan_to_num(), b.metrics.nan_to_num())
    if a.ev_t is not None:
        for i in range(a.counts.shape[0]):
            ta, sa = a.events(i)
            tb, sb = b.events(i)
            assert np.array_equal(ta, tb) and np.array_equal(sa, sb), i


def _on_off(torch, monkeypatch, g, ctrl="opt", blk=1, **kw):
    """The run with the blocked form (the default) and with the word loop: equal.  The plan
    reports the choice; blk=0: a plan that keeps the word loop either way."""
    pkw = {k: v for k, v in kw.items() if k != "check"}
    monkeypatch.delenv("RQ_PHASEC_BLK", raising=False)
    plan = g.run(ctrl, plan_only=True, **pkw)
    assert plan["sweep_blk"] == blk, plan
    if blk:
        assert plan["variant"] == 22, plan   # the merged fused sweep on sink bits
    on = g.run(ctrl, **kw)
    monkeypatch.setenv("RQ_PHASEC_BLK", "0")
    assert g.run(ctrl, plan_only=True, **pkw)["sweep_blk"] == 0
    off = g.run(ctrl, **kw)
    monkeypatch.delenv("RQ_PHASEC_BLK")
    _same(torch, on, off)
    return on


def _seeded(so, u):
    """randomize_other_sources(u): other source idx gets seed u + 99 idx."""
    return dict(so, other_sources=[(n, dict(x, seed=(u + 99 * i) & 0xFFFFFFFF)) if "seed" in x else (n, x)
                                   for i, (n, x) in enumerate(so["other_sources"])])


def _cmp_oracle(O, res, i, so, ctrl, Ks=(1,), max_events=None):
    """Replica i of res == the engine oracle's run of world so under controller ctrl;
    returns the oracle's events (t, source)."""
    met, (t_o, _, s_o) = O.engine_metrics(O.Scenario(so, ctrl, max_events=max_events), Ks)
    c = res.counts[i].cpu().numpy()
    m = res.metrics[i].cpu().numpy()
    assert c[2] == len(t_o), (i, c, len(t_o))
    if res.ev_t is not None:
        t, s = res.events(i)
        assert np.array_equal(s, s_o) and np.array_equal(t, t_o), i
    if met is None:   # no event reached a sink: no row, every metric NaN
        assert c[3] == 0 and np.isnan(m).all(), (i, c, m)
        return t_o, s_o
    top, avg, r2, cnt = met
    assert np.array_equal(m, np.asarray(list(top) + [avg, r2])), (i, m, top, avg, r2)
    assert c[0] == cnt[0] and c[1] == cnt[1] and c[3] == cnt[2], (i, c, cnt)
    return t_o, s_o


def _syn(n_sinks, n_src=12, seed=5, rate=4.0, end_time=3.0, fol=1.0, frac=0.2):
    """n_src Poisson2 walls with random follower sets over n_sinks sinks (every sink has a
    wall source, so every sink gets a row); the controlled source 1 follows the first
    fol x n_sinks sinks of a random order (all of them at fol = 1)."""
    rs = np.random.RandomState(seed)
    sinks = list(range(100, 100 + n_sinks))
    edges = []
    for j in range(n_src):
        take = rs.rand(n_sinks) < frac
        take[j::n_src] = True
        edges += [(1000 + j, sinks[k]) for k in np.nonzero(take)[0]]
    nf = max(1, int(round(fol * n_sinks)))
    edges += [(1, sinks[k]) for k in sorted(rs.permutation(n_sinks)[:nf])]
    return dict(src_id=1, end_time=end_time, s=np.ones(nf), q=float(nf) ** 2, sink_ids=sinks,
                other_sources=[("Poisson2", {"src_id": 1000 + j, "seed": 40 + j, "rate": rate})
                               for j in range(n_src)],
                edge_list=edges)


def _heads(s, ctrl_id, own_arrivals=False):
    """Per tile of a replica's event log (sources s): (n, set of head lanes).  Lane l of tile
    k is merged entry 64 k + l.  RedQueen: the entries are the wall arrivals and a head is
    one with a post right before it; own_arrivals (a Poisson controller): the controlled
    stream's arrivals are entries too, and the heads."""
    tiles, heads, l, post = [], set(), 0, False
    for x in s:
        own = x == ctrl_id
        if own and not own_arrivals:
            post = True
            continue
        if own or post:
            heads.add(l)
        post = False
        l += 1
        if l == 64:
            tiles.append((64, heads))
            heads, l = set(), 0
    if l:
        tiles.append((l, heads))
    return tiles


# the places a head can fall (the blocked tiles of a replica: every tile after its first)
def _head_classes(tiles):
    got = set()
    for n, h in tiles[1:]:
        got |= {"lane %d" % l for l in h if l in (0, 63, 15, 16, 31, 32, 47, 48)}
        got |= {"position %d" % (l & 3) for l in h}
        if any(len([l for l in h if l >> 2 == g]) >= 2 for g in range(16)):
            got.add("two in a group")
        if any(l + 1 in h for l in h):
            got.add("consecutive")
        if not h:
            got.add("none")
        if h and min(h) > 0:
            got.add("first after lane 0")
    return got


CLASSES = ({"lane %d" % l for l in (0, 63, 15, 16, 31, 32, 47, 48)} | {"position %d" % k for k in range(4)} |
           {"two in a group", "consecutive", "none", "first after lane 0"})
Q_GRID = [1e6, 1e4, 1e2, 1.0, 1e-2]


def test_where_the_heads_fall(monkeypatch):
    """C3 at K = 1 over a q grid from a post every tile or two down to several per tile: the
    event logs of the same seeds hold a head at every place of CLASSES."""
    torch, engine, graphs, O = _ctx()
    so = dict(graphs.c3(), end_time=2.4)
    g = _graph(engine, so)
    R = 12
    kw = dict(q=np.asarray(Q_GRID), s=so["s"], n_rep=R, ctrl_seed=100, world_seed=100, randomize=True, Ks=(1,))
    on = _on_off(torch, monkeypatch, g, **kw)
    assert int(on.status.max().item()) == 0
    log = _on_off(torch, monkeypatch, g, event_log=True, **kw)
    assert torch.equal(log.counts, on.counts) and torch.equal(log.metrics, on.metrics)
    got = set()
    for i in range(len(Q_GRID) * R):
        got |= _head_classes(_heads(log.events(i)[1], so["src_id"]))
    assert got == CLASSES, sorted(CLASSES - got)
    for i in (0, R - 1, R, 2 * R + 3, 3 * R + 5, 4 * R, 5 * R - 1):
        _cmp_oracle(O, on, i, _seeded(dict(so, q=Q_GRID[i // R]), 100 + i), ("opt", 100 + i))


def test_heads_that_are_not_posts(monkeypatch):
    """A Poisson controller at a high rate: its arrivals are tile entries that start a
    segment and are no wall events (their mask row is the zero row)."""
    torch, engine, graphs, O = _ctx()
    so = dict(graphs.c3(), end_time=2.4)
    g = _graph(engine, so)
    kw = dict(ctrl_rate=40.0, n_rep=32, ctrl_seed=50, world_seed=50, randomize=True, Ks=(1,))
    on = _on_off(torch, monkeypatch, g, "poisson", **kw)
    assert int(on.status.max().item()) == 0
    log = _on_off(torch, monkeypatch, g, "poisson", event_log=True, **kw)
    assert torch.equal(log.counts, on.counts) and torch.equal(log.metrics, on.metrics)
    got = set()
    for i in range(32):
        got |= _head_classes(_heads(log.events(i)[1], so["src_id"], own_arrivals=True))
    assert {"two in a group", "consecutive", "first after lane 0", "position 0", "position 3"} <= got, got
    for i in (0, 7, 31):
        _cmp_oracle(O, on, i, _seeded(so, 50 + i), ("poisson", 50 + i, 40.0))


@pytest.mark.parametrize("end", [0.03, 0.3, 2.4])
def test_hand_over(end, monkeypatch):
    """C3 over horizons of one tile (the word loop alone), of a few and of many: the top-1
    words pass from the word loop to the blocked loop after the first tile."""
    torch, engine, graphs, O = _ctx()
    so = dict(graphs.c3(), end_time=end)
    g = _graph(engine, so)
    R = 48
    on = _on_off(torch, monkeypatch, g, q=so["q"], s=so["s"], n_rep=R, ctrl_seed=300, world_seed=300,
                 randomize=True, Ks=(1,))
    assert int(on.status.max().item()) == 0
    walls = on.counts[:, 1]
    if end == 0.03:
        assert int(walls.max().item()) <= 64      # a single tile
    if end == 2.4:
        assert int(walls.min().item()) > 64       # every replica reaches the blocked loop
    for i in (0, 1, R // 2, R - 1):
        _cmp_oracle(O, on, i, _seeded(so, 300 + i), ("opt", 300 + i))


def test_follower_set_not_full(monkeypatch):
    """The controller follows 60 % of 430 sinks: F has zero bits inside its words, and the
    sinks become valid one wall event at a time, so the hand-over comes tiles into the run."""
    torch, engine, graphs, O = _ctx()
    so = _syn(430, fol=0.6, frac=0.05, end_time=6.0)
    g = _graph(engine, so)
    R = 32
    on = _on_off(torch, monkeypatch, g, q=so["q"], s=so["s"], n_rep=R, ctrl_seed=70, world_seed=70,
                 randomize=True, Ks=(1,))
    assert int(on.status.max().item()) == 0
    assert int(on.counts[:, 1].min().item()) > 128
    for i in (0, 9, R - 1):
        _cmp_oracle(O, on, i, _seeded(so, 70 + i), ("opt", 70 + i))


# sinks: a partial last word; THRESH_NW - 1, THRESH_NW, THRESH_NW + 1 words; 1000, 1024 and
# 1025 (an odd word count, pad words in the last column block); 2047
@pytest.mark.parametrize("n_sinks", [430, 32 * THRESH_NW - 32, 32 * THRESH_NW, 32 * THRESH_NW + 1, 1000, 1024,
                                     1025, 2047])
def test_word_counts(n_sinks, monkeypatch):
    torch, engine, graphs, O = _ctx()
    so = _syn(n_sinks, n_src=10 + n_sinks % 11, seed=n_sinks, fol=0.8)
    g = _graph(engine, so)
    R = 32
    blk = 1 if (n_sinks + 31) // 32 >= THRESH_NW else 0
    on = _on_off(torch, monkeypatch, g, blk=blk, q=so["q"] / 100, s=so["s"], n_rep=R, ctrl_seed=8, world_seed=8,
                 randomize=True, Ks=(1,))
    assert int(on.status.max().item()) == 0
    assert int(on.counts[:, 1].min().item()) > 64
    for i in (0, 13, R - 1):
        _cmp_oracle(O, on, i, _seeded(dict(so, q=so["q"] / 100), 8 + i), ("opt", 8 + i))


_WALLS = {}


def _wall_times(O, so):
    """The wall arrival times of so's own (unrandomized) world over its whole horizon."""
    if "t" not in _WALLS:
        _, (t, _, s) = O.engine_metrics(O.Scenario(so, ("opt", 7)), (1,))
        _WALLS["t"] = t[s != so["src_id"]]
    return _WALLS["t"]


# merged lengths: no tile, a first tile that is short, full, and one to five entries into the
# second tile (the blocked loop's shortest tiles), a second tile of 63, 64 and a third of 1
@pytest.mark.parametrize("length", [0, 1, 3, 4, 5, 63, 64, 65, 67, 68, 69, 127, 128, 129])
def test_tile_lengths(length, monkeypatch):
    torch, engine, graphs, O = _ctx()
    base = _syn(430, n_src=16, seed=3, end_time=4.0)
    tw = _wall_times(O, base)
    assert len(tw) > 130
    so = dict(base, end_time=0.5 * tw[0] if length == 0 else 0.5 * (tw[length - 1] + tw[length]))
    g = _graph(engine, so)
    kw = dict(q=so["q"] / 1e4, s=so["s"], n_rep=1, ctrl_seed=7, Ks=(1,))
    on = _on_off(torch, monkeypatch, g, **kw)
    assert int(on.counts[0, 1].item()) == length
    assert int(on.status[0].item()) == 0
    _cmp_oracle(O, on, 0, dict(so, q=so["q"] / 1e4), ("opt", 7))
    log = _on_off(torch, monkeypatch, g, event_log=True, **kw)
    assert torch.equal(log.counts, on.counts) and torch.equal(log.metrics, on.metrics)


# the tile's last lane under a max_events cut in the second tile: inside a group of four, the
# last and the first of a group, the last and the first of a DPP row
@pytest.mark.parametrize("lane", [5, 7, 8, 15, 16, 2])
def test_max_events_moves_the_last_lane(lane, monkeypatch):
    torch, engine, graphs, O = _ctx()
    so = _syn(430, n_src=16, seed=3, end_time=4.0)
    so = dict(so, q=so["q"] / 1e4)
    g = _graph(engine, so)
    _, (t_o, _, s_o) = O.engine_metrics(O.Scenario(so, ("opt", 7)), (1,))
    walls = np.nonzero(s_o != so["src_id"])[0]
    me = int(walls[64 + lane]) + 1   # the events up to wall arrival 64 + lane
    for log in (False, True):
        on = _on_off(torch, monkeypatch, g, q=so["q"], s=so["s"], n_rep=1, ctrl_seed=7, Ks=(1,), max_events=me,
                     event_log=log)
        assert int(on.counts[0, 2].item()) == me and int(on.counts[0, 1].item()) == 64 + lane + 1
        _cmp_oracle(O, on, 0, so, ("opt", 7), max_events=me)


def test_more_replicas_than_resident_waves(monkeypatch):
    """5,000 short replicas in one launch: waves take further replicas from the queue and
    initialise their F / T words and the pad words again."""
    torch, engine, graphs, O = _ctx()
    so = dict(graphs.c3(), end_time=1.5)
    g = _graph(engine, so)
    R = 5000
    kw = dict(q=so["q"] / 1e3, s=so["s"], ctrl_seed=11, world_seed=11, randomize=True, Ks=(1,))
    plan = g.run("opt", n_rep=R, plan_only=True, chunk=R, **kw)
    slots = plan["blocks_per_cu"] * plan["waves_per_block"] * torch.cuda.get_device_properties(0).multi_processor_count
    assert plan["chunk"] == R and R > slots
    on = _on_off(torch, monkeypatch, g, n_rep=R, chunk=R, **kw)
    assert int(on.status.max().item()) == 0
    for i in (0, slots - 1, slots, R - 1):
        _cmp_oracle(O, on, i, _seeded(dict(so, q=so["q"] / 1e3), 11 + i), ("opt", 11 + i))


def test_rep_idx(monkeypatch):
    torch, engine, graphs, O = _ctx()
    so = dict(graphs.c3(), end_time=2.4)
    g = _graph(engine, so)
    R = 33
    qs = np.asarray([so["q"], 1e-4 * so["q"]])
    kw = dict(q=qs, s=so["s"], n_rep=R, ctrl_seed=21, world_seed=21, randomize=True, Ks=(1,))
    full = _on_off(torch, monkeypatch, g, **kw)
    pick = np.asarray([0, 5, 32, 33, 40, 65])
    sub = _on_off(torch, monkeypatch, g, rep_idx=pick, **kw)
    for k, i in enumerate(pick):
        assert torch.equal(sub.counts[k], full.counts[i]) and torch.equal(sub.metrics[k], full.metrics[i])
    _cmp_oracle(O, sub, 4, _seeded(dict(so, q=float(qs[1])), 21 + 40), ("opt", 21 + 40))


def test_tie_flagged_replica_and_its_rerun(monkeypatch):
    """Equal event times on the fast sweep (two RealData walls on the same times, sweep_mode=1)
    on a graph of 14 sink words: flagged RQ_ST_TIE by either form, and the rerun Graph.run
    makes of it equals the oracle."""
    torch, engine, graphs, O = _ctx()
    T = np.round(np.linspace(0.05, 2.95, 90), 3)
    so = _syn(430, n_src=6, seed=9, end_time=3.0)
    ea = [(2000, k) for k in so["sink_ids"][:215]] + [(2001, k) for k in so["sink_ids"][215:]]
    so = dict(so, other_sources=so["other_sources"] + [("RealData", {"src_id": 2000, "times": T.tolist()}),
                                                        ("RealData", {"src_id": 2001, "times": T.tolist()})],
              edge_list=so["edge_list"] + ea, q=so["q"] / 1e4)
    g = _graph(engine, so)
    for seed in (1, 2):
        kw = dict(q=so["q"], s=so["s"], n_rep=1, ctrl_seed=seed, Ks=(1,))
        raw = _on_off(torch, monkeypatch, g, sweep_mode=1, check=False, **kw)
        assert int(raw.status[0].item()) & 4   # RQ_ST_TIE
        assert int(raw.counts[0, 1].item()) > 128
        _cmp_oracle(O, raw, 0, so, ("opt", seed))
        monkeypatch.delenv("RQ_PHASEC_BLK", raising=False)
        got = g.run("opt", sweep_mode=1, **kw)   # the flagged replica again, on the exact sequential sweep
        assert g.reruns == 1
        _cmp_oracle(O, got, 0, so, ("opt", seed))


def test_row_capacity_overflow_rerun(monkeypatch):
    """Undersized capacities (RQ_CAP_SQUEEZE): flagged replicas are rerun with doubled
    capacities, and the result equals the normal run."""
    torch, engine, graphs, O = _ctx()
    so = graphs.c3()
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=64, ctrl_seed=9, world_seed=9, randomize=True, Ks=(1,))
    ref = _on_off(torch, monkeypatch, g, **kw)
    monkeypatch.setenv("RQ_CAP_SQUEEZE", "0.45")
    raw = _on_off(torch, monkeypatch, g, check=False, **kw)
    assert int(((raw.status & 3) != 0).sum().item()) > 0   # RQ_ST_ROWS_OVERFLOW | RQ_ST_STREAM_OVERFLOW
    got = _on_off(torch, monkeypatch, g, **kw)
    assert int(got.status.max().item()) == 0
    _same(torch, got, ref)
    _cmp_oracle(O, got, 5, _seeded(so, 9 + 5), ("opt", 9 + 5))


def test_untouched_plans(monkeypatch):
    """One sink word (README, the C4 graph), the column instances (two Ks on C3) and the
    generating fused sweep keep their kernels: sweep_blk 0 and equal results either way."""
    torch, engine, graphs, O = _ctx()
    rd = dict(graphs.readme(), end_time=6.0)
    c3 = dict(graphs.c3(), end_time=2.4)
    for so, extra in ((rd, dict(Ks=(1,))), (c3, dict(Ks=(1, 2))), (c3, dict(Ks=(1,), sweep_mode=7))):
        g = _graph(engine, so)
        kw = dict(q=so["q"], s=so["s"], n_rep=32, ctrl_seed=3, world_seed=3, randomize=True, **extra)
        on = _on_off(torch, monkeypatch, g, blk=0, **kw)
        assert int(on.status.max().item()) == 0
        _cmp_oracle(O, on, 4, _seeded(so, 3 + 4), ("opt", 3 + 4), extra["Ks"])

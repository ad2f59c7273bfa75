"""The call pairs of the merged fused sweep (the default: one Philox call per lane and tile
pair, its two draws handed out by cross-lane reads over both tiles) at the edges of the
tile sequence, against a call per draw (RQ_CTRL_DRAWS=0) and the engine oracle.  Written
for the form that runs the call a tile pair ahead of its use (RQ_MRG_AHEAD, DESIGN §19:
measured, slower, not kept); wherever the call runs, these are the places it can go wrong.

The call index depends on the tile index alone, so what can go wrong sits at the edges of
the tile sequence: a replica with no tile, a last tile that is even or odd, full or short,
a max_events cut inside a tile or between two, and a wave that takes its next replica from
the queue with the previous replica's draws still in its registers.  Bar: bit-exact
metrics, counts, status (and event logs where kept), default == per draw == oracle.

The horizons cut the README graph's own (unrandomized) world after exactly that many wall
arrivals -- the merged length -- and were found with the CPU oracle, which asserts each
here: 300 arrivals are five tiles (the last one even), 350 are six (the last one odd).  On
the 350-arrival horizon under controller seed 7 the first 78 / 154 / 232 events end with
wall arrival 63 / 127 / 191, the last of a tile (the cut falls between two tiles and the
next tile keeps nothing), the first 121 hold 100 arrivals (a cut in the odd tile 1) and
the first 179 hold 150 (a cut in the even tile 2).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HORIZON = {0: 0.014634, 1: 0.030232, 63: 3.252427, 64: 3.357424, 65: 3.430834, 127: 6.650417,
           128: 6.72453, 129: 6.761216, 300: 15.360681, 350: 17.592722}
# max_events -> (wall arrivals among the kept events, the last kept event ends a tile)
CUTS = {78: (64, True), 121: (100, False), 154: (128, True), 179: (150, False), 232: (192, True)}


def _ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from redqueen_amd import engine, graphs
    from oracle import oracle as O
    return torch, engine, graphs, O


def _world(graphs, length):
    return dict(graphs.readme(), end_time=HORIZON[length])


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


def _on_off(torch, monkeypatch, g, **kw):
    """The default run (call pairs) and the run with a call per draw: equal."""
    monkeypatch.delenv("RQ_CTRL_DRAWS", raising=False)
    on = g.run("opt", **kw)
    monkeypatch.setenv("RQ_CTRL_DRAWS", "0")
    off = g.run("opt", **kw)
    monkeypatch.delenv("RQ_CTRL_DRAWS")
    _same(torch, on, off)
    return on


def _seeded(so, u):
    """randomize_other_sources(u): other source idx gets seed u + 99 idx."""
    return dict(so, other_sources=[(n, dict(x, seed=(u + 99 * i) & 0xFFFFFFFF)) if "seed" in x else (n, x)
                                   for i, (n, x) in enumerate(so["other_sources"])])


_ORACLE = {}


def _oracle(O, so, ctrl_seed, Ks, max_events=None):
    """The engine oracle's run, computed once per world (tests share it, nobody writes it)."""
    key = (so["end_time"], float(so["q"]), tuple(x.get("seed") for _, x in so["other_sources"]), ctrl_seed,
           tuple(Ks), max_events)
    if key not in _ORACLE:
        _ORACLE[key] = O.engine_metrics(O.Scenario(so, ("opt", ctrl_seed), max_events=max_events), Ks)
    return _ORACLE[key]


def _cmp_oracle(O, res, i, so, ctrl_seed, Ks, max_events=None):
    """Replica i of res == the oracle's run of world so; returns (wall arrivals, sources)."""
    met, (t_o, _, s_o) = _oracle(O, so, ctrl_seed, Ks, max_events)
    c = res.counts[i].cpu().numpy()
    m = res.metrics[i].cpu().numpy()
    assert c[2] == len(t_o), (i, c, len(t_o))
    if res.ev_t is not None:
        t, s = res.events(i)
        assert np.array_equal(s, s_o) and np.array_equal(t, t_o), i
    walls = int((s_o != so["src_id"]).sum())
    if met is None:
        assert c[3] == 0 and np.isnan(m).all(), (i, c, m)
        return walls, s_o
    top, avg, r2, cnt = met
    assert np.array_equal(m, np.asarray(list(top) + [avg, r2])), (i, m, top, avg, r2)
    assert c[0] == cnt[0] and c[1] == cnt[1] and c[3] == cnt[2], (i, c, cnt)
    assert cnt[1] == walls   # every source of this graph reaches a sink
    return walls, s_o


@pytest.mark.parametrize("length", sorted(HORIZON))
def test_merged_lengths(length, monkeypatch):
    """One replica at each horizon, on the sink-bit instance with its own scan (variant
    22: the flagship's kernel), then with the event log."""
    torch, engine, graphs, O = _ctx()
    so = _world(graphs, length)
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=1, ctrl_seed=7, Ks=(1,))
    assert g.run("opt", plan_only=True, **kw)["variant"] == 22
    on = _on_off(torch, monkeypatch, g, **kw)
    assert _cmp_oracle(O, on, 0, so, 7, (1,))[0] == length
    assert int(on.counts[0, 1].item()) == length
    assert int(on.status[0].item()) == 0
    log = _on_off(torch, monkeypatch, g, event_log=True, **kw)
    assert _cmp_oracle(O, log, 0, so, 7, (1,))[0] == length
    assert torch.equal(log.counts, on.counts) and torch.equal(log.metrics, on.metrics)


@pytest.mark.parametrize("me", sorted(CUTS))
def test_max_events_cuts(me, monkeypatch):
    """A max_events cut in an odd tile, in an even tile and between two tiles."""
    torch, engine, graphs, O = _ctx()
    so = _world(graphs, 350)
    g = _graph(engine, so)
    walls, edge = CUTS[me]
    for log in (False, True):
        kw = dict(q=so["q"], s=so["s"], n_rep=1, ctrl_seed=7, Ks=(1,), max_events=me, event_log=log)
        on = _on_off(torch, monkeypatch, g, **kw)
        assert int(on.counts[0, 2].item()) == me
        got, s_o = _cmp_oracle(O, on, 0, so, 7, (1,), max_events=me)
        assert got == walls
        # between two tiles: the last kept event is the wall arrival that fills a tile
        assert (s_o[-1] != so["src_id"] and walls % 64 == 0) == edge


def test_more_replicas_than_resident_waves(monkeypatch):
    """One replica more than the launch has waves (the shape of test_gpu_sweep_scan.py, by
    its replica count): waves take a second replica from the queue behind one that ended
    in an even tile (the README graph over 2 time units: 19 to 66 arrivals, nearly always one
    tile, tile 0) and start it with their own first call."""
    torch, engine, graphs, O = _ctx()
    so = dict(graphs.readme(), end_time=2.0)
    g = _graph(engine, so)
    Ks = (1,)
    kw = dict(q=so["q"], s=so["s"], ctrl_seed=11, world_seed=11, randomize=True, Ks=Ks)
    plan = g.run("opt", n_rep=4097, plan_only=True, **kw)
    assert plan["variant"] == 22
    slots = plan["blocks_per_cu"] * plan["waves_per_block"] * torch.cuda.get_device_properties(0).multi_processor_count
    R = max(4097, slots + 1)
    assert g.run("opt", n_rep=R, plan_only=True, chunk=R, **kw)["chunk"] == R   # one launch
    on = _on_off(torch, monkeypatch, g, n_rep=R, chunk=R, **kw)
    assert int(on.status.max().item()) == 0
    assert int((on.counts[:, 1] <= 64).sum().item()) > R // 2   # most replicas: one tile
    for i in (0, 1, slots - 1, slots, R - 1, R // 2, R // 3, 64):
        i = min(i, R - 1)
        _cmp_oracle(O, on, i, _seeded(so, 11 + i), 11 + i, Ks)


@pytest.mark.parametrize("Ks", [(1,), (1, 2), (1, 2, 5), (1, 2, 3, 5)])
def test_grid_rep_idx_ks(Ks, monkeypatch):
    """A two-point q grid of 33 randomized replicas around 350 arrivals (last tiles of both
    parities), one to four Ks, and a rep_idx subset of the same batch."""
    torch, engine, graphs, O = _ctx()
    so = _world(graphs, 350)
    g = _graph(engine, so)
    R = 33
    qs = np.asarray([so["q"], 0.25 * so["q"]])
    kw = dict(q=qs, s=so["s"], n_rep=R, ctrl_seed=21, world_seed=21, randomize=True, Ks=Ks)
    assert g.run("opt", plan_only=True, **kw)["variant"] == (22 if Ks == (1,) else 20)
    full = _on_off(torch, monkeypatch, g, **kw)
    assert int(full.status.max().item()) == 0
    last = ((full.counts[:, 1] - 1) // 64) % 2   # parity of the last tile
    assert int(last.min().item()) == 0 and int(last.max().item()) == 1
    for i in (0, R - 1, R, 2 * R - 1):
        u = 21 + i   # replica i of the whole grid takes seed 21 + i
        _cmp_oracle(O, full, i, _seeded(dict(so, q=float(qs[i // R])), u), u, Ks)
    pick = np.asarray([0, 5, 32, 33, 40, 65])
    sub = _on_off(torch, monkeypatch, g, rep_idx=pick, **kw)
    for k, i in enumerate(pick):
        assert torch.equal(sub.counts[k], full.counts[i]) and torch.equal(sub.metrics[k], full.metrics[i])

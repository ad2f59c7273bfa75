"""The RedQueen controller's draws by call pairs in the merged fused sweep (the default:
every other tile a lane runs one Philox call and hands both of its draws out by cross-lane
reads) against a call per draw (RQ_CTRL_DRAWS=0) and the engine oracle.

Draw e of a replica is half e & 1 of Philox call e >> 1; the paired form runs a call once
for both halves, the other form once per half.  Bar: bit-exact metrics, counts, status
and event logs, pairs on == pairs off == oracle.  The horizons below cut the graphs'
own (unrandomized) worlds after exactly 0, 1, 63, 64, 65 and 129 wall arrivals -- the
merged length, so tile edges, a lone second tile of a pair and a half-used last call are
hit; the oracle's world-event count asserts each.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# end_time -> merged length of the unrandomized world (any controller seed)
HORIZON = {
    "c3": {0: 0.003178, 1: 0.031572, 63: 1.265417, 64: 1.274722, 65: 1.281236, 129: 2.411152},
    "readme": {0: 0.014634, 1: 0.030232, 63: 3.252427, 64: 3.357424, 65: 3.430834, 129: 6.761216},
}
WORLDS = ["c3", "readme"]


def _ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from redqueen_amd import engine, graphs
    from oracle import oracle as O
    return torch, engine, graphs, O


def _world(graphs, name, length=129):
    so = getattr(graphs, name)()
    return dict(so, end_time=HORIZON[name][length])


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


def _on_off(torch, monkeypatch, g, ctrl="opt", **kw):
    """The run with the paired draws (the default) and with a call per draw: equal."""
    monkeypatch.delenv("RQ_CTRL_DRAWS", raising=False)
    on = g.run(ctrl, **kw)
    monkeypatch.setenv("RQ_CTRL_DRAWS", "0")
    off = g.run(ctrl, **kw)
    monkeypatch.delenv("RQ_CTRL_DRAWS")
    _same(torch, on, off)
    return on


def _seeded(so, u):
    """randomize_other_sources(u): other source idx gets seed u + 99 idx."""
    return dict(so, other_sources=[(n, dict(x, seed=(u + 99 * i) & 0xFFFFFFFF)) if "seed" in x else (n, x)
                                   for i, (n, x) in enumerate(so["other_sources"])])


def _cmp_oracle(O, res, i, so, ctrl_seed, Ks, max_events=None):
    """Replica i of res == the engine oracle's run of world so; returns its wall arrivals."""
    met, (t_o, _, s_o) = O.engine_metrics(O.Scenario(so, ("opt", ctrl_seed), max_events=max_events), Ks)
    t, s = res.events(i)
    assert np.array_equal(s, s_o) and np.array_equal(t, t_o), i
    c = res.counts[i].cpu().numpy()
    assert c[2] == len(t_o), (c, len(t_o))
    walls = int((s_o != so["src_id"]).sum())
    if met is None:   # no event reached a sink (max_events = 0)
        return walls
    top, avg, r2, cnt = met
    assert np.array_equal(res.metrics[i].cpu().numpy(), np.asarray(list(top) + [avg, r2])), i
    assert c[0] == cnt[0] and c[1] == cnt[1] and c[3] == cnt[2], (c, cnt)
    assert cnt[1] == walls   # every source of these graphs reaches a sink
    return walls


def _ws_bytes(g):
    return sum(int(w.numel()) for w in g._wss.values())


@pytest.mark.parametrize("world", WORLDS)
def test_merged_lengths(world, monkeypatch):
    """One replica at each horizon: merged lengths 0, 1, 63, 64, 65, 129."""
    torch, engine, graphs, O = _ctx()
    Ks = (1,) if world == "c3" else (1, 2, 5)   # C3 at K = 1: the flagship's sink-bit instance
    for length in (0, 1, 63, 64, 65, 129):
        so = _world(graphs, world, length)
        g = _graph(engine, so)
        kw = dict(q=so["q"], s=so["s"], n_rep=1, ctrl_seed=7, Ks=Ks)
        assert g.run("opt", plan_only=True, **kw)["variant"] >= 20   # the merged fused sweep
        on = _on_off(torch, monkeypatch, g, event_log=True, **kw)
        _on_off(torch, monkeypatch, g, **kw)
        assert _cmp_oracle(O, on, 0, so, 7, Ks) == length
        assert int(on.counts[0, 1].item()) == length
        assert int(on.status[0].item()) == 0


@pytest.mark.parametrize("R", [1, 3, 65])
@pytest.mark.parametrize("world", WORLDS)
def test_replicas_grid_seed_mod(world, R, monkeypatch):
    """1, 3 and 65 randomized replicas of a two-point q grid with seed_mod set: replica i
    of the 2 R takes seeds 40 + i % 5."""
    torch, engine, graphs, O = _ctx()
    so = _world(graphs, world)
    g = _graph(engine, so)
    qs = np.asarray([so["q"], 0.25 * so["q"]])
    Ks = {1: (1,), 3: (1, 3), 65: (1,)}[R]
    kw = dict(q=qs, s=so["s"], n_rep=R, ctrl_seed=40, world_seed=40, randomize=True, seed_mod=5,
              Ks=Ks, event_log=True)
    on = _on_off(torch, monkeypatch, g, **kw)
    assert int(on.status.max().item()) == 0
    for i in sorted({0, R - 1, R, R + R // 2, 2 * R - 1}):
        k = i % 5
        _cmp_oracle(O, on, i, _seeded(dict(so, q=float(qs[i // R])), 40 + k), 40 + k, Ks)


@pytest.mark.parametrize("world", WORLDS)
def test_ctrl_seed_array_and_replica_subset(world, monkeypatch):
    """Explicit per-replica controller seeds, and a rep_idx subset of the same batch."""
    torch, engine, graphs, O = _ctx()
    so = _world(graphs, world)
    g = _graph(engine, so)
    R = 65
    seeds = np.random.RandomState(3).randint(0, 2 ** 31 - 1, size=R)
    cs = torch.as_tensor(seeds, dtype=torch.int32, device="cuda")
    kw = dict(q=so["q"], s=so["s"], n_rep=R, ctrl_seed=cs, world_seed=9, randomize=True, Ks=(1, 2),
              event_log=True)
    full = _on_off(torch, monkeypatch, g, **kw)
    pick = np.asarray([0, 3, 17, 40, 64])
    sub = _on_off(torch, monkeypatch, g, rep_idx=pick, **kw)
    for k, i in enumerate(pick):
        assert torch.equal(sub.counts[k], full.counts[i]) and torch.equal(sub.metrics[k], full.metrics[i])
        _cmp_oracle(O, sub, k, _seeded(so, 9 + int(i)), int(seeds[i]), (1, 2))
        _cmp_oracle(O, full, int(i), _seeded(so, 9 + int(i)), int(seeds[i]), (1, 2))


@pytest.mark.parametrize("world", WORLDS)
def test_max_events(world, monkeypatch):
    """A max_events cut ends the replica inside a tile, at its edges, before any event."""
    torch, engine, graphs, O = _ctx()
    so = _world(graphs, world)
    g = _graph(engine, so)
    for me in (0, 1, 63, 64, 65):
        kw = dict(q=so["q"], s=so["s"], n_rep=3, ctrl_seed=11, world_seed=11, randomize=True, Ks=(1,),
                  max_events=me, event_log=True)
        on = _on_off(torch, monkeypatch, g, **kw)
        assert int(on.counts[:, 2].max().item()) == me
        for i in range(3):
            _cmp_oracle(O, on, i, _seeded(so, 11 + i), 11 + i, (1,), max_events=me)


@pytest.mark.parametrize("world", WORLDS)
def test_two_chunks(world, monkeypatch):
    """65 replicas as chunks of 33 + 32 (the second chunk's replicas start at 33) against
    the same run as one chunk."""
    torch, engine, graphs, O = _ctx()
    so = _world(graphs, world)
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=65, ctrl_seed=23, world_seed=23, randomize=True, Ks=(1,),
              event_log=True)
    one = _on_off(torch, monkeypatch, g, chunk=65, **kw)
    assert g.run("opt", plan_only=True, chunk=33, **kw)["chunk"] == 33
    two = _on_off(torch, monkeypatch, g, chunk=33, **kw)
    _same(torch, one, two)
    for i in (32, 33, 64):
        _cmp_oracle(O, two, i, _seeded(so, 23 + i), 23 + i, (1,))


def test_other_plans_untouched(monkeypatch):
    """The paired draws need no buffer: the workspace is the same with the switch on or off,
    for the merged fused RedQueen sweep too.  A Poisson controller on the same graph and a
    RedQueen one on > 64 sources (the general sweep) give the same results either way."""
    torch, engine, graphs, O = _ctx()
    so = _world(graphs, "c3")
    wide = dict(graphs.g120(), end_time=2.0)
    R = 16
    base = dict(n_rep=R, ctrl_seed=5, world_seed=5, randomize=True, Ks=(1, 2), event_log=True)
    cases = [("c3-opt", so, "opt", dict(q=so["q"], s=so["s"])),
             ("c3-poisson", so, "poisson", dict(ctrl_rate=1.5)),
             ("g120-opt", wide, "opt", dict(q=wide["q"], s=wide["s"]))]
    for name, w, ctrl, extra in cases:
        out, nbytes = [], []
        for env in (None, "0"):
            if env is None:
                monkeypatch.delenv("RQ_CTRL_DRAWS", raising=False)
            else:
                monkeypatch.setenv("RQ_CTRL_DRAWS", env)
            g = _graph(engine, w)   # a fresh graph: its workspace is this run's
            out.append(g.run(ctrl, **base, **extra))
            nbytes.append(_ws_bytes(g))
            variant = g.run(ctrl, plan_only=True, **{k: v for k, v in base.items() if k != "event_log"},
                            **extra)["variant"]
        monkeypatch.delenv("RQ_CTRL_DRAWS")
        _same(torch, out[0], out[1])
        assert (variant >= 20) == (name != "g120-opt"), (name, variant)   # 20+: the merged fused sweep
        assert nbytes[0] == nbytes[1], (name, nbytes)

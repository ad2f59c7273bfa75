"""The merged fused sweep's own scan (the default: the wave that swept a replica integrates
its pivot rows before it takes the next replica, and the chunk launches no rq_scan) against
the separate scan kernel (RQ_SWEEP_SCAN=0) and the engine oracle.

Both run the same numpy-order sums (rq_scan_rows.h) over the same rows, so the bar is
bit-exact metrics (NaN pattern included), counts and status: scan on == scan off == oracle.
What differs is who reads the rows and from where: the wave that stored them, right after
its last store, on per-wave LDS that the next replica's sweep reuses.

Row counts are chosen at the edges of numpy's pairwise tree (one leaf up to 128 rows, the
8-row accumulator blocks inside a leaf, a split above 128, blocks of 8192), with the CPU
oracle: the horizons and seeds below give replicas with 0 rows, 1-7, 8-127, exactly 128,
129-136 and 137-300, which each test asserts from counts[:, 3].  The RedQueen controller
posts at the start time, so its replicas have a row; the 0-row replicas come from a Poisson
controller on the same graphs over a horizon shorter than the first arrival.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (controller, end_time, replicas, seed of replica 0) per graph; ("poisson", rate)
RUNS = {
    "readme": [(("poisson", 5.0), 0.02, 32, 50), (("opt",), 0.3, 64, 100), (("opt",), 6.0, 64, 100)],
    "c3": [(("poisson", 20.0), 0.005, 32, 50), (("opt",), 0.03, 64, 100), (("opt",), 2.4, 64, 100)],
}
CLASSES = [(0, 0), (1, 7), (8, 127), (128, 128), (129, 136), (137, 300)]


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


def _on_off(torch, monkeypatch, g, ctrl="opt", scan_on=True, **kw):
    """The run with the sweep's own scan (the default) and with rq_scan: equal.  The plan
    reports the choice; scan_on=False: a run that keeps rq_scan either way."""
    pkw = {k: v for k, v in kw.items() if k != "check"}
    monkeypatch.delenv("RQ_SWEEP_SCAN", raising=False)
    plan = g.run(ctrl, plan_only=True, **pkw)
    assert plan["sweep_scan"] == (1 if scan_on else 0), plan
    if scan_on:
        assert plan["variant"] >= 20, plan   # the merged fused sweep
    on = g.run(ctrl, **kw)
    monkeypatch.setenv("RQ_SWEEP_SCAN", "0")
    assert g.run(ctrl, plan_only=True, **pkw)["sweep_scan"] == 0
    off = g.run(ctrl, **kw)
    monkeypatch.delenv("RQ_SWEEP_SCAN")
    _same(torch, on, off)
    return on


def _seeded(so, u):
    """randomize_other_sources(u): other source idx gets seed u + 99 idx."""
    return dict(so, other_sources=[(n, dict(x, seed=(u + 99 * i) & 0xFFFFFFFF)) if "seed" in x else (n, x)
                                   for i, (n, x) in enumerate(so["other_sources"])])


def _cmp_oracle(O, res, i, so, ctrl, Ks):
    """Replica i of res == the engine oracle's run of world so under controller ctrl."""
    met, (t_o, _, _s) = O.engine_metrics(O.Scenario(so, ctrl), Ks)
    c = res.counts[i].cpu().numpy()
    m = res.metrics[i].cpu().numpy()
    assert c[2] == len(t_o), (i, c, len(t_o))
    if met is None:   # no event reached a sink: no row, every metric NaN
        assert c[3] == 0 and np.isnan(m).all(), (i, c, m)
        return
    top, avg, r2, cnt = met
    assert np.array_equal(m, np.asarray(list(top) + [avg, r2])), (i, m, top, avg, r2)
    assert c[0] == cnt[0] and c[1] == cnt[1] and c[3] == cnt[2], (i, c, cnt)


def _ctrl_kw(so, ctrl):
    if ctrl[0] == "poisson":
        return "poisson", dict(ctrl_rate=ctrl[1])
    return "opt", dict(q=so["q"], s=so["s"])


def _oracle_ctrl(ctrl, seed):
    return ("poisson", seed, ctrl[1]) if ctrl[0] == "poisson" else ("opt", seed)


@pytest.mark.parametrize("world", ["readme", "c3"])
def test_row_counts_at_the_tree_edges(world, monkeypatch):
    """Short replicas whose row counts cover every class of CLASSES; one replica of each
    class (and the first and last of each run) against the oracle."""
    torch, engine, graphs, O = _ctx()
    Ks = (1,) if world == "c3" else (1, 2, 5)   # C3 at K = 1: the flagship's sink-bit instance
    seen = []
    for ctrl, end, R, seed0 in RUNS[world]:
        so = dict(getattr(graphs, world)(), end_time=end)
        g = _graph(engine, so)
        name, ckw = _ctrl_kw(so, ctrl)
        on = _on_off(torch, monkeypatch, g, name, n_rep=R, ctrl_seed=seed0, world_seed=seed0,
                     randomize=True, Ks=Ks, **ckw)
        n = on.counts[:, 3].cpu().numpy()
        seen.append(n)
        assert int((on.status & ~8).max().item()) == 0   # RQ_ST_EMPTY (8) marks the 0-row replicas
        assert torch.equal((on.status & 8) != 0, on.counts[:, 3] == 0)
        assert torch.equal(on.metrics.isnan().all(dim=1), on.counts[:, 3] == 0)
        assert not bool((on.metrics.isnan().any(dim=1) & (on.counts[:, 3] > 0)).any().item())
        pick = {0, R - 1}
        for lo, hi in CLASSES:
            hit = np.nonzero((n >= lo) & (n <= hi))[0]
            if hit.size:
                pick.add(int(hit[0]))
        for i in sorted(pick):
            _cmp_oracle(O, on, i, _seeded(so, seed0 + i), _oracle_ctrl(ctrl, seed0 + i), Ks)
    n = np.concatenate(seen)
    for lo, hi in CLASSES:
        assert int(((n >= lo) & (n <= hi)).sum()) >= 1, (world, lo, hi, np.sort(n))


def test_two_numpy_blocks(monkeypatch):
    """Replicas above 8192 rows (numpy sums blocks of 8192 one after the other): the README
    graph over 400 time units, about 10,000 rows each."""
    torch, engine, graphs, O = _ctx()
    so = dict(graphs.readme(), end_time=400.0)
    g = _graph(engine, so)
    Ks = (1, 2, 5)
    on = _on_off(torch, monkeypatch, g, q=so["q"], s=so["s"], n_rep=3, ctrl_seed=7, world_seed=7,
                 randomize=True, Ks=Ks)
    assert int(on.counts[:, 3].min().item()) > 8192
    assert int(on.status.max().item()) == 0
    for i in range(3):
        _cmp_oracle(O, on, i, _seeded(so, 7 + i), ("opt", 7 + i), Ks)


def test_more_replicas_than_resident_waves(monkeypatch):
    """One replica more than the launch has waves: every wave runs its scan and then sweeps
    another replica on the same LDS (at least one wave takes a third)."""
    torch, engine, graphs, O = _ctx()
    so = dict(graphs.readme(), end_time=3.0)
    g = _graph(engine, so)
    Ks = (1, 2)
    kw = dict(q=so["q"], s=so["s"], ctrl_seed=11, world_seed=11, randomize=True, Ks=Ks)
    plan = g.run("opt", n_rep=4097, plan_only=True, **kw)
    slots = plan["blocks_per_cu"] * plan["waves_per_block"] * torch.cuda.get_device_properties(0).multi_processor_count
    R = max(4097, slots + 1)
    assert g.run("opt", n_rep=R, plan_only=True, chunk=R, **kw)["chunk"] == R   # one launch
    on = _on_off(torch, monkeypatch, g, n_rep=R, chunk=R, **kw)
    assert int(on.status.max().item()) == 0
    for i in (0, 1, slots - 1, slots, R - 1, R // 2, R // 3, 64):
        i = min(i, R - 1)
        _cmp_oracle(O, on, i, _seeded(so, 11 + i), ("opt", 11 + i), Ks)


@pytest.mark.parametrize("draws", ["pairs", "per-draw"])
@pytest.mark.parametrize("Ks", [(1,), (1, 2, 5), (1, 2, 3, 5)])
@pytest.mark.parametrize("world", ["readme", "c3"])
def test_instances(world, Ks, draws, monkeypatch):
    """The sink-bit instance (Ks = (1,)) and the column instances, with the controller's
    draws by call pairs and per draw (RQ_CTRL_DRAWS=0), on a two-point q grid; then a
    rep_idx subset of the same batch."""
    torch, engine, graphs, O = _ctx()
    if draws == "per-draw":
        monkeypatch.setenv("RQ_CTRL_DRAWS", "0")
    else:
        monkeypatch.delenv("RQ_CTRL_DRAWS", raising=False)
    so = dict(getattr(graphs, world)(), end_time=6.0 if world == "readme" else 2.4)
    g = _graph(engine, so)
    R = 33
    qs = np.asarray([so["q"], 0.25 * so["q"]])
    kw = dict(q=qs, s=so["s"], n_rep=R, ctrl_seed=21, world_seed=21, randomize=True, Ks=Ks)
    full = _on_off(torch, monkeypatch, g, **kw)
    assert int(full.status.max().item()) == 0
    for i in (0, R - 1, R, 2 * R - 1):
        u = 21 + i   # replica i of the whole grid takes seed 21 + i
        _cmp_oracle(O, full, i, _seeded(dict(so, q=float(qs[i // R])), u), ("opt", u), Ks)
    pick = np.asarray([0, 5, 32, 33, 40, 65])
    sub = _on_off(torch, monkeypatch, g, rep_idx=pick, **kw)
    for k, i in enumerate(pick):
        assert torch.equal(sub.counts[k], full.counts[i]) and torch.equal(sub.metrics[k], full.metrics[i])


@pytest.mark.parametrize("Ks", [(1,), (1, 2)])
def test_tie_flagged_replica(Ks, monkeypatch):
    """Equal event times on the fast sweep (two RealData walls on the same times feeding
    disjoint sinks, sweep_mode=1): the replica is flagged RQ_ST_TIE, a tied row is written
    twice by the wave before it scans, and keeping the last row is the reference's pivot."""
    torch, engine, graphs, O = _ctx()
    T = np.round(np.linspace(0.5, 19.5, 77), 3)
    so = dict(src_id=1, end_time=20.0, s=np.asarray([1.0, 2.0]), q=0.7, sink_ids=[10, 11, 12],
              other_sources=[("RealData", {"src_id": 2, "times": T.tolist()}),
                             ("RealData", {"src_id": 3, "times": T.tolist()}),
                             ("Poisson", {"src_id": 4, "seed": 5, "rate": 2.0})],
              edge_list=[(1, 10), (1, 11), (2, 10), (3, 12), (4, 11)])
    g = _graph(engine, so)
    for seed in (1, 2):
        on = _on_off(torch, monkeypatch, g, q=so["q"], s=so["s"], n_rep=1, ctrl_seed=seed, Ks=Ks,
                     sweep_mode=1, check=False)
        assert int(on.status[0].item()) & 4   # RQ_ST_TIE
        _cmp_oracle(O, on, 0, so, ("opt", seed), Ks)


def test_row_capacity_overflow_rerun(monkeypatch):
    """Undersized capacities (RQ_CAP_SQUEEZE): the flagged first pass scans whatever rows it
    kept, Graph.run reruns the flagged replicas, and the result equals the normal run."""
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
    _cmp_oracle(O, got, 5, _seeded(so, 9 + 5), ("opt", 9 + 5), (1,))


def test_plans_that_keep_the_scan_kernel(monkeypatch):
    """The event-log and max_events runs, the generating fused sweep (sweep_mode=7) and the
    general sweep (> 64 sources) keep rq_scan, whatever the switch says."""
    torch, engine, graphs, O = _ctx()
    monkeypatch.delenv("RQ_SWEEP_SCAN", raising=False)
    so = dict(graphs.c3(), end_time=2.4)
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=8, ctrl_seed=3, world_seed=3, randomize=True, Ks=(1,))
    assert g.run("opt", plan_only=True, **kw)["sweep_scan"] == 1
    assert g.run("poisson", plan_only=True, ctrl_rate=1.5, **{k: v for k, v in kw.items() if k not in ("q", "s")})["sweep_scan"] == 1
    assert g.run("opt", plan_only=True, event_log=True, **kw)["sweep_scan"] == 0
    assert g.run("opt", plan_only=True, max_events=50, **kw)["sweep_scan"] == 0
    gen = g.run("opt", plan_only=True, sweep_mode=7, **kw)
    assert gen["variant"] == 12 and gen["sweep_scan"] == 0, gen
    wide = dict(graphs.g120(), end_time=2.0)
    gw = _graph(engine, wide)
    assert gw.run("opt", plan_only=True, **dict(kw, q=wide["q"], s=wide["s"]))["sweep_scan"] == 0
    # and they compute what they did: the switch changes nothing for them
    for graph, extra in ((g, dict(event_log=True)), (g, dict(max_events=50)), (g, dict(sweep_mode=7)),
                         (gw, dict(q=wide["q"], s=wide["s"]))):
        _on_off(torch, monkeypatch, graph, scan_on=False, **dict(kw, **extra))

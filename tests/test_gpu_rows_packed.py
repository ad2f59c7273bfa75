"""The merged fused sweep's pivot rows as 16-byte records {t, sumR u32, cnt u16, valid u16}
(the default where the plan reports sweep_rows16 = 1) against the four row arrays
(RQ_ROWS_PACKED=0), the separate scan kernel (RQ_SWEEP_SCAN=0, which reads the arrays) and
the engine oracle.

The records carry the same integers and the scan converts them the same way, so the bar is
bit-exact metrics (NaN pattern included), counts and status:
packed == RQ_ROWS_PACKED=0 == RQ_SWEEP_SCAN=0 == oracle.

What each case is there for is asserted from the CPU oracle's run of the same seeds (row
counts, which event wrote the last row, equal-time pairs, a post and a wall event in one
lane), never from the code under test.

Equal times.  Two wall events at one time that touch disjoint sinks leave every pivot cell
whole, and the fast sweeps' rule (keep the last row of a time) is the reference's pivot: those
flagged results are compared with the oracle as they are (check=False).  A post at the time
of the wall event before it touches the followers twice at one time; the reference averages
such cells, the fast sweeps flag the replica (RQ_ST_TIE) and Graph.run reruns it on the exact
sequential sweep.  There the three fast builds are compared flagged and unchecked, and the
checked run with the oracle.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ST_ROWS_OVERFLOW, ST_STREAM_OVERFLOW, ST_TIE, ST_EMPTY = 1, 2, 4, 8
SCAN_TU = 6   # rows per lane and trip of the packed scan: fws_tu(1, true) in rq_sweep_fw.hip


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


def _three(torch, monkeypatch, g, ctrl="opt", packed=1, **kw):
    """The run on 16-byte rows (the default), on the row arrays (RQ_ROWS_PACKED=0) and with
    rq_scan (RQ_SWEEP_SCAN=0): equal.  The plan reports each choice; packed=0: a run that
    keeps the arrays either way."""
    pkw = {k: v for k, v in kw.items() if k != "check"}
    monkeypatch.delenv("RQ_ROWS_PACKED", raising=False)
    monkeypatch.delenv("RQ_SWEEP_SCAN", raising=False)
    plan = g.run(ctrl, plan_only=True, **pkw)
    assert plan["sweep_scan"] == 1 and plan["variant"] >= 20, plan   # the merged fused sweep, its own scan
    assert plan["sweep_rows16"] == packed, plan
    on = g.run(ctrl, **kw)
    monkeypatch.setenv("RQ_ROWS_PACKED", "0")
    off_plan = g.run(ctrl, plan_only=True, **pkw)
    assert off_plan == dict(plan, sweep_rows16=0), (plan, off_plan)
    soa = g.run(ctrl, **kw)
    monkeypatch.delenv("RQ_ROWS_PACKED")
    monkeypatch.setenv("RQ_SWEEP_SCAN", "0")
    ker_plan = g.run(ctrl, plan_only=True, **pkw)
    assert ker_plan["sweep_scan"] == 0 and ker_plan["sweep_rows16"] == 0, ker_plan
    ker = g.run(ctrl, **kw)
    monkeypatch.delenv("RQ_SWEEP_SCAN")
    _same(torch, on, soa)
    _same(torch, on, ker)
    return on


def _seeded(so, u):
    """randomize_other_sources(u): other source idx gets seed u + 99 idx."""
    return dict(so, other_sources=[(n, dict(x, seed=(u + 99 * i) & 0xFFFFFFFF)) if "seed" in x else (n, x)
                                   for i, (n, x) in enumerate(so["other_sources"])])


_ORACLE = {}


def _oracle(O, so, ctrl, Ks, key=None):
    """The engine oracle's (metrics or None, (t, source)) of world so under ctrl; runs that
    several tests share are computed once (key)."""
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    met, (t_o, _, s_o) = O.engine_metrics(O.Scenario(so, ctrl), Ks)
    out = (met, t_o, s_o)
    if key is not None:
        _ORACLE[key] = out
    return out


def _cmp_oracle(O, res, i, so, ctrl, Ks=(1,), key=None):
    """Replica i of res == the engine oracle's run of world so under controller ctrl;
    returns the oracle's events (t, source)."""
    met, t_o, s_o = _oracle(O, so, ctrl, Ks, key)
    c = res.counts[i].cpu().numpy()
    m = res.metrics[i].cpu().numpy()
    assert c[2] == len(t_o), (i, c, len(t_o))
    if met is None:   # no event reached a sink: no row, every metric NaN
        assert c[3] == 0 and np.isnan(m).all(), (i, c, m)
        return t_o, s_o
    top, avg, r2, cnt = met
    assert np.array_equal(m, np.asarray(list(top) + [avg, r2])), (i, m, top, avg, r2)
    assert c[0] == cnt[0] and c[1] == cnt[1] and c[3] == cnt[2], (i, c, cnt)
    return t_o, s_o


def _syn(n_sinks, n_src=12, seed=5, rate=4.0, end_time=3.0, fol=1.0, frac=0.2):
    """n_src Poisson2 walls with random follower sets over n_sinks sinks (every sink has a
    wall source); the controlled source 1 follows the first fol x n_sinks sinks of a random
    order (all of them at fol = 1)."""
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


# ---- row counts per replica: the scan's leaf and trip edges ----
# README graph at K = 1 (about 25 rows per time unit): (controller, horizon, replicas, first
# seed) and the row counts the run is there for.  A leaf's eight lanes take 8 x SCAN_TU rows
# a trip, so 47 / 48 / 49 rows are a short last trip, one full trip, and one row into the
# serial tail; eight leaves' trips together are 8 x TU x 8 rows, here +- 1 for TU = 6 and for
# 4 and 8, the other two values DESIGN section 34 measured.
ROW_RUNS = [
    (("poisson", 5.0), 0.02, 32, 50, (0,)),
    (("opt",), 0.05, 64, 100, (1,)),
    (("opt",), 0.25, 128, 100, (7, 8, 9)),
    (("opt",), 1.9, 256, 100, (8 * SCAN_TU - 1, 8 * SCAN_TU, 8 * SCAN_TU + 1)),
    (("opt",), 2.55, 256, 100, (63, 64, 65)),
    (("opt",), 5.05, 384, 100, (127, 128, 129)),
    (("opt",), 10.1, 512, 100, (255, 256, 257)),
    (("opt",), 15.15, 640, 100, (383, 384, 385)),
    (("opt",), 20.2, 768, 100, (511, 512, 513)),
]
assert {64 * SCAN_TU - 1, 64 * SCAN_TU, 64 * SCAN_TU + 1} <= {n for r in ROW_RUNS for n in r[4]}


@pytest.mark.parametrize("run", ROW_RUNS, ids=lambda r: "rows_" + "_".join(str(n) for n in r[4]))
def test_row_counts_at_the_scan_edges(run, monkeypatch):
    torch, engine, graphs, O = _ctx()
    ctrl, end, R, seed0, want = run
    so = dict(graphs.readme(), end_time=end)
    g = _graph(engine, so)
    if ctrl[0] == "poisson":
        name, ckw = "poisson", dict(ctrl_rate=ctrl[1])
    else:
        name, ckw = "opt", dict(q=so["q"], s=so["s"])
    on = _three(torch, monkeypatch, g, name, n_rep=R, ctrl_seed=seed0, world_seed=seed0, randomize=True,
                Ks=(1,), **ckw)
    n = on.counts[:, 3].cpu().numpy()
    assert int((on.status & ~ST_EMPTY).max().item()) == 0
    assert torch.equal((on.status & ST_EMPTY) != 0, on.counts[:, 3] == 0)
    assert torch.equal(on.metrics.isnan().all(dim=1), on.counts[:, 3] == 0)
    pick = {0, R - 1}
    for k in want:
        hit = np.nonzero(n == k)[0]
        assert hit.size, (k, np.sort(n))
        pick.add(int(hit[0]))
    for i in sorted(pick):
        u = seed0 + i
        _cmp_oracle(O, on, i, _seeded(so, u), ("poisson", u, ctrl[1]) if ctrl[0] == "poisson" else ("opt", u))


def test_above_8192_rows(monkeypatch):
    """numpy sums blocks of 8192 rows one after the other: the README graph over 400 time
    units, about 10,000 rows a replica."""
    torch, engine, graphs, O = _ctx()
    so = dict(graphs.readme(), end_time=400.0)
    g = _graph(engine, so)
    on = _three(torch, monkeypatch, g, q=so["q"], s=so["s"], n_rep=2, ctrl_seed=7, world_seed=7,
                randomize=True, Ks=(1,))
    assert int(on.counts[:, 3].min().item()) > 8192
    assert int(on.status.max().item()) == 0
    for i in range(2):
        _cmp_oracle(O, on, i, _seeded(so, 7 + i), ("opt", 7 + i))


# ---- which stores wrote the rows ----
def _walls_and_posts(s, ctrl_id):
    """Per merged entry (wall event) k of an event log: whether a post comes right before it;
    and whether the log ends with a post."""
    before, post = [], False
    for x in s:
        if x == ctrl_id:
            post = True
        else:
            before.append(post)
            post = False
    return np.asarray(before, dtype=bool), post


def test_last_row_from_the_final_post_and_both_rows_of_a_lane(monkeypatch):
    """Replicas whose last row is the controller's post after the final arrival (lane 0
    writes it after the tile loop), replicas that end on a wall event, and lanes that hold
    a post row and a wall row (a post right before a wall event, at another time)."""
    torch, engine, graphs, O = _ctx()
    so = dict(graphs.readme(), end_time=3.0)
    g = _graph(engine, so)
    R = 24
    on = _three(torch, monkeypatch, g, q=so["q"], s=so["s"], n_rep=R, ctrl_seed=300, world_seed=300,
                randomize=True, Ks=(1,))
    assert int(on.status.max().item()) == 0
    final_post = final_wall = both = 0
    for i in range(R):
        t_o, s_o = _cmp_oracle(O, on, i, _seeded(so, 300 + i), ("opt", 300 + i))
        before, ends_on_post = _walls_and_posts(s_o, so["src_id"])
        final_post += ends_on_post
        final_wall += not ends_on_post
        # every README source has an edge, so a post before wall entry k puts both rows in lane k % 64
        post_t = t_o[np.nonzero(s_o == so["src_id"])[0]]
        wall_t = t_o[s_o != so["src_id"]]
        assert len(set(post_t) & set(wall_t)) == 0   # no equal times: both rows are kept
        both += int(before[1:].sum())
    assert final_post > 0 and final_wall > 0 and both > 0, (final_post, final_wall, both)


def _post_ties(t, s, ctrl_id):
    """Of an event log under a controller whose posts fall on the time of the wall event
    before them: (ties inside a tile, ties of a tile's first post with the last wall event of
    the tile before it, whether the final post ties the last wall event)."""
    inside = across = 0
    k = 0   # merged entries so far
    for i in range(1, len(s)):
        if s[i - 1] != ctrl_id:
            k += 1
        if s[i] == ctrl_id and s[i - 1] != ctrl_id and t[i] == t[i - 1] and i + 1 < len(s):
            if k % 64 == 0:
                across += 1
            else:
                inside += 1
    final = len(s) >= 2 and s[-1] == ctrl_id and s[-2] != ctrl_id and t[-1] == t[-2]
    return inside, across, bool(final)


def test_posts_on_the_time_of_the_wall_event_before(monkeypatch):
    """q so small that a post's delay rounds away against the time it is added to: a post
    shares the time of the wall event before it.  Inside a tile the wall row is dropped; at a
    tile's first lane the record at nrow - 1 is rewritten (tie0); after the last arrival the
    final post overwrites the last record (the RQ_ST_TIE branch of the lane-0 write)."""
    torch, engine, graphs, O = _ctx()
    so = dict(graphs.readme(), end_time=8.0, q=1e-30)
    g = _graph(engine, so)
    R = 16
    kw = dict(q=so["q"], s=so["s"], n_rep=R, ctrl_seed=40, world_seed=40, randomize=True, Ks=(1,))
    raw = _three(torch, monkeypatch, g, check=False, **kw)
    got = _three(torch, monkeypatch, g, **kw)   # flagged replicas rerun on the exact sweep
    inside = across = final = 0
    for i in range(R):
        t_o, s_o = _cmp_oracle(O, got, i, _seeded(so, 40 + i), ("opt", 40 + i))
        a, b, c = _post_ties(t_o, s_o, so["src_id"])
        if a + b + c > 0:
            assert int(raw.status[i].item()) & ST_TIE, (i, a, b, c)
        assert int(raw.counts[i, 2].item()) == len(t_o)
        inside, across, final = inside + a, across + b, final + c
    assert inside > 0 and across > 0 and final > 0, (inside, across, final)
    assert int((got.status & ~ST_TIE).max().item()) == 0   # the exact sweep reports the ties too


@pytest.mark.parametrize("Ks", [(1,), (2,)])
def test_wall_events_at_one_time(Ks, monkeypatch):
    """Two RealData walls on the same times feeding disjoint sinks (sweep_mode=1 keeps the
    fast sweep): every pair is an equal-time pair of wall rows, the first of them dropped,
    across tile boundaries too (77 pairs and a Poisson wall in tiles of 64); the flagged
    result is the reference's pivot."""
    torch, engine, graphs, O = _ctx()
    T = np.round(np.linspace(0.5, 19.5, 77), 3)
    so = dict(src_id=1, end_time=20.0, s=np.asarray([1.0, 2.0]), q=0.7, sink_ids=[10, 11, 12],
              other_sources=[("RealData", {"src_id": 2, "times": T.tolist()}),
                             ("RealData", {"src_id": 3, "times": T.tolist()}),
                             ("Poisson", {"src_id": 4, "seed": 7, "rate": 2.0})],
              edge_list=[(1, 10), (1, 11), (2, 10), (3, 12), (4, 11)])
    g = _graph(engine, so)
    straddle = 0
    for seed in (1, 2, 3):
        on = _three(torch, monkeypatch, g, q=so["q"], s=so["s"], n_rep=1, ctrl_seed=seed, Ks=Ks,
                    sweep_mode=1, check=False)
        assert int(on.status[0].item()) & ST_TIE
        t_o, s_o = _cmp_oracle(O, on, 0, so, ("opt", seed), Ks)
        walls = np.nonzero(s_o != so["src_id"])[0]
        # a pair whose first wall event is a tile's last entry and whose second opens the next
        # tile without a post between them: the row at nrow - 1 is rewritten (tie0)
        for k in range(63, len(walls) - 1, 64):
            a, b = walls[k], walls[k + 1]
            straddle += int(b == a + 1 and t_o[a] == t_o[b])
    assert straddle > 0


# ---- plans ----
@pytest.mark.parametrize("Ks", [(1,), (2,), (5,)])
def test_readme_grid(Ks, monkeypatch):
    """The one-word graph of C4 on a q grid from its corners: the sink-bit instance at
    Ks = (1,), the uint16 column instance at one other K."""
    torch, engine, graphs, O = _ctx()
    so = dict(graphs.readme(), end_time=6.0)
    g = _graph(engine, so)
    R = 33
    qs = np.asarray([1e-4, 1.0, 1e7])
    kw = dict(q=qs, s=so["s"], n_rep=R, ctrl_seed=21, world_seed=21, randomize=True, Ks=Ks)
    plan = g.run("opt", plan_only=True, **kw)
    assert plan["variant"] == (22 if Ks == (1,) else 20) and plan["columns_in_lds"] == 1, plan
    full = _three(torch, monkeypatch, g, **kw)
    assert int(full.status.max().item()) == 0
    for i in (0, R - 1, R, 2 * R - 1, 2 * R, 3 * R - 1):
        u = 21 + i   # replica i of the whole grid takes seed 21 + i
        _cmp_oracle(O, full, i, _seeded(dict(so, q=float(qs[i // R])), u), ("opt", u), Ks)


@pytest.mark.parametrize("Ks", [(1,), (3,)])
def test_c3_short_horizon(Ks, monkeypatch):
    """C3's graph (1000 sinks: the event-blocked sink-bit instance at Ks = (1,), uint16
    columns at another K) over a few tiles."""
    torch, engine, graphs, O = _ctx()
    so = dict(graphs.c3(), end_time=2.4)
    g = _graph(engine, so)
    R = 40
    on = _three(torch, monkeypatch, g, q=so["q"], s=so["s"], n_rep=R, ctrl_seed=5, world_seed=5,
                randomize=True, Ks=Ks)
    assert int(on.status.max().item()) == 0
    assert int(on.counts[:, 1].min().item()) > 64
    for i in (0, 17, R - 1):
        _cmp_oracle(O, on, i, _seeded(so, 5 + i), ("opt", 5 + i), Ks)


def test_follower_set_not_full(monkeypatch):
    """The controller follows 60 % of 430 sinks and each of 40 wall sources reaches about
    11: after the first tile's 64 wall events sinks are still without a row, so the records
    of the first tiles carry valid < n_sinks."""
    torch, engine, graphs, O = _ctx()
    so = _syn(430, n_src=40, fol=0.6, frac=0.0, rate=1.0, end_time=6.0)
    g = _graph(engine, so)
    R = 32
    on = _three(torch, monkeypatch, g, q=so["q"], s=so["s"], n_rep=R, ctrl_seed=70, world_seed=70,
                randomize=True, Ks=(1,))
    assert int(on.status.max().item()) == 0
    reach = {}
    for a, b in so["edge_list"]:
        reach.setdefault(a, set()).add(b)
    for i in (0, 9, R - 1):
        _, s_o = _cmp_oracle(O, on, i, _seeded(so, 70 + i), ("opt", 70 + i))
        walls = [x for x in s_o if x != so["src_id"]]
        assert len(walls) > 128
        seen = set(reach[so["src_id"]])
        for x in walls[:64]:
            seen |= reach[x]
        assert len(seen) < 430, len(seen)


def test_more_than_65535_sinks_keeps_the_arrays(monkeypatch):
    """70,000 sinks at one K > 1: int columns read from global memory; valid and cnt do not
    fit 16 bits, the plan keeps the row arrays and the switch changes nothing."""
    torch, engine, graphs, O = _ctx()
    so = _syn(70000, n_src=6, seed=2, rate=3.0, end_time=2.0, fol=0.01, frac=0.001)
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=4, ctrl_seed=3, world_seed=3, randomize=True, Ks=(2,))
    plan = g.run("opt", plan_only=True, **kw)
    assert plan["variant"] == 20 and plan["columns_in_lds"] == 0, plan
    on = _three(torch, monkeypatch, g, packed=0, **kw)
    assert int(on.status.max().item()) == 0
    _cmp_oracle(O, on, 1, _seeded(so, 3 + 1), ("opt", 3 + 1), (2,))


# ---- launch shapes ----
def test_more_replicas_than_resident_waves(monkeypatch):
    """One replica more than the launch has waves: every wave scans its records and then
    sweeps another replica into the records of that one."""
    torch, engine, graphs, O = _ctx()
    so = dict(graphs.readme(), end_time=3.0)
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], ctrl_seed=11, world_seed=11, randomize=True, Ks=(1,))
    plan = g.run("opt", n_rep=4097, plan_only=True, **kw)
    slots = plan["blocks_per_cu"] * plan["waves_per_block"] * torch.cuda.get_device_properties(0).multi_processor_count
    R = max(4097, slots + 1)
    assert g.run("opt", n_rep=R, plan_only=True, chunk=R, **kw)["chunk"] == R   # one launch
    on = _three(torch, monkeypatch, g, n_rep=R, chunk=R, **kw)
    assert int(on.status.max().item()) == 0
    for i in (0, 1, slots - 1, slots, R - 1, R // 2):
        i = min(i, R - 1)
        _cmp_oracle(O, on, i, _seeded(so, 11 + i), ("opt", 11 + i))


def test_chunks_and_rep_idx(monkeypatch):
    """chunk= smaller than the call (the last chunk short: its records start at the set's
    base again) and a rep_idx subset of the same batch."""
    torch, engine, graphs, O = _ctx()
    so = dict(graphs.c3(), end_time=2.4)
    g = _graph(engine, so)
    R = 33
    qs = np.asarray([so["q"], 0.25 * so["q"]])
    kw = dict(q=qs, s=so["s"], n_rep=R, ctrl_seed=21, world_seed=21, randomize=True, Ks=(1,))
    full = _three(torch, monkeypatch, g, **kw)
    assert g.run("opt", plan_only=True, chunk=7, **kw)["chunk"] == 7
    cut = _three(torch, monkeypatch, g, chunk=7, **kw)
    _same(torch, cut, full)
    for i in (0, 6, 7, R, 2 * R - 1):
        u = 21 + i
        _cmp_oracle(O, full, i, _seeded(dict(so, q=float(qs[i // R])), u), ("opt", u))
    pick = np.asarray([0, 5, 32, 33, 40, 65])
    sub = _three(torch, monkeypatch, g, rep_idx=pick, **kw)
    for k, i in enumerate(pick):
        assert torch.equal(sub.counts[k], full.counts[i]) and torch.equal(sub.metrics[k], full.metrics[i])


def test_row_capacity_overflow_and_rerun(monkeypatch):
    """Undersized capacities (RQ_CAP_SQUEEZE): the flagged first pass scans the records it
    kept (writes past the capacity are dropped), Graph.run reruns the flagged replicas with
    doubled capacities -- a plan that decides on the layout again -- and the result equals
    the normal run.  Flagged and rerun alike equal the array build's."""
    torch, engine, graphs, O = _ctx()
    so = graphs.c3()
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=64, ctrl_seed=9, world_seed=9, randomize=True, Ks=(1,))
    ref = _three(torch, monkeypatch, g, **kw)
    monkeypatch.setenv("RQ_CAP_SQUEEZE", "0.45")
    raw = _three(torch, monkeypatch, g, check=False, **kw)
    assert int(((raw.status & (ST_ROWS_OVERFLOW | ST_STREAM_OVERFLOW)) != 0).sum().item()) > 0
    got = _three(torch, monkeypatch, g, **kw)
    assert int(got.status.max().item()) == 0
    _same(torch, got, ref)
    _cmp_oracle(O, got, 5, _seeded(so, 9 + 5), ("opt", 9 + 5))


# ---- plans through plan_only=True, no launch ----
def test_what_the_plan_reports(monkeypatch):
    torch, engine, graphs, O = _ctx()
    monkeypatch.delenv("RQ_ROWS_PACKED", raising=False)
    monkeypatch.delenv("RQ_SWEEP_SCAN", raising=False)
    c3 = graphs.c3()
    g3 = _graph(engine, c3)
    kw3 = dict(q=c3["q"], s=c3["s"], n_rep=10000, randomize=True)
    p3 = g3.run("opt", plan_only=True, **kw3)
    assert p3["sweep_rows16"] == 1 and p3["sweep_scan"] == 1 and p3["sweep_blk"] == 1 and p3["variant"] == 22, p3
    assert g3.run("opt", plan_only=True, Ks=(1, 2), **kw3)["sweep_rows16"] == 0     # nK = 2
    assert g3.run("opt", plan_only=True, Ks=(2,), **kw3)["sweep_rows16"] == 1       # one K on columns
    assert g3.run("opt", plan_only=True, event_log=True, **kw3)["sweep_rows16"] == 0   # no scan of its own
    assert g3.run("opt", plan_only=True, sweep_mode=7, **kw3)["sweep_rows16"] == 0
    rd = graphs.readme()
    g4 = _graph(engine, rd)
    grid = graphs.c4_grid()
    kw4 = dict(q=np.array([q for q, _ in grid]), s=np.array([s for _, s in grid], dtype=np.float64), n_rep=1000,
               seed_mod=1000)
    p4 = g4.run("opt", plan_only=True, **kw4)
    assert p4["sweep_rows16"] == 1 and p4["variant"] == 22, p4
    # 2000 sinks: sumR stays below 2^32 up to 2^32 / 2000 = 2,147,483 merged entries a
    # replica.  50 Poisson walls over 100 time units at rate 300 give 1.5 M wall events
    # (+ 8 sigma ~ 10^4), at rate 500 2.5 M.
    under = _syn(2000, n_src=50, seed=9, rate=300.0, end_time=100.0)
    over = _syn(2000, n_src=50, seed=9, rate=500.0, end_time=100.0)
    kwu = dict(q=under["q"], s=under["s"], n_rep=4, randomize=True)
    pu = _graph(engine, under).run("opt", plan_only=True, **kwu)
    po = _graph(engine, over).run("opt", plan_only=True, **kwu)
    assert pu["variant"] == 22 and po["variant"] == 22 and pu["sweep_scan"] == 1 and po["sweep_scan"] == 1, (pu, po)
    assert pu["sweep_rows16"] == 1 and po["sweep_rows16"] == 0, (pu, po)
    # the switch: 0 everywhere, every other key unchanged
    monkeypatch.setenv("RQ_ROWS_PACKED", "0")
    for g, kw, p in ((g3, kw3, p3), (g4, kw4, p4), (_graph(engine, under), kwu, pu)):
        assert g.run("opt", plan_only=True, **kw) == dict(p, sweep_rows16=0)

"""rq_log_timeline / BatchResult.timeline / batch.run_timeline on the GPU against the
host checker tests/timeline_ref.py (oracle.rank_table + exactly rounded per-bin sums;
tests/test_timeline_cpu.py pins it to the reference's own tables).

Tolerance (derived, not measured): a bin value is a sum of at most n non-negative terms
of at most 4 roundings each, so whatever the summation order
|got - exp| <= (n + 8) * 2**-52 * exp with n = counts[i][3], the replica's pivot rows;
a bin whose expectation is 0 must be exactly 0.0; integer outputs must be equal."""
import numpy as np
import pytest

from tests import timeline_ref as TR
from tests.loghelp import (ctx as _ctx, graph as _graph, pack as _pack, raw_timeline as _raw,
                           same_bits as _same_bits)

pytestmark = pytest.mark.gpu


def _assert_close(got, exp, rows, what):
    print(what, "max |got - exp| / (ulp exp) = %.3g over %d rows" % (
        float(np.max(np.abs(got - exp) / np.maximum(TR.ULP * np.abs(exp), 1e-300))) if got.size else 0.0, rows))
    assert got.shape == exp.shape, what
    assert not np.isnan(got).any(), what
    assert (got[exp == 0.0] == 0.0).all(), what
    bad = np.abs(got - exp) > TR.tol(rows, exp)
    assert not bad.any(), (what, np.argwhere(bad)[:4], got[bad][:4], exp[bad][:4])


# ------------------------------------------------------------- 1. fixture logs, raw ABI
def test_fixture_logs_through_the_raw_abi(golden):
    torch, O, L, engine, graphs = _ctx()
    f = golden("timeline.npz")
    Ks = [int(k) for k in f["Ks"]]
    for name in (str(n) for n in f["names"]):
        src_id, end = int(f[name + "_world"][0]), float(f[name + "_world"][1])
        so = dict(src_id=src_id, end_time=end, sink_ids=[int(x) for x in f[name + "_sinks"]],
                  edge_list=[tuple(int(v) for v in e) for e in f[name + "_edges"]],
                  other_sources=[("Poisson2", {"src_id": int(s), "seed": 1, "rate": 1.0})
                                 for s in f[name + "_srcs"]])
        g = _graph(engine, so)
        t, s = f[name + "_t"], f[name + "_src"]
        ev_t, ev_src, counts = _pack([(t, s)], t.size + 77, g)
        rows = int(f[name + "_rows"][0])
        for k in (0, 1):
            edges = f["%s_bins%d" % (name, k)]
            met, pst, sta, w = _raw(torch, L, g, ev_t, ev_src, counts, edges, Ks, wall=True)
            assert sta[0] == 0, name
            _assert_close(met[0], f["%s_met%d" % (name, k)], rows, "%s/%d" % (name, k))
            assert np.array_equal(pst[0], f["%s_posts%d" % (name, k)]), name
            assert np.array_equal(w[0], f["%s_wall%d" % (name, k)]), name


# ------------------------------------------------- 2. README graph, every controller
def _readme_edge_sets(so, t0):
    T = so["end_time"]
    mid = float(t0[len(t0) // 2])
    return {"one": [0.0, T],
            "uneven7": [1.5, 2.0, 9.75, 10.0, 33.0, 60.5, 61.0, 97.5],
            "on_event": [0.0, mid, T],
            "eq65": [T * k / 65 for k in range(65)] + [T],
            "eq1000": [T * k / 1000 for k in range(1000)] + [T]}


@pytest.mark.parametrize("ctrl", ["opt", "poisson", "wall", "times"])
def test_readme_graph_every_edge_set(ctrl):
    torch, O, L, engine, graphs = _ctx()
    so = graphs.readme()
    Ks = (1, 2, 33)
    R = 8
    kw = dict(n_rep=R, ctrl_seed=500, world_seed=900, randomize=True, Ks=Ks, event_log=True)
    if ctrl == "opt":
        kw.update(q=so["q"], s=so["s"])
    if ctrl == "poisson":
        kw.update(ctrl_rate=torch.linspace(0.5, 6.0, R, dtype=torch.float64))
    gkw = {}
    if ctrl == "times":
        gkw["ctrl_a"] = np.sort(np.random.RandomState(3).uniform(0.0, so["end_time"], 120))
    g = _graph(engine, so, **gkw)
    res = g.run(ctrl, **kw)
    ro, cols = res.log_columns()
    host = {k: cols[k].cpu().numpy() for k in ("t", "src_id", "sink_id", "event_id")}
    counts = res.counts.cpu().numpy()
    whole = res.metrics.cpu().numpy()
    assert (res.status.cpu().numpy() == 0).all()
    t0, _ = res.events(0)
    sets = _readme_edge_sets(so, t0)
    assert sets["on_event"][1] in t0
    tabs = []
    for i in range(R):
        a, b = int(ro[i]), int(ro[i + 1])
        tab, idx, _sinks = O.rank_table(host["t"][a:b], host["src_id"][a:b], host["sink_id"][a:b],
                                        g.src_id, True)
        assert tab.shape[0] == counts[i, 3]
        tabs.append((tab, idx, a, b))
    for name, edges in sets.items():
        tl = res.timeline(edges=edges, wall=(name == "uneven7"))
        met, pst = tl.metrics.cpu().numpy(), tl.posts.cpu().numpy()
        assert (tl.status.cpu().numpy() == 0).all(), name
        for i, (tab, idx, a, b) in enumerate(tabs):
            exp = TR.bin_table(tab, idx, so["end_time"], edges, Ks)
            _assert_close(met[i], exp, int(counts[i, 3]), "%s %s replica %d" % (ctrl, name, i))
            assert np.array_equal(pst[i], TR.posts(host["t"][a:b], host["src_id"][a:b], g.src_id,
                                                   edges, host["event_id"][a:b])), (name, i)
            if tl.wall_posts is not None:
                assert np.array_equal(tl.wall_posts[i].cpu().numpy(),
                                      TR.wall_posts(host["t"][a:b], host["src_id"][a:b],
                                                    host["sink_id"][a:b], g.src_id, edges, tl.sink_ids))
        if edges[0] == 0.0 and edges[-1] == so["end_time"]:
            assert np.array_equal(pst.sum(1), counts[:, :2]), name
            tot = met.sum(1)
            for i in range(R):
                lim = TR.tol(int(counts[i, 3]), whole[i])
                assert (np.abs(tot[i] - whole[i]) <= lim).all(), (name, i, tot[i], whole[i])
    # the accessors and bins=n
    tl = res.timeline(bins=65)
    assert np.array_equal(tl.edges, np.asarray(sets["eq65"]))
    assert tl.top_k(33).shape == tl.avg_rank.shape == tl.r_2.shape == (R, 65)
    assert torch.equal(tl.r_2, tl.metrics[:, :, 4]) and torch.equal(tl.top_k(2), tl.metrics[:, :, 1])


# ------------------------------------------------------------------- 3. wide rows
def _wide_world():
    sinks = list(range(1000, 1131))                       # 131 sinks
    edges = [(2, s) for s in sinks[:130]] + [(1, s) for s in sinks[30:100]] + [(3, sinks[130])]
    edges = [edges[i] for i in np.random.RandomState(5).permutation(len(edges))]
    return dict(src_id=1, end_time=10.0, q=100.0, s=1.0, sink_ids=sinks, edge_list=edges,
                other_sources=[("Poisson", {"src_id": 2, "seed": 1, "rate": 25.0}),
                               ("RealData", {"src_id": 3, "times": [8.75, 9.5]})])


def test_wide_rows_and_wall_posts():
    torch, O, L, engine, graphs = _ctx()
    so = _wide_world()
    g = _graph(engine, so)
    R, Ks = 5, (1, 3)
    res = g.run("opt", q=so["q"], s=so["s"], n_rep=R, ctrl_seed=11, world_seed=70, randomize=True,
                Ks=Ks, event_log=True)
    counts = res.counts.cpu().numpy()
    assert (counts[:, 2] > 64).all() and counts[:, 2].mean() > 200 and (counts[:, 0] > 3).all()
    ro, cols = res.log_columns()
    host = {k: cols[k].cpu().numpy() for k in ("t", "src_id", "sink_id", "event_id")}
    for edges in ([0.0, 10.0], [0.5, 1.0, 4.0, 4.25, 8.0, 9.0, 9.75, 10.0]):
        tl = res.timeline(edges=edges, wall=True)
        met, pst, w = tl.metrics.cpu().numpy(), tl.posts.cpu().numpy(), tl.wall_posts.cpu().numpy()
        wi = tl.wall_intensities().cpu().numpy()
        assert (tl.status.cpu().numpy() == 0).all()
        for i in range(R):
            a, b = int(ro[i]), int(ro[i + 1])
            t, s, x = host["t"][a:b], host["src_id"][a:b], host["sink_id"][a:b]
            exp, rows = TR.metrics(O, t, s, x, g.src_id, so["end_time"], edges, Ks)
            assert rows == counts[i, 3]
            _assert_close(met[i], exp, rows, "wide replica %d" % i)
            assert np.array_equal(pst[i], TR.posts(t, s, g.src_id, edges, host["event_id"][a:b]))
            ew = TR.wall_posts(t, s, x, g.src_id, edges, so["sink_ids"])
            assert np.array_equal(w[i], ew)
            assert np.array_equal(wi[i], ew / np.diff(np.asarray(edges)))
        assert w[:, 130, :].sum() == 2 * R and w[:, :130, :].sum() > 0


# ---------------------------------------------------------------- 4. hand-made ties
TIE_WORLD = dict(src_id=1, end_time=20.0, sink_ids=[10, 11, 12, 13],
                 edge_list=[(1, 10), (1, 12), (2, 10), (2, 11), (3, 12), (4, 13), (4, 11)],
                 other_sources=[("Poisson2", {"src_id": s, "seed": 1, "rate": 1.0}) for s in (2, 3, 4, 5)])


def test_hand_made_ties_and_empty():
    torch, O, L, engine, graphs = _ctx()
    so = TIE_WORLD
    g = _graph(engine, so)
    Ks = (1, 2)
    edges = [0.0, 2.0, 5.0, 5.5, 11.0, 20.0]
    plain = ([0.5, 1.0, 2.0, 3.0, 7.0, 11.0, 13.5], [2, 3, 1, 4, 2, 1, 3])
    # equal times on disjoint sinks: (2 | 3), (1 | 4), (3 | 4); source 5 has no edge
    disjoint = ([0.5, 2.0, 2.0, 5.0, 5.0, 5.0, 9.0, 9.0, 16.0], [4, 2, 3, 1, 5, 4, 3, 4, 2])
    # sink 10 gets a wall row and an own row at t = 5
    tied = ([0.5, 2.0, 5.0, 5.0, 9.0, 12.0], [3, 4, 2, 1, 3, 2])
    other = ([1.25, 4.0, 6.0, 6.0 + 2.0 ** -40, 19.0], [1, 2, 3, 1, 4])
    empty = ([], [])
    no_rows = ([1.0, 2.0], [5, 5])     # events of a source without edges only
    logs = [plain, tied, disjoint, empty, other, no_rows]
    ev_t, ev_src, counts = _pack(logs, 16, g)
    met, pst, sta, w = _raw(torch, L, g, ev_t, ev_src, counts, edges, Ks, wall=True)
    assert list(sta) == [0, L.ST_TIE, 0, L.ST_EMPTY, 0, L.ST_EMPTY]
    assert np.isnan(met[1]).all() and np.isnan(met[3]).all() and np.isnan(met[5]).all()
    assert (pst[3] == 0).all() and (pst[5] == 0).all() and (w[3] == 0).all() and (w[5] == 0).all()
    for i in (0, 1, 2, 4):
        t, s, x, eid = TR.frame_of(logs[i][0], logs[i][1], so["edge_list"])
        assert np.array_equal(pst[i], TR.posts(t, s, 1, edges, eid)), i
        assert np.array_equal(w[i], TR.wall_posts(t, s, x, 1, edges, so["sink_ids"])), i
        if i != 1:
            exp, rows = TR.metrics(O, t, s, x, 1, so["end_time"], edges, Ks)
            _assert_close(met[i], exp, rows, "hand-made %d" % i)
    # the neighbours of the flagged replicas: the bits they have without them
    logs2 = [plain, other, disjoint, other, other, plain]
    met2, pst2, sta2, w2 = _raw(torch, L, g, *_pack(logs2, 16, g), edges, Ks, wall=True)
    assert (sta2 == 0).all()
    for i in (0, 2, 4):
        assert _same_bits(met[i], met2[i]) and np.array_equal(pst[i], pst2[i]) and np.array_equal(w[i], w2[i])


# ------------------------------------------------------------------ 5. determinism
def test_same_bits_twice_and_alone():
    torch, O, L, engine, graphs = _ctx()
    so = graphs.readme()
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=8, ctrl_seed=21, world_seed=33, randomize=True, Ks=(1, 2),
              event_log=True)
    res = g.run("opt", **kw)
    a = res.timeline(bins=24, wall=True)
    b = res.timeline(bins=24, wall=True)
    for x, y in ((a.metrics, b.metrics), (a.posts, b.posts), (a.wall_posts, b.wall_posts)):
        assert torch.equal(x, y)
    sub = g.run("opt", rep_idx=[1, 3], **kw)
    c = sub.timeline(bins=24, wall=True)
    at = torch.tensor([1, 3], device=a.metrics.device)
    assert _same_bits(c.metrics.cpu().numpy(), a.metrics[at].cpu().numpy())
    assert torch.equal(c.posts, a.posts[at]) and torch.equal(c.wall_posts, a.wall_posts[at])
    assert (c.status == 0).all()


# ------------------------------------------------------------------- 6. validation
def test_validation():
    torch, O, L, engine, graphs = _ctx()
    g = _graph(engine, TIE_WORLD)
    lib = L.lib()
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    k1 = np.asarray([1, 2, 3, 4, 5], dtype=np.int32)
    k0 = np.asarray([1, 0], dtype=np.int32)

    def call(h=g._h, ev_t=p, ev_src=p, counts=p, n_rep=2, cap=4, edges=p, nb=3, ks=k1, nK=2, met=p,
             pst=p, wp=None, sta=p):
        return lib.rq_log_timeline(h, ev_t, ev_src, counts, n_rep, cap, edges, nb,
                                   ks.ctypes.data_as(L._pi32), nK, met, pst, wp, sta, None)
    bad = [dict(nb=0), dict(nK=0), dict(nK=5), dict(ks=k0), dict(n_rep=0), dict(cap=0), dict(met=None),
           dict(pst=None), dict(sta=None), dict(h=None), dict(ev_t=None), dict(ev_src=None),
           dict(counts=None), dict(edges=None)]
    for kw in bad:
        assert call(**kw) == L.RQ_EINVAL, kw
    torch.cuda.synchronize()
    assert (buf == 0).all()   # nothing was launched
    dup = dict(TIE_WORLD, edge_list=TIE_WORLD["edge_list"] + [(2, 10)])
    assert call(h=_graph(engine, dup)._h) == L.RQ_EUNSUPPORTED
    res = g.run("wall", n_rep=2, Ks=(1,), event_log=True)
    for e in ([0.0, 5.0, 5.0, 20.0], [0.0, 7.0, 3.0], [0.0, float("nan"), 20.0], [0.0, float("inf")], [1.0]):
        with pytest.raises(ValueError):
            res.timeline(edges=e)
    with pytest.raises(ValueError):
        res.timeline()
    with pytest.raises(ValueError):
        res.timeline(bins=0)
    with pytest.raises(ValueError):
        res.timeline(bins=4, Ks=(0,))
    with pytest.raises(ValueError):
        g.run("wall", n_rep=2, Ks=(1,)).timeline(bins=4)   # no event log


def test_sink_limit():
    """RQ_TIMELINE_MAX_SINKS sinks run (the per-sink state of one replica fills 144 KiB of
    LDS with wall_posts); one more is refused."""
    torch, O, L, engine, graphs = _ctx()
    N = L.TIMELINE_MAX_SINKS
    sinks = list(range(1, N + 2))

    def world(n):
        return dict(src_id=1, end_time=10.0, sink_ids=sinks[:n],
                    edge_list=[(2, s) for s in sinks[:n]] + [(1, s) for s in sinks[:n:3]] + [(3, sinks[n - 1])],
                    other_sources=[("Poisson2", {"src_id": 2, "seed": 1, "rate": 1.0}),
                                   ("Poisson2", {"src_id": 3, "seed": 1, "rate": 1.0})])
    so = world(N)
    g = _graph(engine, so)
    logs = [([0.5, 1.0, 2.5, 4.0, 4.0 + 2.0 ** -30, 7.0, 9.0], [3, 1, 2, 2, 1, 2, 3]), ([3.0, 6.0], [2, 1])]
    edges = [0.0, 1.0, 4.0, 8.0, 10.0]
    Ks = (1, 2)
    met, pst, sta, w = _raw(torch, L, g, *_pack(logs, 9, g), edges, Ks, wall=True)
    assert (sta == 0).all()
    for i in range(2):
        t, s, x, eid = TR.frame_of(logs[i][0], logs[i][1], so["edge_list"])
        exp, rows = TR.metrics(O, t, s, x, 1, so["end_time"], edges, Ks)
        _assert_close(met[i], exp, rows, "limit %d" % i)
        assert np.array_equal(pst[i], TR.posts(t, s, 1, edges, eid))
        assert np.array_equal(w[i], TR.wall_posts(t, s, x, 1, edges, so["sink_ids"]))
    g2 = _graph(engine, world(N + 1))
    _raw(torch, L, g2, *_pack(logs, 9, g2), edges, Ks, expect=L.RQ_EUNSUPPORTED)
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rq.h")).read()
    assert int(re.search(r"#define RQ_TIMELINE_MAX_SINKS\s+(\d+)", hdr).group(1)) == N >= 10000


# ------------------------------------------------------------- 7. batch.run_timeline
def test_run_timeline_matches_one_batch_and_any_chunking():
    torch, O, L, engine, graphs = _ctx()
    import pandas as pd
    from redqueen_amd import batch
    from redqueen_amd.opt_model import SimOpts
    so = SimOpts(**graphs.readme())
    seeds = np.arange(300, 364)
    Ks = (1, 2)
    f1 = batch.run_timeline(so, seeds, bins=10, Ks=Ks, chunk_replicas=64)
    f2 = batch.run_timeline(so, seeds, bins=10, Ks=Ks, chunk_replicas=24)
    f3 = batch.run_timeline(so, seeds, bins=10, Ks=Ks)
    pd.testing.assert_frame_equal(f1, f2, check_exact=True)
    pd.testing.assert_frame_equal(f1, f3, check_exact=True)
    g = batch.compiled_graph(so)
    st = torch.as_tensor(seeds)
    res = g.run("opt", q=float(so.q), s=so.s, n_rep=64, ctrl_seed=st, world_seed=st, randomize=True,
                Ks=Ks, event_log=True)
    tl = res.timeline(bins=10)
    assert (tl.status == 0).all()
    v = torch.cat([tl.metrics, tl.posts.to(torch.float64)], dim=2).cpu().numpy()   # [64, 10, 6]
    names = ["top_1", "top_2", "avg_rank", "r_2", "own_posts", "other_posts"]
    assert list(f1.columns) == ["t_lo", "t_hi"] + [c for n in names for c in (n, n + "_se")] + ["n", "n_flagged"]
    assert np.array_equal(f1.t_lo.values, np.arange(10) * 10.0) and np.array_equal(f1.t_hi.values, np.arange(1, 11) * 10.0)
    assert (f1.n == 64).all() and (f1.n_flagged == 0).all()
    for k, n in enumerate(names):
        mean = v[:, :, k].mean(0)
        sem = v[:, :, k].std(0, ddof=1) / np.sqrt(64.0)
        # 64 values summed in another order: a few ulp of the mean / of the error
        assert np.allclose(f1[n].values, mean, rtol=64 * TR.ULP, atol=0.0), n
        assert np.allclose(f1[n + "_se"].values, sem, rtol=1e-12, atol=0.0), n
    # flagged replicas are left out and counted
    fr = batch.timeline_frame(tl.edges, tl.Ks, v[:, :, :4], v[:, :, 4:].astype(np.int64),
                              np.asarray([0, L.ST_TIE, L.ST_EMPTY] + [0] * 61))
    assert (fr.n == 62).all() and (fr.n_flagged == 2).all()
    assert np.allclose(fr.top_1.values, v[[0] + list(range(3, 64)), :, 0].mean(0), rtol=64 * TR.ULP, atol=0.0)


def test_manager_result_timeline():
    """Manager.run_dynamic keeps its BatchResult: the one run's curve needs no further code."""
    torch, O, L, engine, graphs = _ctx()
    from redqueen_amd.opt_model import SimOpts
    so = SimOpts(**graphs.readme())
    m = so.create_manager_with_opt(seed=101)
    m.run_dynamic()
    tl = m.result.timeline(bins=5)            # Ks: the result's own
    assert tl.Ks == m.result.Ks and tl.metrics.shape == (1, 5, len(tl.Ks) + 2)
    df = m.state.get_dataframe()
    exp, rows = TR.metrics(O, df.t.values, df.src_id.values, df.sink_id.values, so.src_id,
                           so.end_time, tl.edges, tl.Ks)
    _assert_close(tl.metrics[0].cpu().numpy(), exp, rows, "manager")
    assert np.array_equal(tl.posts[0].cpu().numpy(),
                          TR.posts(df.t.values, df.src_id.values, so.src_id, tl.edges, df.event_id.values))

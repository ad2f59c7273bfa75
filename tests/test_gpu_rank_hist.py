"""rq_log_rank_hist / BatchResult.rank_hist / batch.run_rank_hist on the GPU against the
host checker tests/rank_hist_ref.py: ``replay`` restates the kernel's sums in the
contract's order, so the GPU must give its bits; ``bin_table`` (exactly rounded sums over
a rank table; tests/test_rank_hist_cpu.py pins it to the reference's own tables) bounds
both.

Tolerance against bin_table, rq_log_timeline and the integral of nvalid (derived, not
measured): a cell is a sum of at most n non-negative terms of at most 4 roundings each,
so whatever the summation order |got - exp| <= (n + 8) * 2**-52 * exp with n =
counts[i][3], the replica's pivot rows (K more roundings for a sum of K cells); a value
whose expectation is 0 must be exactly 0.0; integer outputs must be equal."""
import math

import numpy as np
import pytest

from tests import rank_hist_ref as RH
from tests.loghelp import (ctx as _ctx, graph as _graph, pack as _pack, raw_rank_hist as _raw,
                           same_bits as _same_bits)

pytestmark = pytest.mark.gpu
NRS = (1, 63, 64, 65, 127, 128, 255)   # 64, 65, 128, 129 and 256 cells: 1, 2 and 4 per lane


def _dummy(ids):
    return [("Poisson2", {"src_id": int(s), "seed": 1, "rate": 1.0}) for s in ids]


def _csr(g):
    return RH.csr_of(g.stream_src_ids, g.sink_ids, g._edges)


def _assert_close(got, exp, rows, what):
    print(what, "max |got - exp| / (ulp exp) = %.3g over %d rows" % (
        float(np.max(np.abs(got - exp) / np.maximum(RH.ULP * np.abs(exp), 1e-300))) if got.size else 0.0, rows))
    assert got.shape == exp.shape, what
    assert not np.isnan(got).any(), what
    assert (got[exp == 0.0] == 0.0).all(), what
    bad = np.abs(got - exp) > RH.tol(rows, exp)
    assert not bad.any(), (what, np.argwhere(bad)[:4], got[bad][:4], exp[bad][:4])


def _check_packed(torch, L, g, packed, edge_sets, nrs, end, what):
    """Every replica of packed logs, bit for bit against replay; returns the walks."""
    ev_t, ev_src, counts = packed
    ptr, col = _csr(g)
    walks = []
    for i in range(ev_t.shape[0]):
        n = min(max(int(counts[i, 2]), 0), ev_t.shape[1])
        walks.append(RH.walk(ev_t[i, :n], ev_src[i, :n], ptr, col, g.ctrl_idx))
    for edges in edge_sets:
        for nr in nrs:
            hist, seen, mx, sta = _raw(torch, L, g, ev_t, ev_src, counts, edges, nr)
            for i, (row_t, cnt, S, top, status) in enumerate(walks):
                assert (seen[i], mx[i], sta[i]) == (S, top, status), (what, i, nr)
                exp = RH.integrate(row_t, cnt, S, status, end, edges, nr)
                assert _same_bits(hist[i], exp), (what, i, nr, len(edges))
    return walks


# ------------------------------------------------------------- 1. fixture logs, raw ABI
def test_fixture_logs_through_the_raw_abi(golden):
    torch, O, L, engine, graphs = _ctx()
    f = golden("rank_hist.npz")
    for name in (str(n) for n in f["names"]):
        src_id, end = int(f[name + "_world"][0]), float(f[name + "_world"][1])
        so = dict(src_id=src_id, end_time=end, sink_ids=[int(x) for x in f[name + "_sinks"]],
                  edge_list=[tuple(int(v) for v in e) for e in f[name + "_edges"]],
                  other_sources=_dummy(f[name + "_srcs"]))
        g = _graph(engine, so)
        t, s = f[name + "_t"], f[name + "_src"]
        ev_t, ev_src, counts = _pack([(t, s)], t.size + 77, g)
        rows, S, top = (int(v) for v in f[name + "_rows"])
        ptr, col = _csr(g)
        row_t, cnt, S2, top2, status = RH.walk(t, ev_src[0, :t.size], ptr, col, g.ctrl_idx)
        assert (len(row_t), S2, top2, status) == (rows, S, top, 0)
        for k in (0, 1):
            edges = f["%s_bins%d" % (name, k)]
            for nr in (int(v) for v in f["ranks"]):
                hist, seen, mx, sta = _raw(torch, L, g, ev_t, ev_src, counts, edges, nr)
                assert (seen[0], mx[0], sta[0]) == (S, top, 0), name
                _assert_close(hist[0], f["%s_hist%d_%d" % (name, k, nr)], rows, "%s/%d/%d" % (name, k, nr))
                assert _same_bits(hist[0], RH.integrate(row_t, cnt, S, 0, end, edges, nr)), (name, k, nr)


# ------------------------------------------------- 2. README graph, every controller
def _readme_edge_sets(so, t0):
    T = so["end_time"]
    mid = float(t0[len(t0) // 2])
    return {"default": None,
            "one": [0.0, T],
            "uneven7": [1.5, 2.0, 9.75, 10.0, 33.0, 60.5, 61.0, 97.5],
            "on_event": [0.0, mid, T],
            "eq65": [T * k / 65 for k in range(65)] + [T],
            "eq1000": [T * k / 1000 for k in range(1000)] + [T]}


@pytest.mark.parametrize("ctrl", ["opt", "poisson", "pwconst", "times"])
def test_readme_graph_every_edge_set_and_cell_count(ctrl):
    torch, O, L, engine, graphs = _ctx()
    so = graphs.readme()
    Ks = (1, 2, 33)
    R = 4
    T = so["end_time"]
    kw = dict(n_rep=R, ctrl_seed=500, world_seed=900, randomize=True, Ks=Ks, event_log=True)
    gkw = {}
    if ctrl == "opt":
        kw.update(q=so["q"], s=so["s"])
    if ctrl == "poisson":
        kw.update(ctrl_rate=torch.linspace(0.5, 6.0, R, dtype=torch.float64))
    if ctrl == "pwconst":
        gkw.update(ctrl_a=[0.0, 20.0, 50.0, 80.0], ctrl_b=[3.0, 0.25, 6.0, 1.0])
    if ctrl == "times":
        gkw["ctrl_a"] = np.sort(np.random.RandomState(3).uniform(0.0, T, 120))
    g = _graph(engine, so, **gkw)
    res = g.run(ctrl, **kw)
    counts = res.counts.cpu().numpy()
    assert (res.status.cpu().numpy() == 0).all() and (counts[:, 0] > 3).all()
    ev_t, ev_src = res.ev_t.cpu().numpy(), res.ev_src.cpu().numpy()
    ptr, col = _csr(g)
    walks = [RH.walk(ev_t[i, :counts[i, 2]], ev_src[i, :counts[i, 2]], ptr, col, g.ctrl_idx) for i in range(R)]
    for i, w in enumerate(walks):
        assert len(w[0]) == counts[i, 3] and w[4] == 0
    t0, _ = res.events(0)
    sets = _readme_edge_sets(so, t0)
    assert sets["on_event"][1] in t0
    for name, edges in sets.items():
        e = [g.start_time, T] if edges is None else edges
        tl = res.timeline(edges=e, Ks=Ks).metrics.cpu().numpy()
        nvi = [RH.nvalid_int(w[0], w[1], T, e) for w in walks]
        for nr in NRS:
            rh = res.rank_hist(ranks=nr, edges=edges)
            assert np.array_equal(rh.edges, np.asarray(e)) and rh.ranks == nr
            hist = rh.hist.cpu().numpy()
            assert hist.shape == (R, len(e) - 1, nr + 1) and (rh.status.cpu().numpy() == 0).all()
            seen, mx = rh.n_seen.cpu().numpy(), rh.max_rank.cpu().numpy()
            for i, (row_t, cnt, S, top, status) in enumerate(walks):
                assert (seen[i], mx[i]) == (S, top), (name, nr, i)
                assert _same_bits(hist[i], RH.integrate(row_t, cnt, S, 0, T, e, nr)), (ctrl, name, nr, i)
                rows = int(counts[i, 3])
                for q, K in enumerate(Ks):
                    if K <= nr:
                        got = hist[i, :, :K].sum(-1)
                        lim = (rows + K + 8) * RH.ULP * np.abs(tl[i, :, q])
                        assert (np.abs(got - tl[i, :, q]) <= lim).all(), (ctrl, name, nr, i, K)
                        assert (np.abs(rh.top_k(K)[i].cpu().numpy() - got) <= K * RH.ULP * got).all()
                tot = np.asarray([math.fsum(row.tolist()) for row in hist[i]]) * float(S)
                _assert_close(tot, nvi[i], rows, "%s %s nr=%d replica %d: int nvalid" % (ctrl, name, nr, i))
    # the accessors on device tensors
    rh = res.rank_hist(ranks=64, bins=5)
    assert rh.hist.is_cuda and rh.cdf().shape == (R, 5, 65) and rh.quantile(0.5).shape == (R, 5)
    assert torch.equal(rh.tail, rh.hist[:, :, 64]) and (rh.quantile(1.0) <= 64).all()
    assert np.array_equal(rh.edges, np.asarray([0.0, 20.0, 40.0, 60.0, 80.0, 100.0]))


# ------------------------------------------------ 3. fan-outs and both update extremes
def _fan_world(N):
    """N sinks; source 2 posts to all of them, the controlled source 1 to all but the
    first (to the one sink of N = 1), source 10 + m (1 <= m < min(N, 130)) to the sinks
    m, m + 1, ...: one post of each in turn leaves sink x at rank min(x, M - 1)."""
    sinks = [100 + x for x in range(N)]
    M = min(N, 130)
    edges = [(2, s) for s in sinks] + [(1, s) for s in (sinks[1:] if N > 1 else sinks)]
    for m in range(1, M):
        edges += [(10 + m, s) for s in sinks[m:]]
    return dict(src_id=1, end_time=64.0, sink_ids=sinks, edge_list=edges,
                other_sources=_dummy([2] + [10 + m for m in range(1, M)])), M


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
def test_fan_outs_one_cell_and_many_cells(N):
    torch, O, L, engine, graphs = _ctx()
    so, M = _fan_world(N)
    g = _graph(engine, so)
    # every touched sink at one rank: the 64 lanes of a round update one cell
    s_same = [2, 2, 1, 2, 2, 2, 1, 2, 2, 2, 2, 1, 2]
    same = (0.5 + 1.75 * np.arange(len(s_same)), s_same)
    # staggered first rows: a 64-sink round of source 2 then holds 64 distinct ranks, the
    # rounds of one row more than 64 (N >= 130: ranks 1 .. 129)
    s_stag = [10 + m for m in range(1, M)] + [2, 2, 1, 2] + [10 + m for m in range(1, M, 7)] + [2, 1, 2, 2]
    stag = (0.25 + 0.125 * np.arange(len(s_stag)), s_stag)
    packed = _pack([same, stag, same], max(len(s_same), len(s_stag)) + 3, g)
    edge_sets = ([0.0, 64.0], [1.0, 2.25, 6.0, 17.5, 18.0, 40.0])
    walks = _check_packed(torch, L, g, packed, edge_sets, (1, 3, 64, 100, 255), so["end_time"], "fan %d" % N)
    assert [w[2] for w in walks] == [N, N, N] and walks[0][3] == (10 if N > 1 else 4)
    if N >= 130:
        assert walks[1][3] >= 130 and (walks[1][1] > 0).sum(1).max() > 64   # > 64 distinct ranks in one row
    if N <= 65:   # an independent route: the oracle's rank table, exactly rounded sums
        for i, log in enumerate((same, stag)):
            t, s, x, _eid = RH.frame_of(log[0], log[1], so["edge_list"])
            tab, idx, _ = O.rank_table(t, s, x, 1, True)
            for nr in (3, 64):
                hist, _, _, _ = _raw(torch, L, g, *packed, edge_sets[1], nr)
                _assert_close(hist[i], RH.bin_table(tab, idx, so["end_time"], edge_sets[1], nr), tab.shape[0],
                              "fan %d log %d nr %d" % (N, i, nr))


# ----------------------------------------------- 4. into, within and out of the tail
def test_wall_source_beyond_255_posts_between_own_posts():
    torch, O, L, engine, graphs = _ctx()
    so = dict(src_id=1, end_time=700.0, sink_ids=[7, 8], edge_list=[(1, 7), (1, 8), (2, 7), (2, 8), (3, 8)],
              other_sources=_dummy([2, 3]))
    g = _graph(engine, so)
    s = [1] + [2] * 300 + [1] + [2] * 260 + [3] + [2] * 3
    t = 1.0 + 1.125 * np.arange(len(s))
    packed = _pack([(t, s)], len(s) + 5, g)
    edge_sets = ([0.0, 700.0], [0.0, 3.0, 250.0, 289.0, 290.0, 340.0, 650.0, 699.0])
    walks = _check_packed(torch, L, g, packed, edge_sets, (3, 255), so["end_time"], "tail")
    assert walks[0][3] == 300 and walks[0][2] == 2
    fr = RH.frame_of(t, s, so["edge_list"])
    tab, idx, _ = O.rank_table(fr[0], fr[1], fr[2], 1, True)
    for nr in (3, 255):
        hist, seen, mx, sta = _raw(torch, L, g, *packed, edge_sets[1], nr)
        assert (seen[0], mx[0], sta[0]) == (2, 300, 0) and mx[0] > nr
        assert hist[0, :, nr].sum() > 0 and hist[0, :, 0].sum() > 0
        _assert_close(hist[0], RH.bin_table(tab, idx, so["end_time"], edge_sets[1], nr), tab.shape[0], "tail nr %d" % nr)


# ---------------------------------------------------------------- 5. hand-made ties
TIE_WORLD = dict(src_id=1, end_time=20.0, sink_ids=[10, 11, 12, 13],
                 edge_list=[(1, 10), (1, 12), (2, 10), (2, 11), (3, 12), (4, 13), (4, 11)],
                 other_sources=_dummy([2, 3, 4, 5]))


def test_hand_made_ties_and_empty():
    torch, O, L, engine, graphs = _ctx()
    so = TIE_WORLD
    g = _graph(engine, so)
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
    packed = _pack(logs, 16, g)
    walks = _check_packed(torch, L, g, packed, [edges], (1, 2, 64), so["end_time"], "ties")
    hist, seen, mx, sta = _raw(torch, L, g, *packed, edges, 2)
    assert list(sta) == [0, L.ST_TIE, 0, L.ST_EMPTY, 0, L.ST_EMPTY]
    for i in range(6):
        assert np.isnan(hist[i]).all() if i in (1, 3, 5) else not np.isnan(hist[i]).any(), i
    assert list(seen) == [4, 4, 4, 0, 4, 0] and list(mx) == [w[3] for w in walks] and mx[1] >= 1
    assert mx[3] == mx[5] == -1
    for i in (0, 2, 4):
        t, s, x, _eid = RH.frame_of(logs[i][0], logs[i][1], so["edge_list"])
        tab, idx, _ = O.rank_table(t, s, x, 1, True)
        _assert_close(hist[i], RH.bin_table(tab, idx, so["end_time"], edges, 2), tab.shape[0], "hand-made %d" % i)
    # the neighbours of the flagged replicas: the bits they have without them
    logs2 = [plain, other, disjoint, other, other, plain]
    hist2, seen2, mx2, sta2 = _raw(torch, L, g, *_pack(logs2, 16, g), edges, 2)
    assert (sta2 == 0).all()
    for i in (0, 2, 4):
        assert _same_bits(hist[i], hist2[i]) and seen[i] == seen2[i] and mx[i] == mx2[i]


# ------------------------------------------------------------------ 6. determinism
def test_same_bits_twice_and_alone():
    torch, O, L, engine, graphs = _ctx()
    so = graphs.readme()
    g = _graph(engine, so)
    R = 4
    kw = dict(q=so["q"], s=so["s"], n_rep=R, ctrl_seed=21, world_seed=33, randomize=True, Ks=(1, 2),
              event_log=True)
    res = g.run("opt", **kw)
    for nr in (64, 255):
        a = res.rank_hist(ranks=nr, bins=24)
        b = res.rank_hist(ranks=nr, bins=24)
        assert (a.status == 0).all()
        for x, y in ((a.hist, b.hist), (a.n_seen, b.n_seen), (a.max_rank, b.max_rank), (a.status, b.status)):
            assert torch.equal(x, y)
        for i in range(R):
            c = g.run("opt", rep_idx=[i], **kw).rank_hist(ranks=nr, bins=24)
            assert _same_bits(c.hist[0].cpu().numpy(), a.hist[i].cpu().numpy()), (nr, i)
            assert c.n_seen[0] == a.n_seen[i] and c.max_rank[0] == a.max_rank[i] and c.status[0] == 0


# ------------------------------------------------------------------- 7. validation
def test_validation_on_the_device():
    torch, O, L, engine, graphs = _ctx()
    g = _graph(engine, TIE_WORLD)
    lib = L.lib()
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()

    def call(h=g._h, n_rep=2, cap=4, nb=3, nr=2):
        return lib.rq_log_rank_hist(h, p, p, p, n_rep, cap, p, nb, nr, p, p, p, p, None)
    for kw in (dict(nb=0), dict(nr=0), dict(nr=256), dict(n_rep=-1), dict(cap=-1), dict(h=None)):
        assert call(**kw) == L.RQ_EINVAL, kw
    dup = dict(TIE_WORLD, edge_list=TIE_WORLD["edge_list"] + [(2, 10)])
    assert call(h=_graph(engine, dup)._h) == L.RQ_EUNSUPPORTED
    assert call(n_rep=0) == L.RQ_OK            # nothing to play: nothing is enqueued
    torch.cuda.synchronize()
    assert (buf == 0).all()                    # nothing was launched
    # a stream index outside the graph gives no row; counts beyond ev_cap play ev_cap events,
    # negative counts none
    edges = [0.0, 5.0, 20.0]
    t = np.asarray([0.5, 1.0, 2.0, 3.0, 7.0, 11.0, 13.5])
    s = [2, 3, 1, 4, 2, 1, 3]
    ev_t, ev_src, counts = _pack([(t, s)] * 4, 8, g)
    ev_src[1, [1, 4]] = [g.n_streams, -3]
    ev_src[1, 5] = 10 ** 6
    counts[2, 2] = 10 ** 12
    counts[3, 2] = -1
    ev_t[2, 7], ev_src[2, 7] = 19.0, ev_src[0, 0]
    ptr, col = _csr(g)
    hist, seen, mx, sta = _raw(torch, L, g, ev_t, ev_src, counts, edges, 4)
    keep = np.asarray([0, 2, 3, 6])
    exp = [RH.replay(t, ev_src[0, :7], ptr, col, g.ctrl_idx, 20.0, edges, 4),
           RH.replay(t[keep], ev_src[0, keep], ptr, col, g.ctrl_idx, 20.0, edges, 4),
           RH.replay(ev_t[2], ev_src[2], ptr, col, g.ctrl_idx, 20.0, edges, 4)]
    for i, (h, S, top, status) in enumerate(exp):
        assert _same_bits(hist[i], h) and (seen[i], mx[i], sta[i]) == (S, top, status), i
    assert not _same_bits(hist[0], hist[1]) and not _same_bits(hist[0], hist[2])
    assert sta[3] == L.ST_EMPTY and np.isnan(hist[3]).all() and (seen[3], mx[3]) == (0, -1)
    # the Python surface
    res = g.run("wall", n_rep=2, Ks=(1,), event_log=True)
    for e in ([0.0, 5.0, 5.0, 20.0], [0.0, 7.0, 3.0], [0.0, float("nan"), 20.0], [0.0, float("inf")], [1.0]):
        with pytest.raises(ValueError):
            res.rank_hist(edges=e)
    for kw in (dict(bins=0), dict(ranks=0), dict(ranks=256), dict(bins=2, edges=[0.0, 1.0])):
        with pytest.raises(ValueError):
            res.rank_hist(**kw)
    with pytest.raises(ValueError):
        g.run("wall", n_rep=2, Ks=(1,)).rank_hist()   # no event log
    assert res.rank_hist().hist.shape == (2, 1, 65)


def test_sink_limit():
    """RQ_TIMELINE_MAX_SINKS sinks run with 256 cells (97 KiB of LDS); one more is refused."""
    torch, O, L, engine, graphs = _ctx()
    N = L.TIMELINE_MAX_SINKS
    sinks = list(range(1, N + 2))

    def world(n):
        return dict(src_id=1, end_time=10.0, sink_ids=sinks[:n],
                    edge_list=[(2, s) for s in sinks[:n]] + [(1, s) for s in sinks[:n:3]] + [(3, sinks[n - 1])],
                    other_sources=_dummy([2, 3]))
    so = world(N)
    g = _graph(engine, so)
    logs = [([0.5, 1.0, 2.5, 4.0, 4.0 + 2.0 ** -30, 7.0, 9.0], [3, 1, 2, 2, 1, 2, 3]), ([3.0, 6.0], [2, 1])]
    edges = [0.0, 1.0, 4.0, 8.0, 10.0]
    walks = _check_packed(torch, L, g, _pack(logs, 9, g), [edges], (255, 2), so["end_time"], "limit")
    assert walks[0][2] == N and walks[1][2] == N
    g2 = _graph(engine, world(N + 1))
    _raw(torch, L, g2, *_pack(logs, 9, g2), edges, 255, expect=L.RQ_EUNSUPPORTED)


# ------------------------------------------------------------ 8. batch.run_rank_hist
def test_run_rank_hist_matches_one_batch_and_any_chunking():
    torch, O, L, engine, graphs = _ctx()
    import pandas as pd
    from redqueen_amd import batch
    from redqueen_amd.opt_model import SimOpts
    so = SimOpts(**graphs.readme())
    seeds = np.arange(300, 306)
    R = len(seeds)
    g = batch.compiled_graph(so)
    st = torch.as_tensor(seeds)
    res = g.run("opt", q=float(so.q), s=so.s, n_rep=R, ctrl_seed=st, world_seed=st, randomize=True,
                Ks=(1,), event_log=True)
    rh = res.rank_hist(ranks=16, bins=10)
    assert (rh.status == 0).all()
    exp = batch.rank_hist_frame(rh.edges, rh.ranks, rh.hist.cpu().numpy(), rh.status.cpu().numpy())
    assert len(exp) == 10 * 17 and (exp.n == R).all() and (exp.n_flagged == 0).all()
    for chunk in (1, 3, R, None):
        f = batch.run_rank_hist(so, seeds, ranks=16, bins=10, chunk_replicas=chunk)
        pd.testing.assert_frame_equal(f, exp, check_exact=True)
    v = rh.hist.cpu().numpy().reshape(R, -1)
    assert np.allclose(exp.share.values, v.mean(0), rtol=R * RH.ULP, atol=0.0)
    assert np.allclose(exp.share_se.values, v.std(0, ddof=1) / np.sqrt(float(R)), rtol=1e-12, atol=1e-300)
    # the shares of a bin sum to its length: all three sinks are seen almost at once
    tot = exp.groupby("t_lo").share.sum().values
    assert np.all(tot[1:] > 9.99) and np.all(tot <= 10.0 * (1 + 1e-12))
    one = batch.run_rank_hist(so, seeds[:2], ranks=3, ctrl="poisson", ctrl_rate=[1.0, 2.0])
    assert len(one) == 4 and list(one["tail"]) == [False, False, False, True] and (one.t_hi == so.end_time).all()


def test_manager_result_rank_hist():
    """Manager.run_dynamic keeps its BatchResult: the one run's histogram needs no further code."""
    torch, O, L, engine, graphs = _ctx()
    from redqueen_amd.opt_model import SimOpts
    so = SimOpts(**graphs.readme())
    m = so.create_manager_with_opt(seed=101)
    m.run_dynamic()
    rh = m.result.rank_hist(ranks=5, bins=5)
    assert rh.hist.shape == (1, 5, 6) and int(rh.status[0]) == 0
    df = m.state.get_dataframe()
    tab, idx, _ = O.rank_table(df.t.values, df.src_id.values, df.sink_id.values, so.src_id, True)
    assert int(rh.n_seen[0]) == tab.shape[1] and int(rh.max_rank[0]) == int(np.nanmax(tab))
    _assert_close(rh.hist[0].cpu().numpy(), RH.bin_table(tab, idx, so.end_time, rh.edges, 5), tab.shape[0],
                  "manager")

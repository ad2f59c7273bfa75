"""rq_log_metrics_of / BatchResult.source_metrics / player_metrics / batch.run_sources on
the GPU, bit for bit against the host checker (tests/log_metrics_ref.play handed the tracked
source and, in scope "own", the filtered edge list: tests/log_sources_ref.py), against the
reference's own values for every source (tests/golden/log_sources.npz), against
rq_log_metrics for the controlled source and against the dataframe route (rq_log_expand +
rq_metrics_replay_batch with src_id = c, on all rows and on the rows of c's followers).
Every output buffer of a raw call, the workspace included, carries a sentinel guard."""
import ctypes as C

import numpy as np
import pytest

from tests import log_metrics_ref as LR
from tests import log_sources_ref as SR
from tests import loghelp as LH
from tests.loghelp import D_SENT, GUARD, I_SENT, ctx as _ctx, graph as _graph, pack as _pack

pytestmark = pytest.mark.gpu


def scope_code(L, scope):
    return {"df": L.LOG_OF_DF, "own": L.LOG_OF_OWN}.get(scope, scope)


def raw(torch, L, g, src_ids, scope, ev_t, ev_src, counts, Ks, expect=0, ws_expect=None):
    """rq_log_metrics_of on host arrays; outputs come back as numpy, their guard tails (and
    the workspace's) checked.  Returns (metrics [R, P, nK + 2], counts [R, P, 4], status
    [R, P]).  ``expect``: the entry's status; ``ws_expect``: the workspace query's (default:
    ``expect`` where the query sees the fault, i.e. for RQ_EUNSUPPORTED)."""
    R, cap = ev_t.shape
    nK, P = len(Ks), len(src_ids)
    dt, ds, dc = LH._dev(torch, ev_t, ev_src, counts)
    n_m, n_c, n_s = R * P * (nK + 2), R * P * 4, R * P
    met = torch.full((n_m + GUARD,), D_SENT, dtype=torch.float64, device="cuda")
    cnt = torch.full((n_c + GUARD,), I_SENT, dtype=torch.int64, device="cuda")
    sta = torch.full((n_s + GUARD,), I_SENT, dtype=torch.int32, device="cuda")
    lib = L.lib()
    nb = C.c_size_t(0)
    if ws_expect is None:
        ws_expect = expect if expect in (0, L.RQ_EUNSUPPORTED) else 0
    rc = lib.rq_log_metrics_of_workspace(g._h, min(P, L.LOG_OF_MAX_SRC) if expect else P, R, cap, nK, C.byref(nb))
    assert rc == ws_expect, rc
    n_w = nb.value if rc == 0 else 4096
    ws = torch.full((n_w + 8 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    ks = np.asarray(Ks, dtype=np.int32)
    ids = np.asarray(src_ids, dtype=np.int64)
    rc = lib.rq_log_metrics_of(g._h, ids.ctypes.data_as(L._pi64), P, scope_code(L, scope), dt.data_ptr(),
                               ds.data_ptr(), dc.data_ptr(), R, cap, ks.ctypes.data_as(L._pi32), nK,
                               met.data_ptr(), cnt.data_ptr(), sta.data_ptr(), ws.data_ptr(), n_w,
                               torch.cuda.current_stream().cuda_stream)
    assert rc == expect, rc
    torch.cuda.synchronize()
    met, cnt, sta, w = met.cpu().numpy(), cnt.cpu().numpy(), sta.cpu().numpy(), ws.cpu().numpy()
    assert (met[n_m:] == D_SENT).all() and (cnt[n_c:] == I_SENT).all() and (sta[n_s:] == I_SENT).all()
    assert (w[n_w:] == 0x5A).all()
    if expect != 0:   # a refused call launches nothing
        assert (met == D_SENT).all() and (cnt == I_SENT).all() and (sta == I_SENT).all() and (w == 0x5A).all()
    return met[:n_m].reshape(R, P, nK + 2), cnt[:n_c].reshape(R, P, 4), sta[:n_s].reshape(R, P)


def assert_cell(out, i, k, ref, what):
    met, cnt, sta = out
    assert sta[i, k] == ref["status"], (what, sta[i, k], ref["status"])
    assert np.array_equal(cnt[i, k], ref["counts"]), (what, cnt[i, k], ref["counts"])
    assert LR.same_bits(met[i, k], ref["metrics"]), (what, met[i, k], ref["metrics"])


def check(torch, L, engine, so, logs, src_ids, scope, Ks, cap=None, what="", g=None):
    """The logs as one batch through the raw entry, every (replica, source) against the
    checker.  Returns (refs[i][k], out)."""
    g = g or _graph(engine, so)
    cap = cap or max(len(t) for t, _s in logs) + 7
    out = raw(torch, L, g, src_ids, scope, *_pack(logs, cap, g), Ks)
    refs = [[SR.play(t, s, so["edge_list"], c, so["end_time"], Ks, scope) for c in src_ids] for t, s in logs]
    for i, row in enumerate(refs):
        for k, ref in enumerate(row):
            assert_cell(out, i, k, ref, "%s/%s/replica %d/source %d" % (what, scope, i, src_ids[k]))
    return refs, out


def same_outputs(a, b):
    return LR.same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ------------------------------------------------------------- 1. the reference's values
@pytest.mark.parametrize("scope", SR.SCOPES)
@pytest.mark.parametrize("name", SR.WORLDS)
def test_fixture_worlds(golden, name, scope):
    torch, _O, L, engine, _g = _ctx()
    f, fs = golden("log_metrics.npz"), golden("log_sources.npz")
    Ks = [int(k) for k in fs["Ks"]]
    w = SR.world(f, name)
    so = dict(src_id=w["src_id"], end_time=w["end_time"], sink_ids=w["sinks"], edge_list=w["edges"],
              other_sources=[("Poisson2", {"src_id": s, "seed": 1, "rate": 1.0})
                             for s in sorted({e[0] for e in w["edges"]} - {w["src_id"]})])
    srcs = [int(s) for s in fs[name + "_srcs"]]
    refs, out = check(torch, L, engine, so, [(w["t"], w["src"])], srcs, scope, Ks, cap=w["t"].size + 77, what=name)
    met, posts, empty = (fs[SR.key(name, scope, k)] for k in ("metrics", "posts", "empty"))
    for k, c in enumerate(srcs):
        print(name, scope, c, out[0][0, k], met[k])
        assert LR.same_bits(out[0][0, k], met[k]), (c, out[0][0, k], met[k])
        if empty[k]:
            assert out[2][0, k] == L.ST_EMPTY and not out[1][0, k].any()
        else:
            assert np.array_equal(out[1][0, k, :2], posts[k]) and out[2][0, k] in (0, L.ST_TIE)


# ------------------------------------------------------------- 2. the controlled source
def test_the_controlled_source_equals_rq_log_metrics():
    torch, _O, L, engine, _g = _ctx()
    from tests.test_gpu_log_metrics import WORLD, raw as raw_lm, tie_log
    rng = np.random.RandomState(1)
    logs = [tie_log(rng, n, [1, 2, 3, 4, 5, 6], step=0.125) for n in (0, 1, 63, 64, 65, 129)]
    logs[1] = (logs[1][0], np.asarray([2]))   # the one event has edges
    g = _graph(engine, WORLD)
    Ks = (1, 2)
    packed = _pack(logs, 140, g)
    one = raw_lm(torch, L, g, *packed, Ks)
    of = raw(torch, L, g, [WORLD["src_id"]], "df", *packed, Ks)
    assert same_outputs(one, (of[0][:, 0], of[1][:, 0], of[2][:, 0]))
    assert one[2][0] == L.ST_EMPTY and one[2][1] == 0 and (one[2][2:] == L.ST_TIE).all()
    # beside other tracked sources, in any position
    more = raw(torch, L, g, [6, 2, WORLD["src_id"], 5], "df", *packed, Ks)
    assert same_outputs(one, (more[0][:, 2], more[1][:, 2], more[2][:, 2]))


# ------------------------------------------------------------- 3. the number of tracked sources
def wide_world(n_src=66):
    """66 sources (1 controlled) on sinks 1..6, 1 to 3 sinks each: 64 of them are tracked at
    once, and 65 distinct ones can be named."""
    rng = np.random.RandomState(12)
    edges = []
    for s in range(1, n_src + 1):
        edges += [(s, int(x)) for x in rng.choice(np.arange(1, 7), size=rng.randint(1, 4), replace=False)]
    return dict(src_id=1, end_time=30.0, sink_ids=[1, 2, 3, 4, 5, 6], edge_list=edges,
                other_sources=[("Poisson2", {"src_id": k, "seed": k, "rate": 1.0}) for k in range(2, n_src + 1)])


@pytest.mark.parametrize("scope", SR.SCOPES)
def test_n_src_edges(scope):
    torch, _O, L, engine, _g = _ctx()
    from tests.test_gpu_log_metrics import tie_log
    so = wide_world()
    g = _graph(engine, so)
    rng = np.random.RandomState(13)
    all_ids = list(range(1, 67))
    logs = [tie_log(rng, 80, all_ids), tie_log(rng, 77, all_ids[:20], p_same=0.6)]
    Ks = (1, 3)
    full = rng.permutation(all_ids)[:64].tolist()
    outs = {}
    for n in (1, 2, 63, 64):
        _refs, outs[n] = check(torch, L, engine, so, logs, full[:n], scope, Ks, cap=90, what="n_src %d" % n, g=g)
    # a source's output does not depend on what else is tracked ...
    for n in (1, 2, 63):
        assert same_outputs(tuple(x[:, :n] for x in outs[64]), outs[n])
    # ... nor on its position: permuting src_ids permutes the outputs and changes no bit
    perm = rng.permutation(64)
    shuffled = raw(torch, L, g, [full[p] for p in perm], scope, *_pack(logs, 90, g), Ks)
    assert same_outputs(tuple(x[:, perm] for x in outs[64]), shuffled)


def test_refusals_launch_nothing():
    torch, _O, L, engine, _g = _ctx()
    so = wide_world()
    g = _graph(engine, so)
    packed = _pack([([1.0, 1.0, 2.0], [2, 6, 1])], 8, g)
    Ks = (1,)
    E = L.RQ_EINVAL
    raw(torch, L, g, list(range(1, 66)), "df", *packed, Ks, expect=E)     # 65 distinct streams
    raw(torch, L, g, [2, 3, 2], "own", *packed, Ks, expect=E)              # named twice
    raw(torch, L, g, [2, 67], "df", *packed, Ks, expect=E)                 # no stream of the graph
    raw(torch, L, g, [2, 3], 2, *packed, Ks, expect=E)                     # a scope other than the two
    raw(torch, L, g, [2, 3], -1, *packed, Ks, expect=E)
    raw(torch, L, g, [2, 3], "df", *packed, (0,), expect=E, ws_expect=0)   # rq_log_metrics' own: a K < 1
    nb = C.c_size_t()
    lib = L.lib()
    for n_src in (0, -1, 65):
        assert lib.rq_log_metrics_of_workspace(g._h, n_src, 4, 8, 1, C.byref(nb)) == E
    assert lib.rq_log_metrics_of_workspace(g._h, 2, 0, 8, 1, C.byref(nb)) == E
    assert lib.rq_log_metrics_of_workspace(g._h, 2, 4, 8, 1, None) == E
    assert lib.rq_log_metrics_of_workspace(g._h, 2, 4, (1 << 20) + 1, 1, C.byref(nb)) == L.RQ_EUNSUPPORTED
    raw(torch, L, g, [2, 3], "own", *packed, Ks)                           # and the good call goes through


# ------------------------------------------------------------- 4. run boundaries
@pytest.mark.parametrize("scope", SR.SCOPES)
def test_run_boundaries(monkeypatch, scope):
    """n_rep * n_src just below, at and above the slot count, shrunk to 12 for the test:
    above it a block plays a run of (replica, source) items one after the other in its
    slot and, in scope DF, keeps a replica's columns across the sources of a run."""
    torch, _O, L, engine, _g = _ctx()
    from tests.test_gpu_log_metrics import WORLD, tie_log
    monkeypatch.setenv("RQ_LM_OF_SLOTS", "12")
    g = _graph(engine, WORLD)
    rng = np.random.RandomState(14)
    lib = L.lib()
    nb, one = C.c_size_t(), C.c_size_t()
    Ks = (1, 2)
    assert lib.rq_log_metrics_of_workspace(g._h, 1, 1, 12, len(Ks), C.byref(one)) == 0
    for n_rep, srcs in ((3, [3, 1, 6]), (4, [3, 1, 6]), (5, [3, 1, 6]), (9, [3, 1, 6]), (7, [2, 5, 4, 6, 1]),
                        (13, [4]), (40, [6, 2])):
        logs = [tie_log(rng, int(rng.randint(0, 9)), [1, 2, 3, 4, 5, 6], p_same=0.5) for _k in range(n_rep)]
        assert lib.rq_log_metrics_of_workspace(g._h, len(srcs), n_rep, 12, len(Ks), C.byref(nb)) == 0
        assert nb.value == min(12, n_rep * len(srcs)) * one.value
        check(torch, L, engine, WORLD, logs, srcs, scope, Ks, cap=12, what="%d x %d" % (n_rep, len(srcs)), g=g)


def test_tapered_shares(monkeypatch):
    """More blocks than the device holds at once (4096 blocks of ~24 KiB LDS: six to a CU)
    over at least four items a block: the launch deals falling shares of the items.  The
    same bits as with 1024 blocks, which are all resident and get equal shares, and as the
    checker's on a sample of the replicas."""
    torch, _O, L, engine, _g = _ctx()
    from tests.test_gpu_log_metrics import tie_log
    rng = np.random.RandomState(17)
    sinks = list(range(1, 1201))
    srcs = list(range(1, 65))
    edges = [(s, int(x)) for s in srcs for x in rng.choice(sinks, size=3, replace=False)]
    so = dict(src_id=1, end_time=9.0, sink_ids=sinks, edge_list=edges,
              other_sources=[("Poisson2", {"src_id": k, "seed": k, "rate": 1.0}) for k in srcs[1:]])
    g = _graph(engine, so)
    R, Ks, cap = 260, (1, 2), 8
    assert R * len(srcs) >= 4 * 4096
    logs = [tie_log(rng, int(rng.randint(0, 7)), srcs[:12], p_same=0.5) for _k in range(R)]
    packed = _pack(logs, cap, g)
    for scope in SR.SCOPES:
        out = raw(torch, L, g, srcs, scope, *packed, Ks)
        monkeypatch.setenv("RQ_LM_OF_SLOTS", "1024")
        assert same_outputs(out, raw(torch, L, g, srcs, scope, *packed, Ks))
        monkeypatch.delenv("RQ_LM_OF_SLOTS")
        for i in list(range(0, R, 13)) + [R - 1]:
            for k in range(0, 64, 5):
                ref = SR.play(logs[i][0], logs[i][1], edges, srcs[k], so["end_time"], Ks, scope)
                assert_cell(out, i, k, ref, "taper/%s/%d/%d" % (scope, i, srcs[k]))


# ------------------------------------------------------------- 5. the follower masks of scope OWN
def mask_world():
    """130 sinks 1000..1129 (sink 1000 + b is bit b of the column bits).  Source 2 follows
    bits 0, 31, 32, 33, 63, 64 and 129; 3 has 70 followers (its rows take two rounds); 4
    follows bit 100 alone, which nobody else reaches, and never posts; 5 has no edge; 6 reaches
    129 sinks (three rounds); 7 reaches bits 90 and 91 only -- none of 2's followers -- and 8
    bits 31 and 90; the controlled source 1 follows bits 0..5."""
    sink = lambda b: 1000 + b  # noqa: E731
    edges = [(2, sink(b)) for b in (0, 31, 32, 33, 63, 64, 129)]
    edges += [(3, sink(b)) for b in range(10, 80)]
    edges += [(4, sink(100))]
    edges += [(6, sink(b)) for b in range(130) if b != 100]
    edges += [(7, sink(90)), (7, sink(91)), (8, sink(31)), (8, sink(90))]
    edges += [(1, sink(b)) for b in range(6)]
    edges = [edges[i] for i in np.random.RandomState(15).permutation(len(edges))]
    return dict(src_id=1, end_time=25.0, sink_ids=[sink(b) for b in range(130)], edge_list=edges,
                other_sources=[("Poisson2", {"src_id": k, "seed": k, "rate": 1.0}) for k in range(2, 9)])


def test_own_scope_masks():
    torch, _O, L, engine, _g = _ctx()
    from tests.test_gpu_log_metrics import tie_log
    so = mask_world()
    g = _graph(engine, so)
    Ks = (1, 2, 5)
    # by hand: 7 misses 2's followers.  Alone in a t-group (t = 2) it makes no row; first (t = 3)
    # or last (t = 5) in a group whose other event, 8's, hits bit 31, it neither opens a row
    # of its own nor is counted; between two posts of 2 at one time (t = 7) it changes nothing
    hand = ([1.0, 2.0, 3.0, 3.0, 4.0, 5.0, 5.0, 6.0, 7.0, 7.0, 7.0, 9.0],
            [2, 7, 7, 8, 3, 8, 7, 6, 2, 7, 2, 7])
    rng = np.random.RandomState(16)
    posting = [1, 2, 3, 5, 6, 7, 8]   # 4 never posts
    logs = [hand, tie_log(rng, 70, posting, p_same=0.5), tie_log(rng, 64, [7, 8, 2, 5], p_same=0.7),
            ([1.0, 1.0, 2.0], [7, 5, 7])]
    srcs = [2, 3, 4, 5, 6, 7, 8, 1]
    own, out_own = check(torch, L, engine, so, logs, srcs, "own", Ks, what="masks", g=g)
    df, out_df = check(torch, L, engine, so, logs, srcs, "df", Ks, what="masks", g=g)
    k2, k3, k4, k5 = (srcs.index(c) for c in (2, 3, 4, 5))
    # the hand log for source 2: rows at t = 1, 3, 4 (3 reaches bits 31, 32, 33, 63, 64), 5, 6, 7;
    # its own 3 posts; others with a row: 8, 3, 8, 6 -- 7 never
    assert out_own[1][0, k2].tolist() == [3, 4, 6, 7] and out_own[2][0, k2] == L.ST_TIE
    assert out_df[1][0, k2].tolist() == [3, 9, 8, 129]
    # 3's 70 followers all get a row from 6
    assert out_own[1][1, k3, 3] == 70 and out_df[1][1, k3, 3] == 129
    for i in range(len(logs)):
        # 4: nobody reaches its follower -- EMPTY in its own scope, defined on the df without a post
        assert out_own[2][i, k4] == L.ST_EMPTY and np.isnan(out_own[0][i, k4]).all() and not out_own[1][i, k4].any()
        assert out_df[2][i, k4] != L.ST_EMPTY and out_df[1][i, k4, 0] == 0 and not np.isnan(out_df[0][i, k4]).any()
        # 5: no edge, no follower
        assert out_own[2][i, k5] == L.ST_EMPTY and out_df[1][i, k5, 0] == 0
    # the last log reaches bits 90 and 91 only: EMPTY in scope own for everyone but 6, 7 and 8
    assert [int(s) for s in out_own[2][3]] == [L.ST_EMPTY] * 4 + [0, 0, 0, L.ST_EMPTY]
    assert (out_df[2][3] == 0).all()


# ------------------------------------------------------------- 6. batch independence
@pytest.mark.parametrize("scope", SR.SCOPES)
def test_alone_and_in_a_batch_of_257(scope):
    torch, _O, L, engine, _g = _ctx()
    from tests.test_gpu_log_metrics import WORLD, tie_log
    rng = np.random.RandomState(8)
    logs = [tie_log(rng, int(rng.randint(0, 90)), [1, 2, 3, 4, 5, 6]) for _k in range(257)]
    g = _graph(engine, WORLD)
    Ks = (1, 2)
    cap = 96
    srcs = [6, 1, 5, 3, 2]
    batch = raw(torch, L, g, srcs, scope, *_pack(logs, cap, g), Ks)
    for i in (0, 200, 256):
        one = raw(torch, L, g, srcs, scope, *_pack([logs[i]], cap, g), Ks)
        for k, c in enumerate(srcs):
            ref = SR.play(logs[i][0], logs[i][1], WORLD["edge_list"], c, WORLD["end_time"], Ks, scope)
            assert_cell(one, 0, k, ref, "alone %d/%d" % (i, c))
            assert_cell(batch, i, k, ref, "in the batch %d/%d" % (i, c))
        assert same_outputs(one, tuple(x[i:i + 1] for x in batch))


# ------------------------------------------------------------- 7. against the dataframe replay
def replay_of(torch, res, g, c, Ks, followers=None):
    """rq_metrics_replay_batch with src_id = c on the result's dataframe rows; ``followers``:
    on the rows of these sinks only, df_off recomputed."""
    from redqueen_amd.utils import replay_columns
    ro, cols = res._log_columns(torch.cuda.current_stream())
    keep = None
    if followers is not None:
        fol = torch.as_tensor(np.asarray(followers, dtype=np.int64)).cuda()
        keep = torch.isin(cols["sink_id"], fol)
        rep = np.repeat(np.arange(len(ro) - 1), np.diff(ro))
        kept = np.bincount(rep[keep.cpu().numpy()], minlength=len(ro) - 1)
        ro = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
    sel = (lambda x: x) if keep is None else (lambda x: x[keep].contiguous())
    off = torch.from_numpy(np.ascontiguousarray(ro)).cuda()
    m, n = replay_columns(sel(cols["t"]), sel(cols["src_id"]), sel(cols["sink_id"]), sel(cols["event_id"]), off,
                          c, g.end_time, Ks)
    return m.cpu().numpy(), n.cpu().numpy()


def assert_equals_the_replay(torch, L, res, g, sm, scope, edges, what):
    """A SourceMetrics against the dataframe route, source by source (an EMPTY cell: no row
    to replay; NaN metrics and zero counts)."""
    m, c, s = sm.metrics.cpu().numpy(), sm.counts.cpu().numpy(), sm.status.cpu().numpy()
    for k, src in enumerate(sm.src_ids):
        rm, rc = replay_of(torch, res, g, src, sm.Ks, SR.followers_of(edges, src) if scope == "own" else None)
        empty = s[:, k] == L.ST_EMPTY
        assert np.array_equal(c[~empty, k], rc[~empty]), (what, scope, src)
        assert LR.same_bits(m[~empty, k], rm[~empty]), (what, scope, src)
        assert np.isnan(m[empty, k]).all() and not c[empty, k].any()


def test_ordinary_run_equals_the_replay_for_every_source():
    torch, _O, L, engine, graphs = _ctx()
    so = graphs.followers_graph(200, 10)
    g = _graph(engine, so)
    Ks = (1, 5)
    res = g.run("opt", q=so["q"], s=so["s"], n_rep=64, ctrl_seed=11, world_seed=77, randomize=True, Ks=Ks,
                event_log=True)
    for scope in SR.SCOPES:
        sm = res.source_metrics(scope=scope)   # default: every source of the graph
        assert sm.src_ids == [int(x) for x in g.stream_src_ids] and sm.Ks == [1, 5]
        assert tuple(sm.metrics.shape) == (64, len(sm.src_ids), 4)
        assert_equals_the_replay(torch, L, res, g, sm, scope, so["edge_list"], "followers_graph")
        k = sm.src_ids.index(g.src_id)
        if scope == "df":   # the controlled source follows every sink: its row is the run's own
            assert LR.same_bits(sm.metrics[:, k].cpu().numpy(), res.metrics.cpu().numpy())
            assert LR.same_bits(sm.avg_rank[:, k].cpu().numpy(), res.avg_rank.cpu().numpy())
            assert LR.same_bits(sm.top_k(5)[:, k].cpu().numpy(), res.top_k(5).cpu().numpy())
    # chunked to a small workspace budget, sources in chunks of 4: the same bits
    ids = [int(x) for x in g.stream_src_ids[[3, 0, 5, 1, 4, 2]]]
    whole = res.source_metrics(ids, scope="own", Ks=(5,))
    res.LOG_METRICS_WS_BYTES = 1 << 16
    L_max = L.LOG_OF_MAX_SRC
    try:
        L.LOG_OF_MAX_SRC = 4
        parts = res.source_metrics(ids, scope="own", Ks=(5,))
    finally:
        L.LOG_OF_MAX_SRC = L_max
    assert LR.same_bits(parts.metrics.cpu().numpy(), whole.metrics.cpu().numpy())
    assert np.array_equal(parts.counts.cpu().numpy(), whole.counts.cpu().numpy())
    assert np.array_equal(parts.status.cpu().numpy(), whole.status.cpu().numpy())
    for bad in (dict(src_ids=[1, 1]), dict(src_ids=[4999]), dict(src_ids=[]), dict(scope="all"), dict(Ks=(0,))):
        with pytest.raises(ValueError):
            res.source_metrics(**bad)
    with pytest.raises(ValueError):
        res.player_metrics()   # no players
    with pytest.raises(ValueError):
        g.run("wall", n_rep=2, Ks=(1,)).source_metrics()   # no event log


# ------------------------------------------------------------- 8. games
@pytest.mark.parametrize("n_players,max_events", [(3, None), (5, None), (5, 3)])
def test_player_metrics(n_players, max_events):
    """Every player's metrics against the masked ("own") and the unmasked ("df") replay,
    also with max_events cut inside the start-time tie."""
    torch, _O, L, engine, _g = _ctx()
    from tests.test_gpu_game import small_world
    so = small_world(n_players)
    g = _graph(engine, so)
    res = g.run("wall", n_rep=6, world_seed=31, randomize=True, Ks=(1, 2), max_events=max_events, event_log=True)
    assert res.player_ids == [20 + k for k in range(n_players)]
    for scope in SR.SCOPES:
        pm = res.player_metrics(scope)
        assert pm.src_ids == res.player_ids and pm.Ks == [1, 2]
        assert_equals_the_replay(torch, L, res, g, pm, scope, so["edge_list"], "game %d" % n_players)
        # a player's events with a row are its posts
        assert np.array_equal(pm.counts[:, :, 0].cpu().numpy(), res.player_posts.cpu().numpy())
    # the controlled source (no edge here) on the df is the result's own metrics
    ctrl = res.source_metrics([g.src_id], scope="df")
    assert LR.same_bits(ctrl.metrics[:, 0].cpu().numpy(), res.metrics.cpu().numpy())
    assert (res.source_metrics([g.src_id], scope="own").status.cpu().numpy() == L.ST_EMPTY).all()


def test_player_metrics_with_a_controlled_player():
    torch, _O, L, engine, _g = _ctx()
    from tests import game_ref as G
    so = G.w5()
    g = _graph(engine, so)
    res = g.run("opt", q=so["q"], s=so["s"], n_rep=6, ctrl_seed=5, world_seed=9, randomize=True, Ks=(1, 2),
                event_log=True)
    assert res.player_ids == [4, 5, 1]
    for scope in SR.SCOPES:
        pm = res.player_metrics(scope)
        assert_equals_the_replay(torch, L, res, g, pm, scope, so["edge_list"], "w5")
        # the controlled player follows every sink: both scopes give the result's own metrics
        assert LR.same_bits(pm.metrics[:, 2].cpu().numpy(), res.metrics.cpu().numpy())
    assert res.source_metrics().src_ids == [4, 5, 1]   # default: the players
    with pytest.raises(ValueError):
        g.run("opt", q=so["q"], s=so["s"], n_rep=2, Ks=(1,)).player_metrics()   # no event log


# ------------------------------------------------------------- 9. the ensemble frame
def test_run_sources():
    torch, _O, L, engine, graphs = _ctx()
    from redqueen_amd import batch
    from redqueen_amd.opt_model import SimOpts
    so = graphs.followers_graph(40, 8, end_time=20.0)
    ids = [5002, 1, 5000]
    frame, summ = batch.run_sources(SimOpts(**so), seeds=range(6), src_ids=ids, scope="own", Ks=(1, 2),
                                    chunk_replicas=4)
    assert list(frame.columns) == ["replica", "src_id", "top_1", "top_2", "avg_rank", "r_2", "num_events",
                                   "other_events", "status"]
    assert frame.shape == (18, 9) and list(frame.src_id[:3]) == ids and list(frame.replica[::3]) == list(range(6))
    assert list(summ.src_id) == ids and list(summ.n) == [6, 6, 6] and len(summ.columns) == 1 + 2 * 6 + 2
    # the same replicas in one chunk through the engine
    g = batch.compiled_graph(SimOpts(**so))
    sd = torch.arange(6, dtype=torch.int64)
    res = g.run("opt", q=so["q"], s=so["s"], n_rep=6, ctrl_seed=sd, world_seed=sd, randomize=True, Ks=(1, 2),
                event_log=True)
    sm = res.source_metrics(ids, scope="own")
    m = sm.metrics.cpu().numpy()
    assert LR.same_bits(frame.avg_rank.values.reshape(6, 3), m[:, :, 2])
    assert np.array_equal(frame.num_events.values.reshape(6, 3), sm.counts[:, :, 0].cpu().numpy())
    for k in range(3):
        mean, sem = batch._mean_sem(m[:, k])
        assert LR.same_bits([summ.top_1[k], summ.top_2[k], summ.avg_rank[k], summ.r_2[k]], mean)
        assert LR.same_bits(summ.avg_rank_se[k], sem[2])
    assert np.allclose(summ.avg_rank.values, m[:, :, 2].mean(axis=0), rtol=1e-12)


# ------------------------------------------------------------- 10. limits
def test_limits_are_rq_log_metrics_own():
    torch, _O, L, engine, _g = _ctx()
    from tests.test_gpu_game import small_world
    N = L.LOG_METRICS_MAX_SINKS
    sinks = list(range(1, N + 2))

    def world(n):
        return dict(src_id=1, end_time=10.0, sink_ids=sinks[:n],
                    edge_list=([(2, s) for s in sinks[:n]] + [(1, s) for s in sinks[:n:3]] +
                               [(3, s) for s in sinks[1:n:2]] + [(4, sinks[n - 1])]),
                    other_sources=[("Poisson2", {"src_id": k, "seed": 1, "rate": 1.0}) for k in (2, 3, 4)])
    Ks = (1, 2)
    logs = [([0.5, 1.0, 1.0, 1.0, 2.5, 4.0, 4.0, 7.0], [4, 2, 1, 3, 4, 3, 2, 1]),
            ([0.5, 0.5, 3.0], [3, 1, 4])]
    so = world(N)
    for scope in SR.SCOPES:
        refs, _out = check(torch, L, engine, so, logs, [3, 1, 4], scope, Ks, cap=12, what="limit")
    assert refs[0][0]["counts"][3] == len(sinks[1:N:2])   # own: 3's followers
    g2 = _graph(engine, world(N + 1))
    raw(torch, L, g2, [3, 1], "own", *_pack(logs, 12, g2), Ks, expect=L.RQ_EUNSUPPORTED)
    g3 = _graph(engine, small_world(2, dup=True))
    raw(torch, L, g3, [20, 21], "df", *_pack([([0.0, 0.0, 1.0], [20, 21, 10])], 8, g3), (1,),
        expect=L.RQ_EUNSUPPORTED)
    gw = _graph(engine, so)
    raw(torch, L, gw, [3], "df", *_pack([logs[1]], (1 << 20) + 1, gw), Ks, expect=L.RQ_EUNSUPPORTED)

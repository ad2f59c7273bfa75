"""rq_log_rows / rq_log_scan_k / rq_log_expand on hand-built event logs: replicas of
0 ... 3000 events around the 1024-event chunks of rq_log_expand_k, 1 ... 2049 replicas
around the 1024-replica blocks of rq_log_scan_k, chunks without a row, and event times
whose accumulated State.time rounds ("dirty" events) at the chunk borders.

Expected rows: the oracle's Scenario.expand on State.time's own time_deltas
(O.state_time_deltas); row_off: the cumulative out-degree.  All five columns and
row_off are compared bit for bit; tests/test_analysis_cpu.py asserts that the dirty
chains round where these tests need it."""
import numpy as np
import pytest

from tests import analysis_edges as E

pytestmark = pytest.mark.gpu
COLS = ["event_id", "time_delta", "src_id", "t", "sink_id"]
GUARD = 64
I_SENT, D_SENT = -7777, -1.2345e300
END = 100.0
# stream out-degrees 0 (src 4), 1 (src 1, the controlled one), 3 with a repeated edge
# (src 3) and 40 (src 2), in shuffled edge-list order
SINKS = list(range(500, 545))


def _sim_opts():
    edges = [(1, 507), (3, 511), (3, 502), (3, 511)] + [(2, s) for s in SINKS[3:43]]
    edges = [edges[i] for i in np.random.RandomState(12).permutation(len(edges))]
    return dict(src_id=1, end_time=END, q=1.0, s=1.0, sink_ids=SINKS, edge_list=edges,
                other_sources=[("Poisson", {"src_id": 2, "seed": 1, "rate": 1.0}),
                               ("Poisson", {"src_id": 3, "seed": 2, "rate": 1.0}),
                               ("Poisson", {"src_id": 4, "seed": 3, "rate": 1.0})])


_CTX = {}


def _ctx(start):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import oracle as O
    from redqueen_amd import _lib as L
    from redqueen_amd import engine
    if start not in _CTX:
        so = _sim_opts()
        g = engine.Graph(so["src_id"], so["other_sources"], so["sink_ids"], so["edge_list"],
                         so["end_time"], start_time=start)
        sc = O.Scenario(so, ("opt", 0), start_time=start)
        deg = {1: 1, 2: 40, 3: 3, 4: 0}
        sdeg = np.asarray([deg[int(x)] for x in g.stream_src_ids])
        assert sorted(sdeg) == [0, 1, 3, 40]
        _CTX[start] = (g, sc, sdeg)
    return (torch, O, L) + _CTX[start]


def _expand(torch, L, g, sdeg, ts, srcs, cap):
    """rq_log_rows + rq_log_expand on replicas with event times ts[i] and stream indices
    srcs[i]; the slack slots up to `cap` hold the degree-40 stream and a large time.
    Returns (row_off, columns) on the host; guards are checked here."""
    R = len(ts)
    big = int(np.argmax(sdeg))
    ev_t = np.full((R, cap), 9e29)
    ev_src = np.full((R, cap), big, dtype=np.int32)
    counts = np.full((R, 4), -5, dtype=np.int64)
    for i, (t, s) in enumerate(zip(ts, srcs)):
        assert len(t) == len(s) < cap
        ev_t[i, :len(t)] = t
        ev_src[i, :len(t)] = s
        counts[i, 2] = len(t)
    dt, ds, dc = torch.from_numpy(ev_t).cuda(), torch.from_numpy(ev_src).cuda(), torch.from_numpy(counts).cuda()
    row_off = torch.full((R + 1 + GUARD,), I_SENT, dtype=torch.int64, device="cuda")
    lib = L.lib()
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.rq_log_rows(g._h, ds.data_ptr(), dc.data_ptr(), R, cap, row_off.data_ptr(), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    ro = row_off.cpu().numpy()
    assert (ro[R + 1:] == I_SENT).all()
    ro = ro[:R + 1]
    exp_off = np.concatenate([[0], np.cumsum([int(sdeg[np.asarray(s, dtype=np.int64)].sum()) for s in srcs])])
    assert np.array_equal(ro, exp_off), np.nonzero(ro != exp_off)[0][:4]
    n = int(ro[-1])
    cols = {k: torch.full((n + GUARD,), D_SENT if k in ("time_delta", "t") else I_SENT,
                          dtype=torch.float64 if k in ("time_delta", "t") else torch.int64,
                          device="cuda") for k in COLS}
    rc = lib.rq_log_expand(g._h, dt.data_ptr(), ds.data_ptr(), dc.data_ptr(), R, cap,
                           row_off.data_ptr(), *(cols[k].data_ptr() for k in COLS), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in cols.items()}
    for k in COLS:
        assert (host[k][n:] == (D_SENT if k in ("time_delta", "t") else I_SENT)).all(), k
    return ro, {k: v[:n] for k, v in host.items()}


def _check(O, g, sc, start, ts, srcs, ro, cols):
    for i, (t, s) in enumerate(zip(ts, srcs)):
        ref = sc.expand(t, O.state_time_deltas(t, start), g.stream_src_ids[np.asarray(s, dtype=np.int64)])
        a, b = int(ro[i]), int(ro[i + 1])
        for c in COLS:
            got = cols[c][a:b]
            assert got.shape == ref[c].shape, (i, c)
            bad = np.nonzero(got != ref[c])[0]
            assert bad.size == 0, (i, c, "row %d (event %d): %r != %r" % (
                bad[0], ref["event_id"][bad[0]] - 100, got[bad[0]], ref[c][bad[0]]))


def _series(kind, n, start, seed):
    rs = np.random.RandomState(seed)
    if kind == "exp":
        return start + np.cumsum(rs.exponential(0.01, n))
    if kind == "repeat":
        gaps = rs.exponential(0.01, n)
        gaps[rs.rand(n) < 0.4] = 0.0
        return start + np.cumsum(gaps)
    return E.dirty_chain(n, start, E.DIRTY_SPOTS if kind == "dirty" else E.DIRTY_SPOTS_B)


def _streams(n, seed):
    """Stream indices with every degree, in runs and singly."""
    rs = np.random.RandomState(seed)
    return rs.randint(0, 4, n).astype(np.int32)


@pytest.mark.parametrize("start", [0.0, 20.0])
@pytest.mark.parametrize("kind", ["exp", "repeat", "dirty", "dirty_b"])
def test_log_expand_event_counts(kind, start):
    """Replicas of 0, 1, 1023, 1024, 1025, 2048, 2049 and 3000 events (the 1024-event chunks
    of rq_log_expand_k: full, one over, one short) in calls of 5, 4 and 1 replicas, for
    plain, repeated and dirty event times, from start 0 and from start 20."""
    torch, O, L, g, sc, sdeg = _ctx(start)
    full = _series(kind, 3000, start, 17)
    for call, counts in enumerate(([0, 1, 1023, 1024, 3000], [1025, 2048, 2049, 0], [3000])):
        ts = [full[:n] for n in counts]
        srcs = [_streams(n, 1000 * call + i) for i, n in enumerate(counts)]
        ro, cols = _expand(torch, L, g, sdeg, ts, srcs, 3001 + 7 * call)
        _check(O, g, sc, start, ts, srcs, ro, cols)


def test_log_expand_zero_degree_chunks():
    """Chunks that begin and end with degree-0 events, a chunk of 1024 degree-0 events
    (no row at all) between them, with dirty events in and around it: the state carried
    through a chunk without rows; and a replica with events but no row."""
    torch, O, L, g, sc, sdeg = _ctx(0.0)
    zero = int(np.argmin(sdeg))
    t = E.dirty_chain(3000, 0.0, E.DIRTY_SPOTS)
    a = _streams(3000, 5)
    a[0:3] = zero
    a[1020:1024] = zero
    a[1024:2048] = zero
    a[2048:2051] = zero
    a[2990:3000] = zero
    b = _streams(3000, 6)
    b[1024:2048] = zero
    b[1023], b[2048] = int(np.argmax(sdeg)), int(np.argmax(sdeg))
    c = np.full(2500, zero, dtype=np.int32)
    tb = E.dirty_chain(3000, 0.0, E.DIRTY_SPOTS_B)
    ts, srcs = [t, tb, t[:2500], t[:0]], [a, b, c, a[:0]]
    ro, cols = _expand(torch, L, g, sdeg, ts, srcs, 3010)
    assert ro[3] == ro[2] and ro[4] == ro[3]
    _check(O, g, sc, 0.0, ts, srcs, ro, cols)


@pytest.mark.parametrize("n_rep", [1, 4, 5, 1024, 1025, 2049])
def test_log_rows_replica_counts(n_rep):
    """0 ... 5 events per replica, many replicas with none: rq_log_scan_k's carry across
    its blocks of 1024 replicas (1024: one full block; 1025, 2049: one replica into the
    next), and rq_log_expand's row_off of every replica."""
    torch, O, L, g, sc, sdeg = _ctx(0.0)
    rs = np.random.RandomState(n_rep)
    cnt = np.where(rs.rand(n_rep) < 0.5, 0, rs.randint(0, 6, n_rep))
    cnt[0], cnt[-1] = 3, 2 + (n_rep == 1)
    ts = [np.cumsum(rs.exponential(0.5, n)) for n in cnt]
    srcs = [rs.randint(0, 4, n).astype(np.int32) for n in cnt]
    if n_rep > 1:
        srcs[-1][:] = int(np.argmax(sdeg))
    ro, cols = _expand(torch, L, g, sdeg, ts, srcs, 8)
    assert ro[-1] > 0
    _check(O, g, sc, 0.0, ts, srcs, ro, cols)

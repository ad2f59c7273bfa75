"""What the GPU tests of the log kernels share (test_gpu_timeline.py, test_gpu_followers.py,
test_gpu_rank_hist.py, test_gpu_log_walk.py): the context, packed hand-made logs and the
raw ABI calls, every output buffer of which carries a 64-element sentinel guard."""
import numpy as np
import pytest

from tests import followers_ref as FR

GUARD = 64
D_SENT, I_SENT = -1.2345e300, -7777


def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import oracle as O
    from redqueen_amd import _lib as L
    from redqueen_amd import engine, graphs
    return torch, O, L, engine, graphs


def graph(engine, so, **kw):
    return engine.Graph(so["src_id"], so["other_sources"], so["sink_ids"], so["edge_list"],
                        so["end_time"], **kw)


def pack(logs, cap, g, full=False):
    """(ev_t, ev_src, counts) of event lists [(t, src_id arrays)]: the tail of every
    replica's row holds NaN and -1 and must not be read.  ``full``: a log may fill its
    row (otherwise every row keeps a tail)."""
    R = len(logs)
    ev_t = np.full((R, cap), np.nan)
    ev_src = np.full((R, cap), -1, dtype=np.int32)
    counts = np.full((R, 4), -5, dtype=np.int64)
    idx = {int(s): k for k, s in enumerate(g.stream_src_ids)}
    for i, (t, s) in enumerate(logs):
        assert len(t) == len(s) and (len(t) <= cap if full else len(t) < cap)
        ev_t[i, :len(t)] = t
        ev_src[i, :len(t)] = [idx[int(x)] for x in s]
        counts[i, 2] = len(t)
    return ev_t, ev_src, counts


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def degrees_world():
    """Out-degrees 1, 63, 64, 65 (wall sources) and 129 (the controlled source) over 140
    sinks, edge list shuffled."""
    sinks = list(range(3000, 3140))
    edges = ([(2, sinks[139])] + [(3, x) for x in sinks[:63]] + [(4, x) for x in sinks[20:84]] +
             [(5, x) for x in sinks[70:135]] + [(1, x) for x in sinks[5:134]])
    edges = [edges[i] for i in np.random.RandomState(6).permutation(len(edges))]
    return dict(src_id=1, end_time=6.0, q=400.0, s=1.0, sink_ids=sinks, edge_list=edges,
                other_sources=[("Poisson", {"src_id": k, "seed": k, "rate": 4.0}) for k in (2, 3, 4, 5)])


def _dev(torch, ev_t, ev_src, counts):
    return (torch.from_numpy(np.ascontiguousarray(ev_t, dtype=np.float64)).cuda(),
            torch.from_numpy(np.ascontiguousarray(ev_src, dtype=np.int32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int64)).cuda())


def raw_timeline(torch, L, g, ev_t, ev_src, counts, edges, Ks, wall=False, expect=0):
    """rq_log_timeline on host arrays; outputs come back as numpy, their guard tails
    checked.  Returns (metrics, posts, status, wall_posts or None)."""
    R, cap = ev_t.shape
    nb, nK = len(edges) - 1, len(Ks)
    dt, ds, dc = _dev(torch, ev_t, ev_src, counts)
    de = torch.from_numpy(np.ascontiguousarray(edges, dtype=np.float64)).cuda()
    n_m, n_p, n_w = R * nb * (nK + 2), R * nb * 2, R * g.n_sinks * nb
    met = torch.full((n_m + GUARD,), D_SENT, dtype=torch.float64, device="cuda")
    pst = torch.full((n_p + GUARD,), I_SENT, dtype=torch.int64, device="cuda")
    sta = torch.full((R + GUARD,), I_SENT, dtype=torch.int32, device="cuda")
    wp = torch.full((n_w + GUARD,), I_SENT, dtype=torch.int32, device="cuda") if wall else None
    ks = np.asarray(Ks, dtype=np.int32)
    rc = L.lib().rq_log_timeline(g._h, dt.data_ptr(), ds.data_ptr(), dc.data_ptr(), R, cap,
                                 de.data_ptr(), nb, ks.ctypes.data_as(L._pi32), nK, met.data_ptr(),
                                 pst.data_ptr(), wp.data_ptr() if wall else None, sta.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == expect, rc
    torch.cuda.synchronize()
    met, pst, sta = met.cpu().numpy(), pst.cpu().numpy(), sta.cpu().numpy()
    assert (met[n_m:] == D_SENT).all() and (pst[n_p:] == I_SENT).all() and (sta[R:] == I_SENT).all()
    w = None
    if wall:
        w = wp.cpu().numpy()
        assert (w[n_w:] == I_SENT).all()
        w = w[:n_w].reshape(R, g.n_sinks, nb)
    return met[:n_m].reshape(R, nb, nK + 2), pst[:n_p].reshape(R, nb, 2), sta[:R], w


def raw_followers_dev(torch, L, g, dt, ds, dc, Ks, rows=True, expect=0):
    """rq_log_followers on device arrays; outputs come back as numpy, their guard tails
    checked.  Returns dict(vals, first_t, rows or None, r2_true, status)."""
    R, cap = dt.shape
    nK, NS = len(Ks), g.n_sinks
    n_v, n_f, n_r = R * NS * (nK + 2), R * NS, R * NS * 2
    val = torch.full((n_v + GUARD,), D_SENT, dtype=torch.float64, device="cuda")
    fst = torch.full((n_f + GUARD,), D_SENT, dtype=torch.float64, device="cuda")
    r2 = torch.full((R + GUARD,), D_SENT, dtype=torch.float64, device="cuda")
    sta = torch.full((R + GUARD,), I_SENT, dtype=torch.int32, device="cuda")
    rw = torch.full((n_r + GUARD,), I_SENT, dtype=torch.int32, device="cuda") if rows else None
    ks = np.asarray(Ks, dtype=np.int32)
    rc = L.lib().rq_log_followers(g._h, dt.data_ptr(), ds.data_ptr(), dc.data_ptr(), R, cap,
                                  ks.ctypes.data_as(L._pi32), nK, val.data_ptr(), fst.data_ptr(),
                                  rw.data_ptr() if rows else None, r2.data_ptr(), sta.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == expect, rc
    torch.cuda.synchronize()
    val, fst, r2, sta = val.cpu().numpy(), fst.cpu().numpy(), r2.cpu().numpy(), sta.cpu().numpy()
    assert (val[n_v:] == D_SENT).all() and (fst[n_f:] == D_SENT).all()
    assert (r2[R:] == D_SENT).all() and (sta[R:] == I_SENT).all()
    out = dict(vals=val[:n_v].reshape(R, NS, nK + 2), first_t=fst[:n_f].reshape(R, NS), rows=None,
               r2_true=r2[:R], status=sta[:R])
    if rows:
        w = rw.cpu().numpy()
        assert (w[n_r:] == I_SENT).all()
        out["rows"] = w[:n_r].reshape(R, NS, 2)
    if expect != 0:   # a refused call launches nothing
        assert (val == D_SENT).all() and (sta == I_SENT).all()
    return out


def raw_followers(torch, L, g, ev_t, ev_src, counts, Ks, rows=True, expect=0):
    return raw_followers_dev(torch, L, g, *_dev(torch, ev_t, ev_src, counts), Ks, rows, expect)


def assert_replica(out, i, ref, what, rows=True):
    """Replica i of a raw followers call / followers_host dict against the checker
    (tests/followers_ref.py): bit for bit."""
    assert out["status"][i] == ref["status"], (what, out["status"][i], ref["status"])
    assert FR.same_bits(out["vals"][i], ref["vals"]), what
    assert FR.same_bits(out["r2_true"][i], ref["r2_true"]), (what, out["r2_true"][i], ref["r2_true"])
    assert FR.same_bits(out["first_t"][i], ref["first_t"]), what
    if rows:
        assert np.array_equal(out["rows"][i], ref["rows"]), what


def assert_same(a, b, what, rows=True):
    """Two followers results of one batch: bit for bit."""
    for k in ("vals", "first_t", "r2_true"):
        assert FR.same_bits(a[k], b[k]), (what, k)
    assert np.array_equal(a["status"], b["status"]), what
    if rows:
        assert np.array_equal(a["rows"], b["rows"]), what


def followers_host(fl):
    """An engine.Followers as the dict of numpy arrays that the raw calls return."""
    return dict(vals=fl.vals.cpu().numpy(), first_t=fl.first_t.cpu().numpy(),
                rows=None if fl.rows is None else fl.rows.cpu().numpy(),
                r2_true=fl.r_2_true.cpu().numpy(), status=fl.status.cpu().numpy())


def raw_rank_hist(torch, L, g, ev_t, ev_src, counts, edges, nr, expect=0, cap=None):
    """rq_log_rank_hist on host arrays; outputs come back as numpy, their guard tails
    checked.  Returns (hist, n_seen, max_rank, status)."""
    R = ev_t.shape[0]
    cap = ev_t.shape[1] if cap is None else cap
    nb = len(edges) - 1
    dt, ds, dc = _dev(torch, ev_t, ev_src, counts)
    de = torch.from_numpy(np.ascontiguousarray(edges, dtype=np.float64)).cuda()
    n_h = R * nb * (nr + 1)
    hist = torch.full((n_h + GUARD,), D_SENT, dtype=torch.float64, device="cuda")
    ints = [torch.full((R + GUARD,), I_SENT, dtype=torch.int32, device="cuda") for _ in range(3)]
    rc = L.lib().rq_log_rank_hist(g._h, dt.data_ptr(), ds.data_ptr(), dc.data_ptr(), R, cap,
                                  de.data_ptr(), nb, nr, hist.data_ptr(), ints[0].data_ptr(),
                                  ints[1].data_ptr(), ints[2].data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == expect, rc
    torch.cuda.synchronize()
    hist = hist.cpu().numpy()
    ints = [v.cpu().numpy() for v in ints]
    assert (hist[n_h:] == D_SENT).all() and all((v[R:] == I_SENT).all() for v in ints)
    if expect != 0:
        assert (hist == D_SENT).all() and all((v == I_SENT).all() for v in ints)
    return hist[:n_h].reshape(R, nb, nr + 1), ints[0][:R], ints[1][:R], ints[2][:R]

"""rq_log_followers_tiled / BatchResult.followers(tiled=...) / batch.run_followers past
rq_log_followers' sink limit, on the GPU.  The checker is tests/followers_ref.py (tile-
agnostic: the kernel's sums restated in the kernel's order), and where both entries run,
rq_log_followers itself: every finite output bit for bit, NaN where NaN, integers equal.
Every output buffer of a raw call, the workspace included, carries a 64-element sentinel
guard; the workspace is handed over full of sentinels (its contents on entry do not matter).
The tile size TS is the library's (rq_log_followers_tile_sinks), so the graphs follow it."""
import ctypes as C

import numpy as np
import pytest

from tests import followers_ref as FR
from tests.loghelp import (D_SENT, GUARD, I_SENT, _dev, assert_replica as _assert_replica,
                           assert_same as _assert_same, ctx as _ctx, degrees_world as _degrees_world,
                           followers_host as _host, graph as _graph, pack, raw_followers_dev as _raw_old_dev)

pytestmark = pytest.mark.gpu


def _pack(logs, cap, g):
    return pack(logs, cap, g, full=True)


def _ws_bytes(L, g, R):
    n = C.c_size_t()
    assert L.lib().rq_log_followers_tiled_workspace(g._h, R, C.byref(n)) == 0
    TS = int(L.lib().rq_log_followers_tile_sinks())
    flags = 4 * R * (-(-g.n_sinks // TS))
    assert n.value == -(-flags // 256) * 256, (n.value, flags)     # 4 R tiles, rounded up to 256
    return n.value, flags


def _raw_dev(torch, L, g, dt, ds, dc, Ks, rows=True, expect=0, ws_bytes=None, n_rep=None):
    """rq_log_followers_tiled on device arrays; outputs come back as numpy, their guard
    tails checked.  Returns dict(vals, first_t, rows or None, r2_true, status)."""
    R, cap = dt.shape
    nK, NS = len(Ks), g.n_sinks
    n_v, n_f, n_r = R * NS * (nK + 2), R * NS, R * NS * 2
    val = torch.full((n_v + GUARD,), D_SENT, dtype=torch.float64, device="cuda")
    fst = torch.full((n_f + GUARD,), D_SENT, dtype=torch.float64, device="cuda")
    r2 = torch.full((R + GUARD,), D_SENT, dtype=torch.float64, device="cuda")
    sta = torch.full((R + GUARD,), I_SENT, dtype=torch.int32, device="cuda")
    rw = torch.full((n_r + GUARD,), I_SENT, dtype=torch.int32, device="cuda") if rows else None
    if g.n_sinks <= L.FOLLOWERS_TILED_MAX_SINKS and not getattr(g, "_dup", False):
        need, flags = _ws_bytes(L, g, R)
    else:
        need, flags = 256, 0
    ws = torch.full((need // 4 + GUARD,), I_SENT, dtype=torch.int32, device="cuda")
    ks = np.asarray(Ks, dtype=np.int32)
    rc = L.lib().rq_log_followers_tiled(g._h, dt.data_ptr(), ds.data_ptr(), dc.data_ptr(),
                                        R if n_rep is None else n_rep, cap,
                                        ks.ctypes.data_as(L._pi32), nK, val.data_ptr(), fst.data_ptr(),
                                        rw.data_ptr() if rows else None, r2.data_ptr(), sta.data_ptr(),
                                        ws.data_ptr(), need if ws_bytes is None else ws_bytes,
                                        torch.cuda.current_stream().cuda_stream)
    assert rc == expect, rc
    torch.cuda.synchronize()
    val, fst, r2, sta, ws = (v.cpu().numpy() for v in (val, fst, r2, sta, ws))
    assert (val[n_v:] == D_SENT).all() and (fst[n_f:] == D_SENT).all()
    assert (r2[R:] == D_SENT).all() and (sta[R:] == I_SENT).all()
    assert (ws[flags // 4:] == I_SENT).all()        # only the flags are written
    out = dict(vals=val[:n_v].reshape(R, NS, nK + 2), first_t=fst[:n_f].reshape(R, NS), rows=None,
               r2_true=r2[:R], status=sta[:R])
    if rows:
        w = rw.cpu().numpy()
        assert (w[n_r:] == I_SENT).all()
        out["rows"] = w[:n_r].reshape(R, NS, 2)
    if expect != 0:   # a refused call launches nothing
        assert (val == D_SENT).all() and (fst == D_SENT).all() and (r2 == D_SENT).all()
        assert (sta == I_SENT).all() and (ws == I_SENT).all()
        assert not rows or (rw.cpu().numpy() == I_SENT).all()
    else:
        assert np.isin(ws[:flags // 4], (0, 1)).all()
    return out


def _raw(torch, L, g, ev_t, ev_src, counts, Ks, rows=True, **kw):
    return _raw_dev(torch, L, g, *_dev(torch, ev_t, ev_src, counts), Ks, rows, **kw)


def _prefix(ref4, nK):
    """The checker's result for the first nK of its 4 K values (a K's integral does not
    depend on the other Ks: the columns are [top_K..., rank, rank^2])."""
    v = ref4["vals"]
    return dict(ref4, vals=np.concatenate([v[:, :nK], v[:, 4:]], axis=1))


# ------------------------------------------------- 1. the old entry's bits
@pytest.mark.parametrize("world", ["degrees", "readme"])
def test_same_bits_as_the_plain_entry(world):
    torch, _O, L, engine, graphs = _ctx()
    so, R = (_degrees_world(), 5) if world == "degrees" else (graphs.readme(), 8)
    Ks4 = (1, 2, 3, 5)
    g = _graph(engine, so)
    res = g.run("opt", q=so["q"], s=so["s"], n_rep=R, ctrl_seed=11, world_seed=70, randomize=True,
                Ks=(1,), event_log=True)
    counts = res.counts.cpu().numpy()
    assert counts[:, 0].sum() > 0 and counts[:, 1].sum() > 0
    refs = [FR.play(*res.events(i), so["edge_list"], so["sink_ids"], so["src_id"], so["end_time"], Ks4)
            for i in range(R)]
    assert all(r["status"] == 0 for r in refs)
    for nK in (1, 2, 3, 4):
        for rows in (True, False):
            what = "%s nK %d rows %d" % (world, nK, rows)
            new = _raw_dev(torch, L, g, res.ev_t, res.ev_src, res.counts, Ks4[:nK], rows)
            old = _raw_old_dev(torch, L, g, res.ev_t, res.ev_src, res.counts, Ks4[:nK], rows)
            _assert_same(new, old, what, rows)
            for i in range(R):
                _assert_replica(new, i, _prefix(refs[i], nK), "%s replica %d" % (what, i), rows)


# ------------------------------------------------------------ 2. tile edges
def _tile_world(N, TS):
    """Sinks 1..N (column = id - 1).  The controlled source 1 reaches every third sink, wall
    2 every sink (more than 64 columns in every tile but a last tile of one), wall 3 the last
    sink only (a tile of one column at N = k TS + 1), wall 4 the 64 columns below the tile
    0 / 1 boundary and up to 65 above it, wall 5 no sink, wall 6 the first sink, wall 7 one
    sink of tile 1 (the last sink when there is no tile 1)."""
    sinks = list(range(1, N + 1))
    mid = sinks[min(TS + 5, N - 1)]
    edges = ([(2, s) for s in sinks] + [(1, s) for s in sinks[::3]] + [(3, sinks[-1])] +
             [(4, s) for s in sinks[TS - 64:TS + 65]] + [(6, sinks[0])] + [(7, mid)])
    edges = [edges[i] for i in np.random.RandomState(N).permutation(len(edges))]
    return dict(src_id=1, end_time=10.0, sink_ids=sinks, edge_list=edges,
                other_sources=[("Poisson2", {"src_id": k, "seed": 1, "rate": 1.0}) for k in (2, 3, 4, 5, 6, 7)])


# test_sink_limit's 5 events, one of the straddling source, and two events at t = 8 on sinks
# of different tiles (the first and the last sink): not a tie, one pivot row for r2_true
CLEAN = ([0.5, 1.0, 2.5, 3.0, 4.0, 7.0, 8.0, 8.0], [3, 1, 2, 4, 2, 1, 6, 3])


@pytest.mark.parametrize("shape", ["TS", "TS+1", "2TS", "2TS+1"])
def test_tile_edges(shape):
    torch, _O, L, engine, graphs = _ctx()
    TS = int(L.lib().rq_log_followers_tile_sinks())
    N = {"TS": TS, "TS+1": TS + 1, "2TS": 2 * TS, "2TS+1": 2 * TS + 1}[shape]
    so = _tile_world(N, TS)
    g = _graph(engine, so)
    Ks = (1, 2, 3, 4)
    ref = FR.play(CLEAN[0], CLEAN[1], so["edge_list"], so["sink_ids"], 1, so["end_time"], Ks)
    assert ref["status"] == 0 and ref["n_rows"] == 7
    packed = _dev(torch, *_pack([CLEAN], 9, g))
    for rows in (True, False):
        out = _raw_dev(torch, L, g, *packed, Ks, rows)
        _assert_replica(out, 0, ref, "%s rows %d" % (shape, rows), rows)


# ------------------------------------------------------- 3. flags cross tiles
def test_flags_cross_tiles_and_defensive_rules():
    torch, _O, L, engine, graphs = _ctx()
    TS = int(L.lib().rq_log_followers_tile_sinks())
    N = 2 * TS + 1
    so = _tile_world(N, TS)
    g = _graph(engine, so)
    Ks = (1, 2)
    # (b) walls 2 and 7 at t = 2: two rows at one time for wall 7's sink of tile 1, no other
    tied = ([0.5, 1.0, 2.0, 2.0, 6.0], [3, 1, 2, 7, 6])
    empty = ([1.0, 2.0], [5, 5])                     # (c) a stream without edges only
    last = ([1.0, 4.0, 4.5], [3, 3, 5])              # (d) the last tile only
    full = ([0.5, 1.0, 2.5, 3.0, 4.0, 7.0, 8.0, 9.0], [3, 1, 2, 4, 2, 1, 6, 7])
    short = ([0.5, 1.0, 2.0], [2, 3, 1])
    cap = 8
    logs = [CLEAN, tied, empty, last, full, short, full, full]
    ev_t, ev_src, counts = _pack(logs, cap, g)
    # (e) counts above ev_cap and negative, stream indices outside the graph
    counts[4, 2] = cap + 1000
    counts[5, 2] = -3
    counts[6, 2] = 1 << 40
    n_str = len(g.stream_src_ids)
    bad_at = [1, 4, 5, 7]
    ev_src[7, bad_at] = [n_str, -1, 1 << 30, -(1 << 31)]
    out = _raw(torch, L, g, ev_t, ev_src, counts, Ks)

    def play(log):
        return FR.play(log[0], log[1], so["edge_list"], so["sink_ids"], 1, so["end_time"], Ks)
    keep = [k for k in range(cap) if k not in bad_at]
    kept = ([full[0][k] for k in keep], [full[1][k] for k in keep])
    refs = [play(x) for x in (CLEAN, tied, empty, last, full, ([], []), full, kept)]
    assert [r["status"] for r in refs] == [0, FR.ST_TIE, FR.ST_EMPTY, 0, 0, FR.ST_EMPTY, 0, 0]
    assert FR.ST_TIE == L.ST_TIE and FR.ST_EMPTY == L.ST_EMPTY
    for i, ref in enumerate(refs):
        _assert_replica(out, i, ref, "replica %d" % i)
    # (b): the whole replica is NaN, first_t and rows are valid in every tile
    assert np.isnan(out["vals"][1]).all() and np.isnan(out["r2_true"][1])
    ft = out["first_t"][1]
    assert ft[0] == 1.0 and ft[1] == 2.0 and ft[N - 1] == 0.5 and not np.isnan(ft).any()
    assert out["rows"][1][TS + 5][1] == 2 and np.array_equal(out["rows"][1][0], [1, 2])
    # (c)
    assert np.isnan(out["vals"][2]).all() and np.isnan(out["first_t"][2]).all() and (out["rows"][2] == 0).all()
    # (d): the other tiles hold exactly 0.0 and no first row
    assert (out["vals"][3][:2 * TS] == 0.0).all() and np.isnan(out["first_t"][3][:2 * TS]).all()
    assert (out["rows"][3][:2 * TS] == 0).all() and out["first_t"][3][N - 1] == 1.0
    # the last sink: rank 1 on [1, 4), rank 2 on [4, 10)
    assert np.array_equal(out["vals"][3][N - 1], [0.0, 3.0, 1.0 * 3.0 + 2.0 * 6.0, 1.0 * 3.0 + 4.0 * 6.0])
    # a neighbour's flags do not leak: (a) alone has the bits it has in the batch
    alone = _raw(torch, L, g, *_pack([CLEAN], cap, g), Ks)
    for k in ("vals", "first_t", "r2_true"):
        assert FR.same_bits(alone[k][0], out[k][0]), k
    assert np.array_equal(alone["rows"][0], out["rows"][0]) and alone["status"][0] == 0


# ------------------------------------------------------ 4. validation on device
def test_validation_on_device():
    torch, _O, L, engine, graphs = _ctx()
    lib = L.lib()
    TS = int(lib.rq_log_followers_tile_sinks())
    Ks = (1, 2)
    n = C.c_size_t(77)
    # duplicate edges
    so = _tile_world(TS + 1, TS)
    g_dup = _graph(engine, dict(so, edge_list=so["edge_list"] + [(2, 9)]))
    g_dup._dup = True
    _raw(torch, L, g_dup, *_pack([CLEAN], 9, g_dup), Ks, expect=L.RQ_EUNSUPPORTED)
    assert lib.rq_log_followers_tiled_workspace(g_dup._h, 1, C.byref(n)) == L.RQ_EUNSUPPORTED and n.value == 77
    # one sink past the limit
    MAX = L.FOLLOWERS_TILED_MAX_SINKS

    def big(ns):
        sinks = list(range(1, ns + 1))
        return dict(src_id=1, end_time=10.0, sink_ids=sinks,
                    edge_list=[(2, s) for s in sinks] + [(1, s) for s in sinks[::3]] + [(3, sinks[-1])] +
                              [(6, sinks[0])] + [(4, sinks[5])],
                    other_sources=[("Poisson2", {"src_id": k, "seed": 1, "rate": 1.0}) for k in (2, 3, 4, 6)])
    g_big = _graph(engine, big(MAX + 1))
    _raw(torch, L, g_big, *_pack([CLEAN], 9, g_big), Ks, expect=L.RQ_EUNSUPPORTED)
    assert lib.rq_log_followers_tiled_workspace(g_big._h, 1, C.byref(n)) == L.RQ_EUNSUPPORTED and n.value == 77
    # the limit itself runs: the r2 pass fills one workgroup's LDS with ranks
    so_max = big(MAX)
    g_max = _graph(engine, so_max)
    out = _raw(torch, L, g_max, *_pack([CLEAN], 9, g_max), Ks)
    _assert_replica(out, 0, FR.play(CLEAN[0], CLEAN[1], so_max["edge_list"], so_max["sink_ids"], 1, 10.0, Ks),
                    "the sink limit")
    # a workspace one byte short, and more (replica, tile) blocks than a grid's x axis takes
    g = _graph(engine, _tile_world(2 * TS + 1, TS))
    packed = _pack([CLEAN], 9, g)
    need, _flags = _ws_bytes(L, g, 1)
    _raw(torch, L, g, *packed, Ks, expect=L.RQ_EINVAL, ws_bytes=need - 1)
    _raw(torch, L, g, *packed, Ks, expect=L.RQ_EINVAL, ws_bytes=1 << 40, n_rep=1 << 30)
    _raw(torch, L, g, *packed, Ks)      # and the same call with its workspace runs


# --------------------------------------------------------------- 5. the facade
def _world_5000(graphs):
    return graphs.followers_graph(num_followers=5000, num_sources=40, degree=3, end_time=1.0)


def test_facade_runs_past_the_plain_limit():
    torch, _O, L, engine, graphs = _ctx()
    so = _world_5000(graphs)
    g = _graph(engine, so)
    assert g.n_sinks == 5000
    R, Ks = 3, (1, 2)
    res = g.run("opt", q=so["q"], s=so["s"], n_rep=R, ctrl_seed=7, world_seed=8, randomize=True, Ks=Ks,
                event_log=True)
    out = _host(res.followers(Ks=Ks, rows=True))
    for i in range(R):
        t, s = res.events(i)
        ref = FR.play(t, s, so["edge_list"], so["sink_ids"], so["src_id"], so["end_time"], Ks)
        _assert_replica(out, i, ref, "5000 followers, replica %d" % i)
    assert (out["status"] == 0).all()
    with pytest.raises(L.RQError) as e:
        res.followers(Ks=Ks, rows=True, tiled=False)
    assert e.value.code == L.RQ_EUNSUPPORTED


def test_facade_tiled_equals_plain_on_c3():
    torch, _O, L, engine, graphs = _ctx()
    so = dict(graphs.followers_graph(end_time=1.5), q=2500.0)
    g = _graph(engine, so)
    assert g.n_sinks == 1000
    res = g.run("opt", q=so["q"], s=so["s"], n_rep=8, ctrl_seed=11, world_seed=70, randomize=True, Ks=(1, 3),
                event_log=True)
    counts = res.counts.cpu().numpy()
    assert counts[:, 0].sum() > 0 and counts[:, 1].sum() > 0
    for rows in (True, False):
        a, b = _host(res.followers(rows=rows, tiled=True)), _host(res.followers(rows=rows, tiled=False))
        _assert_same(a, b, "C3 size rows %d" % rows, rows)
        assert (a["status"] == 0).all()
    assert _host(res.followers(rows=False))["rows"] is None


def test_run_followers_on_5000_followers():
    torch, _O, L, engine, graphs = _ctx()
    import pandas as pd
    from redqueen_amd import batch
    from redqueen_amd.opt_model import SimOpts
    so = SimOpts(**_world_5000(graphs))
    seeds = np.arange(300, 306)
    Ks = (1, 2)
    f1 = batch.run_followers(so, seeds, Ks=Ks, chunk_replicas=6)
    f2 = batch.run_followers(so, seeds, Ks=Ks, chunk_replicas=4)
    g = batch.compiled_graph(so)
    st = torch.as_tensor(seeds)
    res = g.run("opt", q=float(so.q), s=so.s, n_rep=6, ctrl_seed=st, world_seed=st, randomize=True,
                Ks=Ks, event_log=True)
    fl = res.followers(Ks=Ks, rows=True)
    exp = batch.followers_frame(fl.sink_ids, fl.Ks, fl.vals.cpu().numpy(), fl.rows.cpu().numpy(),
                                fl.status.cpu().numpy())
    pd.testing.assert_frame_equal(f1, exp, check_exact=True)
    pd.testing.assert_frame_equal(f2, exp, check_exact=True)
    assert len(f1) == 5000 and (f1.n + f1.n_flagged == 6).all()

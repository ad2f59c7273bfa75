"""rq_log_followers / BatchResult.followers / batch.run_followers and the utils losses on
the GPU against the host checker tests/followers_ref.py (the kernel's sums restated in the
kernel's order: bit for bit) and the reference's values in tests/golden/followers.npz.

Tolerance against reference values (derived, not measured; followers_ref's docstring): a
value is a sum of at most n non-negative terms of at most 4 roundings each, so whatever
the summation order |got - exp| <= (n + 8) * 2**-52 * |exp| with n the replica's pivot
rows; a value whose expectation is 0 must be exactly 0.0; integer outputs must be equal.
Every output buffer of a raw call carries a 64-element sentinel guard."""
import functools
import math
import types

import numpy as np
import pytest

from tests import followers_ref as FR
from tests import timeline_ref as TR
from tests.loghelp import (assert_replica as _assert_replica, ctx as _ctx, degrees_world as _degrees_world,
                           followers_host as _host, graph as _graph, pack, raw_followers as _raw,
                           raw_followers_dev as _raw_dev)

pytestmark = pytest.mark.gpu
_pack = functools.partial(pack, full=True)   # a log may fill its row here


def _assert_close(got, exp, rows, what):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    err = np.abs(got - exp) / np.maximum(FR.ULP * np.abs(exp), 1e-300)
    print(what, "max |got - exp| = %.3g ulp over %d rows" % (float(err.max()) if got.size else 0.0, rows))
    assert got.shape == exp.shape, what
    assert not np.isnan(got).any(), what
    assert (got[exp == 0.0] == 0.0).all(), what
    bad = np.abs(got - exp) > FR.tol(rows, exp)
    assert not bad.any(), (what, np.argwhere(bad)[:4], got[bad][:4], exp[bad][:4])


def _fixture_world(f, name):
    src_id, end, q = int(f[name + "_world"][0]), float(f[name + "_world"][1]), float(f[name + "_world"][2])
    so = dict(src_id=src_id, end_time=end, q=q, sink_ids=[int(x) for x in f[name + "_sinks"]],
              edge_list=[tuple(int(v) for v in e) for e in f[name + "_edges"]],
              other_sources=[("Poisson2", {"src_id": int(s), "seed": 1, "rate": 1.0})
                             for s in f[name + "_srcs"]])
    return so


def _fixture_expected(f, name, nK):
    sinks = np.sort(f[name + "_sinks"])
    at = np.searchsorted(sinks, f[name + "_cols"])
    vals = np.zeros((sinks.size, nK + 2))
    first = np.full(sinks.size, np.nan)
    cnt = np.zeros((sinks.size, 2), dtype=np.int32)
    vals[at], first[at], cnt[at] = f[name + "_vals"], f[name + "_first"], f[name + "_cnt"]
    return vals, first, cnt


# ------------------------------------------------------------- 1. fixture logs, raw ABI
def test_fixture_logs_through_the_raw_abi(golden):
    torch, _O, L, engine, graphs = _ctx()
    f = golden("followers.npz")
    Ks = [int(k) for k in f["Ks"]]
    for name in (str(n) for n in f["names"]):
        so = _fixture_world(f, name)
        g = _graph(engine, so)
        t, s = f[name + "_t"], f[name + "_src"]
        out = _raw(torch, L, g, *_pack([(t, s)], t.size + 77, g), Ks)
        ref = FR.play(t, s, so["edge_list"], so["sink_ids"], so["src_id"], so["end_time"], Ks)
        assert ref["status"] == 0
        _assert_replica(out, 0, ref, name)
        rows = int(f[name + "_rows"][0])
        vals, first, cnt = _fixture_expected(f, name, len(Ks))
        _assert_close(out["vals"][0], vals, rows, name)
        _assert_close(out["r2_true"][0], f[name + "_r2true"], rows, name + " r2_true")
        assert FR.same_bits(out["first_t"][0], first) and np.array_equal(out["rows"][0], cnt), name


# ------------------------------------------------- 2. README graph, every controller
@pytest.mark.parametrize("ctrl", ["opt", "poisson", "wall", "times"])
def test_readme_graph_every_controller(ctrl):
    torch, _O, L, engine, graphs = _ctx()
    so = graphs.readme()
    Ks = (1, 2, 33)
    R = 16
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
    assert (res.status.cpu().numpy() == 0).all()
    fl = res.followers(rows=True)           # Ks: the result's own
    assert fl.Ks == list(Ks) and np.array_equal(fl.sink_ids, [1, 2, 3])
    out = _host(fl)
    counts = res.counts.cpu().numpy()
    whole = res.metrics.cpu().numpy()
    for i in range(R):
        t, s = res.events(i)
        ref = FR.play(t, s, so["edge_list"], so["sink_ids"], so["src_id"], so["end_time"], Ks)
        assert ref["status"] == 0 and ref["n_rows"] == counts[i, 3]
        _assert_replica(out, i, ref, "%s replica %d" % (ctrl, i))
        # the sweep's own top_K: the mean over the S seen sinks of the per-sink integrals
        S = int(np.count_nonzero(~np.isnan(out["first_t"][i])))
        for q, K in enumerate(Ks):
            tot = 0.0
            for x in range(g.n_sinks):
                tot = tot + out["vals"][i, x, q]
            _assert_close(np.asarray([tot / S]), whole[i, q:q + 1], int(counts[i, 3]),
                          "%s replica %d top_%d" % (ctrl, i, K))
        assert out["rows"][i].sum() >= counts[i, 2]     # every event has an edge here
    # the accessors
    assert fl.top_k(33).shape == fl.rank_int.shape == fl.rank_sq_int.shape == (R, 3)
    assert torch.equal(fl.top_k(2), fl.vals[:, :, 1]) and torch.equal(fl.rank_int, fl.vals[:, :, 3])
    assert torch.equal(fl.rank_sq_int, fl.vals[:, :, 4])


# ------------------------------------------------------------------- 3. wide rows
@pytest.mark.parametrize("world", ["degrees", "c3_short"])
def test_wide_rows(world):
    torch, _O, L, engine, graphs = _ctx()
    if world == "degrees":
        so, R, Ks = _degrees_world(), 5, (1, 3)
    else:   # C3's 1000 followers (the controlled source reaches all of them): 36 KB of LDS
        so, R, Ks = graphs.followers_graph(end_time=1.5), 8, (1,)
        so = dict(so, q=2500.0)
        assert len(so["sink_ids"]) == 1000
    g = _graph(engine, so)
    res = g.run("opt", q=so["q"], s=so["s"], n_rep=R, ctrl_seed=11, world_seed=70, randomize=True,
                Ks=Ks, event_log=True)
    counts = res.counts.cpu().numpy()
    assert counts[:, 0].sum() > 0 and counts[:, 1].sum() > 0
    for rows in (True, False):
        out = _host(res.followers(rows=rows))
        for i in range(R):
            t, s = res.events(i)
            ref = FR.play(t, s, so["edge_list"], so["sink_ids"], so["src_id"], so["end_time"], Ks)
            _assert_replica(out, i, ref, "%s replica %d" % (world, i), rows=rows)


# ------------------------------------------------------------ 4. ties and empties
TIE_WORLD = dict(src_id=1, end_time=20.0, sink_ids=[10, 11, 12, 13],
                 edge_list=[(1, 10), (1, 12), (2, 10), (2, 11), (3, 12), (4, 13), (4, 11)],
                 other_sources=[("Poisson2", {"src_id": s, "seed": 1, "rate": 1.0}) for s in (2, 3, 4, 5)])


def test_realdata_tie_world():
    """Two RealData sources post at t = 5 and both reach sink 10."""
    torch, _O, L, engine, graphs = _ctx()
    so = dict(src_id=1, end_time=20.0, sink_ids=[10, 11, 12],
              edge_list=[(1, 10), (2, 10), (2, 11), (3, 10), (3, 12)],
              other_sources=[("RealData", {"src_id": 2, "times": [1.0, 5.0, 9.0]}),
                             ("RealData", {"src_id": 3, "times": [2.5, 5.0, 14.0]})])
    g = _graph(engine, so)
    res = g.run("wall", n_rep=1, Ks=(1,), event_log=True)
    t, s = res.events(0)
    assert np.count_nonzero(t == 5.0) == 2
    out = _host(res.followers(rows=True))
    ref = FR.play(t, s, so["edge_list"], so["sink_ids"], 1, 20.0, (1,))
    assert ref["status"] == FR.ST_TIE == L.ST_TIE
    _assert_replica(out, 0, ref, "RealData tie")
    assert np.isnan(out["vals"]).all() and np.isnan(out["r2_true"]).all()
    assert np.array_equal(out["first_t"][0], [1.0, 1.0, 2.5])
    assert np.array_equal(out["rows"][0], [[0, 6], [0, 3], [0, 3]])


def test_hand_made_ties_and_empty():
    torch, _O, L, engine, graphs = _ctx()
    so = TIE_WORLD
    g = _graph(engine, so)
    Ks = (1, 2)
    plain = ([0.5, 1.0, 2.0, 3.0, 7.0, 11.0, 13.5], [2, 3, 1, 4, 2, 1, 3])
    # equal times on disjoint sinks: (2 | 3), (1 | 4), (3 | 4); source 5 has no edge
    disjoint = ([0.5, 2.0, 2.0, 5.0, 5.0, 5.0, 9.0, 9.0, 16.0], [4, 2, 3, 1, 5, 4, 3, 4, 2])
    # sink 10 gets a wall row and an own row at t = 5
    tied = ([0.5, 2.0, 5.0, 5.0, 9.0, 12.0], [3, 4, 2, 1, 3, 2])
    other = ([1.25, 4.0, 6.0, 6.0 + 2.0 ** -40, 19.0], [1, 2, 3, 1, 4])
    empty = ([], [])
    no_rows = ([1.0, 2.0], [5, 5])     # events of a source without edges only
    logs = [plain, tied, disjoint, empty, other, no_rows]
    out = _raw(torch, L, g, *_pack(logs, 16, g), Ks)
    assert list(out["status"]) == [0, L.ST_TIE, 0, L.ST_EMPTY, 0, L.ST_EMPTY]
    for i, (t, s) in enumerate(logs):
        ref = FR.play(t, s, so["edge_list"], so["sink_ids"], 1, so["end_time"], Ks)
        _assert_replica(out, i, ref, "hand-made %d" % i)
    for i in (1, 3, 5):
        assert np.isnan(out["vals"][i]).all() and np.isnan(out["r2_true"][i])
    assert np.isnan(out["first_t"][3]).all() and (out["rows"][3] == 0).all() and (out["rows"][5] == 0).all()
    assert np.array_equal(out["first_t"][1], [5.0, 2.0, 0.5, 2.0])          # valid in a TIE replica
    assert np.array_equal(out["rows"][1], [[1, 2], [0, 3], [1, 2], [0, 1]])
    # the neighbours of the flagged replicas: the bits they have without them
    logs2 = [plain, other, disjoint, other, other, plain]
    out2 = _raw(torch, L, g, *_pack(logs2, 16, g), Ks)
    assert (out2["status"] == 0).all()
    for i in (0, 2, 4):
        assert FR.same_bits(out["vals"][i], out2["vals"][i]) and FR.same_bits(out["r2_true"][i], out2["r2_true"][i])


# ------------------------------------------------------------------ 5. determinism
def test_same_bits_alone_permuted_and_without_rows():
    torch, _O, L, engine, graphs = _ctx()
    so = graphs.readme()
    g = _graph(engine, so)
    R, Ks = 8, (1, 2)
    res = g.run("opt", q=so["q"], s=so["s"], n_rep=R, ctrl_seed=21, world_seed=33, randomize=True, Ks=Ks,
                event_log=True)
    dt, ds, dc = res.ev_t, res.ev_src, res.counts
    a = _raw_dev(torch, L, g, dt, ds, dc, Ks)
    b = _raw_dev(torch, L, g, dt, ds, dc, Ks)
    c = _raw_dev(torch, L, g, dt, ds, dc, Ks, rows=False)
    assert (a["status"] == 0).all() and c["rows"] is None
    keys = ("vals", "first_t", "r2_true")
    for k in keys:
        assert FR.same_bits(a[k], b[k]) and FR.same_bits(a[k], c[k]), k
    assert np.array_equal(a["rows"], b["rows"]) and np.array_equal(a["status"], c["status"])
    perm = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4], device=dt.device)
    p = _raw_dev(torch, L, g, dt[perm].contiguous(), ds[perm].contiguous(), dc[perm].contiguous(), Ks)
    pn = perm.cpu().numpy()
    for k in keys:
        assert FR.same_bits(p[k], a[k][pn]), k
    assert np.array_equal(p["rows"], a["rows"][pn])
    for i in range(R):
        o = _raw_dev(torch, L, g, dt[i:i + 1].contiguous(), ds[i:i + 1].contiguous(), dc[i:i + 1].contiguous(), Ks)
        for k in keys:
            assert FR.same_bits(o[k][0], a[k][i]), (k, i)
        assert np.array_equal(o["rows"][0], a["rows"][i])
    # the method gives the raw call's bits
    m = _host(res.followers(rows=True))
    for k in keys:
        assert FR.same_bits(m[k], a[k]), k


# ------------------------------------------------ 6. clamping and bad stream indices
def test_counts_are_clamped_and_bad_streams_give_no_row():
    torch, _O, L, engine, graphs = _ctx()
    so = TIE_WORLD
    g = _graph(engine, so)
    Ks = (1, 2)
    full = ([0.5, 1.0, 2.0, 3.0, 7.0, 11.0, 13.5, 15.0], [2, 3, 1, 4, 2, 1, 3, 2])
    short = ([0.5, 1.0, 2.0], [2, 3, 1])
    cap = 8
    ev_t, ev_src, counts = _pack([full, short, full, full], cap, g)
    counts[0, 2] = cap + 1000          # above ev_cap: the 8 events of the row
    counts[1, 2] = -3                  # negative: no event
    counts[2, 2] = 1 << 40
    # replica 3: stream indices outside the graph give no row
    n_str = len(g.stream_src_ids)
    bad_at = [1, 4, 5, 7]
    ev_src[3, bad_at] = [n_str, -1, 1 << 30, -(1 << 31)]
    out = _raw(torch, L, g, ev_t, ev_src, counts, Ks)
    ref_full = FR.play(full[0], full[1], so["edge_list"], so["sink_ids"], 1, so["end_time"], Ks)
    _assert_replica(out, 0, ref_full, "count above ev_cap")
    _assert_replica(out, 2, ref_full, "count far above ev_cap")
    assert out["status"][1] == L.ST_EMPTY and np.isnan(out["vals"][1]).all() and (out["rows"][1] == 0).all()
    keep = [k for k in range(cap) if k not in bad_at]
    ref = FR.play([full[0][k] for k in keep], [full[1][k] for k in keep], so["edge_list"], so["sink_ids"], 1,
                  so["end_time"], Ks)
    _assert_replica(out, 3, ref, "bad stream indices")


# ------------------------------------------------------------------- 7. validation
def test_validation():
    torch, _O, L, engine, graphs = _ctx()
    g = _graph(engine, TIE_WORLD)
    lib = L.lib()
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    k1 = np.asarray([1, 2, 3, 4, 5], dtype=np.int32)
    k0 = np.asarray([1, 0], dtype=np.int32)

    def call(h=g._h, ev_t=p, ev_src=p, counts=p, n_rep=2, cap=4, ks=k1, nK=2, vals=p, first=p, rows=None,
             r2=p, sta=p):
        return lib.rq_log_followers(h, ev_t, ev_src, counts, n_rep, cap,
                                    None if ks is None else ks.ctypes.data_as(L._pi32), nK, vals, first,
                                    rows, r2, sta, None)
    bad = [dict(nK=0), dict(nK=5), dict(nK=-1), dict(ks=k0), dict(ks=None), dict(n_rep=0), dict(n_rep=-2),
           dict(n_rep=1 << 31), dict(cap=0), dict(cap=-1), dict(cap=(1 << 24) + 1), dict(vals=None),
           dict(first=None), dict(r2=None), dict(sta=None), dict(h=None), dict(ev_t=None), dict(ev_src=None),
           dict(counts=None)]
    for kw in bad:
        assert call(**kw) == L.RQ_EINVAL, kw
    g_dup = _graph(engine, dict(TIE_WORLD, edge_list=TIE_WORLD["edge_list"] + [(2, 10)]))
    assert call(h=g_dup._h) == L.RQ_EUNSUPPORTED
    torch.cuda.synchronize()
    assert (buf == 0).all()   # nothing was launched
    res = g.run("wall", n_rep=2, Ks=(1,), event_log=True)
    with pytest.raises(ValueError):
        res.followers(Ks=(0,))
    with pytest.raises(ValueError):
        res.followers(Ks=(1, 2, 3, 4, 5))
    with pytest.raises(ValueError):
        g.run("wall", n_rep=2, Ks=(1,)).followers()   # no event log


def test_sink_limit():
    """rq_log_followers_max_sinks(4, 1) sinks run (the per-sink state of one replica fills
    one workgroup's LDS); one more is refused with rows and fits without them."""
    torch, _O, L, engine, graphs = _ctx()
    lib = L.lib()
    N = int(lib.rq_log_followers_max_sinks(4, 1))
    assert 1000 < N < int(lib.rq_log_followers_max_sinks(4, 0)) < int(lib.rq_log_followers_max_sinks(1, 0))
    sinks = list(range(1, N + 2))

    def world(n):
        return dict(src_id=1, end_time=10.0, sink_ids=sinks[:n],
                    edge_list=[(2, s) for s in sinks[:n]] + [(1, s) for s in sinks[:n:3]] + [(3, sinks[n - 1])],
                    other_sources=[("Poisson2", {"src_id": 2, "seed": 1, "rate": 1.0}),
                                   ("Poisson2", {"src_id": 3, "seed": 1, "rate": 1.0})])
    Ks = (1, 2, 3, 4)
    log = ([0.5, 1.0, 2.5, 4.0, 7.0], [3, 1, 2, 2, 1])
    so = world(N)
    g = _graph(engine, so)
    out = _raw(torch, L, g, *_pack([log], 9, g), Ks)
    ref = FR.play(log[0], log[1], so["edge_list"], so["sink_ids"], 1, so["end_time"], Ks)
    assert ref["status"] == 0
    _assert_replica(out, 0, ref, "limit")
    so2 = world(N + 1)
    g2 = _graph(engine, so2)
    _raw(torch, L, g2, *_pack([log], 9, g2), Ks, expect=L.RQ_EUNSUPPORTED)
    out2 = _raw(torch, L, g2, *_pack([log], 9, g2), Ks, rows=False)
    ref2 = FR.play(log[0], log[1], so2["edge_list"], so2["sink_ids"], 1, so2["end_time"], Ks)
    _assert_replica(out2, 0, ref2, "limit + 1 without rows", rows=False)


# ------------------------------------------------- 8. Followers helpers, run_followers
def test_loss_and_u_int_helpers():
    torch, _O, L, engine, graphs = _ctx()
    so = graphs.mixed()
    g = _graph(engine, so)
    R = 6
    res = g.run("opt", q=so["q"], s=so["s"], n_rep=R, ctrl_seed=5, world_seed=6, randomize=True, Ks=(1,),
                event_log=True)
    fl = res.followers()
    assert (fl.status == 0).all() and fl.rows is None
    ri, rs = fl.rank_int.cpu().numpy(), fl.rank_sq_int.cpu().numpy()
    ns = len(fl.sink_ids)
    arr = np.asarray([0.5, 2.0, 0.0, 1.25])
    as_dict = {10: 0.5, 11: 2.0, 13: 1.25}          # sink 12 is not named: weight 0
    q = 3.0
    for s, vec in ((0.75, np.full(ns, 0.75)), (arr, arr), (as_dict, arr)):
        loss, u = fl.loss(s).cpu().numpy(), fl.u_int(s, q).cpu().numpy()
        assert loss.shape == u.shape == (R,)
        w = np.sqrt(vec / q)
        for i in range(R):
            e_loss = 0.5 * math.fsum(float(vec[x] * rs[i, x]) for x in range(ns))
            e_u = math.fsum(float(w[x] * ri[i, x]) for x in range(ns))
            assert abs(loss[i] - e_loss) <= (ns + 8) * FR.ULP * abs(e_loss), (i, loss[i], e_loss)
            assert abs(u[i] - e_u) <= (ns + 8) * FR.ULP * abs(e_u), (i, u[i], e_u)
    with pytest.raises(ValueError):
        fl.loss(np.ones(ns + 1))


def test_run_followers_matches_one_batch_and_any_chunking():
    torch, _O, L, engine, graphs = _ctx()
    import pandas as pd
    from redqueen_amd import batch
    from redqueen_amd.opt_model import SimOpts
    so = SimOpts(**graphs.readme())
    seeds = np.arange(300, 340)
    Ks = (1, 2)
    f1 = batch.run_followers(so, seeds, Ks=Ks, chunk_replicas=40)
    f2 = batch.run_followers(so, seeds, Ks=Ks, chunk_replicas=13)
    g = batch.compiled_graph(so)
    st = torch.as_tensor(seeds)
    res = g.run("opt", q=float(so.q), s=so.s, n_rep=40, ctrl_seed=st, world_seed=st, randomize=True,
                Ks=Ks, event_log=True)
    fl = res.followers(Ks=Ks, rows=True)
    exp = batch.followers_frame(fl.sink_ids, fl.Ks, fl.vals.cpu().numpy(), fl.rows.cpu().numpy(),
                                fl.status.cpu().numpy())
    pd.testing.assert_frame_equal(f1, exp, check_exact=True)
    pd.testing.assert_frame_equal(f2, exp, check_exact=True)
    assert np.array_equal(f1.sink_id.values, [1, 2, 3]) and (f1.n == 40).all() and (f1.n_flagged == 0).all()
    assert (f1.own_rows.values[[0, 2]] > 0).all() and f1.own_rows.values[1] == 0   # source 1 -> sinks 1, 3


# --------------------------------------------------------------- 9. the utils facade
def test_utils_losses_against_the_reference(golden):
    torch, _O, L, engine, graphs = _ctx()
    import pandas as pd
    from redqueen_amd import utils
    f = golden("followers.npz")
    u_const = float(f["u_const"])
    for name in (str(n) for n in f["names"]):
        so = _fixture_world(f, name)
        t, src, sink, eid = TR.frame_of(f[name + "_t"], f[name + "_src"], so["edge_list"])
        df = pd.DataFrame({"event_id": 100 + eid, "src_id": src, "t": t, "sink_id": sink})
        opts = types.SimpleNamespace(src_id=so["src_id"], end_time=so["end_time"], q=so["q"],
                                     s=f[name + "_svec"], sink_ids=sorted(so["sink_ids"]))
        r2 = utils.int_r_2_true(df, opts)
        assert isinstance(r2, np.float64)
        assert abs(r2 - float(f[name + "_r2true"])) <= 1e-12 * abs(float(f[name + "_r2true"])), name
        if (name + "_loss_opt") not in f.files:
            # a sink without a row is no pivot column: KeyError, as the reference
            with pytest.raises(KeyError):
                utils.calc_loss_opt(df, opts)
            with pytest.raises(KeyError):
                utils.calc_loss_poisson(df, u_const, sim_opts=opts)
            continue
        index = pd.Index(f[name + "_index"], name="t")
        for got, key in ((utils.calc_loss_opt(df, opts), "_loss_opt"),
                         (utils.calc_loss_poisson(df, u_const, sim_opts=opts), "_loss_pois")):
            exp = pd.Series(data=f[name + key], index=index)
            assert isinstance(got, pd.Series) and got.dtype == exp.dtype == np.float64, (name, key)
            assert got.index.equals(exp.index) and got.index.dtype == exp.index.dtype, (name, key)
            assert got.index.name == exp.index.name and got.name == exp.name, (name, key)
            assert np.array_equal(np.isnan(got.values), np.isnan(exp.values)), (name, key)
            m = ~np.isnan(exp.values)
            assert m.any() and np.all(np.abs(got.values[m] - exp.values[m]) <= 1e-12 * np.abs(exp.values[m])), \
                (name, key)
        # explicit arguments instead of sim_opts
        lp = utils.calc_loss_poisson(df, u_const, src_id=opts.src_id, end_time=opts.end_time, q=opts.q,
                                     s=opts.s, follower_ids=opts.sink_ids)
        assert lp.equals(utils.calc_loss_poisson(df, u_const, sim_opts=opts))

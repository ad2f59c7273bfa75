"""CPU side of rq_log_rank_hist (no GPU): the host checker tests/rank_hist_ref.py pinned
to the reference (tests/golden/rank_hist.npz: the reference's own rank_of_src_in_df
tables counted per rank value and binned per time bin), the entry's export and first
validation, batch.rank_hist_frame and the RankHist accessors on CPU tensors."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from redqueen_amd import _lib as L
from tests import rank_hist_ref as RH


def fixture_runs(g):
    for name in (str(n) for n in g["names"]):
        src_id, end = int(g[name + "_world"][0]), float(g[name + "_world"][1])
        edge_list = [tuple(int(v) for v in e) for e in g[name + "_edges"]]
        streams = [src_id] + [int(s) for s in g[name + "_srcs"]]
        yield name, src_id, end, edge_list, streams


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def test_bin_table_matches_reference_tables_bit_for_bit(golden):
    g = golden("rank_hist.npz")
    n = 0
    for name, src_id, end, edge_list, _streams in fixture_runs(g):
        t, src, sink, _eid = RH.frame_of(g[name + "_t"], g[name + "_src"], edge_list)
        tab, idx, _sinks = O.rank_table(t, src, sink, src_id, True)
        rows, S, top = (int(v) for v in g[name + "_rows"])
        assert tab.shape == (rows, S) and int(np.nanmax(tab)) == top, name
        for k in (0, 1):
            edges = g["%s_bins%d" % (name, k)]
            for nr in (int(v) for v in g["ranks"]):
                exp = g["%s_hist%d_%d" % (name, k, nr)]
                got = RH.bin_table(tab, idx, end, edges, nr)
                assert exp.shape == (edges.size - 1, nr + 1)
                assert _same_bits(got, exp), (name, k, nr)
                n += 1
    assert n >= 32


def test_replay_is_within_the_bound_of_the_fixture(golden):
    """(n_rows + 8) * 2**-52 relative, exactly 0.0 where the fixture is 0: the bound
    DESIGN section 16 derives for any summation order of a bin's non-negative terms."""
    g = golden("rank_hist.npz")
    worst = 0.0
    for name, src_id, end, edge_list, streams in fixture_runs(g):
        ptr, col = RH.csr_of(streams, g[name + "_sinks"], edge_list)
        ev_src = np.asarray([streams.index(int(s)) for s in g[name + "_src"]])
        row_t, cnt, S, top, status = RH.walk(g[name + "_t"], ev_src, ptr, col, 0)
        rows = int(g[name + "_rows"][0])
        assert status == 0 and [len(row_t), S, top] == [int(v) for v in g[name + "_rows"]], name
        assert (cnt.sum(1) <= S).all() and cnt[-1].sum() == S and (cnt >= 0).all()
        for k in (0, 1):
            edges = g["%s_bins%d" % (name, k)]
            for nr in (int(v) for v in g["ranks"]):
                exp = g["%s_hist%d_%d" % (name, k, nr)]
                got = RH.integrate(row_t, cnt, S, status, end, edges, nr)
                err = np.abs(got - exp) / np.maximum(RH.ULP * np.abs(exp), 1e-300)
                worst = max(worst, float(err.max()))
                assert (got[exp == 0.0] == 0.0).all(), (name, k, nr)
                assert RH.close(got, exp, rows), (name, k, nr, float(err.max()))
                if name in ("rd_ties", "late_sink") or nr == 3:
                    # the accumulate along the time axis is the literal loop acc = acc + cnt * len
                    lit, S2, top2, st2 = RH.replay(g[name + "_t"], ev_src, ptr, col, 0, end, edges, nr,
                                                   literal=True)
                    assert _same_bits(lit, got) and (S2, top2, st2) == (S, top, 0), (name, k, nr)
    print("replay against the fixture: largest error %.3g ulp" % worst)


def test_fixture_covers_the_stated_cases(golden):
    g = golden("rank_hist.npz")
    small = 0
    for name in (str(n) for n in g["names"]):
        top = int(g[name + "_rows"][2])
        for k in (0, 1):
            for nr in (1, 3):
                assert g["%s_hist%d_%d" % (name, k, nr)][:, nr].sum() > 0, (name, k, nr)
            tail = g["%s_hist%d_255" % (name, k)][:, 255]
            if top < 255:
                assert (tail == 0.0).all(), (name, k)
                small += 1
            else:   # README's sink 2 never gets an own row: its rank counts source 2's posts
                assert tail.sum() > 0 and name.startswith("readme"), (name, k)
    assert small >= 4
    # equal times on disjoint sinks, the controlled source among them
    t, src = g["rd_ties_t"], g["rd_ties_src"]
    fans = {}
    for s, x in g["rd_ties_edges"]:
        fans.setdefault(int(s), set()).add(int(x))
    eq = np.flatnonzero(t[1:] == t[:-1])
    assert eq.size >= 2
    for k in eq:
        assert not (fans[int(src[k])] & fans[int(src[k + 1])])
    assert int(g["rd_ties_world"][0]) in {int(src[k]) for k in eq} | {int(src[k + 1]) for k in eq}
    assert g["rd_ties_rows"][0] < t.size
    # the late sink: before its first row only one of S = 2 sinks is seen
    lt, ls = g["late_sink_t"], g["late_sink_src"]
    e = g["late_sink_bins0"]
    assert lt[ls == 3].min() > e[2]
    h = g["late_sink_hist0_64"]
    assert np.all(h[:6].sum(1) <= 0.5 * np.diff(e)[:6] * (1 + 1e-12)) and h[-1].sum() > 0.5 * (e[-1] - e[-2])


def test_entry_is_exported_and_validates_before_hip():
    lib = L.lib()
    assert "rq_log_rank_hist" in L.EXPORTED and hasattr(lib, "rq_log_rank_hist")
    assert L.RANK_HIST_MAX_RANKS == 255
    assert lib.rq_log_rank_hist(None, None, None, None, 1, 1, None, 1, 1, None, None, None, None,
                                None) == L.RQ_EINVAL
    buf = (C.c_double * 64)()
    p = C.addressof(buf)   # never dereferenced: the arguments are refused first

    def call(h=p, ev_t=p, ev_src=p, counts=p, n_rep=1, cap=1, edges=p, nb=1, nr=1, hist=p, seen=p, mx=p,
             sta=p):
        return lib.rq_log_rank_hist(h, ev_t, ev_src, counts, n_rep, cap, edges, nb, nr, hist, seen, mx,
                                    sta, None)
    for kw in (dict(nr=0), dict(nr=256), dict(nr=-1), dict(nb=0), dict(n_rep=-1), dict(cap=-1), dict(h=None),
               dict(ev_t=None), dict(ev_src=None), dict(counts=None), dict(edges=None), dict(hist=None),
               dict(seen=None), dict(mx=None), dict(sta=None)):
        assert call(**kw) == L.RQ_EINVAL, kw
    assert all(v == 0.0 for v in buf)


def test_rank_hist_frame_hand_made():
    import pandas as pd
    from redqueen_amd import batch
    edges = np.asarray([0.0, 1.0, 4.0])
    ranks = 2
    hist = np.asarray([[[1.0, 0.0, 0.0], [0.5, 1.5, 1.0]],
                       [[np.nan] * 3, [np.nan] * 3],
                       [[0.0, 1.0, 0.0], [1.5, 0.5, 1.0]],
                       [[np.nan] * 3, [np.nan] * 3],
                       [[0.5, 0.5, 0.0], [1.0, 1.0, 1.0]]])
    status = np.asarray([0, L.ST_TIE, 0, L.ST_EMPTY, 0])
    f = batch.rank_hist_frame(edges, ranks, hist, status)
    assert list(f.columns) == ["t_lo", "t_hi", "rank", "tail", "share", "share_se", "n", "n_flagged"]
    assert len(f) == 6 and (f.n == 3).all() and (f.n_flagged == 2).all()
    assert list(f["rank"]) == [0, 1, 2, 0, 1, 2] and list(f["tail"]) == [False, False, True] * 2
    assert list(f.t_lo) == [0.0] * 3 + [1.0] * 3 and list(f.t_hi) == [1.0] * 3 + [4.0] * 3
    assert np.array_equal(f.share.values, [0.5, 0.5, 0.0, 1.0, 1.0, 1.0])
    ok = hist[[0, 2, 4]].reshape(3, 6)
    assert np.allclose(f.share_se.values, ok.std(0, ddof=1) / np.sqrt(3.0), rtol=1e-15, atol=0.0)
    # a frame of arrays gathered from any split of the replica axis is the same frame
    for cut in (1, 2, 4):
        parts = [(hist[:cut], status[:cut]), (hist[cut:], status[cut:])]
        f2 = batch.rank_hist_frame(edges, ranks, np.concatenate([h for h, _ in parts]),
                                   np.concatenate([s for _, s in parts]))
        pd.testing.assert_frame_equal(f, f2, check_exact=True)
    # one clean replica: no standard error; none: no mean either
    one = batch.rank_hist_frame(edges, ranks, hist[:2], status[:2])
    assert (one.n == 1).all() and np.array_equal(one.share.values, hist[0].reshape(-1)) and one.share_se.isna().all()
    none = batch.rank_hist_frame(edges, ranks, hist[1:2], status[1:2])
    assert (none.n == 0).all() and none.share.isna().all() and (none.n_flagged == 1).all()


def test_rank_hist_accessors_on_cpu_tensors():
    import torch
    from redqueen_amd.engine import RankHist
    nan = float("nan")
    hist = torch.tensor([[[1.0, 2.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.5, 0.5, 3.0]],
                         [[nan] * 4, [nan] * 4, [nan] * 4]], dtype=torch.float64)
    rh = RankHist(np.asarray([0.0, 1.0, 2.0, 3.0]), 3, hist, torch.tensor([4, 2], dtype=torch.int32),
                  torch.tensor([7, 1], dtype=torch.int32), torch.tensor([0, L.ST_TIE], dtype=torch.int32))
    assert rh.ranks == 3 and rh.hist.shape == (2, 3, 4)
    assert rh.top_k(1)[0].tolist() == [1.0, 0.0, 0.0]
    assert rh.top_k(2)[0].tolist() == [3.0, 0.0, 0.5] and rh.top_k(3)[0].tolist() == [3.0, 0.0, 1.0]
    assert torch.isnan(rh.top_k(2)[1]).all()
    for k in (0, 4, -1):
        with pytest.raises(ValueError):
            rh.top_k(k)
    assert rh.tail[0].tolist() == [1.0, 0.0, 3.0]
    c = rh.cdf()
    assert c.shape == (2, 3, 4)
    assert c[0, 0].tolist() == [0.25, 0.75, 0.75, 1.0] and c[0, 2].tolist() == [0.0, 0.125, 0.25, 1.0]
    assert torch.isnan(c[0, 1]).all() and torch.isnan(c[1]).all()      # an all-zero bin, a flagged replica
    assert rh.quantile(0.5)[0].tolist() == [1, -1, 3]                  # 3 = ranks: in the tail
    assert rh.quantile(0.25)[0].tolist() == [0, -1, 2]
    assert rh.quantile(1.0)[0].tolist() == [3, -1, 3]
    assert rh.quantile(0.5)[1].tolist() == [-1, -1, -1] and rh.quantile(0.5).dtype == torch.int64
    for p in (0.0, 1.5, -0.1):
        with pytest.raises(ValueError):
            rh.quantile(p)

"""The log reader of the three log kernels (log_walk, rq_log_walk.h, and its inline copy
in rq_timeline.hip) at its chunk boundary: 64 events per chunk, the next chunk and the next
event's first 64 sink columns fetched ahead.  Hand-made logs of 0, 1, 63, 64, 65, 128 and 129 events on the 140-sink
degrees world (out-degrees 1, 63, 64, 65 and 129) go through rq_log_timeline,
rq_log_followers and rq_log_rank_hist by the raw ABI.

The logs.  Event k plays at t_k = (k + 1) / 32; the narrow sources 2, 3, 4 take turns, and
the 129-wide own row (source 1) and the 65-wide wall row (source 5) stand at the event
indices 0, 63 and 64 -- own / wall / own in the ``own`` logs, wall / own / wall in the
``wall`` logs -- so the columns fetched across the chunk switch are those of a row of
several rounds.  The logs of 64 and 65 events end at event 63 and 64.  ``tie`` gives the
events 63 and 64 (sources 5 and 1, with sinks in common) one time: RQ_ST_TIE.
``equal_disjoint`` does so with sources 2 and 3, which share no sink: status 0.  Two time
bin edges lie on the times of the events 63 and 64.

The checks.  Followers and rank histogram: followers_ref.play and rank_hist_ref.replay (walk
+ integrate) bit for bit.  Timeline: timeline_ref.tol, (rows + 8) ulp (derived there);
posts and wall rows equal.  Before the first launch the host checkers must agree on every
log: play against followers_ref.column_sums and replay against rank_hist_ref.bin_table over
the oracle's rank table (tol, (rows + 8) ulp); the sum of bin_table's first K cells
against timeline_ref's top_K ((rows + K + 8) ulp: K more roundings for K cells); and the
mean over the S seen sinks of play's top_K integrals against the sum of timeline_ref's
bins -- each side a sum of non-negative terms, <= S * rows and <= rows of them, of <= 4
roundings each, then one division or none: 2 * (S * rows + 8) ulp.  A TIE / EMPTY log has
no table: its outputs are NaN in every checker and on the GPU, its integer outputs equal.

Every output of every kernel must keep its bits when events of the stream indices -1 and
n_str (no row) are put at the positions 0, 63 and 64 of the log, and when ev_cap goes from
n + 77 to n + 1."""
import functools

import numpy as np
import pytest

from tests import followers_ref as FR
from tests import rank_hist_ref as RH
from tests import timeline_ref as TR
from tests import loghelp as LH

pytestmark = pytest.mark.gpu
KS = (1, 3)
NRS = (3, 100, 255)                           # 1, 2 and 4 cells per lane
EDGES = [0.0, 0.75, 2.0, 2.03125, 4.5, 6.0]   # 2.0, 2.03125: the times of the events 63, 64
SIZES = (0, 1, 63, 64, 65, 128, 129)
WIDE_AT = (0, 63, 64)


def _log(n, wide):
    """n events; ``wide``: the sources of the events 0, 63 and 64."""
    t = (np.arange(n) + 1.0) / 32.0
    s = np.asarray([(2, 3, 4)[k % 3] for k in range(n)], dtype=np.int64)
    for k, w in zip(WIDE_AT, wide):
        if k < n:
            s[k] = w
    return t, s


def _logs():
    logs = {"n0": _log(0, ())}
    for n in SIZES[1:]:
        logs["n%d_own" % n] = _log(n, (1, 5, 1))
        logs["n%d_wall" % n] = _log(n, (5, 1, 5))
    t, s = _log(65, (1, 5, 1))
    t[64] = t[63]
    logs["tie"] = (t, s)
    t, s = _log(128, (1, 2, 3))
    t[64] = t[63]
    logs["equal_disjoint"] = (t, s)
    return logs


LOGS = _logs()


def _reference(O, so, g, t, s, idx):
    """What the host checkers say of one log (idx: its stream indices), after they have
    been held against each other."""
    end, sinks = so["end_time"], np.sort(np.asarray(so["sink_ids"]))
    fl = FR.play(t, s, so["edge_list"], so["sink_ids"], so["src_id"], end, KS)
    ptr, col = RH.csr_of(g.stream_src_ids, g.sink_ids, g._edges)
    row_t, cnt, S, top, status = RH.walk(t, idx, ptr, col, g.ctrl_idx)
    hists = {nr: RH.integrate(row_t, cnt, S, status, end, EDGES, nr) for nr in NRS}
    tt, ss, xx, eid = TR.frame_of(t, s, so["edge_list"])
    ref = dict(fl=fl, S=S, top=top, status=status, hists=hists, rows=len(row_t), tl=None,
               posts=TR.posts(tt, ss, so["src_id"], EDGES, eid),
               wall=TR.wall_posts(tt, ss, xx, so["src_id"], EDGES, so["sink_ids"]))
    assert fl["status"] == status and fl["n_rows"] == len(row_t)
    assert S == int(np.count_nonzero(~np.isnan(fl["first_t"])))
    if status != 0:
        assert np.isnan(fl["vals"]).all() and all(np.isnan(h).all() for h in hists.values())
        return ref
    tab, index, cols = O.rank_table(tt, ss, xx, so["src_id"], True)
    rows = tab.shape[0]
    assert rows == len(row_t) and tab.shape[1] == S
    ref["tl"] = tl = TR.bin_table(tab, index, end, EDGES, KS)
    at = np.searchsorted(sinks, cols)
    vals, first = FR.column_sums(tab, index, end, KS)
    assert FR.close(fl["vals"][at], vals, rows) and FR.same_bits(fl["first_t"][at], first)
    assert (np.delete(fl["vals"], at, axis=0) == 0.0).all()
    for nr, h in hists.items():
        table = RH.bin_table(tab, index, end, EDGES, nr)
        assert RH.close(h, table, rows), nr
        for q, K in enumerate(KS):
            if K <= nr:
                got = table[:, :K].sum(-1)
                assert (np.abs(got - tl[:, q]) <= (rows + K + 8) * RH.ULP * tl[:, q]).all(), (nr, K)
    for q in range(len(KS)):
        mean, whole = fl["vals"][:, q].sum() / S, tl[:, q].sum()
        assert abs(mean - whole) <= 2 * (S * rows + 8) * TR.ULP * whole, q
    return ref


def _row(t, idx, cap):
    """(ev_t, ev_src, counts) of one log of stream indices, as loghelp.pack lays it out."""
    ev_t = np.full((1, cap), np.nan)
    ev_src = np.full((1, cap), -1, dtype=np.int32)
    counts = np.full((1, 4), -5, dtype=np.int64)
    ev_t[0, :len(t)], ev_src[0, :len(t)], counts[0, 2] = t, idx, len(t)
    return ev_t, ev_src, counts


def _with_empty_rows(t, idx, n_str):
    """The log with events of no row at its positions 0, 63 and 64, as far as it reaches;
    each at the time of the event it stands before (of the last one at the end)."""
    t, idx = list(t), list(idx)
    for pos, bad in zip(WIDE_AT, (-1, n_str, -1)):
        if pos <= len(t):
            t.insert(pos, t[pos] if pos < len(t) else (t[-1] if t else 0.5))
            idx.insert(pos, bad)
    return t, idx


def _play(torch, L, g, packed):
    """Every output of the three kernels on one packed log."""
    out = {}
    out["tl_metrics"], out["tl_posts"], out["tl_status"], out["tl_wall"] = LH.raw_timeline(
        torch, L, g, *packed, EDGES, KS, wall=True)
    for k, v in LH.raw_followers(torch, L, g, *packed, KS, rows=True).items():
        out["fl_" + k] = v
    for nr in NRS:
        for k, v in zip(("hist", "seen", "max", "status"), LH.raw_rank_hist(torch, L, g, *packed, EDGES, nr)):
            out["rh%d_%s" % (nr, k)] = v
    return out


def _same_outputs(a, b):
    return a.keys() == b.keys() and all(
        a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in a)


@functools.lru_cache(maxsize=None)
def _world():
    torch, O, L, engine, graphs = LH.ctx()
    so = LH.degrees_world()
    return torch, O, L, so, LH.graph(engine, so)


@pytest.mark.parametrize("name", list(LOGS))
def test_log_at_the_chunk_boundary(name):
    torch, O, L, so, g = _world()
    t, s = LOGS[name]
    n = len(t)
    packed = LH.pack([(t, s)], n + 77, g)
    idx = packed[1][0, :n]
    ref = _reference(O, so, g, t, s, idx)
    assert ref["status"] == {"tie": L.ST_TIE, "n0": L.ST_EMPTY}.get(name, 0)

    out = _play(torch, L, g, packed)
    # timeline
    assert out["tl_status"][0] == ref["status"]
    if ref["status"] == 0:
        err = np.abs(out["tl_metrics"][0] - ref["tl"]) / np.maximum(TR.ULP * np.abs(ref["tl"]), 1e-300)
        print(name, "timeline max |got - exp| = %.3g ulp over %d rows" % (float(err.max()), ref["rows"]))
        assert TR.close(out["tl_metrics"][0], ref["tl"], ref["rows"])
    else:
        assert np.isnan(out["tl_metrics"]).all()
    assert np.array_equal(out["tl_posts"][0], ref["posts"]) and np.array_equal(out["tl_wall"][0], ref["wall"])
    # followers
    fl = ref["fl"]
    assert out["fl_status"][0] == fl["status"]
    assert FR.same_bits(out["fl_vals"][0], fl["vals"]) and FR.same_bits(out["fl_r2_true"][0], fl["r2_true"])
    assert FR.same_bits(out["fl_first_t"][0], fl["first_t"]) and np.array_equal(out["fl_rows"][0], fl["rows"])
    # rank histogram
    for nr in NRS:
        got = tuple(int(out["rh%d_%s" % (nr, k)][0]) for k in ("seen", "max", "status"))
        assert got == (ref["S"], ref["top"], ref["status"]), nr
        assert LH.same_bits(out["rh%d_hist" % nr][0], ref["hists"][nr]), nr
    # without the wall rows and the row counts: the same bits
    met, pst, sta, _w = LH.raw_timeline(torch, L, g, *packed, EDGES, KS, wall=False)
    assert met.tobytes() == out["tl_metrics"].tobytes() and np.array_equal(pst, out["tl_posts"])
    bare = LH.raw_followers(torch, L, g, *packed, KS, rows=False)
    assert all(bare[k].tobytes() == out["fl_" + k].tobytes() for k in ("vals", "first_t", "r2_true", "status"))

    # rows that no event has, at the positions 0, 63 and 64
    t2, idx2 = _with_empty_rows(t, idx, len(g.stream_src_ids))
    assert len(t2) == n + sum(p <= n + k for k, p in enumerate(WIDE_AT))
    assert _same_outputs(_play(torch, L, g, _row(t2, idx2, len(t2) + 77)), out)
    # a row that the log all but fills
    assert _same_outputs(_play(torch, L, g, LH.pack([(t, s)], n + 1, g)), out)

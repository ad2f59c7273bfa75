"""Host checker for rq_log_timeline (tests/test_timeline_cpu.py, tests/test_gpu_timeline.py).

Plain numpy over a replica's dataframe columns (t, src, sink): the pivot table comes
from ``oracle.rank_table(..., fill=True)`` (pinned to the reference's
rank_of_src_in_df), every pivot row holds from its t to the next row's t (the last to
end_time), and a bin's value is the exactly rounded sum (math.fsum) of
integrand x overlap over the rows that meet the bin.  Integrands per row:
(#cells <= K-1) / S for every K, m = nanmean(row), m * m.
Counts use the half-open bin rule edges[b] <= t < edges[b+1]
(np.searchsorted(edges, t, side="right") - 1)."""
import math

import numpy as np

ULP = 2.0 ** -52


def bin_table(table, index, end_time, edges, Ks):
    """[n_bins][len(Ks) + 2] from a filled rank table (rows = unique t, columns = the
    df's sinks; NaN = no row of that sink yet)."""
    table = np.asarray(table, dtype=np.float64)
    index = np.asarray(index, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    n_t, S = table.shape
    nxt = np.append(index[1:], float(end_time))
    seen = ~np.isnan(table)
    F = np.empty((n_t, len(Ks) + 2))
    for q, K in enumerate(Ks):
        F[:, q] = np.count_nonzero(seen & (np.where(seen, table, 0.0) <= K - 1), axis=1) / float(S)
    for k in range(n_t):
        F[k, len(Ks)] = np.nanmean(table[k])
    F[:, len(Ks) + 1] = F[:, len(Ks)] * F[:, len(Ks)]
    out = np.zeros((edges.size - 1, F.shape[1]))
    for b in range(edges.size - 1):
        e0, e1 = float(edges[b]), float(edges[b + 1])
        # rows that can meet [e0, e1): they end after e0 and start before e1
        k0 = int(np.searchsorted(nxt, e0, side="right"))
        k1 = int(np.searchsorted(index, e1, side="left"))
        if k1 <= k0:
            continue
        ov = np.minimum(nxt[k0:k1], e1) - np.maximum(index[k0:k1], e0)
        keep = ov > 0
        if not keep.any():
            continue
        for q in range(F.shape[1]):
            out[b, q] = math.fsum((F[k0:k1, q][keep] * ov[keep]).tolist())
    return out


def bin_of(t, edges):
    """Bin of every t (edges[b] <= t < edges[b+1]); -1 outside the edges."""
    edges = np.asarray(edges, dtype=np.float64)
    b = np.searchsorted(edges, np.asarray(t, dtype=np.float64), side="right") - 1
    return np.where((b >= 0) & (b < edges.size - 1), b, -1)


def metrics(O, t, src, sink, src_id, end_time, edges, Ks):
    """The per-bin metrics of one dataframe, and its pivot row count."""
    tab, idx, _ = O.rank_table(t, src, sink, src_id, True)
    return bin_table(tab, idx, end_time, edges, Ks), tab.shape[0]


def posts(t, src, src_id, edges, event_id=None):
    """[n_bins][2] (own, other) events of a dataframe: rows of one event share
    event_id (default: a new event wherever (t, src) changes)."""
    t, src = np.asarray(t, dtype=np.float64), np.asarray(src, dtype=np.int64)
    out = np.zeros((len(edges) - 1, 2), dtype=np.int64)
    if t.size == 0:
        return out
    if event_id is None:
        first = np.ones(t.size, dtype=bool)
        first[1:] = (t[1:] != t[:-1]) | (src[1:] != src[:-1])
    else:
        e = np.asarray(event_id)
        first = np.ones(t.size, dtype=bool)
        first[1:] = e[1:] != e[:-1]
    b = bin_of(t[first], edges)
    other = (src[first] != src_id).astype(np.int64)
    ok = b >= 0
    np.add.at(out, (b[ok], other[ok]), 1)
    return out


def wall_posts(t, src, sink, src_id, edges, sink_ids):
    """[len(sink_ids)][n_bins] rows of every sink (ascending sink id) from the other
    sources."""
    cols = np.sort(np.asarray(sink_ids, dtype=np.int64))
    out = np.zeros((cols.size, len(edges) - 1), dtype=np.int32)
    t, src = np.asarray(t, dtype=np.float64), np.asarray(src, dtype=np.int64)
    b = bin_of(t, edges)
    ok = (b >= 0) & (src != src_id)
    np.add.at(out, (np.searchsorted(cols, np.asarray(sink, dtype=np.int64)[ok]), b[ok]), 1)
    return out


def tol(n_rows, exp):
    """|got - exp| allowed: a bin is a sum of <= n_rows non-negative terms of <= 4
    roundings each, so any summation order stays within (n_rows + 8) ulp of it."""
    return (n_rows + 8) * ULP * np.abs(exp)


def close(got, exp, n_rows):
    """got within tol of exp, and exactly 0.0 wherever exp is 0."""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    return got.shape == exp.shape and bool(np.all(np.abs(got - exp) <= tol(n_rows, exp)))


def frame_of(ev_t, ev_src, edge_list):
    """Dataframe columns (t, src, sink, event number) of an event list: one row per
    (event, sink of an edge of its source), edge-list order within an event; events of
    a source without edges give no row."""
    fans = {}
    for s, x in edge_list:
        fans.setdefault(int(s), []).append(int(x))
    t, src, sink, eid = [], [], [], []
    for k, (tk, sk) in enumerate(zip(ev_t, ev_src)):
        for x in fans.get(int(sk), ()):
            t.append(float(tk))
            src.append(int(sk))
            sink.append(x)
            eid.append(k)
    return (np.asarray(t, dtype=np.float64), np.asarray(src, dtype=np.int64),
            np.asarray(sink, dtype=np.int64), np.asarray(eid, dtype=np.int64))

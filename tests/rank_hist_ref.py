"""Host checker for rq_log_rank_hist (tests/test_rank_hist_cpu.py, tests/test_gpu_rank_hist.py).

Two routes to hist[b][rho], the seen sink-time at rank rho (last cell: rank >= n_ranks)
per time bin over S seen sinks:

``replay``     restates the kernel in the contract's order (include/rq.h): events in log
               order, rank_x = 0 on an own row, + 1 on any other (1 for an unseen sink),
               the integer counts cnt_rho after the last event of every time, and per
               (bin, cell) the sequential sum acc = acc + float(cnt) * len over the rows
               in time order, every product rounded, non-positive overlaps skipped, one
               division by S.  The GPU must give the same bits.  ``walk`` + ``integrate``
               are its two halves, so a test walks a log once for many (edges, n_ranks).
``bin_table``  works on a filled rank table (oracle.rank_table(fill=True) or the
               reference's own rank_of_src_in_df): count(row == rho), count(row >=
               n_ranks), math.fsum over the overlaps, then / S -- timeline_ref.bin_table's
               scheme.  Any summation order stays within timeline_ref.tol of it.
"""
import math

import numpy as np

try:
    from tests.timeline_ref import ULP, close, frame_of, tol  # noqa: F401  (re-exported)
except ImportError:   # the fixture generator runs with tests/ itself on the path
    from timeline_ref import ULP, close, frame_of, tol  # noqa: F401

FULL = 256          # walk() keeps the cells 0..FULL-1 and, last, rank >= FULL
ST_TIE, ST_EMPTY = 4, 8


def csr_of(stream_src_ids, sink_ids, edge_list):
    """(csr_ptr, csr_col) of a world: stream k's sinks as columns in ascending sink-id
    order; a duplicate edge stays a duplicate column."""
    cols = {int(x): i for i, x in enumerate(sorted(int(v) for v in sink_ids))}
    fans = {}
    for s, x in edge_list:
        fans.setdefault(int(s), []).append(cols[int(x)])
    ptr, col = [0], []
    for s in stream_src_ids:
        col.extend(fans.get(int(s), ()))
        ptr.append(len(col))
    return np.asarray(ptr, dtype=np.int64), np.asarray(col, dtype=np.int64)


def walk(ev_t, ev_src, csr_ptr, csr_col, ctrl):
    """The pivot rows of one log (ev_src: stream indices; one outside the graph gives no
    row): row_t [n_rows], cnt [n_rows][FULL + 1] after the last event of each row_t, S,
    max_rank and status."""
    n_str = len(csr_ptr) - 1
    n_sinks = int(csr_col.max()) + 1 if len(csr_col) else 0
    rank = np.full(n_sinks, -1, dtype=np.int64)
    grp = np.full(n_sinks, -1, dtype=np.int64)   # the time group of the sink's last row
    cnt = np.zeros(FULL + 1, dtype=np.int64)
    row_t, rows = [], []
    tie, max_rank, g = False, -1, 0
    for t, j in zip(np.asarray(ev_t, dtype=np.float64), np.asarray(ev_src, dtype=np.int64)):
        if not 0 <= j < n_str or csr_ptr[j] == csr_ptr[j + 1]:
            continue
        t = float(t)
        if row_t and row_t[-1] == t:   # the row of this time is the one after its last event
            rows.pop()
            row_t.pop()
        else:
            g += 1
        for x in csr_col[csr_ptr[j]:csr_ptr[j + 1]]:
            rk = int(rank[x])
            if grp[x] == g:
                tie = True
            nr = 0 if j == ctrl else (1 if rk < 0 else rk + 1)
            if rk >= 0:
                cnt[min(rk, FULL)] -= 1
            cnt[min(nr, FULL)] += 1
            rank[x], grp[x] = nr, g
            max_rank = max(max_rank, nr)
        row_t.append(t)
        rows.append(cnt.copy())
    S = int((rank >= 0).sum())
    status = ST_TIE if tie else (0 if row_t else ST_EMPTY)
    return (np.asarray(row_t, dtype=np.float64),
            np.asarray(rows, dtype=np.int64).reshape(len(rows), FULL + 1), S, max_rank, status)


def cells(cnt, n_ranks):
    """cnt [n_rows][FULL + 1] folded to n_ranks rank cells and the tail."""
    return np.concatenate([cnt[:, :n_ranks], cnt[:, n_ranks:].sum(1, keepdims=True)], axis=1)


def integrate(row_t, cnt, S, status, end_time, edges, n_ranks, literal=False):
    """hist [n_bins][n_ranks + 1] of walk()'s rows.  Per bin the rows' terms
    float(cnt) * len are added one after the other from the first on
    (np.add.accumulate along the time axis: out[k] = out[k-1] + term[k]); ``literal``
    spells the same loop out in Python floats."""
    edges = np.asarray(edges, dtype=np.float64)
    nb = edges.size - 1
    if status != 0:
        return np.full((nb, n_ranks + 1), np.nan)
    c = cells(cnt, n_ranks).astype(np.float64)
    nxt = np.append(row_t[1:], float(end_time))
    out = np.zeros((nb, n_ranks + 1))
    for b in range(nb):
        e0, e1 = float(edges[b]), float(edges[b + 1])
        lo, up = np.maximum(row_t, e0), np.minimum(nxt, e1)
        keep = up > lo
        if not keep.any():
            continue
        ln = up[keep] - lo[keep]
        if literal:
            for k, row in enumerate(c[keep]):
                for q in range(n_ranks + 1):
                    out[b, q] = float(out[b, q]) + float(row[q]) * float(ln[k])
        else:
            out[b] = np.add.accumulate(c[keep] * ln[:, None], axis=0)[-1]
    return out / float(S)


def replay(ev_t, ev_src, csr_ptr, csr_col, ctrl, end_time, edges, n_ranks, literal=False):
    """(hist, S, max_rank, status) of one log, in the kernel's order."""
    row_t, cnt, S, max_rank, status = walk(ev_t, ev_src, csr_ptr, csr_col, ctrl)
    return integrate(row_t, cnt, S, status, end_time, edges, n_ranks, literal), S, max_rank, status


def nvalid_int(row_t, cnt, end_time, edges):
    """[n_bins] exactly rounded integral of nvalid (the seen sinks) over every bin."""
    edges = np.asarray(edges, dtype=np.float64)
    nv = cnt.sum(1).astype(np.float64)
    nxt = np.append(row_t[1:], float(end_time))
    out = np.zeros(edges.size - 1)
    for b in range(edges.size - 1):
        ov = np.minimum(nxt, edges[b + 1]) - np.maximum(row_t, edges[b])
        keep = ov > 0
        out[b] = math.fsum((nv[keep] * ov[keep]).tolist())
    return out


def bin_table(table, index, end_time, edges, n_ranks):
    """hist [n_bins][n_ranks + 1] from a filled rank table (rows = unique t, columns =
    the df's sinks; NaN = no row of that sink yet)."""
    table = np.asarray(table, dtype=np.float64)
    index = np.asarray(index, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    n_t, S = table.shape
    nxt = np.append(index[1:], float(end_time))
    seen = ~np.isnan(table)
    tab = np.where(seen, table, -1.0)
    C = np.empty((n_t, n_ranks + 1))
    for q in range(n_ranks):
        C[:, q] = np.count_nonzero(tab == q, axis=1)
    C[:, n_ranks] = np.count_nonzero(tab >= n_ranks, axis=1)
    out = np.zeros((edges.size - 1, n_ranks + 1))
    for b in range(edges.size - 1):
        e0, e1 = float(edges[b]), float(edges[b + 1])
        k0 = int(np.searchsorted(nxt, e0, side="right"))
        k1 = int(np.searchsorted(index, e1, side="left"))
        if k1 <= k0:
            continue
        ov = np.minimum(nxt[k0:k1], e1) - np.maximum(index[k0:k1], e0)
        keep = ov > 0
        if not keep.any():
            continue
        terms = C[k0:k1][keep] * ov[keep][:, None]
        for q in np.flatnonzero(terms.any(axis=0)):
            out[b, q] = math.fsum(terms[:, q].tolist())
    return out / float(S)

"""Host checker for rq_log_metrics (tests/test_log_metrics_cpu.py, tests/test_gpu_log_metrics.py):
the entry's contract (include/rq.h) restated in plain Python on one replica's event list
(t, src_id per event) plus the graph's edge list.  No dataframe is built.

    play(t, src, edges, ctrl, end_time, Ks) -> dict(metrics [nK + 2], counts [4], status)

The pivot table: events play in log order; an event of source j gives every sink of j's
edges one row; the rank rule is an own row -> 0, any other row -> + 1 (1 on a sink without a
row so far).  A t-group is the maximal run of consecutive events with equal t; if one of
them has an edge the group makes a pivot row, in which a touched sink's cell is
float64(sum of its ranks in the group) / float64(their number) and an untouched sink keeps
its cell.  rowsum is the exact integer sum while every cell is integral, else np.sum
(numpy's pairwise order) over the replica's pivot columns -- the sinks that get a row
anywhere in the log, ascending -- with a cell-less column as 0.0.  The integrals are np.sum
of (c_K / S) * dt, m * dt and (m * m) * dt with m = rowsum / nvalid, float64 throughout.
"""
import numpy as np

ST_TIE, ST_EMPTY = 4, 8


def adjacency(edges):
    adj = {}
    for s, x in edges:
        adj.setdefault(int(s), []).append(int(x))
    return adj


def play(t, src, edges, ctrl, end_time, Ks, lead_zeros=0):
    """``lead_zeros`` (tests only): that many 0.0 columns in front of the pivot columns in
    every fractional row's sum -- what summing over never-seen graph sinks would do.  The
    dict also carries ``frac_rows``, the pivot rows with a fractional cell, and ``dens``,
    the row counts (> 1) behind those cells."""
    adj = adjacency(edges)
    n = len(t)
    assert len(src) == n
    seen = sorted({x for s in src for x in adj.get(int(s), ())})
    col = {x: c for c, x in enumerate(seen)}
    S = len(seen)
    nK = len(Ks)
    if S == 0:
        return dict(metrics=np.full(nK + 2, np.nan), counts=np.zeros(4, dtype=np.int64), status=ST_EMPTY,
                    frac_rows=0, dens=set())
    rank = [-1] * S
    num, den = [0] * S, [0] * S      # the cell of a column: num / den (den == 0: none yet)
    rows_t, rows_sum, rows_valid, rows_c = [], [], [], []
    n_own = n_oth = 0
    tie = False
    frac_rows, dens = 0, set()
    i = 0
    while i < n:
        j = i + 1
        while j < n and t[j] == t[i]:
            j += 1
        grp = {}
        for k in range(i, j):
            row = adj.get(int(src[k]), ())
            if not row:
                continue
            own = int(src[k]) == int(ctrl)
            if own:
                n_own += 1
            else:
                n_oth += 1
            for x in row:
                c = col[x]
                rank[c] = 0 if own else (1 if rank[c] < 0 else rank[c] + 1)
                g = grp.setdefault(c, [0, 0])
                g[0] += rank[c]
                g[1] += 1
                tie = tie or g[1] > 1
        if grp:
            for c, (sm, cnt) in grp.items():
                num[c], den[c] = sm, cnt
            live = [c for c in range(S) if den[c]]
            if all(num[c] % den[c] == 0 for c in live):
                rowsum = np.float64(sum(num[c] // den[c] for c in live))
            else:
                cells = np.zeros(lead_zeros + S, dtype=np.float64)
                for c in live:
                    cells[lead_zeros + c] = np.float64(num[c]) / np.float64(den[c])
                rowsum = np.sum(cells)
                frac_rows += 1
                dens |= {den[c] for c in live if num[c] % den[c]}
            rows_t.append(t[i])
            rows_sum.append(rowsum)
            rows_valid.append(len(live))
            # cell <= K - 1 on the float64 cell, as the pivot table compares
            rows_c.append([sum(1 for c in live if np.float64(num[c]) / np.float64(den[c]) <= K - 1) for K in Ks])
        i = j
    T = np.asarray(rows_t, dtype=np.float64)
    dt = np.append(T[1:], np.float64(end_time)) - T
    m = np.asarray(rows_sum, dtype=np.float64) / np.asarray(rows_valid, dtype=np.float64)
    cK = np.asarray(rows_c, dtype=np.float64).reshape(len(T), nK)
    met = [np.sum((cK[:, q] / np.float64(S)) * dt) for q in range(nK)]
    met += [np.sum(m * dt), np.sum((m * m) * dt)]
    return dict(metrics=np.asarray(met, dtype=np.float64),
                counts=np.asarray([n_own, n_oth, len(T), S], dtype=np.int64),
                status=ST_TIE if tie else 0, frac_rows=frac_rows, dens=dens)


def expand(t, src, edges):
    """The dataframe rows of a log (State.get_dataframe's order): (t, src_id, sink_id,
    event_id) arrays, one row per edge of every event, events numbered in log order."""
    adj = adjacency(edges)
    rt, rs, rx, re_ = [], [], [], []
    for k, (tk, sk) in enumerate(zip(t, src)):
        for x in sorted(adj.get(int(sk), ())):
            rt.append(tk)
            rs.append(int(sk))
            rx.append(x)
            re_.append(k)
    return (np.asarray(rt, dtype=np.float64), np.asarray(rs, dtype=np.int64), np.asarray(rx, dtype=np.int64),
            np.asarray(re_, dtype=np.int64))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))

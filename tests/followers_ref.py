"""Host checker for rq_log_followers (tests/test_followers_cpu.py, tests/test_gpu_followers.py).

Plain Python over an event list [(t, src_id)] and an edge list [(src_id, sink_id)]: it
restates the kernel's sums in the kernel's operation order, so the GPU must equal it bit
for bit on every finite output.

Per sink x (ascending sink id).  An event at t of a source with an edge to x is a row of
x.  With rank_x >= 0 the rank x holds (own row -> 0, other row -> rank + 1, 1 for x's
first row) and tlast_x the time of x's last row, a row at t first closes the interval:
    len = t - tlast_x;  if len > 0:  acc_q = acc_q + f_q(rank_x) * len
with f = I(rank <= K - 1) for every K, rank, rank * rank (as doubles, every product and sum
rounded on its own), sequentially in time order from 0.0; when the log ends the last rank
holds until end_time under the same rule.  A row of x at tlast_x itself (one sink, two
rows at one time) makes the replica a TIE; a replica without any row is EMPTY.  first_t is
the time of x's first row (NaN without one), rows the count of x's own / other rows.

Per replica (int_r_2_true).  nvalid = sinks seen so far, sumR2 = the exact integer sum of
their rank^2.  A pivot row is the state after the last event of its time; per row in time
order  acc = acc + (float(sumR2) / float(nvalid)) * (t_next - t_row),  the last row to
end_time.

Tolerance against the REFERENCE's values (tol; derived, not measured).  The reference
sums the same integrals in another order (per pivot row, numpy's pairwise or BLAS order).
Every value is a sum of at most n non-negative terms (n = the run's pivot rows) of at most
4 roundings each (a mean or a square, a difference of times, a product, the term's entry
into the sum), so two summation orders differ by at most (n + 8) * 2**-52 * |exp| -- the
argument of timeline_ref.tol -- and a value whose expectation is 0 is a sum of zeros: it
must be exactly 0.0."""
import math

import numpy as np

ULP = 2.0 ** -52
ST_TIE, ST_EMPTY = 4, 8


def play(ev_t, ev_src, edge_list, sink_ids, src_id, end_time, Ks):
    """One replica.  Returns a dict: vals [S][len(Ks) + 2], first_t [S], rows [S][2] int32,
    r2_true, status, n_rows (pivot rows: distinct times with a row).  vals and r2_true
    are NaN for a TIE / EMPTY replica; first_t and rows stay valid."""
    sinks = sorted(int(x) for x in sink_ids)
    col = {x: i for i, x in enumerate(sinks)}
    fans = {}
    for s, x in edge_list:
        fans.setdefault(int(s), []).append(col[int(x)])
    S, nK = len(sinks), len(Ks)
    end_time = float(end_time)
    rank = [-1] * S
    tlast = [0.0] * S
    acc = [[0.0] * (nK + 2) for _ in range(S)]
    first_t = [float("nan")] * S
    rows = np.zeros((S, 2), dtype=np.int32)
    nvalid, sum_r2 = 0, 0
    have, tie = False, False
    cur_t, r2 = 0.0, 0.0
    n_rows = 0

    def close_span(x, hi):
        ln = hi - tlast[x]
        if ln > 0.0:
            rk = rank[x]
            rho = float(rk)
            a = acc[x]
            for q, K in enumerate(Ks):
                a[q] = a[q] + (1.0 if rk <= K - 1 else 0.0) * ln
            a[nK] = a[nK] + rho * ln
            a[nK + 1] = a[nK + 1] + (rho * rho) * ln

    for t, s in zip(ev_t, ev_src):
        t, s = float(t), int(s)
        fan = fans.get(s)
        if not fan:
            continue
        if have and t != cur_t:
            r2 = r2 + (float(sum_r2) / float(nvalid)) * (t - cur_t)
        if not have or t != cur_t:
            n_rows += 1
        have, cur_t = True, t
        own = s == int(src_id)
        for x in fan:
            rk = rank[x]
            if rk >= 0:
                if tlast[x] == t:
                    tie = True
                close_span(x, t)
                sum_r2 += -(rk * rk) if own else 2 * rk + 1
            else:
                first_t[x] = t
                nvalid += 1
                if not own:
                    sum_r2 += 1
            rank[x] = 0 if own else (1 if rk < 0 else rk + 1)
            tlast[x] = t
            rows[x, 0 if own else 1] += 1
    if have:
        r2 = r2 + (float(sum_r2) / float(nvalid)) * (end_time - cur_t)
    for x in range(S):
        if rank[x] >= 0:
            close_span(x, end_time)
    vals = np.asarray(acc, dtype=np.float64).reshape(S, nK + 2)
    status = ST_TIE if tie else (0 if have else ST_EMPTY)
    if status:
        vals = np.full((S, nK + 2), np.nan)
        r2 = float("nan")
    return dict(vals=vals, first_t=np.asarray(first_t, dtype=np.float64), rows=rows,
                r2_true=np.float64(r2), status=status, n_rows=n_rows, sink_ids=np.asarray(sinks))


def column_sums(table, index, end_time, Ks):
    """The expectation from a filled rank table (rank_of_src_in_df: rows = unique t,
    columns = the df's sinks, NaN before a sink's first row): per column the exactly
    rounded sum (math.fsum) of f(r) * dt over its non-NaN rows, dt the time to the next
    pivot row (end_time after the last), and the column's first non-NaN index.
    Returns ([n_cols][len(Ks) + 2], [n_cols])."""
    table = np.asarray(table, dtype=np.float64)
    index = np.asarray(index, dtype=np.float64)
    dt = np.diff(np.append(index, float(end_time)))
    out = np.zeros((table.shape[1], len(Ks) + 2))
    first = np.full(table.shape[1], np.nan)
    for c in range(table.shape[1]):
        r = table[:, c]
        ok = ~np.isnan(r)
        if not ok.any():
            continue
        first[c] = index[ok][0]
        rr, dd = r[ok], dt[ok]
        for q, K in enumerate(Ks):
            out[c, q] = math.fsum((np.where(rr <= K - 1, 1.0, 0.0) * dd).tolist())
        out[c, len(Ks)] = math.fsum((rr * dd).tolist())
        out[c, len(Ks) + 1] = math.fsum(((rr * rr) * dd).tolist())
    return out, first


def tol(n_rows, exp):
    """|got - exp| allowed against a reference value (module docstring)."""
    return (n_rows + 8) * ULP * np.abs(exp)


def close(got, exp, n_rows):
    """got within tol of exp (exactly 0.0 wherever exp is 0), no NaN."""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    return (got.shape == exp.shape and not np.isnan(got).any() and
            bool(np.all(np.abs(got - exp) <= tol(n_rows, exp))))


def same_bits(a, b):
    """Equal float64 arrays bit for bit where finite, NaN exactly where NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    m = ~np.isnan(a)
    return np.array_equal(a[m].view(np.int64), b[m].view(np.int64))

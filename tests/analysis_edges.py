"""Inputs for the analysis / export edge tests (tests/test_gpu_analysis_edges.py,
tests/test_gpu_export_edges.py) and their CPU preconditions (tests/test_analysis_cpu.py).

Everything here is plain numpy on the host: the GPU tests feed these inputs to the
kernels of rq_analysis.hip, the CPU tests assert that the inputs really have the
properties the GPU tests rely on (numpy's pairwise order, a dot where a fused
multiply-add would show, event times whose accumulated State.time rounds)."""
import math
from fractions import Fraction

import numpy as np

# ----------------------------------------------------------------- oracle walls
# one rq_oracle_dp launch per row: (n_max, instance sizes); n_max picks the arm
ORACLE_LAUNCHES = [
    (257, [0, 1, 2, 63, 64, 65, 127, 128, 255, 256, 257]),   # LDS columns, 256 threads
    (4094, [0, 64, 1023, 4094]),                              # ... its last size
    (4095, [0, 1, 1023, 1024, 1025, 4095]),                   # LDS columns, 1024 threads
    (8190, [65, 8190]),                                       # ... exactly 131072 B of LDS
    (8191, [0, 65, 1025, 8191]),                              # global columns
]
WALL_KINDS = ["exp", "zeros", "tie", "qsmall", "qbig"]


def wall_w(times, end):
    """w of utils.oracle_ranking (utils.py:209) for event times and end_time."""
    return np.diff(np.concatenate([[0.0], [0.0], np.asarray(times, dtype=np.float64), [end]]))


def make_wall(kind, n, i, rs):
    """(w, q, s) of instance i: exponential gaps / 20 % zero gaps with a q that mixes
    posts and waits, the all-tie wall (every gap 0, q = 0: no post), q = 1e-12 (a post
    after every event) and q = 1e12 (never: ranks 0..n)."""
    s = 0.5 + 0.125 * i
    if kind == "tie":
        return np.zeros(n + 2), 0.0, s
    gaps = rs.exponential(0.01, n)
    if kind == "zeros":
        gaps[rs.rand(n) < 0.2] = 0.0
    times = np.cumsum(gaps)
    end = (float(times[-1]) if n else 0.0) + 0.5
    q = {"exp": 0.02 * (1 + 0.37 * i), "zeros": 0.3 * (1 + 0.37 * i), "qsmall": 1e-12,
         "qbig": 1e12}[kind]
    return wall_w(times, end), q, s


def oracle_launch(n_max, sizes):
    """[(n, kind, w, q, s)] of one launch: the kinds rotate over the sizes, sizes below
    n_max appear under every kind when they are cheap, and the largest size once more
    with q = 1e12 (the walk's rank reaches n: the last bit word of every column)."""
    rs = np.random.RandomState(7000 + n_max)
    spec = []
    for j, n in enumerate(sizes):
        kinds = WALL_KINDS if n in (64, 65) else [WALL_KINDS[(j + n_max) % 5]]
        if n == n_max:
            kinds = ["exp", "qbig"] if n_max < 8000 else ["zeros" if n_max == 8190 else "qbig"]
        for kind in kinds:
            spec.append((n, kind))
    out = []
    for i, (n, kind) in enumerate(spec):
        w, q, s = make_wall(kind, n, i, rs)
        out.append((n, kind, w, q, s))
    return out


# ------------------------------------------------------------------ rank frames
RT_COLS = [1, 63, 64, 65, 128, 129, 200]
RT_ROWS = [1, 63, 64, 65, 127, 129, 3001]


def random_frame(n_cols, n_rows, seed, tie_p=0.3, dup_p=0.05):
    """(t, src, raw sink id per row, all n_cols raw sink ids): t repeats with
    probability tie_p, a row repeats the previous (t, sink) with probability dup_p,
    own posts (src 1) are a fifth of the rows; sink ids spread over +-1e12."""
    rs = np.random.RandomState(seed)
    ids = np.unique(rs.randint(-10 ** 12, 10 ** 12, 2 * n_cols + 8, dtype=np.int64))
    ids = rs.permutation(ids)[:n_cols]
    t = np.empty(n_rows)
    col = np.empty(n_rows, dtype=np.int64)
    src = np.where(rs.rand(n_rows) < 0.2, 1, rs.randint(2, 6, n_rows)).astype(np.int64)
    tie, dup = rs.rand(n_rows) < tie_p, rs.rand(n_rows) < dup_p
    gap, pick = rs.exponential(0.5, n_rows), rs.randint(0, n_cols, n_rows)
    cur = 0.5
    for i in range(n_rows):
        if i and dup[i]:
            col[i] = col[i - 1]
        else:
            col[i] = pick[i]
            if i and not tie[i]:
                cur = cur + gap[i]
        t[i] = cur
    return t, src, ids[col], ids


def expected_table(O, t, src, sink, all_ids, src_id, fill):
    """O.rank_table spread over all n_cols columns: a sink without a row is a column
    of NaN (nothing to average, nothing to fill from).  Returns (table, index, column
    of every row)."""
    tab, idx, present = O.rank_table(t, src, sink, src_id, fill)
    cols = np.sort(np.asarray(all_ids))
    full = np.full((tab.shape[0], cols.size), np.nan)
    full[:, np.searchsorted(cols, present)] = tab
    return full, idx, np.searchsorted(cols, sink).astype(np.int32)


def same_bits(a, b):
    """Bit-for-bit equality of float64 arrays up to the NaN payload: the NaN pattern
    and every other value's bits."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    m = ~np.isnan(a)
    return np.array_equal(a[m].view(np.int64), b[m].view(np.int64))


# ------------------------------------------------------------------------ u_int
UI_NT = [1, 7, 8, 9, 127, 128, 129, 255, 256, 8191, 8192, 8193, 16385, 20000]
UI_NF = [0, 1, 2, 5, 70]
UI_NCOLS = 75
# seeds other than 0: with seed 0 the left-to-right sum of x happens to equal np.sum(x)
UI_SEED = {(255, 5): 1}


def u_int_case(n_t, n_f, seed=None):
    """table [n_t, 75] of k/3 ranks, index, fcol (unsorted, one repeat from n_f = 2 on),
    wts = sqrt(s / q) and end_time."""
    seed = UI_SEED.get((n_t, n_f), 0) if seed is None else seed
    rs = np.random.RandomState(911 * n_t + 31 * n_f + seed)
    table = rs.randint(0, 400, (n_t, UI_NCOLS)) / 3.0
    index = np.cumsum(rs.exponential(0.37, n_t)) + 0.11
    end = float(index[-1]) + float(rs.exponential(0.37))
    fcol = rs.permutation(UI_NCOLS)[:n_f].astype(np.int32)
    if n_f >= 2:
        fcol[-1] = fcol[0]
    wts = np.sqrt(rs.uniform(0.1, 3.0, n_f) / rs.uniform(0.05, 2.0))
    return table, index, fcol, wts, end


def u_int_x(table, index, fcol, wts, end):
    """x_k = u_k dt_k in float64 numpy, the dot in follower order (two roundings per
    term); the reference's value is np.sum(x)."""
    u = np.zeros(table.shape[0])
    for f in range(len(fcol)):
        u = u + table[:, fcol[f]] * wts[f]
    return u * np.diff(np.concatenate([index, [end]]))


def seq_sum(x):
    s = 0.0
    for v in x:
        s = s + float(v)
    return s


def fma(a, b, c):
    """a * b + c with one rounding."""
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def u_rows_fma(table, fcol, wts):
    out = np.zeros(table.shape[0])
    for k in range(table.shape[0]):
        u = 0.0
        for f in range(len(fcol)):
            u = fma(float(table[k, fcol[f]]), float(wts[f]), u)
        out[k] = u
    return out


# -------------------------------------------------------------- event-log times
DIRTY_SPOTS = (1, 1023, 1024, 1500, 2048)     # the issue's chain: 1023 and 1024 adjacent
DIRTY_SPOTS_B = (1, 1023, 1500, 2048, 2500)   # 1023 dirty, 1024 plain: the carry alone


def _low_bit(x):
    """Exponent p of the lowest set bit of the double x > 0 (x = odd * 2**p)."""
    m, e = math.frexp(x)
    i = int(m * (1 << 53))
    return e - 53 + ((i & -i).bit_length() - 1)


def _with_bits(x, bits):
    """The double just above x's truncation to `bits` significant bits whose lowest
    set bit is the last of them."""
    m, e = math.frexp(x)
    return math.ldexp(int(m * (1 << bits)) | 1, e - bits)


def _dirty_after(s, rs, then_bits=None):
    """t > 2 s with s + (t - s) != t.  With u = ulp(t), s must be (A + 1/2) u: t - s is
    then a tie, rounds to even, and s + (t - s) is the tie (M -+ 1/2) u of an odd M,
    which rounds away from t = M u.  then_bits: make the resulting state s' = (M -+ 1) u
    a number of that many significant bits, so the next event can be dirty as well."""
    p = _low_bit(s)                       # u = 2**(p + 1)
    A = int(s / math.ldexp(1.0, p + 1))   # s = (A + 1/2) u
    lo, hi = (1 << 52) + (1 << 50) + A, (1 << 53) - (1 << 50)
    if then_bits is None:
        M = int(rs.randint(lo >> 20, hi >> 20)) << 20 | int(rs.randint(0, 1 << 20)) | 1
    else:
        z = 53 - then_bits
        K = int(rs.randint(lo >> z, hi >> z)) | 1
        M = (K << z) + (1 if A % 2 == 0 else -1)   # A even: s' = (M - 1) u, else (M + 1) u
    return math.ldexp(M, p + 1)


def dirty_chain(n, start=0.0, spots=DIRTY_SPOTS, seed=3):
    """n non-decreasing event times from `start`: increments of about 1e-3 relative,
    except at `spots`, where t_k is 2e3 - 8e3 times the accumulated State.time and
    the reference's time += t_k - time lands one ulp off t_k."""
    rs = np.random.RandomState(seed)
    bits = 42                                    # t_k / s of about 2**(53 - bits)
    t = np.empty(n)
    s = float(start)
    for k in range(n):
        if k in spots:
            tk = _dirty_after(s, rs, bits if k + 1 in spots else None)
        else:
            tk = (s if k else float(start) + 1.0) * (1.0 + 1e-3 * (0.1 + rs.rand()))
            if k + 1 in spots:
                tk = _with_bits(tk, bits)
        t[k] = tk
        s = s + (tk - s)
    return t


def state_times(t, start=0.0):
    """State.time after every event (opt_model.py:68, :304) and the time_deltas."""
    st, td = np.empty(len(t)), np.empty(len(t))
    s = float(start)
    for k, tk in enumerate(t):
        td[k] = tk - s
        s = s + td[k]
        st[k] = s
    return st, td

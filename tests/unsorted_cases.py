"""Dataframes whose rows are NOT in time order, for the unsorted replay
(rq_metrics_replay_unsorted, rq_replay_sort.hip), built from numpy and pandas alone.

The reference's metrics take such frames (utils.py:38-56): ranks per sink in dataframe
order, then a pivot on the sorted unique t.  Nothing here touches the GPU library: the
claims are checked on the CPU by tests/test_unsorted_cases_cpu.py and the frames are
replayed by tests/test_gpu_replay_unsorted.py.  golden_frames() are the frames of
tests/golden/unsorted.npz (gen_unsorted.py records the reference's values on them).
"""
import numpy as np
import pandas as pd

from tests import replay_cases as RC

KS_GOLDEN = (1, 2, 5)
I64_MAX = np.iinfo(np.int64).max
EDGE_ROWS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 4097)   # wave / tile (1024 rows) edges
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key].copy()


def is_unsorted(df):
    return bool((np.diff(df.t.values) < 0).any())


def shuffled(df, seed):
    return df.sample(frac=1.0, random_state=seed).reset_index(drop=True)


def stable_sorted(df):
    return df.sort_values("t", kind="stable").reset_index(drop=True)


def swap_rows(df, seed, pairs=3):
    """The frame with a few pairs of rows of different t exchanged: t decreases somewhere
    (a frame of one row, or of one t, comes back as it is)."""
    rs = np.random.RandomState(seed)
    t = df.t.values
    order = np.arange(len(df))
    done = 0
    for _ in range(200):
        if done == pairs or len(df) < 2:
            break
        i, j = sorted(rs.randint(0, len(df), 2))
        if t[i] != t[j] and order[i] == i and order[j] == j:
            order[i], order[j] = j, i
            done += 1
    return df.iloc[order].reset_index(drop=True)


# ---------------------------------------------------------------------------- golden frames
def golden_frames():
    """name -> frame, every one with a decreasing t somewhere (a few hundred to a few
    thousand rows)."""
    def make():
        rs = np.random.RandomState(5)
        out = {}
        a = RC.random_df(rs, 120, np.arange(10, 30), dup_p=0.0, tie_p=0.1)
        b = RC.random_df(rs, 90, np.arange(20, 45), dup_p=0.0, tie_p=0.1)
        out["concat"] = pd.concat([a, b], ignore_index=True)   # overlapping sinks, repeated event ids
        out["shuffle"] = shuffled(a, 3)
        c = RC.random_df(rs, 100, np.arange(8), dup_p=0.3, tie_p=0.3)
        out["shuffle_dup"] = shuffled(c, 4)
        out["concat_same"] = pd.concat([a, a], ignore_index=True)   # every cell a duplicate
        out["reversed"] = a.iloc[::-1].reset_index(drop=True)
        z = a.copy()
        z["t"] = z.t - z.t.values[len(z) // 3]
        z.loc[z.t == 0.0, "t"] = -0.0
        h = len(z) // 2
        z = pd.concat([z.iloc[h:], z.iloc[:h]], ignore_index=True)
        z.loc[int(np.flatnonzero(z.t.values == 0.0)[0]), "t"] = 0.0   # -0.0 and +0.0: one pivot row
        out["negzero"] = z
        out["one_sink"] = shuffled(RC.random_df(rs, 600, np.asarray([7]), tie_p=0.0), 1)
        ids = np.asarray([RC.I64_MIN, -5, 0, 2 ** 62, I64_MAX], dtype=np.int64)
        e = RC.random_df(rs, 200, ids, tie_p=0.1)
        e["t"] = e.t - 7.0
        e = shuffled(e, 2)
        e["event_id"] = (e.event_id - 100) % 60 - 30   # negative and repeated event ids
        out["extremes"] = e
        big = RC.build_frame(rs, [dict(pool=RC.sink_ids(rs, 150), cover=True, rows=3000, tie_p=0.15)])
        h = len(big) // 2
        out["halves"] = pd.concat([big.iloc[h:], big.iloc[:h]], ignore_index=True)
        return out
    if "golden" not in _CACHE:
        _CACHE["golden"] = make()
    return {k: v.copy() for k, v in _CACHE["golden"].items()}


def golden_end(df):
    return float(df.t.max()) + 0.5


def frame_of(d, name):
    """A golden frame from the columns recorded in unsorted.npz."""
    return pd.DataFrame({"event_id": d[name + "_eid"], "src_id": d[name + "_src"], "t": d[name + "_t"],
                         "sink_id": d[name + "_sink"]})[RC.COLUMNS]


# ---------------------------------------------------------------------------- kernel edges
def edge_frame(n):
    """n rows over 37 sinks, a few rows exchanged (n = 1: trivially sorted)."""
    def make():
        rs = np.random.RandomState(300 + n)
        df = RC.build_frame(rs, [dict(pool=RC.sink_ids(rs, 37), rows=n, width=(1, 6), tie_p=0.1)])
        return swap_rows(df, n)
    return _cached(("edge", n), make)


def one_group_frame(n=300):
    """All rows at one t but two early stragglers: one pivot row of duplicate cells."""
    def make():
        rs = np.random.RandomState(41)
        df = RC.random_df(rs, n // 3, np.arange(6), tie_p=0.0)
        df["t"] = 2.5
        df.loc[3, "t"] = 1.0
        df.loc[len(df) - 10, "t"] = 0.5
        return df
    return _cached(("one_group", n), make)


def decreasing_frame(n=1500):
    """Every t distinct, strictly decreasing."""
    def make():
        rs = np.random.RandomState(42)
        t = np.cumsum(rs.exponential(0.1, n) + 1e-3)[::-1]
        return pd.DataFrame({"event_id": 100 + np.arange(n), "src_id": np.where(rs.rand(n) < 0.2, RC.SRC, 3),
                             "t": t, "sink_id": rs.randint(0, 50, n).astype(np.int64)})[RC.COLUMNS]
    return _cached(("decreasing", n), make)


def _bits_frame(bits, seed):
    rs = np.random.RandomState(seed)
    t = np.asarray(bits, dtype=np.uint64).view(np.float64)
    assert np.isfinite(t).all()
    n = len(t)
    return pd.DataFrame({"event_id": 100 + np.arange(n), "src_id": np.where(rs.rand(n) < 0.25, RC.SRC, 4),
                         "t": t, "sink_id": rs.randint(0, 9, n).astype(np.int64)})[RC.COLUMNS]


def low_bit_frame(n=400):
    """Times that differ only in the lowest mantissa bits (1 + k 2^-52, k < 4), shuffled."""
    def make():
        rs = np.random.RandomState(43)
        one = np.float64(1.0).view(np.uint64)
        return _bits_frame(one + rs.randint(0, 4, n).astype(np.uint64), 44)
    return _cached(("low_bit", n), make)


def every_digit_frame(n=600):
    """Times whose bit patterns differ from 1.0's in ONE byte each (every byte of the
    eight, the sign and the top exponent byte among them), so that every radix digit
    decides the order of some pair; shuffled."""
    def make():
        rs = np.random.RandomState(45)
        one = int(np.float64(1.0).view(np.uint64))
        pool = [one]
        for b in range(7):
            pool += [one ^ (v << (8 * b)) for v in (1, 2, 3)]
        pool += [one ^ (v << 56) for v in (0x80, 0x7F, 0xFF, 0x3F)]   # sign / top exponent byte alone
        return _bits_frame([pool[i] for i in rs.randint(0, len(pool), n)], 46)
    return _cached(("every_digit", n), make)


def wide_frame(dup=False):
    """3100 unique sinks in about 6500 rows (past the LDS sink tables), a few rows
    exchanged; dup: one duplicate cell."""
    def make():
        df = RC.wide_frame(3100, 6500, seed=3)
        if dup:
            df = RC.with_dup_cell(df)
        return swap_rows(df, 77 + dup, pairs=5)
    return _cached(("wide", dup), make)


# ---------------------------------------------------------------------------- order kept per sink
def property_base(n_rows):
    """A sorted frame without duplicate cells."""
    def make():
        rs = np.random.RandomState(600 + n_rows)
        return RC.build_frame(rs, [dict(pool=RC.sink_ids(rs, 60), cover=True, rows=n_rows, tie_p=0.15)])
    return _cached(("prop", n_rows), make)


def by_sink(df):
    """Rows grouped by sink, every sink's rows in their order."""
    return df.sort_values("sink_id", kind="stable").reset_index(drop=True)


def interleaved(df, seed):
    """A random interleave of the sinks' row sequences, every sink's rows in their order."""
    rs = np.random.RandomState(seed)
    key = rs.rand(len(df))
    k2 = np.empty(len(df))
    for _, idx in df.groupby("sink_id").indices.items():
        k2[idx] = np.sort(key[idx])
    return df.iloc[np.argsort(k2, kind="stable")].reset_index(drop=True)


# ---------------------------------------------------------------------------- a mixed batch
def nan_frame():
    """Unsorted, with a NaN in t: not evaluated (RQ_EUNSORTED)."""
    df = edge_frame(65)
    df.loc[20, "t"] = np.nan
    return df


def mixed_batch():
    """(name, frame, what the unsorted entry returns for it): 'batch' = the bits of
    rq_metrics_replay_batch, 'oracle' = the C oracle's, 'empty', 'nan'."""
    rs = np.random.RandomState(91)
    sorted_df = RC.build_frame(rs, [dict(pool=np.arange(40), rows=1500, tie_p=0.1)])
    sorted_dup = RC.with_dup_cell(RC.build_frame(rs, [dict(pool=np.arange(30), rows=900, tie_p=0.1)]))
    return [("sorted", sorted_df, "batch"),
            ("unsorted", edge_frame(2049), "oracle"),
            ("empty", sorted_df.iloc[:0], "empty"),
            ("unsorted_dup", shuffled(RC.random_df(rs, 150, np.arange(12), dup_p=0.3, tie_p=0.3), 5), "oracle"),
            ("sorted_dup", sorted_dup, "batch"),
            ("nan", nan_frame(), "nan"),
            ("wide", wide_frame(), "oracle")]

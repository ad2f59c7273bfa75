"""Dataframes for the replay kernels (rq_replay.hip), built from numpy and pandas alone.

Nothing here touches the GPU library: the cases are checked on the CPU by
tests/test_replay_cases_cpu.py and replayed by tests/test_gpu_replay_tiers.py.  Every
frame has the reference's dataframe layout (opt_model.py get_dataframe: columns
event_id, src_id, t, sink_id; rows in time order, an event's rows together).

The sizes below restate limits of rq_replay.hip / rq_internal.h as literals; the GPU
tests pin them from the outside (3071 sinks replay without the large workspace, 3072 do
not), so a drifted constant fails there.
"""
import numpy as np
import pandas as pd

COLUMNS = ["event_id", "src_id", "t", "sink_id"]
I64_MIN = np.iinfo(np.int64).min
SRC = 1                         # the broadcaster whose ranks are measured
KS_ALL = (1, 2, 5, 10)

HASH_MUL = 0x9E3779B97F4A7C15   # rp_hash's multiplier (rq_replay.hip)
_M64 = (1 << 64) - 1

SMALL_MAX = 1023     # RP_HMAX_S: unique sinks the small LDS table takes
SMALL_SLOTS = 2048   # RP_HS
SMALL_BITS = 11      # RP_LOG_HS
LDS_MAX = 3071       # RP_HMAX: unique sinks the full LDS table takes
LDS_SLOTS = 4096     # RP_H
LDS_BITS = 12        # RP_LOG_H
SEQ_LDS_MAX = 3072   # rq_rp_seq: S * 40 B <= RP_SEQ_LDS (120 KB)
KEYS_LDS_MAX = 8192  # RP_KEYS_LDS
CHUNK_ROWS = 4096    # RC_L
CHUNK_MAX = 4096     # RC_S
CHUNK_SLOTS = 8192   # RC_HT
CHUNK_BITS = 13      # RC_HBITS
BATCH = 1024         # RP_B: rows per batch at one row per thread
BATCH2 = 2048        # ... at two rows per thread (no more dataframes than CUs)


# ---------------------------------------------------------------------------- hashing
def rp_hash(k, bits):
    """rp_hash of rq_replay.hip: the top `bits` bits of k * HASH_MUL mod 2^64."""
    return (((int(k) & _M64) * HASH_MUL) & _M64) >> (64 - bits)


def gbits(n_rows):
    """rp_gbits: log2 of the global table's capacity for a dataframe of n_rows rows."""
    b = 1
    while b < 24 and (1 << b) < 2 * n_rows:
        b += 1
    return b


def colliding_ids(slot, bits, n):
    """n distinct int64 ids with rp_hash(id, bits) == slot (never INT64_MIN)."""
    assert 0 <= slot < (1 << bits) and n <= (1 << (64 - bits)) - 1
    inv = pow(HASH_MUL, -1, 1 << 64)
    out, j = [], 0
    while len(out) < n:
        x = ((((slot << (64 - bits)) + j) & _M64) * inv) & _M64
        j += 1
        if x == 1 << 63:
            continue
        out.append(x - (1 << 64) if x >= (1 << 63) else x)
    return np.asarray(out, dtype=np.int64)


# ---------------------------------------------------------------------------- builders
def random_df(rs, n_events, sinks, dup_p=0.0, tie_p=0.0, own_p=0.2, max_width=40):
    """Events of 1..min(max_width, #sinks) distinct sinks (+ a duplicated sink row with
    probability dup_p), equal times with probability tie_p, own posts own_p."""
    rows, t = [], 0.0
    hi = min(max_width, len(sinks)) + 1
    for e in range(n_events):
        if rs.rand() >= tie_p:
            t += float(rs.exponential(0.1))
        src = 1 if rs.rand() < own_p else int(rs.randint(2, 9))
        ss = list(rs.choice(sinks, rs.randint(1, hi), replace=False))
        if rs.rand() < dup_p:
            ss.append(ss[0])
        rows += [(100 + e, src, t, int(y)) for y in ss]
    return pd.DataFrame.from_records(rows, columns=COLUMNS)


def _draw(rs, pool, w):
    """w distinct sinks of pool (a full permutation only where the pool is small)."""
    n = len(pool)
    if w >= n:
        return [int(x) for x in rs.permutation(pool)]
    if 4 * w >= n:
        return [int(x) for x in rs.choice(pool, w, replace=False)]
    seen = {}
    while len(seen) < w:
        seen[int(rs.randint(0, n))] = 1
    return [int(pool[i]) for i in seen]


def build_frame(rs, segments, t0=0.0, eid0=100):
    """The four columns of a dataframe made of segments, in order.  A segment is a dict:

      pool       sink ids its random events draw from
      events     number of random events (default 0), or
      rows       the exact number of rows the segment's random events fill (the last
                 event is cut short to end there)
      width      an event's sinks: an int or (lo, hi) inclusive (default (1, 40))
      cover      True: before the random events, events that sweep the pool once
      tie_p, dup_p, own_p   probability that an event shares the previous event's t /
                 repeats one of its sinks / is the broadcaster's own post
      broadcast  events emitted first, each at one new t: a list of (sinks, own)
    """
    rows, t, e = [], float(t0), int(eid0)
    group = set()   # sinks of the open t-group: an event that ties with it avoids them

    def emit(ss, own, tie=False, dup=False):
        nonlocal t, e
        ss = [int(y) for y in ss]
        if tie:
            ss = [y for y in ss if y not in group]
        if not tie or not ss:
            t += float(rs.exponential(0.1)) + 1e-3
            group.clear()
        if not ss:
            return
        group.update(ss)
        if dup:
            ss.append(ss[0])
        src = SRC if own else int(rs.randint(2, 9))
        rows.extend((e, src, t, y) for y in ss)
        e += 1

    for seg in segments:
        pool = np.asarray(seg.get("pool", ()), dtype=np.int64)
        width = seg.get("width", (1, 40))
        lo, hi = (width, width) if np.isscalar(width) else width
        hi = max(1, min(hi, len(pool)))
        lo = max(1, min(lo, hi))
        tie_p, dup_p, own_p = seg.get("tie_p", 0.0), seg.get("dup_p", 0.0), seg.get("own_p", 0.2)
        for ss, own in seg.get("broadcast", ()):
            emit(ss, own)
        start = len(rows)
        if seg.get("cover"):
            order = rs.permutation(pool)
            for k in range(0, len(order), hi):
                emit(order[k:k + hi], rs.rand() < own_p)
        target = seg.get("rows")
        n_ev = seg.get("events", 0)
        k = 0
        while (len(rows) - start < target) if target is not None else (k < n_ev):
            ss = _draw(rs, pool, int(rs.randint(lo, hi + 1)))
            dup = rs.rand() < dup_p
            if target is not None:
                ss = ss[:target - (len(rows) - start) - dup]
            emit(ss, rs.rand() < own_p, tie=rs.rand() < tie_p, dup=dup)
            k += 1
        if target is not None:
            assert len(rows) - start == target, "cover sweep longer than the segment's rows"
    return pd.DataFrame.from_records(rows, columns=COLUMNS)


def sink_ids(rs, n, with_min=False):
    """n distinct random int64 sink ids of either sign (with_min: INT64_MIN among them)."""
    ids = np.unique(rs.randint(-10 ** 15, 10 ** 15, n + 64, dtype=np.int64))
    ids = rs.permutation(ids)[:n]
    if with_min:
        ids[n // 2] = I64_MIN
    return ids


def has_dup_cell(df):
    return bool(df.duplicated(["t", "sink_id"]).any())


def first_row_of_nth_sink(df, n):
    """Row at which the n-th distinct sink id (1-based) first appears, or None."""
    first = np.sort(df.reset_index(drop=True).groupby("sink_id", sort=False).head(1).index.values)
    return int(first[n - 1]) if len(first) >= n else None


def end_of(df):
    return float(df.t.max()) + 0.5


def relabel(df):
    """The same frame with its sink ids replaced by their rank among the sorted unique
    ids (arange), which keeps the pivot's column order."""
    out = df.copy()
    out["sink_id"] = np.searchsorted(np.unique(df.sink_id.values), df.sink_id.values).astype(np.int64)
    return out


def with_dup_cell(df):
    """One foreign event in the middle of the frame posts twice to its first sink: a
    (t, sink) cell of two different ranks, whose pivot mean is fractional."""
    mid = len(df) // 2
    i = next(j for j in range(mid, len(df)) if df.src_id.values[j] != SRC)
    return pd.concat([df.iloc[:i + 1], df.iloc[i:]], ignore_index=True)


# ---------------------------------------------------------------------------- tier limits
TIER_COUNTS = (1023, 1024, 3071, 3072, 3073, 4096, 4097)
FALLBACK_COUNTS = (3072, 3073, 8192, 8193)
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key].copy()


def gradual_base(n_sinks):
    lim = max([x for x in (SMALL_MAX, LDS_MAX) if x < n_sinks] or [0])
    return lim if lim and n_sinks - lim <= 1100 else n_sinks - 40


def gradual_frame(n_sinks):
    """n_sinks unique sinks, the last of them arriving a few at a time: two full
    2048-row batches and more on a base pool that stays at or under the nearest tier
    limit below n_sinks (1023 / 3071 where that leaves at most 1100 late sinks, else
    n_sinks - 40), then the late sinks one per event, then posts that reach them again.
    With at most 6144 rows the late sinks all arrive in the third and last batch."""
    def make():
        rs = np.random.RandomState(7000 + n_sinks)
        ids = sink_ids(rs, n_sinks)
        base = gradual_base(n_sinks)
        late = ids[base:]
        segs = [dict(pool=ids[:base], cover=True, rows=max(2 * BATCH2 + 100, base + 100),
                     tie_p=0.1, own_p=0.2)]
        # every late sink in an event of its own, every third of them with an old sink
        for k, y in enumerate(late):
            ss = [int(y)] + ([int(ids[rs.randint(0, base)])] if k % 3 == 0 else [])
            segs.append(dict(broadcast=[(ss, k % 5 == 0)]))
        segs.append(dict(pool=np.concatenate([late, ids[:20]]), events=25, width=(1, 8),
                         own_p=0.3, tie_p=0.1))
        return build_frame(rs, segs)
    return _cached(("gradual", n_sinks), make)


def broadcast_frame(n_sinks):
    """n_sinks unique sinks, the late ones arriving in single posts: two full batches on
    a small base pool, then one foreign post to up to 2048 fresh sinks starting at a
    batch boundary (2048 rows: one whole batch of new sinks, more than a 2048-slot
    table has free), one more batch of own and foreign posts to those sinks, then --
    above 3071 -- one own post to the remaining fresh sinks (with 4097 sinks, one more
    than a 4096-slot table holds) and further posts to them."""
    def make():
        rs = np.random.RandomState(9000 + n_sinks)
        ids = sink_ids(rs, n_sinks)
        if n_sinks <= BATCH2 + 900:
            base, f1 = n_sinks - 1000, 1000
        else:
            base, f1 = 900, BATCH2
        b1 = ids[base:base + f1]
        b2 = ids[base + f1:]
        segs = [dict(pool=ids[:base], cover=True, rows=2 * BATCH2, tie_p=0.1),
                dict(broadcast=[(b1, False)], pool=np.concatenate([b1, ids[:min(50, base)]]),
                     rows=2 * BATCH2 - f1, width=(1, 30), own_p=0.3, tie_p=0.1)]
        if len(b2):
            segs.append(dict(broadcast=[(b2, True)], pool=np.concatenate([b2, b1[:200]]),
                             events=40, width=(1, 30), own_p=0.3))
        return build_frame(rs, segs)
    return _cached(("broadcast", n_sinks), make)


def tier_frame(pattern, n_sinks):
    return gradual_frame(n_sinks) if pattern == "gradual" else broadcast_frame(n_sinks)


def crossing_row(pattern, n_sinks):
    """First row of the frame's first late sink: the event that takes the frame past its
    base pool (gradual) or the first broadcast (the row after two full batches)."""
    if pattern == "broadcast":
        return 2 * BATCH2
    return first_row_of_nth_sink(gradual_frame(n_sinks), gradual_base(n_sinks) + 1)


# ---------------------------------------------------------------------------- colliding ids
def _mapped(df, ids):
    out = df.copy()
    out["sink_id"] = np.asarray(ids, dtype=np.int64)[df.sink_id.values]
    return out


def colliding_small():
    """1000 sinks that all hash to the last slot of the 2048-slot table: every probe
    chain starts at slot 2047 and wraps to slot 0."""
    def make():
        rs = np.random.RandomState(31)
        ids = rs.permutation(colliding_ids(SMALL_SLOTS - 1, SMALL_BITS, 1000))
        return build_frame(rs, [dict(pool=ids, cover=True, rows=5000, tie_p=0.1)])
    return _cached("coll_small", make)


def colliding_lds():
    """3000 sinks on the last slot of the 4096-slot table."""
    def make():
        rs = np.random.RandomState(32)
        ids = rs.permutation(colliding_ids(LDS_SLOTS - 1, LDS_BITS, 3000))
        return build_frame(rs, [dict(pool=ids, cover=True, rows=6000, tie_p=0.1)])
    return _cached("coll_lds", make)


def colliding_global():
    """3500 sinks, a thousand of them on the last slot of the frame's global table
    (2^rp_gbits(rows) slots), the rest anywhere."""
    def make():
        rs = np.random.RandomState(33)
        df = build_frame(rs, [dict(pool=np.arange(3500), cover=True, rows=6000, tie_p=0.1)])
        bits = gbits(len(df))
        coll = colliding_ids((1 << bits) - 1, bits, 1000)
        rest = np.setdiff1d(sink_ids(rs, 2600), coll)[:2500]
        return _mapped(df, rs.permutation(np.concatenate([coll, rest])))
    return _cached("coll_global", make)


def colliding_chunked():
    """4050 sinks over three chunks, 4000 of them on the last slot of the chunk table."""
    def make():
        rs = np.random.RandomState(34)
        coll = colliding_ids(CHUNK_SLOTS - 1, CHUNK_BITS, 4000)
        rest = np.setdiff1d(sink_ids(rs, 100), coll)[:50]
        ids = rs.permutation(np.concatenate([coll, rest]))
        return build_frame(rs, [dict(pool=ids, cover=True, rows=2 * CHUNK_ROWS + 900, tie_p=0.1)])
    return _cached("coll_chunked", make)


# ---------------------------------------------------------------------------- INT64_MIN
def int64_min_frame(n_sinks, rows):
    """n_sinks sinks, one of them INT64_MIN (first posted to in the middle of the sweep,
    then again among the random events).  Eight ids each hash to the last slot of the
    small, full, chunk and -- for this row count -- global table, next to the slot the
    sentinel id has for itself."""
    def make():
        rs = np.random.RandomState(4000 + n_sinks + rows)
        ids = sink_ids(rs, n_sinks, with_min=True)
        edge = np.concatenate([colliding_ids((1 << b) - 1, b, 8)
                               for b in sorted({SMALL_BITS, LDS_BITS, CHUNK_BITS, gbits(rows)})])
        edge = np.setdiff1d(edge, ids)
        ids[:len(edge)] = edge
        assert len(np.unique(ids)) == n_sinks and I64_MIN in ids
        df = build_frame(rs, [dict(pool=ids, cover=True, rows=rows - 40, tie_p=0.1),
                              dict(pool=np.concatenate([[I64_MIN], ids[:30]]), rows=40, width=(1, 6),
                                   own_p=0.4)])
        return df
    return _cached(("min", n_sinks, rows), make)


def wide_frame(n_sinks, rows, seed=0):
    """n_sinks random sinks swept once, then random events, `rows` rows in all."""
    def make():
        rs = np.random.RandomState(5000 + n_sinks + rows + seed)
        return build_frame(rs, [dict(pool=sink_ids(rs, n_sinks), cover=True, rows=rows, tie_p=0.1)])
    return _cached(("wide", n_sinks, rows, seed), make)


# ---------------------------------------------------------------------------- batch boundaries
BOUNDARY_LENGTHS = (1, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097)
BOUNDARY_KINDS = ("tgroup", "own_last", "one_sink", "split_event", "dup_across")
# frames for the chunked path (chunks of 4096 rows): a second chunk of one row, two full
# chunks (the last batch full, the last chunk ending with the frame), a last chunk of 8 rows
CHUNK_EDGE_LENGTHS = (4097, 8192, 8200)


def boundary_frame(n, kind, seed=0):
    """n rows with one construction at every multiple of 1024 (the batch boundary at one
    row per thread; every other one is the boundary at two):

      tgroup       a t-group of distinct sinks straddles the boundary
      own_last     an own post ends on the row before it, and the same sink's next row
                   is the first row after it
      one_sink     the first 2048 rows are one sink at distinct t (one bucket list of a
                   whole batch), the rest ordinary
      split_event  one event's rows lie on both sides (its id and t repeat across it)
      dup_across   the rows on both sides are one sink at one t, in two events: a
                   duplicate (t, sink) cell whose two rows no batch sees together.  Only
                   at the multiples of the largest of 1024, 2048, 4096 below n, so that
                   no duplicate inside a batch (or a chunk, 4096 rows) gives it away
    """
    def make():
        rs = np.random.RandomState(100 * n + BOUNDARY_KINDS.index(kind) + 17 * seed)
        sinks = sink_ids(rs, 37)
        m = min(n, BATCH2) if kind == "one_sink" else 0   # rows of the one-sink batch
        width = rs.randint(1, 5, n)                       # events: runs of 1..4 rows
        width[:m] = 1
        ev = np.repeat(np.arange(n), width)[:n]
        step = BATCH
        if kind == "dup_across":
            step = max([x for x in (BATCH, BATCH2, CHUNK_ROWS) if x < n] or [BATCH])
        bounds = list(range(step, n, step))
        for b in bounds:
            if kind in ("own_last", "dup_across") and ev[b] == ev[b - 1]:
                ev[b:] += 1                               # the boundary separates two events
            if kind == "split_event" and ev[b] != ev[b - 1]:
                ev[b:] -= ev[b] - ev[b - 1]               # ... or lies inside one
        ne = int(ev[-1]) + 1
        tie = rs.rand(ne) < 0.1
        tie[:m + 1] = False
        for b in bounds:
            if kind in ("tgroup", "dup_across"):
                tie[ev[b]] = True
            if kind == "own_last":
                tie[ev[b]] = False
        tie[0] = False
        ev_t = np.cumsum(np.where(tie, 0.0, rs.exponential(0.1, ne) + 1e-3))
        ev_own = rs.rand(ne) < 0.25
        if kind == "own_last":
            ev_own[ev[np.asarray(bounds, dtype=np.int64) - 1]] = True
        t = ev_t[ev]
        sink = np.zeros(n, dtype=np.int64)                # distinct within every t-group
        g0 = 0
        for g1 in list(np.flatnonzero(np.diff(t) != 0) + 1) + [n]:
            sink[g0:g1] = rs.choice(sinks, g1 - g0, replace=False)
            g0 = g1
        sink[:m] = sinks[0]
        if kind in ("own_last", "dup_across"):
            for b in bounds:
                g = np.flatnonzero(t == t[b])
                hit = g[(sink[g] == sink[b - 1]) & (g != b - 1)]
                if len(hit):
                    sink[hit[0]] = sink[b]
                sink[b] = sink[b - 1]
        src = np.where(ev_own[ev], SRC, 2 + ev % 7)
        return pd.DataFrame({"event_id": 100 + ev, "src_id": src, "t": t, "sink_id": sink})[COLUMNS]
    return _cached(("boundary", n, kind, seed), make)


N_WIDE_IN_SET = 8


def boundary_set():
    """Every length x construction, then the wide frames of a batch: 1100 sinks (the small
    table given up in the first batches), 1024 (given up in the last batch, after pivot
    rows were written), 3072 (the same for the full table), 3500, a duplicate cell under
    and above 3071 sinks, and two neighbours in the global tier -- 4097 rows each, whose
    16384-slot table and INT64_MIN slot end three slots short of the next frame's region."""
    frames = [boundary_frame(n, k) for n in BOUNDARY_LENGTHS for k in BOUNDARY_KINDS]
    return frames + [wide_frame(1100, 4500), gradual_frame(1024), gradual_frame(3072),
                     wide_frame(3500, 5000), with_dup_cell(wide_frame(500, 3000)),
                     with_dup_cell(wide_frame(3500, 5000)), int64_min_frame(3500, 4097),
                     wide_frame(3200, 4097)]


def filler_frames(count):
    rs = np.random.RandomState(77)
    pool = np.arange(50, 60, dtype=np.int64)
    return [build_frame(rs, [dict(pool=pool, events=6, width=(1, 3), own_p=0.3)]) for _ in range(count)]


# ---------------------------------------------------------------------------- oracle
def oracle_vec(O, df, end=None, Ks=KS_ALL):
    """The C oracle on a frame: (top_K..., avg_rank, r_2) and its counts."""
    top, avg, r2, cnt = O.metrics_df(df.t.values, df.src_id.values, df.sink_id.values,
                                     df.event_id.values, SRC, end_of(df) if end is None else end, Ks)
    return np.asarray(list(top) + [avg, r2]), cnt


def select_ks(vec, Ks, all_ks=KS_ALL):
    """The entries of an oracle_vec over all_ks that a replay with Ks returns."""
    return np.asarray([vec[all_ks.index(k)] for k in Ks] + list(vec[len(all_ks):]))

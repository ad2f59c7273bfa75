"""The replay case builder (tests/replay_cases.py) checked without a GPU: the
constructed ids hash where they claim to, every named case has the unique-sink count,
row count and duplicate-cell presence its name says, the C oracle evaluates each of
them, and none is degenerate -- in particular the expected vector changes when the frame
is cut just before the event that crosses the limit under test, so a kernel that lost
the late sinks could not pass tests/test_gpu_replay_tiers.py."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import replay_cases as RC


def _check_live(df, n_sinks=None, dup=False):
    """Shape claims and a non-degenerate expectation; returns the oracle's vector."""
    assert list(df.columns) == RC.COLUMNS
    assert (np.diff(df.t.values) >= 0).all() and (np.diff(df.event_id.values) >= 0).all()
    assert df.groupby("event_id").src_id.nunique().max() == 1   # one source per event
    if n_sinks is not None:
        assert df.sink_id.nunique() == n_sinks
    assert RC.has_dup_cell(df) == dup
    vec, cnt = RC.oracle_vec(O, df)
    assert np.isfinite(vec).all()
    assert cnt[2] == df.t.nunique() and cnt[3] == df.sink_id.nunique()
    assert cnt[0] > 0 and cnt[1] > 0
    span = RC.end_of(df) - float(df.t.min())
    for k in range(len(RC.KS_ALL)):
        assert 0.0 < vec[k] < span, (k, vec[k], span)    # top_K: a time in (0, horizon)
    assert vec[len(RC.KS_ALL)] > 0.0                       # avg_rank
    return vec


def _differs_when_cut(df, row):
    """The expectation of the whole frame is not that of the frame cut before `row`
    (same horizon)."""
    end = RC.end_of(df)
    full, _ = RC.oracle_vec(O, df, end)
    cut, _ = RC.oracle_vec(O, df.iloc[:row], end)
    return not np.array_equal(full, cut) and (full != cut).all()


@pytest.mark.parametrize("bits", [11, 12, 13, 14, 24])
def test_colliding_ids_hash_to_their_slot(bits):
    for slot in (0, 1, (1 << bits) - 1):
        ids = RC.colliding_ids(slot, bits, 4000)
        assert ids.dtype == np.int64 and len(np.unique(ids)) == 4000
        assert RC.I64_MIN not in ids
        assert all(RC.rp_hash(int(x), bits) == slot for x in ids)
    # the hash restated on unsigned 64-bit numpy arithmetic agrees with the Python one
    ids = RC.colliding_ids((1 << bits) - 1, bits, 100)
    with np.errstate(over="ignore"):
        h = (ids.astype(np.uint64) * np.uint64(RC.HASH_MUL)) >> np.uint64(64 - bits)
    assert (h == (1 << bits) - 1).all()


def test_colliding_ids_skip_the_sentinel():
    """INT64_MIN hashes to some slot for every bit count; asked for that slot, the
    builder leaves it out."""
    for bits in (11, 12, 13):
        slot = RC.rp_hash(RC.I64_MIN, bits)
        ids = RC.colliding_ids(slot, bits, 1 << 12)
        assert RC.I64_MIN not in ids and len(np.unique(ids)) == 1 << 12


def test_gbits_restates_rp_gbits():
    assert [RC.gbits(n) for n in (1, 2, 3, 4096, 4097, 6000, 1 << 23, (1 << 23) + 1)] == \
        [1, 2, 3, 13, 14, 14, 24, 24]


@pytest.mark.parametrize("n_sinks", RC.TIER_COUNTS)
def test_gradual_frames(n_sinks):
    df = RC.gradual_frame(n_sinks)
    _check_live(df, n_sinks)
    assert len(df) <= 3 * RC.BATCH2            # three batches at two rows per thread
    row = RC.crossing_row("gradual", n_sinks)
    # the base pool stays at the limit the late sinks cross (or, for the counts that
    # cross none, 40 under the count); the first late sink arrives in the last batch,
    # after two full ones
    base = {1024: RC.SMALL_MAX, 3072: RC.LDS_MAX, 3073: RC.LDS_MAX, 4096: RC.LDS_MAX,
            4097: RC.LDS_MAX}.get(n_sinks, n_sinks - 40)
    assert RC.gradual_base(n_sinks) == base
    assert 2 * RC.BATCH2 <= row and df.iloc[:row].sink_id.nunique() == base
    assert _differs_when_cut(df, row)


@pytest.mark.parametrize("n_sinks", RC.TIER_COUNTS)
def test_broadcast_frames(n_sinks):
    df = RC.broadcast_frame(n_sinks)
    _check_live(df, n_sinks)
    first = df.reset_index(drop=True).groupby("sink_id", sort=False).head(1)
    new_per_batch = np.bincount(first.index.values // RC.BATCH2)
    assert new_per_batch[2] >= 1000 and df.t.values[2 * RC.BATCH2] != df.t.values[2 * RC.BATCH2 - 1]
    seen = np.cumsum(new_per_batch)
    if n_sinks > RC.SMALL_SLOTS:
        # one batch brings more new sinks than the small table has slots left, on a
        # table still under its limit
        assert seen[1] <= RC.SMALL_MAX and seen[2] > RC.SMALL_SLOTS
        # the second broadcast starts the fifth batch
        assert new_per_batch[4] == n_sinks - seen[2] and seen[3] == seen[2]
        assert seen[3] <= RC.LDS_MAX
    if n_sinks > RC.LDS_SLOTS:
        assert seen[4] > RC.LDS_SLOTS   # ... and more than the full table has
    # every late sink is posted to again after its broadcast (its rank changes)
    late = first.sink_id.values[first.index.values >= 2 * RC.BATCH2]
    again = df.iloc[2 * RC.BATCH2:].sink_id.value_counts()
    assert (again[late] >= 1).all() and (again[late] >= 2).mean() > 0.5
    assert _differs_when_cut(df, 2 * RC.BATCH2)
    if n_sinks > RC.LDS_MAX:
        assert _differs_when_cut(df, 4 * RC.BATCH2)


@pytest.mark.parametrize("pattern", ["gradual", "broadcast"])
@pytest.mark.parametrize("n_sinks", RC.FALLBACK_COUNTS)
def test_fallback_frames(pattern, n_sinks):
    plain = RC.tier_frame(pattern, n_sinks)
    df = RC.with_dup_cell(plain)
    assert len(df) == len(plain) + 1 and not RC.has_dup_cell(plain)
    vec = _check_live(df, n_sinks, dup=True)
    # exactly one cell is a mean, and it is fractional: the replay needs rq_rp_seq
    d = df[df.duplicated(["t", "sink_id"], keep=False)]
    assert len(d) == 2 and d.src_id.iloc[0] != RC.SRC
    assert not np.array_equal(vec, RC.oracle_vec(O, plain, RC.end_of(df))[0])
    row = RC.crossing_row(pattern, n_sinks)
    assert _differs_when_cut(df, row + (row > d.index[0]))


@pytest.mark.parametrize("case,n_sinks,slot,bits,n_coll", [
    ("colliding_small", 1000, RC.SMALL_SLOTS - 1, RC.SMALL_BITS, 1000),
    ("colliding_lds", 3000, RC.LDS_SLOTS - 1, RC.LDS_BITS, 3000),
    ("colliding_global", 3500, None, None, 1000),
    ("colliding_chunked", 4050, RC.CHUNK_SLOTS - 1, RC.CHUNK_BITS, 4000),
])
def test_colliding_frames(case, n_sinks, slot, bits, n_coll):
    df = getattr(RC, case)()
    vec = _check_live(df, n_sinks)
    if bits is None:
        bits = RC.gbits(len(df))
        slot = (1 << bits) - 1
        assert n_sinks > RC.LDS_MAX and (1 << bits) >= 2 * len(df)
    ids = np.unique(df.sink_id.values)
    assert sum(RC.rp_hash(int(x), bits) == slot for x in ids) == n_coll
    if case == "colliding_chunked":
        assert len(df) > 2 * RC.CHUNK_ROWS and n_sinks <= RC.CHUNK_MAX
    # the order-preserving relabelling has the same expectation
    rel = RC.relabel(df)
    assert np.array_equal(np.unique(rel.sink_id.values), np.arange(n_sinks))
    assert np.array_equal(np.argsort(np.argsort(ids)), np.arange(n_sinks))
    assert np.array_equal(RC.oracle_vec(O, rel)[0], vec)


@pytest.mark.parametrize("n_sinks,rows", [(1100, 4500), (3500, 5000), (600, 2 * RC.CHUNK_ROWS + 500)])
def test_int64_min_frames(n_sinks, rows):
    df = RC.int64_min_frame(n_sinks, rows)
    assert len(df) == rows
    _check_live(df, n_sinks)
    hits = np.flatnonzero(df.sink_id.values == RC.I64_MIN)
    assert len(hits) >= 2 and hits[0] < rows - 40 <= hits[-1]
    # real ids sit on the last slot of every table, where the sentinel's own slot follows
    ids = np.unique(df.sink_id.values)
    for bits in (RC.SMALL_BITS, RC.LDS_BITS, RC.CHUNK_BITS, RC.gbits(rows)):
        assert sum(RC.rp_hash(int(x), bits) == (1 << bits) - 1 for x in ids) >= 8
    # the sentinel's column counts: without its rows the expectation differs
    rest = df[df.sink_id != RC.I64_MIN]
    assert not np.array_equal(RC.oracle_vec(O, rest, RC.end_of(df))[0], RC.oracle_vec(O, df)[0])


@pytest.mark.parametrize("n_sinks", [4096, 4097, 8193])
def test_chunked_limit_frames(n_sinks):
    df = RC.wide_frame(n_sinks, 2 * RC.CHUNK_ROWS + 600)
    assert len(df) > 2 * RC.CHUNK_ROWS
    _check_live(df, n_sinks)
    if n_sinks > RC.CHUNK_SLOTS:
        # the last chunk still brings sinks the full 8192-slot table has no room for
        assert df.iloc[:2 * RC.CHUNK_ROWS].sink_id.nunique() < n_sinks


@pytest.mark.parametrize("kind", RC.BOUNDARY_KINDS)
@pytest.mark.parametrize("n", RC.BOUNDARY_LENGTHS + (8192, 8200))
def test_boundary_frames(n, kind):
    df = RC.boundary_frame(n, kind)
    assert len(df) == n
    t, sink, src, eid = (df[c].values for c in ("t", "sink_id", "src_id", "event_id"))
    if n == 1:   # one pivot row: only that the oracle takes it
        vec, cnt = RC.oracle_vec(O, df)
        assert np.isfinite(vec).all() and cnt[2] == 1
        return
    step = RC.BATCH
    if kind == "dup_across":   # only at the coarsest boundaries, and no other duplicate
        step = {1025: 1024, 2047: 1024, 2048: 1024, 2049: 2048, 4096: 2048, 4097: 4096, 8192: 4096,
                8200: 4096}.get(n, n)
        assert n not in RC.CHUNK_EDGE_LENGTHS or step == RC.CHUNK_ROWS   # only at the chunk edge
        assert df.duplicated(["t", "sink_id"], keep=False).sum() == 2 * len(range(step, n, step))
    _check_live(df, dup=kind == "dup_across" and n > 1024)
    for b in range(step, n, step):
        if kind == "tgroup":
            assert t[b] == t[b - 1] and sink[b] != sink[b - 1]
        elif kind == "own_last":
            assert src[b - 1] == RC.SRC and sink[b] == sink[b - 1] and t[b] > t[b - 1]
            assert eid[b] != eid[b - 1]
        elif kind == "split_event":
            assert eid[b] == eid[b - 1] and t[b] == t[b - 1] and src[b] == src[b - 1]
        elif kind == "dup_across":
            assert eid[b] != eid[b - 1] and t[b] == t[b - 1] and sink[b] == sink[b - 1]
    if kind == "one_sink":
        m = min(n, RC.BATCH2)
        assert len(set(sink[:m])) == 1 and len(set(t[:m])) == m
        assert 0 < (src[:m] == RC.SRC).sum() < m
        if n > m:
            assert df.sink_id.nunique() > 1 and t[m] > t[m - 1]


def test_boundary_set_and_fillers():
    frames = RC.boundary_set()
    nb = len(RC.BOUNDARY_LENGTHS) * len(RC.BOUNDARY_KINDS)
    assert len(frames) == nb + RC.N_WIDE_IN_SET
    assert len(frames) <= 64                       # fits a batch of one frame per CU
    for df, n_sinks, dup in zip(frames[nb:], (1100, 1024, 3072, 3500, 500, 3500, 3500, 3200),
                                (False, False, False, False, True, True, False, False)):
        _check_live(df, n_sinks, dup)
    # the two last: 2^rp_gbits slots and the sentinel's end just inside the frame's region
    assert len(frames[-2]) == len(frames[-1]) == 4097 and RC.I64_MIN in frames[-2].sink_id.values
    assert (1 << RC.gbits(4097)) + 1 == 4 * 4097 - 3
    fill = RC.filler_frames(5)
    assert all(0 < len(f) <= 18 for f in fill)
    assert not np.array_equal(fill[0].t.values, fill[1].t.values)


def test_random_df_keeps_its_draws():
    """The shared random_df draws what the two copies it replaces drew, so the existing
    replay tests' frames are unchanged: widths 1..40 (the chunked tests' copy), or 1..39
    with max_width=39 (the batch tests').  The figures were taken from those copies."""
    sinks = np.arange(50, 90)
    a = RC.random_df(np.random.RandomState(3), 200, sinks, 0.05, 0.3)
    assert (len(a), int(a.sink_id.sum())) == (4087, 284403) and float(a.t.sum()) == 33912.1284617269
    b = RC.random_df(np.random.RandomState(3), 200, sinks, 0.05, 0.3, max_width=39)
    assert (len(b), int(b.sink_id.sum())) == (4011, 279199) and float(b.t.sum()) == 33378.02061311784

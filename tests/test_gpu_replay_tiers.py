"""The replay's sink-table tiers at their limits (rq_replay.hip; launch code rp_launch_t,
rp_run in rq_api.cpp): the small table's hand-off to the full one, the full one's to the
global one, the table-full path, colliding and wrapping ids, the INT64_MIN id in every
tier, batch boundaries at one and two rows per thread, the chunked path's limits, a
mixed batch, and a workspace nobody cleared.

Expected values: the C oracle's restatement of utils.py Appendix B (oracle/rq_oracle.c,
pinned to the reference's fixtures by tests/test_oracle.py) on the same columns, compared
bit for bit on every metric and on counts[0], counts[1], counts[3].  The frames come
from tests/replay_cases.py, whose claims tests/test_replay_cases_cpu.py checks.

The limits are literals here on purpose; each names the constant it mirrors.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest

from tests import replay_cases as RC
from tests.test_gpu_replay_batch import _ctx, _dev

pytestmark = pytest.mark.gpu

KS_SETS = [(1,), (1, 2), (1, 2, 5), (1, 2, 5, 10)]
_EXP = {}


def _expect(O, df, Ks, end=None):
    """The oracle on df (evaluated once per frame and horizon, for every K at once)."""
    end = RC.end_of(df) if end is None else end
    key = (int(pd.util.hash_pandas_object(df, index=False).values.sum()), len(df), end)
    if key not in _EXP:
        _EXP[key] = RC.oracle_vec(O, df, end)
    vec, cnt = _EXP[key]
    return RC.select_ks(vec, Ks), cnt


@contextlib.contextmanager
def _env(name, value):
    """An RQ_* knob around one call (the library reads its knobs per call)."""
    old = os.environ.get(name)
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


def _abi(df, Ks, large=False, chunked=False, fill=None, end=None):
    """rq_metrics_replay through the C ABI on a workspace of exactly the size asked for
    (fill: every byte of it set to that value first)."""
    torch, O, L, U = _ctx()
    lib = L.lib()
    n = len(df)
    Kc = np.ascontiguousarray(Ks, dtype=np.int32)
    flags = (L.REPLAY_LARGE if large else 0) | (L.REPLAY_CHUNKED if chunked else 0)
    nb = C.c_size_t()
    assert lib.rq_replay_workspace_size(n, 1, len(Ks), flags, C.byref(nb)) == 0
    if fill is None:
        ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    else:
        ws = torch.full((nb.value,), fill, dtype=torch.uint8, device="cuda")
    tt, ts = _dev(torch, df.t.values, np.float64), _dev(torch, df.src_id.values, np.int64)
    tk, te = _dev(torch, df.sink_id.values, np.int64), _dev(torch, df.event_id.values, np.int64)
    out = torch.empty(len(Ks) + 2, dtype=torch.float64, device="cuda")
    cnt = torch.empty(4, dtype=torch.int64, device="cuda")
    with _env("RQ_RP_CHUNK", "1" if chunked else None):
        rc = lib.rq_metrics_replay(tt.data_ptr(), ts.data_ptr(), tk.data_ptr(), te.data_ptr(), n,
                                   RC.SRC, float(RC.end_of(df) if end is None else end),
                                   Kc.ctypes.data_as(L._pi32), len(Ks), out.data_ptr(), cnt.data_ptr(),
                                   ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return out.cpu().numpy(), cnt.cpu().numpy()


def _columns(frames):
    torch, O, L, U = _ctx()
    cat = lambda c, dt: _dev(torch, np.concatenate([f[c].values for f in frames]), dt)  # noqa: E731
    off = _dev(torch, np.concatenate([[0], np.cumsum([len(f) for f in frames])]), np.int64)
    return cat("t", np.float64), cat("src_id", np.int64), cat("sink_id", np.int64), \
        cat("event_id", np.int64), off


def _batch(frames, Ks, end, chunked=None):
    """One replay_columns call on the frames: (metrics [n, nK + 2], counts [n, 4])."""
    torch, O, L, U = _ctx()
    t, s, k, e, off = _columns(frames)
    m, c = U.replay_columns(t, s, k, e, off, RC.SRC, end, Ks, chunked=chunked)
    return m.cpu().numpy(), c.cpu().numpy()


def _single(df, Ks, chunked, end=None, fresh=True):
    """replay_columns on one frame, the chunked path forced on or off.  fresh: drop the
    cached workspace first, so that the call gets one of exactly the layout it asks for
    (the library tells the layouts apart by size, and a larger cached workspace of
    another layout would leave the chunk area out)."""
    torch, O, L, U = _ctx()
    if fresh:
        U._WS.clear()
    t, s, k, e, _ = _columns([df])
    with _env("RQ_RP_CHUNK", "1" if chunked else "0"):
        m, c = U.replay_columns(t, s, k, e, None, RC.SRC, RC.end_of(df) if end is None else end, Ks,
                                chunked=chunked)
    return m[0].cpu().numpy(), c[0].cpu().numpy()


def _same(got, cnt, exp, ecnt, what=None):
    assert np.array_equal(got, exp), (what, got - exp)
    assert cnt[0] == ecnt[0] and cnt[1] == ecnt[1] and cnt[3] == ecnt[3], (what, cnt, ecnt)
    assert cnt[2] == ecnt[2], (what, cnt, ecnt)   # pivot rows


# ---------------------------------------------------------------------------- tier limits
@pytest.mark.parametrize("pattern", ["gradual", "broadcast"])
@pytest.mark.parametrize("n_sinks", RC.TIER_COUNTS)   # 1023 / 1024: RP_HMAX_S, 3071 / 3072: RP_HMAX,
@pytest.mark.parametrize("Ks", KS_SETS, ids=str)      # 4096 / 4097: RP_H (table full) and RC_S
def test_tier_limits(Ks, n_sinks, pattern):
    """Every count in both growth patterns, for one to four Ks (one K starts in the small
    table).  Without the large workspace 3071 sinks replay and 3072 do not -- the pin of
    RP_HMAX; with it every count gives the oracle's values."""
    torch, O, L, U = _ctx()
    df = RC.tier_frame(pattern, n_sinks)
    exp, ecnt = _expect(O, df, Ks)
    got, cnt = _abi(df, Ks, large=False)
    if n_sinks <= 3071:   # RP_HMAX
        _same(got, cnt, exp, ecnt, "small workspace")
    else:
        assert cnt[2] == L.RQ_EOVERFLOW and np.isnan(got).all(), (cnt, got)
    got, cnt = _abi(df, Ks, large=True)
    _same(got, cnt, exp, ecnt, "large workspace")


@pytest.mark.parametrize("pattern", ["gradual", "broadcast"])
@pytest.mark.parametrize("n_sinks", [1023, 1024])   # RP_HMAX_S and one more
def test_small_tier_knob_changes_nothing(n_sinks, pattern):
    """One K with the small first tier (1024 sinks: abandoned in the last batch, rerun on
    the full table) and with RQ_RP_SMALL=0 (the full table at once): identical."""
    torch, O, L, U = _ctx()
    df = RC.tier_frame(pattern, n_sinks)
    exp, ecnt = _expect(O, df, (1,))
    with _env("RQ_RP_SMALL", None):
        got_s, cnt_s = _abi(df, (1,))
    with _env("RQ_RP_SMALL", "0"):
        got_f, cnt_f = _abi(df, (1,))
    _same(got_s, cnt_s, exp, ecnt, "small tier first")
    assert np.array_equal(got_s, got_f) and np.array_equal(cnt_s, cnt_f)


@pytest.mark.parametrize("pattern", ["gradual", "broadcast"])
@pytest.mark.parametrize("n_sinks", RC.FALLBACK_COUNTS)   # 3072 / 3073: RP_SEQ_LDS / 40 B,
@pytest.mark.parametrize("Ks", [(1,), (1, 2, 5)], ids=str)  # 8192 / 8193: RP_KEYS_LDS
def test_fallback_at_the_limits(Ks, n_sinks, pattern):
    """One duplicated (t, sink) cell hands the frame to rq_rp_keys / rq_rp_seq: per-sink
    state in LDS (3072 sinks) against HBM (3073), keys sorted in LDS (8192) against the
    global buffer (8193)."""
    torch, O, L, U = _ctx()
    df = RC.with_dup_cell(RC.tier_frame(pattern, n_sinks))
    exp, ecnt = _expect(O, df, Ks)
    got, cnt = _abi(df, Ks, large=True)
    _same(got, cnt, exp, ecnt)


# ---------------------------------------------------------------------------- hashing
@pytest.mark.parametrize("case,Ks,large,chunked", [
    ("colliding_small", (1,), False, False),      # slot 2047 of RP_HS = 2048
    ("colliding_lds", (1, 2, 5), False, False),   # slot 4095 of RP_H = 4096
    ("colliding_lds", (1,), False, False),        # ... reached through the small tier's hand-off
    ("colliding_global", (1, 2), True, False),    # the last slot of the 2^rp_gbits table
    ("colliding_chunked", (1, 2), False, True),   # slot 8191 of RC_HT = 8192
])
def test_colliding_and_wrapping_ids(case, Ks, large, chunked):
    """Every id on the table's last slot: all probe chains wrap to slot 0 and run through
    each other.  The result equals the oracle's and that of the same frame with its ids
    relabelled 0, 1, 2, ... in id order (same pivot columns, short chains)."""
    torch, O, L, U = _ctx()
    df = getattr(RC, case)()
    exp, ecnt = _expect(O, df, Ks)
    got, cnt = _abi(df, Ks, large=large, chunked=chunked)
    _same(got, cnt, exp, ecnt, "colliding ids")
    got_r, cnt_r = _abi(RC.relabel(df), Ks, large=large, chunked=chunked)
    assert np.array_equal(got, got_r) and np.array_equal(cnt, cnt_r)
    if chunked:   # (more than 3071 sinks: one workgroup needs the global table)
        got_o, cnt_o = _abi(df, Ks, large=True, chunked=False)
        assert np.array_equal(got, got_o) and np.array_equal(cnt, cnt_o)


# ---------------------------------------------------------------------------- INT64_MIN
def test_int64_min_small_tier_and_handoff():
    """INT64_MIN among 1100 sinks under one K: its slot (index RP_HS) in the small table,
    then -- the frame has more than 1023 sinks -- in the full one (index RP_H); real ids
    occupy the last hash slot before it.  With a duplicate cell the id is also the first
    of the sorted keys rq_rp_seq searches."""
    torch, O, L, U = _ctx()
    df = RC.int64_min_frame(1100, 4500)
    keep = np.unique(df.sink_id.values)[:700]
    keep = np.union1d(keep, [x for x in np.unique(df.sink_id.values) if RC.rp_hash(int(x), 11) == 2047])
    small = df[df.sink_id.isin(keep)].reset_index(drop=True)   # stays in the small table
    assert RC.I64_MIN in small.sink_id.values and 700 <= small.sink_id.nunique() <= 1023
    for frame in (df, small, RC.with_dup_cell(df), RC.with_dup_cell(small)):
        exp, ecnt = _expect(O, frame, (1,))
        got, cnt = _abi(frame, (1,))
        _same(got, cnt, exp, ecnt, len(frame))


@pytest.mark.parametrize("Ks", [(1,), (1, 2, 5, 10)], ids=str)
def test_int64_min_global_tier(Ks):
    """... among 3500 sinks: its slot lies in the workspace, after the frame's table."""
    torch, O, L, U = _ctx()
    df = RC.int64_min_frame(3500, 5000)
    exp, ecnt = _expect(O, df, Ks)
    got, cnt = _abi(df, Ks, large=False)
    assert cnt[2] == L.RQ_EOVERFLOW and np.isnan(got).all()
    got, cnt = _abi(df, Ks, large=True)
    _same(got, cnt, exp, ecnt)
    dup = RC.with_dup_cell(df)   # ... and is dumped from there for rq_rp_keys
    exp, ecnt = _expect(O, dup, Ks)
    got, cnt = _abi(dup, Ks, large=True)
    _same(got, cnt, exp, ecnt, "duplicate cell")


@pytest.mark.parametrize("Ks", [(1,), (1, 2)], ids=str)
def test_int64_min_forced_chunked(Ks):
    """... in a forced-chunked call: the chunk table cannot hold the id (its empty mark), so
    the frame comes back through the one-workgroup path with the same values."""
    torch, O, L, U = _ctx()
    df = RC.int64_min_frame(600, 2 * 4096 + 500)   # more than two chunks of RC_L rows
    exp, ecnt = _expect(O, df, Ks)
    got_c, cnt_c = _single(df, Ks, True)
    got_o, cnt_o = _single(df, Ks, False)
    _same(got_c, cnt_c, exp, ecnt, "forced chunked")
    assert np.array_equal(got_c, got_o) and np.array_equal(cnt_c, cnt_o)
    got_a, cnt_a = _abi(df, Ks, chunked=True)
    assert np.array_equal(got_a, got_c) and np.array_equal(cnt_a, cnt_c)


# ---------------------------------------------------------------------------- batch boundaries
@pytest.mark.parametrize("Ks", [(1,), (5,), (1, 2, 5), (10, 1)], ids=str)
def test_batch_boundaries_at_one_and_two_rows_per_thread(Ks):
    """Frames of 1 .. 4097 rows with a t-group, an own post and its sink's next row, a
    one-sink batch and a split event at every multiple of 1024 rows, then the wide frames
    of replay_cases.boundary_set: as a batch of no more frames than CUs (2048-row
    batches) and padded to CUs + 1 frames (1024-row batches; rq_rp_fast_s<1, 1> and its
    hand-off for one K, rq_rp_fast<NK, true, 1> for the widest frames).  Every frame's
    result is the same in both and the oracle's; an unsorted and an empty frame at the end
    of the padded batch keep their codes."""
    torch, O, L, U = _ctx()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    frames = RC.boundary_set()
    assert len(frames) + 2 <= cus
    small = frames[5]
    fill = RC.filler_frames(cus + 1 - len(frames) - 2) + [small.iloc[::-1].reset_index(drop=True),
                                                          small.iloc[:0]]
    end = max(RC.end_of(f) for f in frames + fill[:-1])
    m_few, c_few = _batch(frames, Ks, end)
    m_many, c_many = _batch(frames + fill, Ks, end)
    assert len(m_few) == len(frames) <= cus and len(m_many) == cus + 1
    for i, df in enumerate(frames):
        exp, ecnt = _expect(O, df, Ks, end)
        _same(m_few[i], c_few[i], exp, ecnt, ("few", i, len(df)))
        _same(m_many[i], c_many[i], exp, ecnt, ("many", i, len(df)))
    for i in (len(frames), len(frames) + 1, cus - 2):
        exp, ecnt = _expect(O, fill[i - len(frames)], Ks, end)
        _same(m_many[i], c_many[i], exp, ecnt, ("filler", i))
    assert c_many[cus - 1, 2] == L.RQ_EUNSORTED and np.isnan(m_many[cus - 1]).all()
    assert c_many[cus, 2] == 0 and np.isnan(m_many[cus]).all()


@pytest.mark.parametrize("kind", RC.BOUNDARY_KINDS)
def test_chunk_boundary_constructions(kind):
    """The same constructions at every multiple of 1024 rows of an 8200-row frame, so also
    at the chunk edges (RC_L = 4096 rows: rows 4096 and 8192), forced through the chunked
    path: a sink's entering state, the t-group a chunk continues and a duplicate cell whose
    rows two chunks hold.  Equal to the one-workgroup path and to the oracle.  Likewise
    4097 rows (a second chunk of one row) and 8192 (two full chunks: the last batch full,
    the last chunk ending with the frame), each for one, three and four Ks (rq_rc_apply<1>,
    <3>, <4>)."""
    torch, O, L, U = _ctx()
    for n in RC.CHUNK_EDGE_LENGTHS:
        df = RC.boundary_frame(n, kind)
        for Ks in ((1,), (1, 2, 5), RC.KS_ALL):
            exp, ecnt = _expect(O, df, Ks)
            got_c, cnt_c = _abi(df, Ks, large=True, chunked=True)
            got_o, cnt_o = _abi(df, Ks, large=True, chunked=False)
            _same(got_c, cnt_c, exp, ecnt, ("chunked", n, Ks))
            _same(got_o, cnt_o, exp, ecnt, ("one workgroup", n, Ks))


# ---------------------------------------------------------------------------- chunked limits
@pytest.mark.parametrize("n_sinks", [4096, 4097, 8193])   # RC_S, one more; RC_HT + 1: table full
@pytest.mark.parametrize("Ks", [(1,), (1, 2)], ids=str)
def test_chunked_limits(Ks, n_sinks):
    """4096 sinks replay in chunks, 4097 are handed to the one-workgroup path after the
    chunk table counted them, 8193 after it filled up: identical to the unchunked call
    and to the oracle."""
    torch, O, L, U = _ctx()
    df = RC.wide_frame(n_sinks, 2 * 4096 + 600)
    exp, ecnt = _expect(O, df, Ks)
    got_c, cnt_c = _single(df, Ks, True)
    got_o, cnt_o = _single(df, Ks, False)
    _same(got_o, cnt_o, exp, ecnt, "unchunked")
    _same(got_c, cnt_c, exp, ecnt, "chunked")
    assert np.array_equal(cnt_c, cnt_o)


# ---------------------------------------------------------------------------- a mixed batch
def test_mixed_batch_in_any_order():
    """Small-tier, 1024-sink, 3072-sink, duplicate-cell, unsorted, empty and INT64_MIN
    frames in one replay_columns call for one K: each well-formed frame gives the oracle's
    values, each bad one its code, in this order and in another."""
    torch, O, L, U = _ctx()
    small = RC.boundary_frame(2049, "tgroup")
    frames = [small, RC.gradual_frame(1024), RC.broadcast_frame(3072),
              RC.with_dup_cell(RC.wide_frame(500, 3000)), small.iloc[::-1].reset_index(drop=True),
              small.iloc[:0], RC.int64_min_frame(1100, 4500)]
    end = max(RC.end_of(f) for f in frames if len(f))
    for order in (list(range(7)), [4, 2, 6, 0, 5, 3, 1]):
        m, c = _batch([frames[i] for i in order], (1,), end)
        for pos, i in enumerate(order):
            if i == 4:
                assert c[pos, 2] == L.RQ_EUNSORTED and np.isnan(m[pos]).all(), (order, c[pos])
            elif i == 5:
                assert c[pos, 2] == 0 and np.isnan(m[pos]).all(), (order, c[pos])
            else:
                exp, ecnt = _expect(O, frames[i], (1,), end)
                _same(m[pos], c[pos], exp, ecnt, (order, i))


# ---------------------------------------------------------------------------- workspace
_WS_CASES = {   # name: (frame, Ks, large, chunked)
    "small": (lambda: RC.wide_frame(500, 3000), (1,), False, False),
    "handoff": (lambda: RC.wide_frame(1100, 4500), (1,), False, False),
    "full": (lambda: RC.wide_frame(2000, 5000), (1, 2), False, False),
    "global": (lambda: RC.wide_frame(3500, 5000), (1, 2), True, False),
    "fallback": (lambda: RC.with_dup_cell(RC.wide_frame(500, 3000)), (1, 2), False, False),
    "fallback_global": (lambda: RC.with_dup_cell(RC.wide_frame(3500, 5000)), (1, 2), True, False),
    "chunked": (lambda: RC.wide_frame(600, 2 * 4096 + 600), (1, 2), False, True),
    "chunked_fallback": (lambda: RC.with_dup_cell(RC.wide_frame(600, 2 * 4096 + 600)), (1, 2), False, True),
}


@pytest.mark.parametrize("name", list(_WS_CASES))
def test_workspace_contents_do_not_matter(name):
    """The host never clears the replay workspace: a workspace of 0x00 bytes and one of
    0xFF bytes give the same result, the oracle's."""
    torch, O, L, U = _ctx()
    make, Ks, large, chunked = _WS_CASES[name]
    df = make()
    exp, ecnt = _expect(O, df, Ks)
    got0, cnt0 = _abi(df, Ks, large=large, chunked=chunked, fill=0)
    got1, cnt1 = _abi(df, Ks, large=large, chunked=chunked, fill=255)
    _same(got0, cnt0, exp, ecnt, "0x00")
    assert np.array_equal(got0, got1) and np.array_equal(cnt0, cnt1), (cnt0, cnt1)


@pytest.mark.parametrize("Ks", [(1,), (1, 2)], ids=str)
def test_rejected_frame_reports_no_stale_counts(Ks):
    """A frame that needs the large workspace and gets the small one reports
    RQ_EOVERFLOW and nothing left over from the workspace's earlier contents."""
    torch, O, L, U = _ctx()
    df = RC.wide_frame(3500, 5000)
    got0, cnt0 = _abi(df, Ks, fill=0)
    got1, cnt1 = _abi(df, Ks, fill=255)
    assert cnt0[2] == L.RQ_EOVERFLOW and np.isnan(got0).all() and np.isnan(got1).all()
    assert np.array_equal(cnt0, cnt1), (cnt0, cnt1)


def test_cached_workspace_after_a_larger_call():
    """utils.replay_columns reuses one cached workspace: each path right after a larger
    call (chunked and global tables, 8193 sinks) has used it."""
    torch, O, L, U = _ctx()
    big = RC.wide_frame(8193, 2 * 4096 + 600)
    for name, (make, Ks, large, chunked) in _WS_CASES.items():
        got_b, cnt_b = _single(big, (1, 2, 5, 10), True, fresh=name == "small")
        _same(got_b, cnt_b, *_expect(O, big, (1, 2, 5, 10)), what="the larger call")
        df = make()
        got, cnt = _single(df, Ks, chunked, fresh=False)
        _same(got, cnt, *_expect(O, df, Ks), what=name)

"""The replay of dataframes in any row order (rq_metrics_replay_unsorted,
rq_replay_sort.hip; utils.replay_columns(unsorted="sort"), utils.accept_unsorted).

Expected values: the reference's own recorded values on the frames of
tests/golden/unsorted.npz, and the C oracle (oracle/rq_oracle.c, pinned to those by
tests/test_unsorted_cases_cpu.py) on the kernel-edge frames of tests/unsorted_cases.py.
Every comparison is exact: np.array_equal on the metrics, equality on all four counts.
"""
import ctypes as C

import numpy as np
import pytest

from tests import replay_cases as RC
from tests import unsorted_cases as UC
from tests.test_gpu_replay_batch import _ctx, _dev

pytestmark = pytest.mark.gpu

GOLDEN_NAMES = ("concat", "shuffle", "shuffle_dup", "concat_same", "reversed", "negzero", "one_sink",
                "extremes", "halves")
KS_SETS = [(1,), (1, 2, 5, 10)]
_EXP = {}


def _expect(O, key, df, Ks, end):
    """The oracle on df (evaluated once per frame, for every K at once)."""
    if key not in _EXP:
        vec, cnt = RC.oracle_vec(O, df, end)
        _EXP[key] = (vec, tuple(int(x) for x in cnt))
    vec, cnt = _EXP[key]
    return RC.select_ks(vec, Ks), cnt


def _columns(torch, frames, eid=True):
    cat = lambda c, dt: _dev(torch, np.concatenate([f[c].values for f in frames]), dt)  # noqa: E731
    off = _dev(torch, np.concatenate([[0], np.cumsum([len(f) for f in frames])]), np.int64)
    return (cat("t", np.float64), cat("src_id", np.int64), cat("sink_id", np.int64),
            cat("event_id", np.int64) if eid else None, off)


def _abi(frames, Ks, end, flags=0, eid=True, entry="rq_metrics_replay_unsorted", one=False):
    """The entry through the C ABI on a workspace of exactly the size its query returns
    (one: df_off = NULL, a single dataframe)."""
    torch, O, L, U = _ctx()
    lib = L.lib()
    t, s, k, e, off = _columns(torch, frames, eid)
    n, n_df = int(t.numel()), len(frames)
    Kc = np.ascontiguousarray(Ks, dtype=np.int32)
    nb = C.c_size_t()
    size = lib.rq_replay_unsorted_workspace_size if entry.endswith("unsorted") else lib.rq_replay_workspace_size
    assert size(n, n_df, len(Ks), flags, C.byref(nb)) == 0
    ws = torch.full((nb.value,), 0xA5, dtype=torch.uint8, device="cuda")   # nobody cleared it
    out = torch.empty((n_df, len(Ks) + 2), dtype=torch.float64, device="cuda")
    cnt = torch.empty((n_df, 4), dtype=torch.int64, device="cuda")
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None  # noqa: E731
    rc = getattr(lib, entry)(ptr(t), ptr(s), ptr(k), ptr(e), None if one else off.data_ptr(), n_df, n,
                             RC.SRC, float(end), Kc.ctypes.data_as(L._pi32), len(Ks), out.data_ptr(),
                             cnt.data_ptr(), ws.data_ptr(), ws.numel(),
                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return out.cpu().numpy(), cnt.cpu().numpy()


def _via_utils(frames, Ks, end):
    torch, O, L, U = _ctx()
    t, s, k, e, off = _columns(torch, frames)
    m, c = U.replay_columns(t, s, k, e, off, RC.SRC, end, Ks, unsorted="sort")
    return m.cpu().numpy(), c.cpu().numpy()


def _same(got, cnt, exp, ecnt, what=None):
    assert np.array_equal(got, exp), (what, got, exp)
    assert tuple(int(x) for x in cnt) == tuple(int(x) for x in ecnt), (what, cnt, ecnt)


# ---------------------------------------------------------------------------- golden frames
def test_golden_names(golden):
    assert tuple(str(x) for x in golden("unsorted.npz")["names"]) == GOLDEN_NAMES


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_golden_replay_columns(golden, name):
    d = golden("unsorted.npz")
    Ks = tuple(int(k) for k in d["Ks"])
    got, cnt = _via_utils([UC.frame_of(d, name)], Ks, float(d[name + "_end"]))
    _same(got[0], cnt[0], d[name + "_metrics"], d[name + "_counts"], name)


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_golden_abi(golden, name):
    """The raw ABI on an exactly sized, uncleared workspace: as a batch of one and with
    df_off = NULL."""
    d = golden("unsorted.npz")
    Ks = tuple(int(k) for k in d["Ks"])
    for one in (False, True):
        got, cnt = _abi([UC.frame_of(d, name)], Ks, float(d[name + "_end"]), one=one)
        _same(got[0], cnt[0], d[name + "_metrics"], d[name + "_counts"], (name, one))


# ---------------------------------------------------------------------------- kernel edges
@pytest.mark.parametrize("Ks", KS_SETS, ids=str)
@pytest.mark.parametrize("n", UC.EDGE_ROWS)
def test_edge_rows(n, Ks):
    """Row counts around a wavefront and around the 1024-row tile, a few rows exchanged."""
    torch, O, L, U = _ctx()
    df = UC.edge_frame(n)
    end = RC.end_of(df)
    exp, ecnt = _expect(O, ("edge", n), df, Ks, end)
    got, cnt = _abi([df], Ks, end)
    _same(got[0], cnt[0], exp, ecnt, n)


EDGE_KINDS = {
    "one_group": UC.one_group_frame,          # one pivot row of duplicate cells + two stragglers
    "decreasing": UC.decreasing_frame,        # every t distinct, strictly decreasing
    "low_bit": UC.low_bit_frame,              # times apart in the lowest mantissa bits only
    "every_digit": UC.every_digit_frame,      # every radix digit decides some pair
    "wide": lambda: UC.wide_frame(False),     # 3100 sinks: past the LDS sink tables
    "wide_dup": lambda: UC.wide_frame(True),  # ... with one duplicate cell (sequential replay, state in HBM)
}


@pytest.mark.parametrize("Ks", KS_SETS, ids=str)
@pytest.mark.parametrize("kind", sorted(EDGE_KINDS))
def test_edge_kinds(kind, Ks):
    torch, O, L, U = _ctx()
    df = EDGE_KINDS[kind]()
    end = RC.end_of(df)
    exp, ecnt = _expect(O, kind, df, Ks, end)
    got, cnt = _abi([df], Ks, end)
    _same(got[0], cnt[0], exp, ecnt, kind)
    if kind.startswith("wide"):   # the same with the large replay workspace in front of the sort area
        got, cnt = _abi([df], Ks, end, flags=L.REPLAY_LARGE)
        _same(got[0], cnt[0], exp, ecnt, (kind, "large"))


@pytest.mark.parametrize("n_rows", [106, 5502])
def test_order_within_sinks_is_all_that_counts(n_rows):
    """The sink-grouped and the interleaved frame return the bits rq_metrics_replay_batch
    returns for the sorted frame (the sorts are stable: dataframe order inside a sink)."""
    torch, O, L, U = _ctx()
    base = UC.property_base(n_rows)
    end = RC.end_of(base)
    exp, ecnt = _abi([base], RC.KS_ALL, end, entry="rq_metrics_replay_batch")
    got, cnt = _abi([UC.by_sink(base), UC.interleaved(base, n_rows), base], RC.KS_ALL, end)
    for i, name in enumerate(("by_sink", "interleaved", "sorted")):
        _same(got[i], cnt[i], exp[0], ecnt[0], name)


# ---------------------------------------------------------------------------- a mixed batch
@pytest.mark.parametrize("Ks", KS_SETS, ids=str)
def test_mixed_batch(Ks):
    torch, O, L, U = _ctx()
    cases = UC.mixed_batch()
    frames = [df for _, df, _ in cases]
    end = max(RC.end_of(df) for df in frames if len(df))
    got, cnt = _abi(frames, Ks, end)
    ref, rcnt = _abi(frames, Ks, end, entry="rq_metrics_replay_batch")
    bare, bcnt = _abi(frames, Ks, end, eid=False)
    for i, (name, df, kind) in enumerate(cases):
        if kind == "batch":
            assert rcnt[i][2] > 0
            _same(got[i], cnt[i], ref[i], rcnt[i], name)
        elif kind == "empty":
            assert cnt[i][2] == 0 and np.isnan(got[i]).all(), (name, cnt[i])
        elif kind == "nan":
            assert cnt[i][2] == L.RQ_EUNSORTED and np.isnan(got[i]).all(), (name, cnt[i])
        else:
            assert rcnt[i][2] in (L.RQ_EUNSORTED, L.RQ_EOVERFLOW), (name, rcnt[i])
            exp, ecnt = _expect(O, ("mixed", name), df, Ks, end)
            _same(got[i], cnt[i], exp, ecnt, name)
        # without event ids: counts -1, everything else unchanged
        assert np.array_equal(bare[i], got[i], equal_nan=True), name
        assert tuple(bcnt[i]) == (-1, -1, cnt[i][2], cnt[i][3]), (name, bcnt[i], cnt[i])


def test_mixed_batch_via_utils_matches_abi():
    torch, O, L, U = _ctx()
    frames = [df for _, df, _ in UC.mixed_batch()]
    end = max(RC.end_of(df) for df in frames if len(df))
    got, cnt = _via_utils(frames, (1, 2), end)
    exp, ecnt = _abi(frames, (1, 2), end)
    assert np.array_equal(got, exp, equal_nan=True) and np.array_equal(cnt, ecnt)


# ---------------------------------------------------------------------------- the facade
class _Opts(object):
    def __init__(self, end):
        self.src_id = RC.SRC
        self.end_time = end


def test_facade_switch(golden):
    torch, O, L, U = _ctx()
    d = golden("unsorted.npz")
    df = UC.frame_of(d, "concat")
    end = float(d["concat_end"])
    so = _Opts(end)
    Ks = [int(k) for k in d["Ks"]]
    m, c = d["concat_metrics"], d["concat_counts"]
    assert U.accept_unsorted.enabled is False
    with U.accept_unsorted(True):
        for i, K in enumerate(Ks):
            assert U.time_in_top_k(df, K, src_id=RC.SRC, end_time=end) == m[i]
        assert U.average_rank(df, sim_opts=so) == m[len(Ks)]
        assert U.int_r_2(df, so) == m[len(Ks) + 1]
        assert U.num_tweets_of(df, sim_opts=so) == float(c[0])
        op = U.add_perf({}, df, so, Ks)
        assert [op["top_%d" % K] for K in Ks] == list(m[:len(Ks)])
        assert (op["avg_rank"], op["r_2"], op["num_events"], op["world_events"]) == \
            (m[len(Ks)], m[len(Ks) + 1], int(c[0]), int(c[1]))
        res = U.replay_frames([df, UC.frame_of(d, "halves")], RC.SRC, end, Ks, unsorted="sort")
        assert res["avg_rank"][0] == m[len(Ks)] and res["pivot_rows"][0] == c[2]
    assert U.accept_unsorted.enabled is False
    with pytest.raises(L.RQError) as ei:
        U.average_rank(df, sim_opts=so)
    assert ei.value.code == L.RQ_EUNSORTED
    # the plain switch, and the batch entries' default
    U.accept_unsorted(True)
    try:
        assert U.int_r_2(df, so) == m[len(Ks) + 1]
    finally:
        U.accept_unsorted(False)
    with pytest.raises(L.RQError):
        U.int_r_2(df, so)
    res = U.replay_frames([df], RC.SRC, end, Ks)
    assert res["pivot_rows"][0] == L.RQ_EUNSORTED

"""The claims of tests/unsorted_cases.py and tests/golden/unsorted.npz, on the CPU.

The C oracle (oracle/rq_oracle.c rqo_metrics_df: ranks in row order, a stable order by
t, == on times, distinct event ids by sort) equals the reference's recorded values on
every golden frame bit for bit, so it is the yardstick for the frames that have no
fixture; a kernel that merely sorts the rows by t cannot pass, because the oracle on the
sorted rows gives other values; and a reordering that keeps every sink's rows in their
order changes nothing.
"""
import numpy as np
import pytest

from tests import replay_cases as RC
from tests import unsorted_cases as UC


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as O
    return O


@pytest.fixture(scope="module")
def data(golden):
    return golden("unsorted.npz")


def _names(d):
    return [str(x) for x in d["names"]]


def _oracle(O, df, end, Ks):
    vec, cnt = RC.oracle_vec(O, df, end, tuple(int(k) for k in Ks))
    return vec, tuple(int(x) for x in cnt)


def test_fixture_is_the_builders_frames(data):
    """unsorted.npz holds golden_frames(): at least eight frames of a few hundred to a
    few thousand rows, the eight kinds among them."""
    frames = UC.golden_frames()
    assert _names(data) == list(frames) and len(frames) >= 8
    for kind in ("concat", "shuffle", "shuffle_dup", "concat_same", "reversed", "negzero", "one_sink",
                 "extremes"):
        assert kind in frames
    for name, df in frames.items():
        got = UC.frame_of(data, name)
        assert 200 <= len(df) <= 5000, name
        for c in RC.COLUMNS:
            assert np.array_equal(got[c].values.view(np.int64), df[c].values.view(np.int64)), (name, c)
        assert float(data[name + "_end"]) == UC.golden_end(df)
    z = frames["negzero"].t.values
    assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any()
    e = frames["extremes"]
    assert set(e.sink_id.values) >= {RC.I64_MIN, UC.I64_MAX, 2 ** 62, -5} and (e.t.values < 0).any()
    assert (e.event_id.values < 0).any() and e.event_id.nunique() < e.groupby(["event_id", "t"]).ngroups
    assert frames["one_sink"].sink_id.nunique() == 1 and len(frames["one_sink"]) == 600
    assert RC.has_dup_cell(frames["shuffle_dup"]) and RC.has_dup_cell(frames["concat_same"])


def test_oracle_equals_reference_on_golden(O, data):
    for name in _names(data):
        df = UC.frame_of(data, name)
        vec, cnt = _oracle(O, df, float(data[name + "_end"]), data["Ks"])
        assert np.array_equal(vec, data[name + "_metrics"]), (name, vec - data[name + "_metrics"])
        assert cnt == tuple(int(x) for x in data[name + "_counts"]), (name, cnt)


def test_golden_frames_are_unsorted_and_sorting_first_is_wrong(O, data):
    for name in _names(data):
        df = UC.frame_of(data, name)
        end = float(data[name + "_end"])
        assert UC.is_unsorted(df), name
        vec, _ = _oracle(O, df, end, data["Ks"])
        svec, _ = _oracle(O, UC.stable_sorted(df), end, data["Ks"])
        assert not np.array_equal(vec, svec), name


@pytest.mark.parametrize("n_rows", [106, 5502, 7989])
def test_order_within_sinks_is_all_that_counts(O, n_rows):
    """A reordering that keeps every sink's rows in their order has no duplicate cell and
    gives exactly the sorted frame's vector and counts."""
    base = UC.property_base(n_rows)
    assert len(base) == n_rows and not UC.is_unsorted(base) and not RC.has_dup_cell(base)
    end = RC.end_of(base)
    exp = _oracle(O, base, end, RC.KS_ALL)
    for name, df in (("by_sink", UC.by_sink(base)), ("interleaved", UC.interleaved(base, n_rows))):
        assert UC.is_unsorted(df) and not RC.has_dup_cell(df), name
        for s, rows in df.groupby("sink_id").indices.items():   # every sink's rows in their order
            assert np.array_equal(df.event_id.values[rows], base.event_id.values[base.sink_id.values == s])
        got = _oracle(O, df, end, RC.KS_ALL)
        assert np.array_equal(got[0], exp[0]) and got[1] == exp[1], name


def test_edge_frames_are_what_they_say():
    for n in UC.EDGE_ROWS:
        df = UC.edge_frame(n)
        assert len(df) == n and UC.is_unsorted(df) == (n > 1), n
    g = UC.one_group_frame()
    assert g.t.nunique() == 3 and UC.is_unsorted(g) and RC.has_dup_cell(g)
    d = UC.decreasing_frame()
    assert (np.diff(d.t.values) < 0).all()
    lo = UC.low_bit_frame()
    assert UC.is_unsorted(lo) and 2 <= lo.t.nunique() <= 4 and np.ptp(lo.t.values) <= 3 * 2.0 ** -52
    ev = UC.every_digit_frame()
    bits = np.unique(ev.t.values.view(np.uint64))
    one = np.float64(1.0).view(np.uint64)
    for b in range(8):   # some value differs from 1.0 in byte b alone
        assert any(x != one and ((x ^ one) & ~np.uint64(0xFF << (8 * b))) == 0 for x in bits), b
    assert UC.is_unsorted(ev) and one in bits
    for dup in (False, True):
        w = UC.wide_frame(dup)
        assert w.sink_id.nunique() == 3100 and 6400 <= len(w) <= 6600 and UC.is_unsorted(w)
        assert RC.has_dup_cell(w) == dup
    kinds = [k for _, _, k in UC.mixed_batch()]
    assert kinds == ["batch", "oracle", "empty", "oracle", "batch", "nan", "oracle"]
    for name, df, kind in UC.mixed_batch():
        if kind == "batch":
            assert not UC.is_unsorted(df), name
        if kind in ("oracle", "nan"):
            assert UC.is_unsorted(df.dropna()), name
    assert np.isnan(UC.nan_frame().t.values).sum() == 1

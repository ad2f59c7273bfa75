"""CPU side of rq_log_timeline (no GPU): the host checker tests/timeline_ref.py pinned to
the reference (tests/golden/timeline.npz: the reference's own rank_of_src_in_df tables
binned per time bin), and the entry's export and first validation."""
import numpy as np

from oracle import oracle as O
from redqueen_amd import _lib as L
from tests import timeline_ref as TR


def fixture_runs(g):
    Ks = [int(k) for k in g["Ks"]]
    for name in g["names"]:
        name = str(name)
        src_id, end = int(g[name + "_world"][0]), float(g[name + "_world"][1])
        edge_list = [tuple(int(v) for v in e) for e in g[name + "_edges"]]
        yield name, src_id, end, edge_list, Ks


def test_checker_matches_reference_tables_bit_for_bit(golden):
    g = golden("timeline.npz")
    n = 0
    for name, src_id, end, edge_list, Ks in fixture_runs(g):
        t, src, sink, eid = TR.frame_of(g[name + "_t"], g[name + "_src"], edge_list)
        for k in (0, 1):
            edges = g["%s_bins%d" % (name, k)]
            got, rows = TR.metrics(O, t, src, sink, src_id, end, edges, Ks)
            exp = g["%s_met%d" % (name, k)]
            assert rows == int(g[name + "_rows"][0]), name
            assert got.shape == exp.shape == (edges.size - 1, len(Ks) + 2)
            assert np.array_equal(got.view(np.int64), exp.view(np.int64)), (name, k)
            assert np.array_equal(TR.posts(t, src, src_id, edges, eid), g["%s_posts%d" % (name, k)])
            assert np.array_equal(TR.posts(t, src, src_id, edges), g["%s_posts%d" % (name, k)])
            assert np.array_equal(TR.wall_posts(t, src, sink, src_id, edges, g[name + "_sinks"]),
                                  g["%s_wall%d" % (name, k)])
            n += 1
    assert n >= 8


def test_fixture_covers_the_stated_cases(golden):
    """What the GPU test relies on: equal times on disjoint sinks in rd_ties, a sink that
    starts after the second bin in late_sink, an edge exactly on an event time."""
    g = golden("timeline.npz")
    t, src = g["rd_ties_t"], g["rd_ties_src"]
    fans = {}
    for s, x in g["rd_ties_edges"]:
        fans.setdefault(int(s), set()).add(int(x))
    eq = np.flatnonzero(t[1:] == t[:-1])
    assert eq.size >= 2
    for k in eq:
        assert not (fans[int(src[k])] & fans[int(src[k + 1])])
    assert int(g["rd_ties_world"][0]) in {int(src[k]) for k in eq} | {int(src[k + 1]) for k in eq}
    assert g["rd_ties_rows"][0] < t.size
    lt, ls = g["late_sink_t"], g["late_sink_src"]
    assert lt[ls == 3].min() > g["late_sink_bins0"][2]
    # covering bins: the top-K fields of S = 2 sinks reach at most half the bin before then
    assert np.all(g["late_sink_met0"][:6, 0] <= 2.5)
    for name in ("readme_opt", "readme_pois"):
        assert np.isin(g[name + "_bins1"], g[name + "_t"]).any()


def test_entry_is_exported_and_validates_before_hip():
    lib = L.lib()
    assert "rq_log_timeline" in L.EXPORTED and hasattr(lib, "rq_log_timeline")
    k = np.asarray([1], dtype=np.int32)
    assert lib.rq_log_timeline(None, None, None, None, 1, 1, None, 1, k.ctypes.data_as(L._pi32), 1,
                               None, None, None, None, None) == L.RQ_EINVAL

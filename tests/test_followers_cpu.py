"""CPU side of rq_log_followers (no GPU): the host checker tests/followers_ref.py against
the reference (tests/golden/followers.npz: per sink column of the reference's own
rank_of_src_in_df table the exactly rounded integrals, the first-row times and row
counts, and the reference's int_r_2_true) at the derived bound (n + 8) * 2**-52 * |exp|
(followers_ref's docstring), batch.followers_frame on hand-made arrays, and the entry's
export and first validation."""
import numpy as np
import pandas as pd

from redqueen_amd import _lib as L
from redqueen_amd import batch
from tests import followers_ref as FR


def fixture_runs(g):
    Ks = [int(k) for k in g["Ks"]]
    for name in g["names"]:
        name = str(name)
        src_id, end = int(g[name + "_world"][0]), float(g[name + "_world"][1])
        edge_list = [tuple(int(v) for v in e) for e in g[name + "_edges"]]
        yield name, src_id, end, edge_list, Ks


def expected(g, name, sinks, nK):
    """The fixture's per-column values spread over all sinks of the world (ascending): a
    sink that is no pivot column has 0 integrals, no first row and no rows."""
    sinks = np.sort(np.asarray(sinks, dtype=np.int64))
    at = np.searchsorted(sinks, g[name + "_cols"])
    vals = np.zeros((sinks.size, nK + 2))
    first = np.full(sinks.size, np.nan)
    cnt = np.zeros((sinks.size, 2), dtype=np.int32)
    vals[at], first[at], cnt[at] = g[name + "_vals"], g[name + "_first"], g[name + "_cnt"]
    return vals, first, cnt


def test_checker_matches_the_reference_within_the_bound(golden):
    g = golden("followers.npz")
    n = 0
    for name, src_id, end, edge_list, Ks in fixture_runs(g):
        got = FR.play(g[name + "_t"], g[name + "_src"], edge_list, g[name + "_sinks"], src_id, end, Ks)
        rows = int(g[name + "_rows"][0])
        vals, first, cnt = expected(g, name, g[name + "_sinks"], len(Ks))
        assert got["status"] == 0 and got["n_rows"] == rows, name
        err = np.abs(got["vals"] - vals) / np.maximum(FR.ULP * np.abs(vals), 1e-300)
        print(name, "max error %.3g ulp over %d rows" % (err.max(), rows))
        assert (got["vals"][vals == 0.0] == 0.0).all(), name
        assert FR.close(got["vals"], vals, rows), name
        assert FR.close(got["r2_true"], g[name + "_r2true"], rows), name
        # exact: first-row times and row counts
        assert FR.same_bits(got["first_t"], first), name
        assert np.array_equal(got["rows"], cnt) and got["rows"].dtype == np.int32, name
        n += 1
    assert n == 6


def test_fixture_covers_the_stated_cases(golden):
    g = golden("followers.npz")
    # wide: out-degrees 130, 65, 129 -- 3, 2 and 3 rounds of 64 lanes with partial last
    # ones -- and every source posts
    fan = {}
    for s, _x in g["wide_edges"]:
        fan[int(s)] = fan.get(int(s), 0) + 1
    assert sorted(fan.values()) == [65, 129, 130] and g["wide_sinks"].size == 130
    assert set(g["wide_src"].tolist()) == {1, 2, 3}
    # lonely: a sink without a column
    assert g["lonely_cols"].size == g["lonely_sinks"].size - 1 and "lonely_loss_opt" not in g.files
    # rd_ties: equal times (disjoint sinks: status 0 above), fewer pivot rows than events
    assert g["rd_ties_rows"][0] < g["rd_ties_t"].size
    # late_sink: a column whose first row comes late
    assert np.nanmax(g["late_sink_first"]) >= 31.0
    for name in ("readme_opt", "readme_pois", "rd_ties", "late_sink", "wide"):
        assert g[name + "_loss_opt"].shape == g[name + "_loss_pois"].shape == g[name + "_index"].shape


def test_checker_ties_and_empties():
    edge_list = [(1, 10), (1, 12), (2, 10), (2, 11), (3, 12), (4, 13), (4, 11)]
    sinks = [10, 11, 12, 13]
    tied = FR.play([0.5, 2.0, 5.0, 5.0, 9.0], [3, 4, 2, 1, 3], edge_list, sinks, 1, 20.0, (1,))
    assert tied["status"] == FR.ST_TIE and np.isnan(tied["vals"]).all() and np.isnan(tied["r2_true"])
    assert FR.same_bits(tied["first_t"], [5.0, 2.0, 0.5, 2.0])
    assert np.array_equal(tied["rows"], [[1, 1], [0, 2], [1, 2], [0, 1]])
    disjoint = FR.play([2.0, 2.0, 5.0, 5.0], [2, 3, 1, 4], edge_list, sinks, 1, 20.0, (1,))
    assert disjoint["status"] == 0 and disjoint["n_rows"] == 2
    # sink 10: rank 1 on [2, 5), rank 0 on [5, 20); sink 13: rank 1 on [5, 20)
    assert np.array_equal(disjoint["vals"][0], [15.0, 3.0, 3.0])
    assert np.array_equal(disjoint["vals"][3], [0.0, 15.0, 15.0])
    # rows: t = 2 -> ranks (1, 1, 1, -), mean r^2 = 1; t = 5 -> (0, 2, 0, 1), mean 5 / 4
    assert disjoint["r2_true"] == 1.0 * 3.0 + 1.25 * 15.0
    for log in (([], []), ([1.0, 2.0], [5, 5])):
        e = FR.play(log[0], log[1], edge_list, sinks, 1, 20.0, (1, 2))
        assert e["status"] == FR.ST_EMPTY and np.isnan(e["vals"]).all() and np.isnan(e["first_t"]).all()
        assert (e["rows"] == 0).all()


def test_followers_frame_chunk_order_and_flags():
    rs = np.random.RandomState(8)
    R, S, Ks = 11, 5, (1, 3)
    vals = rs.uniform(0.0, 50.0, (R, S, 4))
    rows = rs.randint(0, 40, (R, S, 2)).astype(np.int32)
    status = np.zeros(R, dtype=np.int32)
    status[[2, 7]] = [L.ST_TIE, L.ST_EMPTY]
    vals[[2, 7]] = np.nan
    sink_ids = np.asarray([3, 4, 9, 10, 77])
    fr = batch.followers_frame(sink_ids, Ks, vals, rows, status)
    names = ["top_1", "top_3", "rank_int", "rank_sq_int", "own_rows", "wall_rows"]
    assert list(fr.columns) == ["sink_id"] + [c for n in names for c in (n, n + "_se")] + ["n", "n_flagged"]
    assert np.array_equal(fr.sink_id.values, sink_ids) and (fr.n == 9).all() and (fr.n_flagged == 2).all()
    ok = status == 0
    full = np.concatenate([vals, rows.astype(np.float64)], axis=2)[ok]
    for k, nm in enumerate(names):
        assert np.allclose(fr[nm].values, full[:, :, k].mean(0), rtol=16 * FR.ULP, atol=0.0), nm
        assert np.allclose(fr[nm + "_se"].values, full[:, :, k].std(0, ddof=1) / 3.0, rtol=1e-12, atol=0.0), nm
    # what run_followers does: per-chunk arrays concatenated in seed order -- any chunking
    # concatenates to the same arrays, hence to the same frame, bit for bit
    for cut in ([4, 8], [1, 2, 3, 10], []):
        parts = np.split(np.arange(R), cut)
        fr2 = batch.followers_frame(sink_ids, Ks, np.concatenate([vals[p] for p in parts]),
                                    np.concatenate([rows[p] for p in parts]),
                                    np.concatenate([status[p] for p in parts]))
        pd.testing.assert_frame_equal(fr, fr2, check_exact=True)
    # the flagged replicas' values do not matter
    v2 = vals.copy()
    v2[[2, 7]] = 1e9
    pd.testing.assert_frame_equal(fr, batch.followers_frame(sink_ids, Ks, v2, rows, status), check_exact=True)
    # nothing left / one left
    none = batch.followers_frame(sink_ids, Ks, vals[[2]], rows[[2]], status[[2]])
    assert (none.n == 0).all() and none.top_1.isna().all()
    one = batch.followers_frame(sink_ids, Ks, vals[[0]], rows[[0]], status[[0]])
    assert np.array_equal(one.rank_int.values, vals[0, :, 2]) and one.rank_int_se.isna().all()


def test_entries_are_exported_and_validate_before_hip():
    lib = L.lib()
    assert "rq_log_followers" in L.EXPORTED and hasattr(lib, "rq_log_followers")
    assert hasattr(lib, "rq_log_followers_max_sinks")
    k = np.asarray([1], dtype=np.int32)
    assert lib.rq_log_followers(None, None, None, None, 1, 1, k.ctypes.data_as(L._pi32), 1,
                                None, None, None, None, None, None) == L.RQ_EINVAL
    # 160 KiB over 12 + 8 (nK + 2) bytes per sink, 8 more with rows
    for nK in (1, 2, 3, 4):
        for wr in (0, 1):
            assert lib.rq_log_followers_max_sinks(nK, wr) == 163840 // (12 + 8 * (nK + 2) + 8 * wr)
    assert lib.rq_log_followers_max_sinks(1, 0) == 4551
    assert lib.rq_log_followers_max_sinks(0, 0) == 0 and lib.rq_log_followers_max_sinks(5, 1) == 0

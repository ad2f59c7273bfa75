"""CPU side of the analysis helpers (no GPU): the oracle restatements of
utils.oracle_ranking / rank_of_src_in_df pinned to the reference's outputs
(tests/golden/oracle.npz, sweepq.npz), the sweep_q / find_opt_oracle control
flow of the facade driven by the reference's recorded capacities, and the
argument validation of rq_oracle_dp / rq_rank_table / rq_u_int."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

from oracle import oracle as O
from tests import analysis_edges as E
from redqueen_amd import _lib as L
from redqueen_amd import utils as U
from redqueen_amd.opt_model import SimOpts

COLS = ["event_id", "time_delta", "src_id", "t", "sink_id"]


def df_of(g, key):
    return pd.DataFrame({c: g[key + "_" + c] for c in COLS})


def oracle_cases(g):
    for c in g["cases"]:
        c = str(c)
        df = df_of(g, c)
        om = g[c + "_omit"]
        if om.size:
            df = df[~df.src_id.isin(om)]
        et, w = U._oracle_w(df, float(g[c + "_end"][0]))
        for i, q in enumerate(g[c + "_q"]):
            yield c, i, df, et, w, float(q), float(g[c + "_s"][0])


def test_oracle_dp_restatement_matches_reference(golden):
    g = golden("oracle.npz")
    n_checked = 0
    for c, i, df, et, w, q, s in oracle_cases(g):
        cost, ev, rk = O.oracle_dp(w, q, s)
        key = "%s_%d" % (c, i)
        assert cost == g[key + "_cost"][0], key
        assert np.array_equal(ev, g[key + "_events"]), key
        assert np.array_equal(rk, g[key + "_ranks"]), key
        assert np.array_equal(np.concatenate([[0.0], et.values]), g[key + "_t"]), key
        assert np.array_equal(w[1:], g[key + "_tdelta"]), key
        n_checked += 1
    assert n_checked == 16


def test_oracle_dp_edge_cases():
    # n = 0: J is 1 x 2, nothing to decide (utils.py:211-221)
    cost, ev, rk = O.oracle_dp(np.asarray([0.0, 3.0]), 1.0, 1.0)
    assert cost == 0.0 and list(ev) == [0] and list(rk) == [0]
    # q -> 0: post after every event; q -> inf: never post
    w = np.diff(np.concatenate([[0.0, 0.0], np.arange(1, 11) * 0.1, [2.0]]))
    _, ev, rk = O.oracle_dp(w, 1e-12, 1.0)
    assert ev[:-1].all() and not rk.any()
    _, ev, rk = O.oracle_dp(w, 1e12, 1.0)
    assert not ev.any() and list(rk) == list(range(11))


def test_rank_table_restatement_matches_reference(golden):
    g = golden("sweepq.npz")
    df = df_of(g, "rt_readme")
    for src in (1, 2, -1):
        for fill, key in ((True, "rt_readme_%d" % (src + 1)), (False, "rt_readme_%d_nofill" % (src + 1))):
            tab, idx, sinks = O.rank_table(df.t.values, df.src_id.values, df.sink_id.values, src, fill)
            assert np.array_equal(tab, g[key], equal_nan=True), key
            assert np.array_equal(idx, g["rt_readme_index"])
            assert np.array_equal(sinks, g["rt_readme_cols"])
    d5 = df_of(g, "rt_k5")
    tab, _, _ = O.rank_table(d5.t.values, d5.src_id.values, d5.sink_id.values, 1)
    assert np.array_equal(tab, g["rt_k5_tab"], equal_nan=True)


def edge_walls(g):
    """(key, w, q, s, cost, events, ranks) of every wall x q of analysis_edges.npz."""
    for key in g["walls"]:
        key = str(key)
        w = E.wall_w(g[key + "_t"], float(g[key + "_end"][0]))
        for i, q in enumerate(g[key + "_q"]):
            k = "%s_%d" % (key, i)
            yield k, w, float(q), float(g[key + "_s"][0]), g[k + "_cost"][0], g[k + "_events"], \
                g[k + "_ranks"]


def test_oracle_dp_restatement_matches_edge_fixtures(golden):
    """The C oracle equals the reference on walls of n = 63 ... 1025 (repeated times, the
    q = 0 all-tie wall): it stands in for the reference at the sizes the reference's
    pure-Python double loop cannot reach."""
    n_checked = 0
    for k, w, q, s, cost, ev, rk in edge_walls(golden("analysis_edges.npz")):
        c2, e2, r2 = O.oracle_dp(w, q, s)
        assert c2 == cost and np.array_equal(e2, ev) and np.array_equal(r2, rk), k
        assert ev[-1] == 0 and rk[0] == 0
        n_checked += 1
    assert n_checked == 2 * (11 + 3) + 1


def test_rank_table_restatement_matches_edge_fixtures(golden):
    g = golden("analysis_edges.npz")
    assert [str(f) for f in g["frames"]] == ["rt1", "rt63", "rt64", "rt65", "rt129", "rt_one"]
    for key in g["frames"]:
        key = str(key)
        df = df_of(g, key)
        for src in (1, -1):
            for fill, k in ((True, "%s_%d" % (key, src + 1)), (False, "%s_%d_nofill" % (key, src + 1))):
                tab, idx, sinks = O.rank_table(df.t.values, df.src_id.values, df.sink_id.values,
                                               src, fill)
                assert E.same_bits(tab, g[k]), k
                assert np.array_equal(idx, g[key + "_index"]), k
                assert np.array_equal(sinks, g[key + "_cols"]), k
    d = df_of(g, "rt65")
    tab, idx, _ = O.rank_table(d.event_id.values.astype(np.float64), d.src_id.values,
                               d.sink_id.values, 1)
    assert E.same_bits(tab, g["rt65_eid_2"]) and np.array_equal(idx, g["rt65_eid_index"])


def test_u_int_inputs_show_sum_order_and_fma():
    """What tests/test_gpu_analysis_edges.py relies on: numpy's np.sum is the pairwise
    sum the oracle restates, a left-to-right sum of the same x differs from it from
    n_t = 129 on (every case with a follower; without one x is all zeros), and a fused
    multiply-add in the follower dot changes bits."""
    for n_t in E.UI_NT:
        for n_f in E.UI_NF:
            x = E.u_int_x(*E.u_int_case(n_t, n_f))
            assert np.sum(x) == O.npsum(x), (n_t, n_f)
            if n_t >= 129 and n_f >= 1:
                assert E.seq_sum(x) != np.sum(x), (n_t, n_f)
            if n_f == 0:
                assert not x.any()
    table, index, fcol, wts, end = E.u_int_case(9, 5)
    u = np.zeros(9)
    for f in range(5):
        u = u + table[:, fcol[f]] * wts[f]
    assert (E.u_rows_fma(table, fcol, wts) != u).any()
    assert E.fma(1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, -1.0) == -2.0 ** -60


def test_dirty_chains_round_where_the_export_tests_need_it():
    """The event times of tests/test_gpu_export_edges.py: at every spot the reference's
    accumulated State.time misses t_k (s + (t_k - s) != t_k), and after a spot the
    next time_delta differs from t_{k+1} - t_k, so the carried state matters."""
    for start in (0.0, 20.0):
        for spots in (E.DIRTY_SPOTS, E.DIRTY_SPOTS_B):
            t = E.dirty_chain(3000, start, spots)
            assert t[0] >= start and (np.diff(t) >= 0).all()
            st, td = E.state_times(t, start)
            assert np.array_equal(td, O.state_time_deltas(t, start))
            prev = np.concatenate([[start], st[:-1]])
            dirty = np.nonzero(prev + (t - prev) != t)[0]
            assert list(dirty) == sorted(spots)
            for k in spots:
                assert 1e3 < t[k] / prev[k] < 1e4
            after = [k for k in spots if td[k + 1] != t[k + 1] - t[k]]
            assert len(after) >= 2
            # a dirty event closes chunk 0 (index 1023) and a plain one opens chunk 1:
            # its time_delta needs the carried State.time, not t[1023]
            if 1024 not in spots:
                assert 1023 in after
    assert 1023 in E.DIRTY_SPOTS and 1024 in E.DIRTY_SPOTS and 1024 not in E.DIRTY_SPOTS_B


def test_sweep_q_control_flow_matches_reference(golden, monkeypatch):
    """The facade's sweep_q, fed the capacities the reference measured, retraces the
    reference's q sequence and returns its q bit for bit (utils.py:521-607)."""
    g = golden("sweepq.npz")
    trace_q, trace_cap = list(g["sq_trace_q"]), list(g["sq_trace_cap"])
    seen = []

    def fake_cap(sim_opts, q, seeds=None, **kw):
        i = len(seen)
        assert q == trace_q[i], (i, q, trace_q[i])
        seen.append(q)
        return trace_cap[i]
    monkeypatch.setattr(U, "calc_q_capacity_iter", fake_cap)
    monkeypatch.setattr(U, "_wall_df", lambda so: None)
    last_mean = float(g["sq_rlast_mean"][0])
    monkeypatch.setattr(U, "rank_of_src_in_df",
                        lambda df, src: pd.DataFrame([[last_mean]]))
    so = SimOpts.std_poisson(world_seed=1, world_rate=100.0)
    assert U.sweep_q(so, capacity_cap=50.0, parallel=False) == g["sq_q"][0]
    q2 = U.sweep_q(so, capacity_cap=20.0, parallel=False, tol=1e-3, only_tol=True, max_iters=6)
    assert q2 == g["sq_q2"][0]
    assert len(seen) == len(trace_q)
    # the notebook's own q_init (opt_broadcast.ipynb:2813) from that wall mean
    q_init = (4 * last_mean ** 2 * 1.0 ** 2) / (np.pi * np.pi * (50.0 + 1) ** 4)
    assert q_init == 0.0005753494376300199


def test_find_opt_oracle_control_flow(golden, monkeypatch):
    """find_opt_oracle's search, with the oracle DP restated on the CPU standing in
    for rq_oracle_dp, reaches the reference's (q, cost, #events)."""
    g = golden("oracle.npz")
    wall = df_of(g, "p100")
    monkeypatch.setattr(U, "_wall_df", lambda so: wall)

    def cpu_batch(ws, qs, ss):
        return [O.oracle_dp(w, q, s) for w, q, s in zip(ws, qs, ss)]
    monkeypatch.setattr(U, "oracle_dp_batch", cpu_batch)
    so = SimOpts.std_poisson(world_seed=1, world_rate=100.0).update({"end_time": 10.0})
    res = U.find_opt_oracle(50, so)
    assert res["q"] == g["fo_q"][0] and res["cost"] == g["fo_cost"][0]
    assert res["df"].events.sum() == g["fo_events"][0]
    with pytest.raises(AssertionError):
        U.oracle_ranking(pd.concat([wall, wall.assign(sink_id=7)]), so)


def test_analysis_abi_validation():
    lib = L.lib()
    b = C.c_size_t()
    assert lib.rq_oracle_workspace_size(-1, 10, C.byref(b)) == L.RQ_EINVAL
    assert lib.rq_oracle_workspace_size(2, 2_000_000, C.byref(b)) == L.RQ_EINVAL
    assert lib.rq_oracle_workspace_size(2, 100, C.byref(b)) == 0 and b.value >= 2 * 101 * 2 * 8
    assert lib.rq_oracle_dp(None, None, None, None, 0, 10, None, None, None, None, None, 0, None) == 0
    assert lib.rq_oracle_dp(None, None, None, None, 1, 10, None, None, None, None, None, 0,
                            None) == L.RQ_EINVAL
    assert lib.rq_rank_table(None, None, None, 10, 2, 1, 1, 5, None, None, None, None) == L.RQ_EINVAL
    assert lib.rq_u_int(None, None, 10, 2, None, None, 1, 1.0, None, None, 0, None) == L.RQ_EINVAL

#!/usr/bin/env python
"""Generate the golden fixtures under tests/golden/ from the REFERENCE itself.

Run in the build container only (the reference never travels to the GPU box):

    MPLBACKEND=Agg python tests/golden/gen_golden.py [--dist N]

It imports MPI-SWS/RedQueen from /root/reference with the local
``_shim/decorated_options.py`` stand-in on sys.path (the real package is not
installed and there is no network) and records, as plain data:

  npsum.npz        arrays and np.sum() of them (numpy's pairwise float64 sum)
  mt_draws.npz     numpy legacy RandomState draws (random_sample, exponential,
                   poisson, uniform) -- pins the oracle's MT19937 restatement
  readme_runs.npz  README graph (README.md:60-81) runs create_manager_with_opt
                   for several seeds: event arrays + metrics from utils.py
  kat_runs.npz     notebook KATs K1-K6
  adversarial.npz  hand-made tie-heavy / duplicate (t, sink) / many-sink dfs
                   with the reference's time_in_top_k / average_rank / int_r_2
  frac.npz         dfs whose pivot has fractional (k/3) cells on 8-130 columns
  oracle.npz       utils.oracle_ranking on single-follower wall dfs (Poisson2 / Hawkes
                   walls, duplicated edges, omitted sources, n = 0 / 1), the
                   find_opt_oracle bisection and opt_runs.worker_oracle's outputs
  sweepq.npz       utils.sweep_q (sequential) on std_poisson(1, 100): q_init, the
                   returned q and calc_q_capacity_iter per (q, seed);
                   rank_of_src_in_df tables and u_int_opt values
  analysis_edges.npz (--analysis-edges) utils.oracle_ranking on synthetic single-follower
                   walls with n on rq_oracle_dp's wavefront / block widths (63 ... 1025;
                   repeated times; a q = 0, all-zero-gap wall of lhs == rhs ties) and
                   utils.rank_of_src_in_df on frames of 1 / 63 / 64 / 65 / 129 sinks with
                   100+ row t groups, double and triple (t, sink) rows, a late first row
                   and an absent src_id; one frame with a single unique t
  scale_logs.npz   (--scale-logs) whole reference runs at the headline scale: 8 C3 runs
                   and 2 runs of graphs.c5_mid (500 bursty Hawkes sources, T = 1000):
                   event logs, df shape + column crc32s, utils.py's metrics on the df
  dist_c3.npz      (--c3-dist N) N-replica RedQueen ensemble on the C3 bench network
  dist_g120.npz    (--g120-dist N) N-replica RedQueen ensemble on graphs.g120 (> 64
                   sources: the general sweep's instances)
  dist_c5m.npz     (--c5m-dist N) RedQueen ensemble on graphs.c5_mid: C5's 500 bursty
                   Hawkes broadcasters at T = 1000 on 100 followers (grown in chunks)
  dist_c5s.npz     (--c5s-dist N) RedQueen ensemble on graphs.c5_small: C5's bursty
                   Hawkes (l_0 0.5, alpha 1, beta 2) at T = 1000 on 4 followers
  dist_hawkes0.npz (--hawkes-seed0) the 10k-replica Hawkes world draw at seed0 0 that
                   round 1 replaced by dist_world's 30k draw (kept to state its z)
  dist_sig.npz     (--sig-dist N) N-replica OptPWSignificance ensemble (K3 network,
                   24-segment follower significance, randomized worlds)
  realdata.npz     all-RealData worlds (create_manager_with_times): the reference's whole
                   df (deterministic), its metrics and final State.time
  plugin.npz       a registered static broadcaster (registerSource): df + metrics of the
                   seeded world and of randomize_other_sources(u), u = 0..15
  dynplugin.npz    a registered DYNAMIC self-driven broadcaster (Renewal) beside a static
                   one: df + metrics of the seeded world and of randomize_other_sources(u);
                   the same for a REACTIVE one (KnockedOff, knock_*)
  gridtie.npz      a reactive dynamic plugin whose posts meet static sources' times exactly
                   (all sources on binary grids): df + metrics, 32 randomized worlds
  dist_knock.npz   (--knock-dist N) the reactive plugin beside RedQueen: N reference runs
  errors.npz       reference behaviour on a scalar-s u_int_opt and on OptPWSignificance
                   events that reach no follower with positive significance
  sig_runs.npz     OptPWSignificance runs (notebook "Testing out significance",
                   opt_broadcast.ipynb:5469, :5569): events + metrics
  graphs.npz       opt_runs.make_edge_list networks (C3 parameters) and a
                   prepare_multiple_followers_sim_opts network
  dist_c2.npz      (--dist N) N-replica C2 ensemble: RedQueen vs Poisson stats
  dist_world.npz   (--dist N) wall-only ensembles for Hawkes / PiecewiseConst /
                   Poisson sources (event counts and metrics)
"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "_shim"))
sys.path.insert(0, "/root/reference")
warnings.filterwarnings("ignore")
os.environ.setdefault("MPLBACKEND", "Agg")

from redqueen.opt_model import SimOpts  # noqa: E402
import redqueen.utils as U  # noqa: E402
import pandas as pd  # noqa: E402

README = dict(src_id=1, end_time=100.0, s={1: 1.0, 3: 1.0}, q=1.0, sink_ids=[1, 2, 3],
              other_sources=[("Poisson2", {"src_id": 2, "seed": 42, "rate": 10}),
                             ("Hawkes", {"src_id": 3, "seed": 43, "l_0": 10, "alpha": 1.0,
                                         "beta": 10.0})],
              edge_list=[(1, 1), (1, 3), (2, 1), (2, 2), (2, 3), (3, 3)])

KAT_BASE = dict(src_id=1, end_time=100.0, q=1.0, sink_ids=[5001, 5002],
                other_sources=[("Poisson2", {"src_id": 1000, "seed": 42, "rate": 10.0}),
                               ("Poisson2", {"src_id": 1001, "seed": 43, "rate": 10.0})],
                edge_list=[(1000, 5001), (1001, 5002), (1, 5001), (1, 5002)])

KS = [1, 2, 5, 10]
POISSON_SEED_OFFSET = 10 ** 6


def metrics(df, so):
    top = [U.time_in_top_k(df=df, K=k, sim_opts=so) for k in KS]
    avg = U.average_rank(df, sim_opts=so)
    r2 = U.int_r_2(df, so)
    own = len(df.event_id[df.src_id == so.src_id].unique())
    world = len(df.event_id[df.src_id != so.src_id].unique())
    return np.asarray(top + [avg, r2], dtype=np.float64), own, world


def events_of(df):
    g = df.groupby("event_id", sort=True).first()
    return g.t.values, g.time_delta.values, g.src_id.values.astype(np.int64)


def gen_npsum():
    # the inputs are regenerated from (seed, n) by the tests: legacy RandomState
    # streams are frozen by numpy's compatibility policy, so only sums are stored
    sizes = list(range(0, 140)) + [255, 256, 257, 1000, 4095, 8191, 8192, 8193, 12345,
                                   16384, 16385, 50000, 131073]
    sums = [np.sum(npsum_input(n)) for n in sizes]
    np.savez_compressed(os.path.join(HERE, "npsum.npz"), sizes=np.asarray(sizes),
                        sums=np.asarray(sums))


def npsum_input(n):
    rs = np.random.RandomState(1000003 + n)
    return rs.standard_normal(n) * np.exp(rs.uniform(-30, 30, n))


def gen_draws():
    out = {}
    for seed in [0, 1, 42, 43, 101, 2**31 + 7, 2**32 - 1]:
        r = np.random.RandomState(seed)
        out["rs_%d" % seed] = r.random_sample(256)
        out["exp_%d" % seed] = np.random.RandomState(seed).exponential(0.37, 256)
        out["uni_%d" % seed] = np.random.RandomState(seed).uniform(3.0, 100.0, 256)
        for lam in [0.5, 3.0, 9.99, 10.0, 37.5, 1000.0]:
            r = np.random.RandomState(seed)
            out["poi_%d_%g" % (seed, lam)] = np.asarray([r.poisson(lam) for _ in range(64)],
                                                        dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "mt_draws.npz"), **out)


def gen_readme():
    so = SimOpts(**README)
    rec = {}
    seeds = [101, 1, 2, 3, 5, 7, 11, 13]
    for seed in seeds:
        m = so.create_manager_with_opt(seed=seed)
        m.run_dynamic()
        df = m.state.get_dataframe()
        t, dt, s = events_of(df)
        met, own, world = metrics(df, so)
        rec["t_%d" % seed], rec["dt_%d" % seed], rec["src_%d" % seed] = t, dt, s
        rec["met_%d" % seed] = met
        rec["cnt_%d" % seed] = np.asarray([own, world, len(df)])
    # wall-only and Poisson-controlled variants of the same world
    m = so.create_manager_for_wall()
    m.run_dynamic()
    df = m.state.get_dataframe()
    rec["t_wall"], rec["dt_wall"], rec["src_wall"] = events_of(df)
    rec["met_wall"], own, world = metrics(df, so)
    rec["cnt_wall"] = np.asarray([own, world, len(df)])
    m = so.create_manager_with_poisson(seed=7, capacity=400)
    m.run_dynamic()
    df = m.state.get_dataframe()
    rec["t_pois"], rec["dt_pois"], rec["src_pois"] = events_of(df)
    rec["met_pois"], own, world = metrics(df, so)
    rec["cnt_pois"] = np.asarray([own, world, len(df)])
    # a long horizon: > 8192 pivot rows, exercises the chunked np.sum
    so_long = so.update({"end_time": 400.0})
    m = so_long.create_manager_with_opt(seed=3)
    m.run_dynamic()
    df = m.state.get_dataframe()
    rec["t_long"], rec["dt_long"], rec["src_long"] = events_of(df)
    rec["met_long"], own, world = metrics(df, so_long)
    rec["cnt_long"] = np.asarray([own, world, len(df)])
    # max_events truncation
    m = so.create_manager_with_opt(seed=101)
    m.run_dynamic(max_events=500)
    df = m.state.get_dataframe()
    rec["t_max"], rec["dt_max"], rec["src_max"] = events_of(df)
    rec["met_max"], own, world = metrics(df, so)
    rec["cnt_max"] = np.asarray([own, world, len(df)])
    np.savez_compressed(os.path.join(HERE, "readme_runs.npz"), seeds=np.asarray(seeds), **rec)
    # a PiecewiseConst + Poisson(dynamic) + RealData world, all kinds in one run
    so2 = SimOpts(src_id=1, end_time=50.0, s=np.asarray([1.0, 2.0, 0.5]), q=2.0,
                  sink_ids=[10, 11, 12, 13],
                  other_sources=[("PiecewiseConst", {"src_id": 4, "seed": 9,
                                                     "change_times": [0.0, 10.0, 30.0],
                                                     "rates": [2.0, 8.0, 1.0]}),
                                 ("Poisson", {"src_id": 5, "seed": 10, "rate": 3.0}),
                                 ("RealData", {"src_id": 6, "times": [0.5, 7.25, 7.5, 33.0, 49.0, 60.0]}),
                                 ("Hawkes", {"src_id": 7, "seed": 11, "l_0": 1.5, "alpha": 0.5,
                                             "beta": 2.0})],
                  edge_list=[(1, 10), (1, 11), (1, 12), (4, 10), (4, 13), (5, 11), (5, 12),
                             (6, 10), (6, 11), (6, 12), (6, 13), (7, 12), (7, 13)])
    rec2 = {}
    for seed in [3, 4]:
        m = so2.create_manager_with_opt(seed=seed)
        m.run_dynamic()
        df = m.state.get_dataframe()
        rec2["t_%d" % seed], rec2["dt_%d" % seed], rec2["src_%d" % seed] = events_of(df)
        rec2["met_%d" % seed], own, world = metrics(df, so2)
        rec2["cnt_%d" % seed] = np.asarray([own, world, len(df)])
    np.savez_compressed(os.path.join(HERE, "mixed_runs.npz"), **rec2)


def gen_kats():
    rec = {}
    # K1/K2: std_poisson(world_seed=42, world_rate=1000.0), Opt seed 1, run()
    so = SimOpts.std_poisson(world_seed=42, world_rate=1000.0)
    m = so.create_manager_with_opt(1)
    m.run()
    df = m.state.get_dataframe()
    rec["k1_t"], rec["k1_dt"], rec["k1_src"] = events_of(df)
    rec["k1_uint"] = np.asarray([U.u_int_opt(df, sim_opts=so)])
    rec["k2_top10"] = np.asarray([U.time_in_top_k(df, src_id=x, K=10, end_time=1.0)
                                  for x in (1, 2)])
    # K3..K6 (opt_broadcast.ipynb:5443-5615)
    so3 = SimOpts(s=np.asarray([1.0, 1.0]), **KAT_BASE)
    so5 = SimOpts(s=np.asarray([0.5, 1.5]), **KAT_BASE)
    for name, so_, kind, seed, cap in [("k3", so3, "opt", 1, None), ("k4", so3, "poisson", 45, 324),
                                       ("k5", so5, "opt", 1, None), ("k6", so5, "poisson", 4, 325)]:
        if kind == "opt":
            m = so_.create_manager_with_opt(seed)
        else:
            m = so_.create_manager_with_poisson(seed, capacity=cap)
        m.run_dynamic()
        df = m.state.get_dataframe()
        rec[name + "_t"], rec[name + "_dt"], rec[name + "_src"] = events_of(df)
        met, own, world = metrics(df, so3)  # notebook evaluates with sim_opts_1's src/end
        rec[name + "_met"] = met
        rec[name + "_cnt"] = np.asarray([own, world, len(df), df.shape[1]])
    np.savez_compressed(os.path.join(HERE, "kat_runs.npz"), **rec)


def adversarial_df(rs, n_events, sinks, src_id, tie_p, dup_p, n_sources=4):
    rows = []
    t = 0.0
    for e in range(n_events):
        if rs.rand() > tie_p:
            t = t + float(rs.exponential(0.5))
        src = src_id if rs.rand() < 0.2 else int(rs.randint(2, 2 + n_sources))
        k = rs.randint(1, min(len(sinks), 6) + 1)
        ss = list(rs.choice(sinks, k, replace=False))
        if rs.rand() < dup_p:
            ss.append(ss[0])
        for y in ss:
            rows.append((100 + e, 0.0, src, t, int(y)))
    return pd.DataFrame.from_records(rows, columns=["event_id", "time_delta", "src_id", "t",
                                                    "sink_id"])


def gen_adversarial():
    rs = np.random.RandomState(777)
    rec = {}
    cases = []
    specs = [(40, [1, 2, 3], 0.0, 0.0), (40, [1, 2, 3], 0.5, 0.0), (60, [1, 2, 3], 0.4, 0.3),
             (200, list(range(50, 62)), 0.3, 0.3), (200, list(range(50, 62)), 0.6, 0.5),
             (300, list(range(1000, 1040)), 0.2, 0.2), (30, [7], 0.5, 0.5),
             (500, list(range(10, 30)), 0.5, 0.4)]
    for ci, (ne, sinks, tie_p, dup_p) in enumerate(specs):
        for rep in range(4):
            df = adversarial_df(rs, ne, sinks, 1, tie_p, dup_p)
            end = float(df.t.max()) + 1.0
            top = [U.time_in_top_k(df=df, K=k, src_id=1, end_time=end) for k in KS]
            avg = U.average_rank(df, src_id=1, end_time=end)
            r2 = np.sum(U.rank_of_src_in_df(df, 1).mean(1) ** 2 *
                        np.diff(np.concatenate([U.rank_of_src_in_df(df, 1).index.values, [end]])))
            key = "c%d_%d" % (ci, rep)
            rec[key + "_eid"] = df.event_id.values
            rec[key + "_src"] = df.src_id.values
            rec[key + "_t"] = df.t.values
            rec[key + "_sink"] = df.sink_id.values
            rec[key + "_end"] = np.asarray([end])
            rec[key + "_met"] = np.asarray(top + [avg, r2])
            cases.append(key)
    np.savez_compressed(os.path.join(HERE, "adversarial.npz"), cases=np.asarray(cases), **rec)


def gen_graphs():
    """opt_runs.make_edge_list for the C3/C5 networks (the host-side generator is
    pinned against it) and prepare_multiple_followers_sim_opts' Opt edge order."""
    import redqueen.opt_runs as R
    rec = {}
    for name, (nf, nb, deg, seed) in {"c3": (1000, 50, 5, 1024), "small": (20, 7, 3, 5)}.items():
        e = R.make_edge_list(num_followers=nf, num_broadcasters=nb, degree=deg, seed=seed,
                             follower_id_offset=1000, broadcaster_id_offset=5000,
                             opts=R.mk_edge_list_opts)
        rec[name] = np.asarray(e, dtype=np.int64)
    so = R.prepare_multiple_followers_sim_opts(num_followers=50, opts=R.multiple_follower_opts.set_new(
        kind="Hawkes", num_other_broadcasters=20, max_num_followers=80))
    rec["mf_edges"] = np.asarray(so.edge_list, dtype=np.int64)
    rec["mf_sinks"] = np.asarray(so.sink_ids, dtype=np.int64)
    rec["mf_q"] = np.asarray([so.q])
    rec["mf_src"] = np.asarray([x[1]["src_id"] for x in so.other_sources], dtype=np.int64)
    # the PiecewiseConst (phased semi-sinusoids) and Poisson2 (randomised rates) kinds
    for kind in ("PiecewiseConst", "Poisson2"):
        so = R.prepare_multiple_followers_sim_opts(num_followers=10, opts=R.multiple_follower_opts.set_new(
            kind=kind, num_other_broadcasters=6, max_num_followers=20, follower_other_degree=2))
        k = "mf_" + kind.lower()
        rec[k + "_edges"] = np.asarray(so.edge_list, dtype=np.int64)
        rec[k + "_src"] = np.asarray([x[1]["src_id"] for x in so.other_sources], dtype=np.int64)
        rec[k + "_seed"] = np.asarray([x[1]["seed"] for x in so.other_sources], dtype=np.int64)
        if kind == "PiecewiseConst":
            rec[k + "_rates"] = np.asarray([x[1]["rates"] for x in so.other_sources])
            rec[k + "_times"] = np.asarray([x[1]["change_times"] for x in so.other_sources])
        else:
            rec[k + "_rates"] = np.asarray([x[1]["rate"] for x in so.other_sources])
    rec["pwc24"] = np.asarray(R.make_piecewise_const(24))
    np.savez_compressed(os.path.join(HERE, "graphs.npz"), **rec)


def gen_frac():
    """dfs whose pivot has fractional cells (3 rows of one sink at one t with an own
    row among them) on >= 8 sink columns: pins the pairwise row sum of df.mean(1)."""
    rs = np.random.RandomState(4242)
    rec, cases = {}, []
    for ci in range(6):
        S = [8, 12, 20, 33, 64, 130][ci]
        sinks = list(range(200, 200 + S))
        rows, t, eid = [], 0.0, 100
        for e in range(120):
            t += float(rs.exponential(0.3))
            for rep in range(rs.randint(1, 4)):        # 1-3 events at the same t
                src = 1 if rs.rand() < 0.3 else int(rs.randint(2, 6))
                ss = list(rs.choice(sinks, rs.randint(1, min(S, 9) + 1), replace=False))
                if rs.rand() < 0.5:
                    ss += [ss[0], ss[-1]]
                for y in ss:
                    rows.append((eid, 0.0, src, t, int(y)))
                eid += 1
        df = pd.DataFrame.from_records(rows, columns=["event_id", "time_delta", "src_id", "t",
                                                      "sink_id"])
        end = float(df.t.max()) + 0.5
        top = [U.time_in_top_k(df=df, K=k, src_id=1, end_time=end) for k in KS]
        avg = U.average_rank(df, src_id=1, end_time=end)
        r_t = U.rank_of_src_in_df(df, 1).mean(1)
        r2 = np.sum(r_t ** 2 * np.diff(np.concatenate([r_t.index.values, [end]])))
        key = "f%d" % ci
        for col in ["event_id", "src_id", "t", "sink_id"]:
            rec[key + "_" + col] = df[col].values
        rec[key + "_end"] = np.asarray([end])
        rec[key + "_met"] = np.asarray(top + [avg, r2])
        cases.append(key)
    np.savez_compressed(os.path.join(HERE, "frac.npz"), cases=np.asarray(cases), **rec)


def _df_cols(rec, key, df):
    for col in ["event_id", "time_delta", "src_id", "t", "sink_id"]:
        rec[key + "_" + col] = df[col].values


def gen_oracle():
    """utils.oracle_ranking (utils.py:181-245) on reference wall dfs; find_opt_oracle
    (:260-340) and opt_runs.worker_oracle (opt_runs.py:129-155)."""
    import redqueen.opt_runs as R
    rec, cases = {}, []

    def case(key, df, so, qs, omit=None):
        _df_cols(rec, key, df)
        rec[key + "_end"] = np.asarray([so.end_time])
        rec[key + "_s"] = np.asarray([float(np.asarray(so.s).ravel()[0])])
        rec[key + "_omit"] = np.asarray(omit if omit else [], dtype=np.int64)
        rec[key + "_q"] = np.asarray(qs, dtype=np.float64)
        for i, q in enumerate(qs):
            odf, cost = U.oracle_ranking(df=df, sim_opts=so.update({"q": q}), omit_src_ids=omit)
            rec["%s_%d_cost" % (key, i)] = np.asarray([cost])
            rec["%s_%d_ranks" % (key, i)] = odf.ranks.values.astype(np.int64)
            rec["%s_%d_events" % (key, i)] = odf.events.values.astype(np.int64)
            rec["%s_%d_t" % (key, i)] = odf.t.values
            rec["%s_%d_tdelta" % (key, i)] = odf.t_delta.values
        cases.append(key)

    def wall(so):
        m = so.create_manager_for_wall()
        m.run_dynamic()
        return m.state.get_dataframe()

    so = SimOpts.std_poisson(world_seed=42, world_rate=1000.0)
    case("p1000", wall(so), so, [1.0, 0.01, 100.0, 1e-6, 1e6])
    so = SimOpts.std_hawkes(world_seed=7, world_lambda_0=100.0, world_alpha=1.0, world_beta=10.0)
    case("hawkes", wall(so), so, [1.0, 0.1, 3.0])
    so10 = SimOpts.std_poisson(world_seed=1, world_rate=100.0).update({"end_time": 10.0})
    case("p100", wall(so10), so10, [38.5, 1.0])
    # duplicated edge: every wall event reaches the follower twice (groupby mean of t)
    sod = SimOpts.std_poisson(world_seed=5, world_rate=200.0).update(
        {"edge_list": [(1, 1001), (2, 1001), (2, 1001)], "s": 2.5})
    case("dup", wall(sod), sod, [0.5, 4.0])
    # a df with the broadcaster's own posts, omitted by omit_src_ids
    som = SimOpts.std_poisson(world_seed=9, world_rate=300.0)
    m = som.create_manager_with_opt(3)
    m.run_dynamic()
    case("omit", m.state.get_dataframe(), som, [1.0, 0.05], omit=[1])
    # degenerate walls: one event, and one event exactly at end_time's neighbourhood
    so1 = SimOpts.std_poisson(world_seed=0, world_rate=1.0).update({"end_time": 0.9})
    d1 = wall(so1)
    case("n%d" % d1.event_id.nunique(), d1, so1, [1.0, 0.001])
    cases_arr = cases
    # find_opt_oracle on the p100 world, and worker_oracle
    res = U.find_opt_oracle(50, so10)
    rec["fo_q"] = np.asarray([res["q"]])
    rec["fo_cost"] = np.asarray([res["cost"]])
    rec["fo_events"] = np.asarray([res["df"].events.sum()])
    op = R.worker_oracle((1, 50, None, so10, None))
    for k in ["r0_num_events", "num_events", "top_1", "avg_rank", "r_2", "world_events"]:
        rec["wo_" + k] = np.asarray([float(op[k])])
    # the df worker_oracle scores (RealData oracle posts + the same world)
    odf = res["df"]
    mm = so10.create_manager_with_times(odf.t[odf.events == 1] + R.perf_opts.oracle_eps)
    mm.run_dynamic()
    _df_cols(rec, "wo_df", mm.state.get_dataframe())
    np.savez_compressed(os.path.join(HERE, "oracle.npz"), cases=np.asarray(cases_arr), **rec)


def gen_sweepq():
    """utils.sweep_q (utils.py:521-607) with parallel=False, its q_init from
    rank_of_src_in_df(wall, -1) (:38-56), calc_q_capacity_iter (:447-470); u_int_opt
    (:59-81) on README / K1 dfs."""
    rec = {}
    so = SimOpts.std_poisson(world_seed=1, world_rate=100.0)
    qs = []
    orig = U.calc_q_capacity_iter

    def spy(sim_opts, q, **kw):
        c = orig(sim_opts, q, **kw)
        qs.append((q, c))
        return c
    U.calc_q_capacity_iter = spy
    try:
        rec["sq_q"] = np.asarray([U.sweep_q(so, capacity_cap=50.0, parallel=False)])
        rec["sq_q2"] = np.asarray([U.sweep_q(so, capacity_cap=20.0, parallel=False, tol=1e-3,
                                             only_tol=True, max_iters=6)])
    finally:
        U.calc_q_capacity_iter = orig
    rec["sq_trace_q"] = np.asarray([q for q, _ in qs])
    rec["sq_trace_cap"] = np.asarray([c for _, c in qs])
    w = so.create_manager_for_wall()
    w.run_dynamic()
    r_t = U.rank_of_src_in_df(w.state.get_dataframe(), -1)
    rec["sq_rlast_mean"] = np.asarray([r_t.iloc[-1].mean()])
    # rank tables: README run (3 sinks) and K3 df, with and without ffill
    rd = SimOpts(**README)
    m = rd.create_manager_with_opt(seed=101)
    m.run_dynamic()
    df = m.state.get_dataframe()
    _df_cols(rec, "rt_readme", df)
    for src in (1, 2, -1):
        tab = U.rank_of_src_in_df(df, src)
        rec["rt_readme_%d" % (src + 1)] = tab.values
        rec["rt_readme_%d_nofill" % (src + 1)] = U.rank_of_src_in_df(df, src, fill=False).values
    rec["rt_readme_index"] = tab.index.values
    rec["rt_readme_cols"] = tab.columns.values.astype(np.int64)
    rec["rt_readme_uint"] = np.asarray([U.u_int_opt(df, sim_opts=rd.update({"s": np.asarray([1.0, 1.0])}),
                                                    follower_ids=[1, 3])])
    so3 = SimOpts(s=np.asarray([0.5, 1.5]), **KAT_BASE)
    m = so3.create_manager_with_opt(1)
    m.run_dynamic()
    df3 = m.state.get_dataframe()
    _df_cols(rec, "rt_k5", df3)
    rec["rt_k5_uint"] = np.asarray([U.u_int_opt(df3, sim_opts=so3)])
    rec["rt_k5_tab"] = U.rank_of_src_in_df(df3, 1).values
    np.savez_compressed(os.path.join(HERE, "sweepq.npz"), **rec)


EDGE_WALL_N = [63, 64, 65, 127, 128, 255, 256, 257, 1023, 1024, 1025]
EDGE_WALL_ZERO_N = [64, 257, 1024]   # a second wall with ~20 % repeated times


def edge_rank_frame(rs, S, n_events):
    """A df for rank_of_src_in_df at rq_rank_table's edges: S sinks, own posts (src 1)
    first and last, a burst of 100+ rows at one t, double and triple (t, sink) rows,
    a world / own / world cell (a k/3 mean) and one sink first seen in the last third."""
    sinks = np.sort(rs.choice(np.arange(10, 5000), S, replace=False)).astype(np.int64)
    late = int(sinks[rs.randint(S)]) if S > 1 else None
    early = [int(x) for x in sinks if x != late]
    rows = []
    t = 0.25

    def post(e, src, ss):
        for y in ss:
            rows.append((100 + e, 0.0, int(src), t, int(y)))

    burst_at, frac_at, late_at = n_events // 3, n_events // 2, (2 * n_events) // 3 + 2
    e = 0
    for step in range(n_events):
        pool = early if (late is None or step < late_at) else early + [late]
        if step > 0 and rs.rand() > 0.3:
            t = t + float(rs.exponential(0.5))
        own = step == 0 or step == n_events - 1 or rs.rand() < 0.2
        k = rs.randint(1, min(len(pool), 6) + 1)
        ss = [int(x) for x in rs.choice(pool, k, replace=False)]
        u = rs.rand()
        if u < 0.10:
            ss += [ss[0], ss[0]]
        elif u < 0.25:
            ss.append(ss[0])
        if late is not None and step == late_at:
            ss.append(late)
        post(e, 1 if own else rs.randint(2, 6), ss)
        e += 1
        if step == burst_at:       # 100+ rows at this t: spans rq_rank_table's 64-row batches
            n0 = len(rows)
            while len(rows) - n0 < 110:
                k = rs.randint(1, min(len(pool), 6) + 1)
                post(e, 1 if rs.rand() < 0.2 else rs.randint(2, 6),
                     [int(x) for x in rs.choice(pool, k, replace=False)])
                e += 1
        if step == frac_at:        # world, own, world on one sink at a fresh t: (r + 2) / 3
            t = t + 0.125
            for src in (2, 1, 3):
                post(e, src, [pool[0]])
                e += 1
            t = t + 0.125
    return pd.DataFrame.from_records(rows, columns=["event_id", "time_delta", "src_id", "t",
                                                    "sink_id"])


def gen_analysis_edges():
    """utils.oracle_ranking (utils.py:181-245) on synthetic single-follower walls whose n
    sits on rq_oracle_dp's wavefront / block widths, and utils.rank_of_src_in_df
    (:38-56) on frames at rq_rank_table's 64-column / 64-row boundaries."""
    rec, walls = {}, []
    rs = np.random.RandomState(20240607)
    base = SimOpts.std_poisson(world_seed=1, world_rate=100.0)

    def wall(key, times, end, qs, s):
        n = len(times)
        df = pd.DataFrame({"event_id": np.arange(100, 100 + n), "time_delta": np.zeros(n),
                           "src_id": np.full(n, 2), "t": times, "sink_id": np.full(n, 1001)})
        rec[key + "_t"] = np.asarray(times, dtype=np.float64)
        rec[key + "_end"] = np.asarray([end])
        rec[key + "_q"] = np.asarray(qs, dtype=np.float64)
        rec[key + "_s"] = np.asarray([s])
        for i, q in enumerate(qs):
            odf, cost = U.oracle_ranking(df=df, sim_opts=base.update({"q": q, "s": s,
                                                                      "end_time": end}))
            assert np.array_equal(odf.t.values[1:], times)
            rec["%s_%d_cost" % (key, i)] = np.asarray([cost])
            rec["%s_%d_events" % (key, i)] = odf.events.values.astype(np.int64)
            rec["%s_%d_ranks" % (key, i)] = odf.ranks.values.astype(np.int64)
        walls.append(key)

    for i, n in enumerate(EDGE_WALL_N):
        for zp in ([0.0, 0.2] if n in EDGE_WALL_ZERO_N else [0.0]):
            gaps = rs.exponential(0.01, n)
            gaps[rs.rand(n) < zp] = 0.0
            times = np.cumsum(gaps)
            s = [1.0, 2.5, 0.5][i % 3]
            # the first q posts every other event or so, the second rarely
            wall("w%d%s" % (n, "z" if zp else ""), times, float(times[-1]) + 0.5,
                 [0.01 * (1 + 0.3 * i), 1.0 + i], s)
            ev = rec["w%d%s_0_events" % (n, "z" if zp else "")]
            assert 0 < ev.sum() < n
    # every gap zero and q = 0: lhs == rhs in every cell the walk visits -> no post
    wall("wtie", np.zeros(65), 0.0, [0.0], 1.0)
    assert rec["wtie_0_events"].sum() == 0 and rec["wtie_0_ranks"][-1] == 65
    rec["walls"] = np.asarray(walls)

    frames = []
    for S, ne in ((1, 60), (63, 110), (64, 110), (65, 110), (129, 100)):
        key = "rt%d" % S
        df = edge_rank_frame(rs, S, ne)
        _df_cols(rec, key, df)
        for src in (1, -1):
            tab = U.rank_of_src_in_df(df, src)
            nof = U.rank_of_src_in_df(df, src, fill=False)
            rec["%s_%d" % (key, src + 1)] = tab.values
            rec["%s_%d_nofill" % (key, src + 1)] = nof.values
            own_nof = nof if src == 1 else own_nof
        rec[key + "_index"] = tab.index.values
        rec[key + "_cols"] = tab.columns.values.astype(np.int64)
        # what the frame must contain
        cell = df.groupby(["t", "sink_id"]).size()
        assert df.groupby("t").size().max() >= 100 and (cell == 2).any() and (cell == 3).any()
        tri = [own_nof.values[own_nof.index.get_loc(tt), own_nof.columns.get_loc(kk)] * 3
               for (tt, kk), c in cell.items() if c == 3]
        assert any(abs(x - round(x)) < 1e-9 and round(x) % 3 for x in tri)   # a k/3 cell
        assert df.src_id.values[0] == 1 and df.src_id.values[-1] == 1 and tab.shape[0] <= 200
        if S > 1:
            first = np.argmax(~np.isnan(nof.values), axis=0)
            assert first.max() >= (2 * tab.shape[0]) // 3
        frames.append(key)
    d65 = pd.DataFrame({c: rec["rt65_" + c] for c in ["event_id", "time_delta", "src_id", "t",
                                                      "sink_id"]})
    by_eid = U.rank_of_src_in_df(d65, 1, with_time=False)
    rec["rt65_eid_2"] = by_eid.values
    rec["rt65_eid_index"] = by_eid.index.values.astype(np.int64)
    # one unique t
    n1 = 40
    d1 = pd.DataFrame({"event_id": np.arange(100, 100 + n1), "time_delta": np.zeros(n1),
                       "src_id": np.where(rs.rand(n1) < 0.3, 1, 2), "t": np.full(n1, 3.5),
                       "sink_id": rs.choice([7, 8, 9, 11, 12], n1)})
    _df_cols(rec, "rt_one", d1)
    for src in (1, -1):
        rec["rt_one_%d" % (src + 1)] = U.rank_of_src_in_df(d1, src).values
        rec["rt_one_%d_nofill" % (src + 1)] = U.rank_of_src_in_df(d1, src, fill=False).values
    rec["rt_one_index"] = np.asarray([3.5])
    rec["rt_one_cols"] = np.unique(d1.sink_id.values).astype(np.int64)
    frames.append("rt_one")
    rec["frames"] = np.asarray(frames)
    path = os.path.join(HERE, "analysis_edges.npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) <= 1000000, os.path.getsize(path)


def gen_errors():
    """Reference behaviour on inputs where it does not compute what the engine would:
    u_int_opt with a SCALAR s (utils.py:78-81: .dot(scalar) keeps the [n_t, F] rank
    block and `u_values * u_dt` broadcasts: an [n_t, n_t] sum for one follower, an
    error for two) and OptPWSignificance on an event that reaches no follower with
    positive significance (take_one_sample: s_max = 0 -> int(nan), opt_model.py:557-566):
    an edge-less source, and a source whose only follower has zero significance."""
    rec = {}
    rd = SimOpts(**README)
    m = rd.create_manager_with_opt(seed=101)
    m.run_dynamic()
    df = m.state.get_dataframe()
    _df_cols(rec, "ui", df)
    rec["ui_scalar_f1"] = np.asarray([U.u_int_opt(df, src_id=1, end_time=100.0, s=1.0, q=2.0,
                                                  follower_ids=[1])])
    try:
        U.u_int_opt(df, src_id=1, end_time=100.0, s=1.0, q=2.0, follower_ids=[1, 3])
        rec["ui_scalar_f2_err"] = np.asarray(["none"])
    except Exception as e:
        rec["ui_scalar_f2_err"] = np.asarray([type(e).__name__])
    worlds = {
        "edgeless": (dict(src_id=1, end_time=20.0, q=1.0, s=np.asarray([1.0, 1.0]), sink_ids=[5001, 5002],
                          other_sources=[("Poisson2", {"src_id": 1000, "seed": 42, "rate": 10.0}),
                                         ("Poisson2", {"src_id": 1001, "seed": 43, "rate": 10.0})],
                          edge_list=[(1, 5001), (1, 5002), (1000, 5001)]), None),
        "zerosig": (dict(src_id=1, end_time=20.0, q=1.0, s=np.asarray([1.0, 1.0]), sink_ids=[5001, 5002],
                         other_sources=[("Poisson2", {"src_id": 1000, "seed": 42, "rate": 10.0}),
                                        ("Poisson2", {"src_id": 1001, "seed": 43, "rate": 10.0})],
                         edge_list=[(1, 5001), (1, 5002), (1000, 5001), (1001, 5002)]),
                    np.asarray([[1.0, 2.0, 1.0, 0.5], [0.0, 0.0, 0.0, 0.0]])),
        "ok": (dict(src_id=1, end_time=20.0, q=1.0, s=np.asarray([1.0, 1.0]), sink_ids=[5001, 5002],
                    other_sources=[("Poisson2", {"src_id": 1000, "seed": 42, "rate": 10.0}),
                                   ("Poisson2", {"src_id": 1001, "seed": 43, "rate": 10.0})],
                    edge_list=[(1, 5001), (1, 5002), (1000, 5001), (1001, 5002)]),
               np.asarray([[1.0, 2.0, 1.0, 0.5], [0.0, 1.0, 0.0, 0.0]])),
    }
    for name, (w, sig) in worlds.items():
        so = SimOpts(**w)
        m = so.create_manager_with_significance(3, time_period=10.0, significance=sig,
                                                num_segments=None if sig is not None else 4)
        try:
            m.run_dynamic()
            rec["sig_%s_err" % name] = np.asarray(["none"])
        except Exception as e:
            rec["sig_%s_err" % name] = np.asarray([type(e).__name__])
    # under a max_events cap run_dynamic stops before it hands the last event to the
    # controller (opt_model.py:271-281): a capped run whose LAST event is the first one
    # of the unreached source does not raise, one event more does
    so = SimOpts(**worlds["zerosig"][0])
    sig = worlds["zerosig"][1]
    m = so.create_manager_with_significance(3, time_period=10.0, significance=sig)
    try:
        m.run_dynamic()
    except ValueError:
        pass
    k = m.state.get_num_events() - 1   # the offending event was applied, then raised on
    rec["sig_cap_k"] = np.asarray([k])
    rec["sig_cap_k_src"] = np.asarray([m.state.events[k].src_id])
    for cap in (k + 1, k + 2):
        m = so.create_manager_with_significance(3, time_period=10.0, significance=sig)
        try:
            m.run_dynamic(max_events=cap)
            rec["sig_cap_%d_err" % (cap - k)] = np.asarray(["none"])
        except Exception as e:
            rec["sig_cap_%d_err" % (cap - k)] = np.asarray([type(e).__name__])
    np.savez_compressed(os.path.join(HERE, "errors.npz"), **rec)


from realdata_worlds import realdata_worlds  # noqa: E402  (plain data, shared with the tests)


def gen_realdata():
    rec = {}
    names = []
    for name, w, ctrl, maxev in realdata_worlds():
        so = SimOpts(**w)
        m = so.create_manager_with_times(np.asarray(ctrl))
        m.run_dynamic(max_events=maxev if maxev is not None else float("inf"))
        df = m.state.get_dataframe()
        _df_cols(rec, name, df)
        met, own, world = metrics(df, so)
        rec[name + "_met"] = met
        rec[name + "_cnt"] = np.asarray([own, world, len(df), m.state.get_num_events()])
        rec[name + "_state_time"] = np.asarray([m.state.time])
        names.append(name)
    np.savez_compressed(os.path.join(HERE, "realdata.npz"), names=np.asarray(names), **rec)


def gen_plugin():
    """A registered static broadcaster (SimOpts.registerSource, opt_model.py:768-771)
    in a deterministic world (RealData controlled): the df of the given seeds, and the
    metrics of randomize_other_sources(u) for u in 0..15."""
    from realdata_worlds import BurstyMixin, plugin_world
    from redqueen.opt_model import Broadcaster

    class Bursty(BurstyMixin, Broadcaster):
        pass
    SimOpts.registerSource("Bursty", Bursty)
    w, ctrl, us = plugin_world()
    so = SimOpts(**w)
    rec = {}
    m = so.create_manager_with_times(np.asarray(ctrl))
    m.run_dynamic()
    df = m.state.get_dataframe()
    _df_cols(rec, "base", df)
    met, own, world = metrics(df, so)
    rec["base_met"], rec["base_cnt"] = met, np.asarray([own, world, len(df)])
    mets, cnts = [], []
    for u in us:
        m = so.randomize_other_sources(u).create_manager_with_times(np.asarray(ctrl))
        m.run_dynamic()
        df = m.state.get_dataframe()
        met, own, world = metrics(df, so)
        mets.append(met)
        cnts.append([own, world, m.state.get_num_events()])
    rec["rand_met"], rec["rand_cnt"], rec["rand_u"] = np.asarray(mets), np.asarray(cnts), np.asarray(us)
    np.savez_compressed(os.path.join(HERE, "plugin.npz"), **rec)


def gen_dynplugin():
    """A registered DYNAMIC, self-driven broadcaster (Renewal: gamma gaps on its own
    events, None on the others') beside a static one, in a deterministic world (RealData
    controlled): the df of the given seeds, the metrics of randomize_other_sources(u) for
    u in 0..15; and the reference running a reactive dynamic plugin (KnockedOff) to the
    end (the engine refuses that one)."""
    from realdata_worlds import BurstyMixin, KnockedOffMixin, RenewalMixin, dyn_plugin_world
    from redqueen.opt_model import Broadcaster

    class Bursty(BurstyMixin, Broadcaster):
        pass

    class Renewal(RenewalMixin, Broadcaster):
        pass

    class KnockedOff(KnockedOffMixin, Broadcaster):
        pass
    SimOpts.registerSource("Bursty", Bursty)
    SimOpts.registerSource("Renewal", Renewal)
    SimOpts.registerSource("KnockedOff", KnockedOff)
    w, ctrl, us = dyn_plugin_world()
    so = SimOpts(**w)
    rec = {}
    m = so.create_manager_with_times(np.asarray(ctrl))
    m.run_dynamic()
    df = m.state.get_dataframe()
    _df_cols(rec, "base", df)
    met, own, world = metrics(df, so)
    rec["base_met"], rec["base_cnt"] = met, np.asarray([own, world, len(df)])
    mets, cnts = [], []
    for u in us:
        m = so.randomize_other_sources(u).create_manager_with_times(np.asarray(ctrl))
        m.run_dynamic()
        df = m.state.get_dataframe()
        met, own, world = metrics(df, so)
        mets.append(met)
        cnts.append([own, world, m.state.get_num_events()])
    rec["rand_met"], rec["rand_cnt"], rec["rand_u"] = np.asarray(mets), np.asarray(cnts), np.asarray(us)
    w2 = dict(w, other_sources=[("KnockedOff", {"src_id": 2, "seed": 21, "rate": 1.0})] + w["other_sources"][1:])
    so2 = SimOpts(**w2)
    m = so2.create_manager_with_times(np.asarray(ctrl))
    m.run_dynamic()
    rec["knocked_events"] = np.asarray([m.state.get_num_events()])
    # the reactive plugin's run: df + metrics, and randomize_other_sources(u) for u in us
    df = m.state.get_dataframe()
    _df_cols(rec, "knock", df)
    met, own, world = metrics(df, so2)
    rec["knock_met"], rec["knock_cnt"] = met, np.asarray([own, world, m.state.get_num_events()])
    mets, cnts = [], []
    for u in us:
        m = so2.randomize_other_sources(u).create_manager_with_times(np.asarray(ctrl))
        m.run_dynamic()
        df = m.state.get_dataframe()
        met, own, world = metrics(df, so2)
        mets.append(met)
        cnts.append([own, world, m.state.get_num_events()])
    rec["knock_rand_met"], rec["knock_rand_cnt"] = np.asarray(mets), np.asarray(cnts)
    np.savez_compressed(os.path.join(HERE, "dynplugin.npz"), **rec)


def gen_gridtie():
    """gridtie.npz: a reactive dynamic plugin whose posts meet static sources' times
    exactly (realdata_worlds.grid_tie_world): the reference's df of the seeded world and
    the metrics + counts of randomize_other_sources(u), u = 0..31."""
    from realdata_worlds import GridBurstyMixin, GridKnockMixin, grid_tie_world
    from redqueen.opt_model import Broadcaster

    class GridBursty(GridBurstyMixin, Broadcaster):
        pass

    class GridKnock(GridKnockMixin, Broadcaster):
        pass
    SimOpts.registerSource("GridBursty", GridBursty)
    SimOpts.registerSource("GridKnock", GridKnock)
    w, ctrl, us = grid_tie_world()
    so = SimOpts(**w)
    rec = {}
    m = so.create_manager_with_times(np.asarray(ctrl))
    m.run_dynamic()
    df = m.state.get_dataframe()
    _df_cols(rec, "base", df)
    met, own, world = metrics(df, so)
    rec["base_met"], rec["base_cnt"] = met, np.asarray([own, world, len(df)])
    mets, cnts, ties = [], [], []
    for u in us:
        m = so.randomize_other_sources(u).create_manager_with_times(np.asarray(ctrl))
        m.run_dynamic()
        df = m.state.get_dataframe()
        met, own, world = metrics(df, so)
        mets.append(met)
        cnts.append([own, world, m.state.get_num_events()])
        # equal-time events of the plugin (src 7) and a static source: the order under test
        g = df.groupby("event_id").first()
        t7 = set(g.t[g.src_id == 7])
        ties.append(sum(1 for t, s in zip(g.t, g.src_id) if s != 7 and t in t7))
    rec["rand_met"], rec["rand_cnt"], rec["rand_u"] = np.asarray(mets), np.asarray(cnts), np.asarray(us)
    rec["rand_ties"] = np.asarray(ties)
    np.savez_compressed(os.path.join(HERE, "gridtie.npz"), **rec)


KNOCK_SEED_STRIDE = 1000   # > 99 x the broadcaster count: no shared streams
KNOCK_OPT_SEED_OFFSET = 500


def _knock_worker(r):
    from realdata_worlds import BurstyMixin, KnockedOffMixin, dyn_plugin_world
    from redqueen.opt_model import Broadcaster

    class Bursty(BurstyMixin, Broadcaster):
        pass

    class KnockedOff(KnockedOffMixin, Broadcaster):
        pass
    SimOpts.registerSource("Bursty", Bursty)
    SimOpts.registerSource("KnockedOff", KnockedOff)
    w, _ctrl, _us = dyn_plugin_world()
    w2 = dict(w, other_sources=[("KnockedOff", {"src_id": 2, "seed": 21, "rate": 1.0})] +
              w["other_sources"][1:])
    so = SimOpts(**w2)
    u = KNOCK_SEED_STRIDE * r
    m = so.randomize_other_sources(u).create_manager_with_opt(seed=u + KNOCK_OPT_SEED_OFFSET)
    m.run_dynamic()
    df = m.state.get_dataframe()
    met, own, world = metrics(df, so)
    return np.concatenate([[own, world, m.state.get_num_events()], met])


def gen_knock_dist(n, procs=0):
    """The reactive plugin (KnockedOff: it reschedules when another source's event reaches
    its followers) beside the RedQueen broadcaster, whose posts react to the plugin's
    events in turn: replica r runs world randomize_other_sources(1000 r), RedQueen seed
    1000 r + 500, through the reference itself."""
    with mp.Pool(procs or os.cpu_count()) as pool:
        res = np.asarray(pool.map(_knock_worker, range(n), chunksize=16))
    cols = ["posts", "world", "events"] + ["top%d" % k for k in KS] + ["avg", "r2"]
    np.savez_compressed(os.path.join(HERE, "dist_knock.npz"), data=res, cols=np.asarray(cols),
                        seed_stride=np.asarray([KNOCK_SEED_STRIDE]),
                        opt_seed_offset=np.asarray([KNOCK_OPT_SEED_OFFSET]))


def gen_sig():
    """OptPWSignificance (opt_model.py:547-623) via create_manager_with_significance
    (:850-884): the notebook cells opt_broadcast.ipynb:5469 and :5569 plus variants."""
    rec = {}
    so3 = SimOpts(s=np.asarray([1.0, 1.0]), **KAT_BASE)
    so5 = SimOpts(s=np.asarray([0.5, 1.5]), **KAT_BASE)
    runs = {"s1": (so3, 1, 10.0, 24, None), "s41": (so5, 41, 10.0, 24, None),
            "s7": (so5, 7, 25.0, 5, None)}
    num_segs = 24
    sig = np.square(np.sin(np.arange(0, num_segs, step=1.0) * 4 * np.pi / num_segs))
    sig = (sig / sig.sum()).reshape((1, -1))
    so_sig = SimOpts(src_id=1, s=1.0, q=1.0, end_time=20.0,
                     other_sources=[("Poisson2", {"src_id": 1000, "seed": 42, "rate": 50.0})],
                     sink_ids=[5001], edge_list=[(1, 5001), (1000, 5001)])
    runs["sig"] = (so_sig, 10, so_sig.end_time, None, sig)
    for key, (so_, seed, period, nseg, signif) in runs.items():
        m = so_.create_manager_with_significance(seed, time_period=period, significance=signif,
                                                 num_segments=nseg)
        sig_used = np.asarray(m.sources[0].s_pw, dtype=np.float64)
        m.run_dynamic()
        df = m.state.get_dataframe()
        rec[key + "_t"], rec[key + "_dt"], rec[key + "_src"] = events_of(df)
        met, own, world = metrics(df, so_)
        rec[key + "_met"] = met
        rec[key + "_cnt"] = np.asarray([own, world, len(df), df.shape[1]])
        rec[key + "_sig"] = sig_used
        rec[key + "_par"] = np.asarray([seed, period, float(so_.q)])
    np.savez_compressed(os.path.join(HERE, "sig_runs.npz"), **rec)


# OptPWSignificance ensemble: the K3 network with a follower- and phase-dependent
# significance (24 segments of a period 10), worlds randomize_other_sources(r), seed r
SIG_SEGS = 24


def sig_matrix():
    k = np.arange(SIG_SEGS)
    return np.stack([0.2 + np.sin(np.pi * k / SIG_SEGS) ** 2,
                     1.5 * (0.1 + np.cos(2 * np.pi * k / SIG_SEGS) ** 2)])


def _sig_worker(r):
    so = SimOpts(s=np.asarray([1.0, 1.0]), **KAT_BASE)
    w = so.randomize_other_sources(r)
    m = w.create_manager_with_significance(r, time_period=10.0, significance=sig_matrix())
    m.run_dynamic()
    df = m.state.get_dataframe()
    met, own, world = metrics(df, so)
    return np.concatenate([[own, world, m.state.get_num_events()], met])


def gen_sig_dist(n):
    with mp.Pool(os.cpu_count()) as pool:
        res = np.asarray(pool.map(_sig_worker, range(n), chunksize=16))
    cols = ["posts", "world", "events"] + ["top%d" % k for k in KS] + ["avg", "r2"]
    np.savez_compressed(os.path.join(HERE, "dist_sig.npz"), data=res, cols=np.asarray(cols),
                        sig=sig_matrix())


C3_SEED_STRIDE = 5000


def _c3_worker(r):
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from redqueen_amd import graphs as G
    d = G.c3()
    so = SimOpts(**d)
    u = C3_SEED_STRIDE * r   # disjoint seed sets per replica (50 sources x 99 < 5000)
    w = so.randomize_other_sources(u)
    m = w.create_manager_with_opt(seed=u)
    m.run_dynamic()
    df = m.state.get_dataframe()
    top = U.time_in_top_k(df=df, K=1, sim_opts=so)
    avg = U.average_rank(df, sim_opts=so)
    own = len(df.event_id[df.src_id == so.src_id].unique())
    world = len(df.event_id[df.src_id != so.src_id].unique())
    return np.asarray([own, world, m.state.get_num_events(), top, avg])


def gen_c3_dist(n, start=0, procs=0):
    """C3 (the bench network) through the reference itself: n replicas, replica r runs
    world randomize_other_sources(5000 r) and RedQueen seed 5000 r, so no two replicas
    share a source stream (~41 s per replica per core).  start > 0 appends replicas
    start .. start + n - 1 to the existing file (which must hold exactly start rows)."""
    path = os.path.join(HERE, "dist_c3.npz")
    with mp.Pool(procs or os.cpu_count()) as pool:
        res = np.asarray(pool.map(_c3_worker, range(start, start + n), chunksize=1))
    if start:
        old = np.load(path)["data"]
        assert old.shape[0] == start, (old.shape, start)
        res = np.concatenate([old, res])
    tmp = path + ".tmp.npz"   # written whole, then renamed: a reader never sees half a file
    np.savez_compressed(tmp, data=res,
                        cols=np.asarray(["posts", "world", "events", "top1", "avg"]),
                        seed_stride=np.asarray([C3_SEED_STRIDE]))
    os.replace(tmp, path)


# Reference runs at the headline scale, kept whole: the event log (t, time_delta, src),
# the df's shape and column checksums, and what utils.py returns on that df.  C3 replica r
# is dist_c3's replica r (world randomize_other_sources(5000 r), RedQueen seed 5000 r);
# c5_mid replica r runs world randomize_other_sources(100000 r), RedQueen seed 100000 r + 1.
SCALE_RUNS = {"c3": (8, C3_SEED_STRIDE, 0), "c5m": (2, 100000, 1)}


def _crc(a):
    import zlib
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def _scale_worker(args):
    name, r = args
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from redqueen_amd import graphs as G
    so = SimOpts(**(G.c3() if name == "c3" else G.c5_mid()))
    _, stride, off = SCALE_RUNS[name]
    u = stride * r
    m = so.randomize_other_sources(u).create_manager_with_opt(seed=u + off)
    m.run_dynamic()
    df = m.state.get_dataframe()
    met, own, world = metrics(df, so)
    t, dt, src = events_of(df)
    shape = np.asarray([len(df), own, world, m.state.get_num_events(), df.sink_id.nunique()],
                       dtype=np.int64)
    crc = np.asarray([_crc(df.t.values), _crc(df.src_id.values.astype(np.int64)),
                      _crc(df.sink_id.values.astype(np.int64)),
                      _crc(df.event_id.values.astype(np.int64))], dtype=np.int64)
    return name, r, t, dt, src, met, shape, crc


def gen_scale_logs(procs=0):
    """scale_logs.npz: SCALE_RUNS through the reference, every event's (t, src_id) kept (the tests
    rebuild the df with the reference's row layout, check it against the recorded shape
    and crc32 of each column, and replay it)."""
    jobs = [(n, r) for n, (cnt, _, _) in SCALE_RUNS.items() for r in range(cnt)]
    jobs.sort(key=lambda j: j[0] != "c5m")   # the long runs first
    rec = {}
    with mp.Pool(procs or os.cpu_count()) as pool:
        for name, r, t, dt, src, met, shape, crc in pool.imap_unordered(_scale_worker, jobs):
            k = "%s_%d" % (name, r)
            # time_delta is not a metric input: the tests rebuild the df without it
            rec.update({k + "_t": t, k + "_src": src.astype(np.int32), k + "_met": met,
                        k + "_shape": shape, k + "_crc": crc})
            print("scale run", k, shape.tolist(), flush=True)
    rec["runs"] = np.asarray(sorted("%s_%d" % j for j in jobs))
    rec["shape_cols"] = np.asarray(["rows", "own", "world", "events", "sinks"])
    rec["crc_cols"] = np.asarray(["t", "src_id", "sink_id", "event_id"])
    np.savez_compressed(os.path.join(HERE, "scale_logs.npz"), **rec)


C5M_SEED_STRIDE = 100000   # > 99 x the 500 broadcasters: no shared streams
C5M_OPT_SEED_OFFSET = 77777


def _c5m_worker(r):
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from redqueen_amd import graphs as G
    so = SimOpts(**G.c5_mid())
    u = C5M_SEED_STRIDE * (r + 1000)   # disjoint from scale_logs' c5m runs (r = 0, 1)
    m = so.randomize_other_sources(u).create_manager_with_opt(seed=u + C5M_OPT_SEED_OFFSET)
    m.run_dynamic()
    df = m.state.get_dataframe()
    met, own, world = metrics(df, so)
    return np.concatenate([[own, world, m.state.get_num_events()], met])


def gen_c5m_dist(n, start=0, procs=0):
    """graphs.c5_mid (C5's 500 bursty Hawkes broadcasters at T = 1000, 100 followers)
    through the reference itself (~8 min per replica per core): replica r runs world
    randomize_other_sources(100000 (r + 1000)) and RedQueen seed that + 77777.  start > 0
    appends to dist_c5m.npz (which must hold exactly start rows)."""
    path = os.path.join(HERE, "dist_c5m.npz")
    with mp.Pool(procs or os.cpu_count()) as pool:
        res = np.asarray(pool.map(_c5m_worker, range(start, start + n), chunksize=1))
    if start:
        old = np.load(path)["data"]
        assert old.shape[0] == start, (old.shape, start)
        res = np.concatenate([old, res])
    cols = ["posts", "world", "events"] + ["top%d" % k for k in KS] + ["avg", "r2"]
    tmp = path + ".tmp.npz"
    np.savez_compressed(tmp, data=res, cols=np.asarray(cols),
                        seed_stride=np.asarray([C5M_SEED_STRIDE]), seed_base=np.asarray([1000]),
                        opt_seed_offset=np.asarray([C5M_OPT_SEED_OFFSET]))
    os.replace(tmp, path)


# C4 corners: README graph at the extreme q of the reference's grid (opt_runs.py:289-291)
# x three follower-significance vectors (the notebook's sim_opts_unequal (0.5, 1.5),
# opt_broadcast.ipynb:5550, and a strongly unequal (1, 0.25)).  Replica r runs world
# randomize_other_sources(200 r) (seeds 200 r, 200 r + 99) and RedQueen seed 200 r + 50:
# no stream is shared between replicas or between the controller and a wall source.
C4_CORNER_Q = [1e-4, 1e7]
C4_CORNER_S = [(1.0, 1.0), (0.5, 1.5), (1.0, 0.25)]
C4_SEED_STRIDE = 200
C4_OPT_SEED_OFFSET = 50


def c4_corners():
    return [(q, s) for q in C4_CORNER_Q for s in C4_CORNER_S]


def _c4_worker(args):
    p, r = args
    q, s = c4_corners()[p]
    kw = dict(README)
    kw.update(q=q, s=np.asarray(s, dtype=float))
    so = SimOpts(**kw)
    u = C4_SEED_STRIDE * r
    m = so.randomize_other_sources(u).create_manager_with_opt(seed=u + C4_OPT_SEED_OFFSET)
    m.run_dynamic()
    df = m.state.get_dataframe()
    met, own, world = metrics(df, so)
    return np.concatenate([[own, world, m.state.get_num_events()], met])


def gen_c4_dist(n, start=0, procs=0):
    """The reference's ensembles at the six C4 corners (c4_corners()): n replicas per
    point, appended to dist_c4.npz from replica `start` (which must be the file's
    current count), data[point, replica, col]."""
    path = os.path.join(HERE, "dist_c4.npz")
    pts = len(c4_corners())
    jobs = [(p, r) for r in range(start, start + n) for p in range(pts)]
    with mp.Pool(procs or os.cpu_count()) as pool:
        res = np.asarray(pool.map(_c4_worker, jobs, chunksize=8))
    res = res.reshape(n, pts, -1).transpose(1, 0, 2)
    if start:
        old = np.load(path)["data"]
        assert old.shape[1] == start, (old.shape, start)
        res = np.concatenate([old, res], axis=1)
    cols = ["posts", "world", "events"] + ["top%d" % k for k in KS] + ["avg", "r2"]
    tmp = path + ".tmp.npz"
    np.savez_compressed(tmp, data=res, cols=np.asarray(cols),
                        q=np.asarray([q for q, _ in c4_corners()]),
                        s=np.asarray([s for _, s in c4_corners()]),
                        seed_stride=np.asarray([C4_SEED_STRIDE]),
                        opt_seed_offset=np.asarray([C4_OPT_SEED_OFFSET]))
    os.replace(tmp, path)


C5S_SEED_STRIDE = 1000     # > 99 x the 4 broadcasters: no shared streams
C5S_OPT_SEED_OFFSET = 900  # the controller's RandomState differs from every wall source's


def _c5s_worker(r):
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from redqueen_amd import graphs as G
    so = SimOpts(**G.c5_small())
    u = C5S_SEED_STRIDE * r
    m = so.randomize_other_sources(u).create_manager_with_opt(seed=u + C5S_OPT_SEED_OFFSET)
    m.run_dynamic()
    df = m.state.get_dataframe()
    met, own, world = metrics(df, so)
    return np.concatenate([[own, world, m.state.get_num_events()], met])


def gen_c5s_dist(n, start=0, procs=0):
    """graphs.c5_small (C5's Hawkes l_0 0.5 / alpha 1 / beta 2 at T = 1000 on 4 followers)
    through the reference itself: replica r runs world randomize_other_sources(1000 r) and
    RedQueen seed 1000 r + 900.  start > 0 appends to dist_c5s.npz (which must hold exactly
    start rows)."""
    path = os.path.join(HERE, "dist_c5s.npz")
    with mp.Pool(procs or os.cpu_count()) as pool:
        res = np.asarray(pool.map(_c5s_worker, range(start, start + n), chunksize=4))
    if start:
        old = np.load(path)["data"]
        assert old.shape[0] == start, (old.shape, start)
        res = np.concatenate([old, res])
    cols = ["posts", "world", "events"] + ["top%d" % k for k in KS] + ["avg", "r2"]
    tmp = path + ".tmp.npz"
    np.savez_compressed(tmp, data=res, cols=np.asarray(cols),
                        seed_stride=np.asarray([C5S_SEED_STRIDE]),
                        opt_seed_offset=np.asarray([C5S_OPT_SEED_OFFSET]))
    os.replace(tmp, path)


G120_SEED_STRIDE = 20000   # > 99 x the broadcaster count: no shared streams


def _g120_worker(r):
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from redqueen_amd import graphs as G
    so = SimOpts(**G.g120())
    u = G120_SEED_STRIDE * r
    m = so.randomize_other_sources(u).create_manager_with_opt(seed=u)
    m.run_dynamic()
    df = m.state.get_dataframe()
    met, own, world = metrics(df, so)
    return np.concatenate([[own, world, m.state.get_num_events()], met])


def gen_g120_dist(n, procs=0):
    """graphs.g120 (> 64 sources: the general sweep) through the reference itself:
    replica r runs world randomize_other_sources(20000 r), RedQueen seed 20000 r."""
    with mp.Pool(procs or os.cpu_count()) as pool:
        res = np.asarray(pool.map(_g120_worker, range(n), chunksize=4))
    cols = ["posts", "world", "events"] + ["top%d" % k for k in KS] + ["avg", "r2"]
    np.savez_compressed(os.path.join(HERE, "dist_g120.npz"), data=res, cols=np.asarray(cols),
                        seed_stride=np.asarray([G120_SEED_STRIDE]))


# ---------------------------------------------------------------- ensembles
def _c2_worker(r):
    so = SimOpts(**README)
    w = so.randomize_other_sources(r)
    m = w.create_manager_with_opt(seed=r)
    m.run_dynamic()
    df = m.state.get_dataframe()
    met, own, world = metrics(df, so)
    n_ev = m.state.get_num_events()
    # comparator seed r + 10**6: with seed r the controlled Poisson2 would share
    # RandomState(r) with world source 0 (randomize_other_sources gives idx 0 seed r) and
    # draw the same uniforms -- its posts would coincide with that source's posts
    m2 = w.create_manager_with_poisson(seed=r + POISSON_SEED_OFFSET, capacity=float(own))
    m2.run_dynamic()
    df2 = m2.state.get_dataframe()
    met2, own2, world2 = metrics(df2, so)
    return np.concatenate([[own, world, n_ev], met, [own2, world2, m2.state.get_num_events()],
                           met2])


def _world_worker(args):
    name, r = args
    so = WORLDS[name]
    w = so.randomize_other_sources(r)
    m = w.create_manager_for_wall()
    m.run_dynamic()
    df = m.state.get_dataframe()
    counts = [int(np.sum(df.groupby("event_id").first().src_id.values == x["src_id"]))
              for _, x in so.other_sources]
    met, own, world = metrics(df, so)
    return np.concatenate([counts, met])


WORLDS = {
    "hawkes": SimOpts(src_id=1, end_time=50.0, s=1.0, q=1.0, sink_ids=[1, 2],
                      other_sources=[("Hawkes", {"src_id": 2, "seed": 0, "l_0": 2.0,
                                                 "alpha": 1.0, "beta": 2.0}),
                                     ("Hawkes", {"src_id": 3, "seed": 0, "l_0": 5.0,
                                                 "alpha": 2.0, "beta": 10.0})],
                      edge_list=[(2, 1), (3, 1), (3, 2)]),
    "pwconst": SimOpts(src_id=1, end_time=60.0, s=1.0, q=1.0, sink_ids=[1, 2],
                       other_sources=[("PiecewiseConst", {"src_id": 2, "seed": 0,
                                                          "change_times": [0.0, 20.0, 45.0],
                                                          "rates": [3.0, 0.5, 6.0]}),
                                      ("Poisson", {"src_id": 3, "seed": 0, "rate": 4.0}),
                                      ("Poisson2", {"src_id": 4, "seed": 0, "rate": 2.5})],
                       edge_list=[(2, 1), (3, 2), (4, 1), (4, 2)]),
}


def gen_dist(n, worlds=True):
    with mp.Pool(os.cpu_count()) as pool:
        res = np.asarray(pool.map(_c2_worker, range(n), chunksize=16))
    cols = (["opt_posts", "opt_world", "opt_events"] + ["opt_top%d" % k for k in KS] +
            ["opt_avg", "opt_r2", "poi_posts", "poi_world", "poi_events"] +
            ["poi_top%d" % k for k in KS] + ["poi_avg", "poi_r2"])
    np.savez_compressed(os.path.join(HERE, "dist_c2.npz"), data=res, cols=np.asarray(cols),
                        poisson_seed_offset=np.asarray([POISSON_SEED_OFFSET]))
    if not worlds:
        return
    gen_worlds(n)


# (replicas, first seed) per world: seeds u = seed0 + r feed randomize_other_sources(u),
# i.e. source idx k gets seed u + 99 k, so replicas r and r + 99 share a stream and the
# test uses a cluster-robust variance (clusters r mod 99).  The Hawkes ensemble is
# larger (30k, seed0 3e6): a 10k draw at seed0 0 sat 3 sd off the engine's mean.
WORLD_SAMPLES = {"hawkes": (30000, 3_000_000), "pwconst": (10000, 0)}


def gen_hawkes_seed0(procs=0):
    """The 10k-replica Hawkes world draw at seed0 0 that round 1 replaced by the 30k draw
    at seed0 3e6 (WORLD_SAMPLES): regenerated so the test can state its z under the
    cluster-robust variance (dist_hawkes0.npz, same columns as dist_world's hawkes)."""
    with mp.Pool(procs or os.cpu_count()) as pool:
        res = np.asarray(pool.map(_world_worker, [("hawkes", r) for r in range(10000)],
                                  chunksize=16)).astype(np.float32)
    np.savez_compressed(os.path.join(HERE, "dist_hawkes0.npz"), hawkes=res,
                        hawkes_seed0=np.asarray([0]))


def gen_worlds(n=0):
    rec = {}
    for name in WORLDS:
        cnt, seed0 = WORLD_SAMPLES[name]
        if n:
            cnt = n
        with mp.Pool(os.cpu_count()) as pool:
            rec[name] = np.asarray(pool.map(_world_worker, [(name, seed0 + r) for r in range(cnt)],
                                            chunksize=16)).astype(np.float32)
        rec[name + "_seed0"] = np.asarray([seed0])
    np.savez_compressed(os.path.join(HERE, "dist_world.npz"), **rec)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dist", type=int, default=0)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-worlds", action="store_true")
    ap.add_argument("--worlds", action="store_true", help="only dist_world.npz")
    ap.add_argument("--sig-dist", type=int, default=0, help="only dist_sig.npz with N replicas")
    ap.add_argument("--c3-dist", type=int, default=0, help="only dist_c3.npz with N replicas")
    ap.add_argument("--c3-start", type=int, default=0, help="append to dist_c3.npz from this replica")
    ap.add_argument("--procs", type=int, default=0)
    ap.add_argument("--g120-dist", type=int, default=0, help="only dist_g120.npz with N replicas")
    ap.add_argument("--c4-dist", type=int, default=0, help="only dist_c4.npz: N more replicas")
    ap.add_argument("--c4-start", type=int, default=0, help="append to dist_c4.npz from here")
    ap.add_argument("--c5s-dist", type=int, default=0, help="only dist_c5s.npz: N more replicas")
    ap.add_argument("--c5s-start", type=int, default=0, help="append to dist_c5s.npz from here")
    ap.add_argument("--knock-dist", type=int, default=0,
                    help="only dist_knock.npz: N reference runs of the reactive plugin beside RedQueen")
    ap.add_argument("--hawkes-seed0", action="store_true",
                    help="only dist_hawkes0.npz: the discarded 10k seed0-0 Hawkes world draw")
    ap.add_argument("--c5m-dist", type=int, default=0, help="only dist_c5m.npz: N more replicas")
    ap.add_argument("--c5m-start", type=int, default=0, help="append to dist_c5m.npz from here")
    ap.add_argument("--scale-logs", action="store_true",
                    help="only scale_logs.npz: whole reference runs of C3 and c5_mid")
    ap.add_argument("--analysis-edges", action="store_true",
                    help="only analysis_edges.npz: oracle walls and rank tables at kernel edges")
    a = ap.parse_args()
    steps = {"npsum": gen_npsum, "draws": gen_draws, "readme": gen_readme, "kats": gen_kats,
             "adv": gen_adversarial, "graphs": gen_graphs, "frac": gen_frac,
             "oracle": gen_oracle, "sweepq": gen_sweepq, "sig": gen_sig, "realdata": gen_realdata,
             "plugin": gen_plugin, "errors": gen_errors, "dynplugin": gen_dynplugin,
             "gridtie": gen_gridtie}
    if a.analysis_edges:
        gen_analysis_edges()
        print("done analysis edges", flush=True)
        a.worlds = True   # nothing else
    elif a.c5m_dist:
        gen_c5m_dist(a.c5m_dist, a.c5m_start, a.procs)
        print("done c5m dist", flush=True)
        a.worlds = True   # nothing else
    elif a.scale_logs:
        gen_scale_logs(a.procs)
        print("done scale logs", flush=True)
        a.worlds = True   # nothing else
    elif a.c4_dist:
        gen_c4_dist(a.c4_dist, a.c4_start, a.procs)
        print("done c4 dist", flush=True)
        a.worlds = True   # nothing else
    elif a.c5s_dist:
        gen_c5s_dist(a.c5s_dist, a.c5s_start, a.procs)
        print("done c5s dist", flush=True)
        a.worlds = True   # nothing else
    elif a.knock_dist:
        gen_knock_dist(a.knock_dist, a.procs)
        print("done knock dist", flush=True)
        a.worlds = True   # nothing else
    elif a.hawkes_seed0:
        gen_hawkes_seed0(a.procs)
        print("done hawkes seed0", flush=True)
        a.worlds = True   # nothing else
    elif a.g120_dist:
        gen_g120_dist(a.g120_dist, a.procs)
        print("done g120 dist", flush=True)
        a.worlds = True   # nothing else
    elif a.c3_dist:
        gen_c3_dist(a.c3_dist, a.c3_start, a.procs)
        print("done c3 dist", flush=True)
        a.worlds = True   # nothing else
    elif a.sig_dist:
        gen_sig_dist(a.sig_dist)
        print("done sig dist", flush=True)
        a.worlds = True   # nothing else
    elif a.worlds:
        gen_worlds()
        print("done worlds", flush=True)
    for k, f in steps.items():
        if a.worlds:
            break
        if not a.only or k in a.only.split(","):
            f()
            print("done", k, flush=True)
    if a.dist:
        gen_dist(a.dist, worlds=not a.no_worlds)
        print("done dist", flush=True)
    with open(os.path.join(HERE, "README.md"), "w") as fh:
        fh.write(__doc__)

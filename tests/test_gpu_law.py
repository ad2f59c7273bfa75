"""The law of every arrival stream and of the controller's posts on the GPU, checked
directly by time rescaling (tests/lawcheck.py): the compensator increments of each
process, rebuilt in float64 numpy from the event log and the user-visible parameters
alone, must be iid Exp(1).  Unlike the bit-exact parity tests (which share rq_spec.h and
the generator rules with the oracle) and the end-of-run ensembles, this sees a wrong
inter-arrival structure directly: ~1e6 increments per world resolve a 1 % error in a
Hawkes parameter ("Law tests").

Every test holds its whole family of statistics to a false-alarm level of 1e-3
(Bonferroni); seeds are fixed (replica r: STRIDE * r + c, disjoint streams), so the
outcome is deterministic.  The ``analyse_*`` functions take logs from anywhere: the
same inputs were driven through the CPU oracle (engine law) and, for the bursty and
README worlds, through the MT19937 restatement of the reference (reference law) before
they ran here.
"""
import numpy as np
import pytest

import lawcheck as LC
from redqueen_amd import graphs

pytestmark = pytest.mark.gpu
STRIDE = 100003


# --------------------------------------------------------------------------- worlds
EDGES_START = 20.0


def edges_world():
    """One source from each regime no other test visits; 2 sinks, T = 200 from
    start_time = EDGES_START: the engine, like the reference (opt_model.py:644), refuses a
    PiecewiseConst source whose first change time is not the start time."""
    return dict(
        src_id=1, end_time=220.0, q=4.0, s=np.asarray([1.0, 1.0]), sink_ids=[10, 11],
        other_sources=[
            # decay argument -beta * gap below -745: exp underflows (rq_exp_special)
            ("Hawkes", {"src_id": 2, "seed": 11, "l_0": 2.0, "alpha": 50.0, "beta": 1e4}),
            ("Hawkes", {"src_id": 3, "seed": 12, "l_0": 2.0, "alpha": 0.0, "beta": 1.0}),
            # branching ratio 0.9, memory 1 / beta = 20
            ("Hawkes", {"src_id": 4, "seed": 13, "l_0": 2.0, "alpha": 0.045, "beta": 0.05}),
            ("Hawkes", {"src_id": 5, "seed": 14, "l_0": 0.0, "alpha": 1.0, "beta": 2.0}),
            # a zero-rate segment, a half-unit spike, a first change time above 0
            ("PiecewiseConst", {"src_id": 6, "seed": 15, "change_times": [20.0, 50.0, 50.5, 120.0],
                                "rates": [3.0, 0.0, 40.0, 0.5]}),
            ("Poisson2", {"src_id": 7, "seed": 16, "rate": 0.01}),
            ("Poisson", {"src_id": 8, "seed": 17, "rate": 5.0})],
        edge_list=[(1, 10), (1, 11), (2, 10), (3, 11), (4, 10), (5, 11), (6, 10), (6, 11),
                   (7, 11), (8, 10)])


def wide_world():
    """80 sources (> 64: the general sweep on merged streams): 40 Poisson2 at rate 2 and
    40 Hawkes at branching 0.5 with stationary rate 2, each on one of 8 sinks; T = 100, so
    every source expects >= 200 arrivals."""
    others, edges = [], [(1, 100 + f) for f in range(8)]
    for k in range(80):
        sid = 1000 + k
        if k < 40:
            others.append(("Poisson2", {"src_id": sid, "seed": 50 + k, "rate": 2.0}))
        else:
            others.append(("Hawkes", {"src_id": sid, "seed": 50 + k, "l_0": 1.0, "alpha": 1.0,
                                      "beta": 2.0}))
        edges.append((sid, 100 + k % 8))
    return dict(src_id=1, end_time=100.0, q=64.0, s=np.ones(8), sink_ids=[100 + f for f in range(8)],
                other_sources=others, edge_list=edges)


SIG_S_PW = np.asarray([[1.0, 0.0, 0.5],     # follower 1
                       [2.0, 0.0, 0.0]])    # follower 3: segment 1 is zero for everyone
SIG_PERIOD = 10.0
OPT_GRID_Q = [1e-2, 1.0, 1e3]
OPT_GRID_S = [(1.0, 1.0), (0.5, 1.5)]
CTRL_RATES = [0.0, 0.5, 4.0, 9.5]


def seeds(R, c):
    """Replica r: seed STRIDE * r + c (controller) and + 99 idx for other source idx."""
    return np.arange(R, dtype=np.int64) * STRIDE + c


def seeded(so, u):
    """randomize_other_sources(u) (opt_model.py:795-804)."""
    return dict(so, other_sources=[(n, dict(kw, seed=(int(u) + 99 * i) & 0xFFFFFFFF))
                                   for i, (n, kw) in enumerate(so["other_sources"])])


# --------------------------------------------------------------------------- analyses
def _hawkes_rate(kw, T):
    """Mean count of a Hawkes source over [0, T] from rest (the mean-intensity ODE)."""
    l0, n, b = kw["l_0"], kw["alpha"] / kw["beta"], kw["beta"]
    g = (1.0 - n) * b
    return l0 * T / (1.0 - n) - l0 * n / (1.0 - n) * (-np.expm1(-g * T)) / g


def analyse_edges(logs, so, name="edges", start=EDGES_START):
    """Per source (every regime on its own): fixed-m + count where arrivals are
    plentiful, count + conditional-uniform KS for the rate 0.01 source."""
    LC.check_support(logs, so, start=start)
    T, R = so["end_time"] - start, logs.R
    procs = LC.world(logs, so, start)
    fam = LC.Family(name)
    for kind, kw in so["other_sources"]:
        p = procs[kw["src_id"]]
        if kind == "Hawkes" and kw["l_0"] == 0.0:
            continue                                    # check_support: no arrivals at all
        if kind == "Hawkes":
            # at least the Poisson(l_0 T) immigrants arrive; at most half the expected count
            m = min(LC.poisson_m(kw["l_0"] * T, R), int(_hawkes_rate(kw, T) / 2))
        elif kind == "PiecewiseConst":
            m = LC.poisson_m(LC.pw_integral(so["end_time"], kw["change_times"], kw["rates"], start), R)
        else:
            m = LC.poisson_m(kw["rate"] * T, R)
        if m >= 20:
            fam.fixed_m(p.name, p, m)
        else:
            fam.p(p.name + " uniform", LC.uniform_ks(p)[1])
        fam.martingale(p.name, p)
    c = LC.controller(logs, so, ("opt", 0), start=start)
    fam.fixed_m("opt", c, 300)      # ~ 690 posts per replica (fewest: 635)
    fam.martingale("opt", c)
    return fam


def analyse_bursty(logs, so, name="bursty"):
    """graphs.c5_small: the four identical Hawkes sources pooled, m = 500 = half the
    expected count (stationary rate 1, T = 1000; the count's sd is ~ 63), and the
    controller (~ 960 posts per replica, m = 400)."""
    LC.check_support(logs, so)
    procs = list(LC.world(logs, so).values())
    fam = LC.Family(name)
    fam.fixed_m("Hawkes", procs, 500)
    fam.martingale("Hawkes", procs)
    c = LC.controller(logs, so, ("opt", 0))
    fam.fixed_m("opt", c, 400)
    fam.martingale("opt", c)
    return fam


def analyse_wide(logs, so, name="wide"):
    LC.check_support(logs, so)
    procs = LC.world(logs, so)
    poi = [procs[kw["src_id"]] for k, kw in so["other_sources"] if k == "Poisson2"]
    haw = [procs[kw["src_id"]] for k, kw in so["other_sources"] if k == "Hawkes"]
    fam = LC.Family(name)
    fam.fixed_m("Poisson2", poi, LC.poisson_m(200.0, logs.R * len(poi)))
    fam.martingale("Poisson2", poi)
    fam.fixed_m("Hawkes", haw, 100)                     # half the expected 200
    fam.martingale("Hawkes", haw)
    c = LC.controller(logs, so, ("opt", 0))
    fam.fixed_m("opt", c, 150)                          # ~ 355 posts per replica (fewest: 326)
    fam.martingale("opt", c)
    return fam


# m by q on the README graph at T = 100: at most half the mean posts per replica
# (~ 1080 / 415 / 79; the fewest in any replica: 994 / 375 / 64)
OPT_GRID_M = {1e-2: 500, 1.0: 200, 1e3: 30}


def opt_grid(n_rep):
    """(q [P], s [P, 2]) of the grid and the per-replica sim_opts rows (replica i = g * n_rep + r)."""
    qs = np.repeat(OPT_GRID_Q, len(OPT_GRID_S)).astype(np.float64)
    sm = np.asarray(OPT_GRID_S * len(OPT_GRID_Q), dtype=np.float64)
    return qs, sm, np.repeat(qs, n_rep), np.repeat(sm, n_rep, axis=0)


def analyse_opt_grid(logs, so, n_rep, name="opt grid"):
    qs, sm, q_rep, s_rep = opt_grid(n_rep)
    LC.check_support(logs, so)
    c = LC.controller(logs, dict(so, q=q_rep, s=s_rep), ("opt", 0))
    fam = LC.Family(name)
    for g in range(len(qs)):
        rows = slice(g * n_rep, (g + 1) * n_rep)
        p = LC.Proc("opt q=%g s=(%g, %g)" % (qs[g], sm[g, 0], sm[g, 1]), c.inc[rows], c.n[rows], c.tail[rows])
        fam.fixed_m(p.name, p, OPT_GRID_M[float(qs[g])])
        fam.martingale(p.name, p)
    return fam


def analyse_poisson_ctrl(logs, so, rates, name="poisson ctrl"):
    ctrl = ("poisson", 0, rates)
    LC.check_support(logs, so, ctrl)
    c = LC.controller(logs, so, ctrl)
    fam = LC.Family(name)
    for rate in sorted(set(rates.tolist())):
        rows = np.flatnonzero(rates == rate)
        p = LC.Proc("poisson %g" % rate, c.inc[rows], c.n[rows], c.tail[rows])
        if rate == 0.0:
            assert int(p.n.sum()) == 0 and float(p.total.sum()) == 0.0
            continue
        m = LC.poisson_m(rate * so["end_time"], len(rows))
        if m >= 20:
            fam.fixed_m(p.name, p, m)
        else:
            fam.p(p.name + " uniform", LC.uniform_ks(p)[1])
        fam.martingale(p.name, p)
    return fam


def analyse_sig(logs, so, name="sig"):
    ctrl = ("sig", 0, SIG_S_PW, SIG_PERIOD)
    LC.check_support(logs, so)
    # no own post where every follower's significance is zero
    own = logs.t[logs.src == so["src_id"]]
    seg = np.minimum((3 * np.mod(own, SIG_PERIOD) / SIG_PERIOD).astype(np.int64), 2)
    assert (SIG_S_PW[:, 1] == 0.0).all() and not (seg == 1).any(), own[seg == 1][:5]
    assert (seg == 2).any()          # follower 3 is zero there, follower 1 is not
    c = LC.controller(logs, so, ctrl)
    fam = LC.Family(name)
    fam.fixed_m("sig", c, 100)       # ~ 227 posts per replica (fewest: 203)
    fam.martingale("sig", c)
    return fam


# --------------------------------------------------------------------------- GPU side
def _ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from redqueen_amd import engine
    from oracle import oracle as O
    return torch, engine, O


def _graph(engine, so, start_time=0.0):
    return engine.Graph(so["src_id"], so["other_sources"], so["sink_ids"], so["edge_list"],
                        so["end_time"], start_time=start_time)


def _logs(res):
    """BatchResult -> lawcheck.Logs (one device-to-host copy)."""
    assert int(res.status.abs().max().item()) == 0
    n = res.counts[:, 2].cpu().numpy()
    N = int(n.max())
    idx = res.ev_src[:, :N].cpu().numpy().astype(np.int64)
    pad = np.arange(N)[None, :] >= n[:, None]
    src = res.graph.stream_src_ids[np.where(pad, 0, idx)]
    return LC.from_padded(res.ev_t[:, :N].cpu().numpy(), src, n)


def _run_opt(torch, g, so, R, c, **kw):
    u = torch.from_numpy(seeds(R, c))
    return g.run("opt", q=so["q"], s=so["s"], n_rep=R, ctrl_seed=u, world_seed=u, randomize=True,
                 Ks=(1,), event_log=True, check=True, **kw)


def _bit_exact(O, res, so, c, replicas, start_time=0.0):
    from tests.test_gpu_engine import _cmp_replica
    for r in replicas:
        u = int(seeds(r + 1, c)[r])
        sc = O.Scenario(seeded(so, u), ("opt", u), start_time=start_time)
        met, (t_o, _, s_o) = O.engine_metrics(sc, (1,))
        _cmp_replica(res, r, met, t_o, s_o, (1,))


@pytest.mark.parametrize("sweep_mode", [0, 7])
def test_edges_world(sweep_mode):
    """Both instantiations of the generator: rq_gen_streams + merge + fused sweep (mode 0)
    and the fused sweep generating in-kernel (mode 7)."""
    torch, engine, O = _ctx()
    so = edges_world()
    res = _run_opt(torch, _graph(engine, so, EDGES_START), so, 512, 3, sweep_mode=sweep_mode)
    _bit_exact(O, res, so, 3, (0, 255, 511), EDGES_START)
    analyse_edges(_logs(res), so, "edges mode %d" % sweep_mode).check()


@pytest.mark.parametrize("sweep_mode", [0, 2])
def test_bursty_world(sweep_mode):
    torch, engine, O = _ctx()
    so = graphs.c5_small()
    res = _run_opt(torch, _graph(engine, so), so, 512, 5, sweep_mode=sweep_mode)
    analyse_bursty(_logs(res), so, "bursty mode %d" % sweep_mode).check()


def test_wide_world():
    torch, engine, O = _ctx()
    so = wide_world()
    g = _graph(engine, so)
    plan = g.run("opt", q=so["q"], s=so["s"], n_rep=128, Ks=(1,), event_log=True, plan_only=True)
    assert g.n_streams > 64 and plan["sources_per_lane"] == 0, plan     # general sweep, merged streams
    res = _run_opt(torch, g, so, 128, 7)
    _bit_exact(O, res, so, 7, (0, 64, 127))
    analyse_wide(_logs(res), so).check()


def test_controller_opt_grid():
    torch, engine, O = _ctx()
    so = graphs.readme()
    n_rep = 256
    qs, sm, _, _ = opt_grid(n_rep)
    u = torch.from_numpy(seeds(len(qs) * n_rep, 11))
    res = _graph(engine, so).run("opt", q=qs, s=sm, n_rep=n_rep, ctrl_seed=u, world_seed=u,
                                 randomize=True, Ks=(1,), event_log=True, check=True)
    analyse_opt_grid(_logs(res), so, n_rep).check()


def test_controller_poisson():
    torch, engine, O = _ctx()
    so = graphs.readme()
    rates = np.repeat(CTRL_RATES, 128).astype(np.float64)
    u = torch.from_numpy(seeds(len(rates), 13))
    res = _graph(engine, so).run("poisson", n_rep=len(rates), ctrl_seed=u, world_seed=u,
                                 randomize=True, ctrl_rate=torch.from_numpy(rates), Ks=(1,),
                                 event_log=True, check=True)
    analyse_poisson_ctrl(_logs(res), so, rates).check()


def test_controller_sig():
    torch, engine, O = _ctx()
    so = graphs.readme()
    u = torch.from_numpy(seeds(512, 17))
    res = _graph(engine, so).run("sig", q=so["q"], s_pw=SIG_S_PW, period=SIG_PERIOD, n_rep=512,
                                 ctrl_seed=u, world_seed=u, randomize=True, Ks=(1,),
                                 event_log=True, check=True)
    analyse_sig(_logs(res), so).check()

"""The law checker itself (tests/lawcheck.py), validated without a GPU: a green
test_gpu_law.py proves something only if the checker passes the right law and rejects
a wrong one.

* The reference's law passes: logs of oracle.ref_run, the MT19937 restatement of the
  reference (its stale Hawkes bound, its own draw order) -- independent of the engine's
  generator rules.
* The engine's law passes: oracle.engine_run on the same worlds.
* Power: on the engine's logs the same family of statistics REJECTS, at its own level,
  a checker handed alpha x 1.05, beta x 1.05, l_0 x 1.05, q x 1.10, a PiecewiseConst rate
  x 1.05, or an Opt compensator that forgets to reset the ranks at an own post.
* Unit checks of the compensators against direct sums and hand-computed integrals.
"""
import numpy as np
import pytest

import lawcheck as LC
from oracle import oracle as O
from redqueen_amd import graphs
from tests.test_gpu_law import analyse_bursty, seeded, seeds


def _logs(so, ctrl_of, us, law):
    run = O.engine_run if law == "engine" else O.ref_run
    out = []
    for u in us:
        t, _, s = run(O.Scenario(seeded(so, u), ctrl_of(int(u))))
        out.append((t, s))
    return LC.pack(out)


@pytest.fixture(scope="module")
def bursty_engine():
    """40 replicas of graphs.c5_small on the engine oracle: ~160k Hawkes arrivals, ~38k posts."""
    so = graphs.c5_small()
    return so, _logs(so, lambda u: ("opt", u), seeds(40, 5), "engine")


@pytest.fixture(scope="module")
def mixed_engine():
    """120 replicas of graphs.mixed (PiecewiseConst, Poisson, RealData, Hawkes; T = 50)."""
    so = graphs.mixed()
    return so, _logs(so, lambda u: ("opt", u), seeds(120, 9), "engine")


def _readme_family(logs, so, name):
    LC.check_support(logs, so)
    procs = LC.world(logs, so)
    fam = LC.Family(name)
    fam.fixed_m("Poisson2", procs[2], LC.poisson_m(1000.0, logs.R))
    fam.martingale("Poisson2", procs[2])
    fam.fixed_m("Hawkes", procs[3], 500)          # expected 1111
    fam.martingale("Hawkes", procs[3])
    c = LC.controller(logs, so, ("opt", 0))
    fam.fixed_m("opt", c, 200)                    # ~ 410 posts per replica at q = 1
    fam.martingale("opt", c)
    return fam


def _mixed_family(logs, so, name):
    """The PiecewiseConst source of graphs.mixed (Lambda(T) = 200) and the controller."""
    LC.check_support(logs, so)
    p = LC.world(logs, so)[4]
    fam = LC.Family(name)
    fam.fixed_m("PiecewiseConst", p, LC.poisson_m(200.0, logs.R))
    fam.martingale("PiecewiseConst", p)
    fam.p("PiecewiseConst uniform", LC.uniform_ks(p)[1])
    return fam


# --------------------------------------------------------------------------- the right laws pass
def test_reference_law_passes():
    so = graphs.c5_small()
    analyse_bursty(_logs(so, lambda u: ("opt", u), seeds(16, 5), "ref"), so, "c5_small ref_run").check()
    so = graphs.readme()
    _readme_family(_logs(so, lambda u: ("opt", u), seeds(40, 11), "ref"), so, "readme ref_run").check()


def test_engine_law_passes(bursty_engine, mixed_engine):
    so, logs = bursty_engine
    analyse_bursty(logs, so, "c5_small engine").check()
    so = graphs.readme()
    _readme_family(_logs(so, lambda u: ("opt", u), seeds(40, 11), "engine"), so, "readme engine").check()
    so, logs = mixed_engine
    _mixed_family(logs, so, "mixed engine").check()


def test_edge_regimes_from_time_zero_on_the_oracle():
    """test_gpu_law's edge-regime world started at 0, below the PiecewiseConst source's
    first change time (the rate there wraps to the last one).  The oracle plays it; the
    engine's graph build refuses it as the reference's assert does, so only the oracle's
    law can be checked for the wrap-around."""
    from tests.test_gpu_law import analyse_edges, edges_world
    so = dict(edges_world(), end_time=200.0)
    logs = _logs(so, lambda u: ("opt", u), seeds(64, 3), "engine")
    early = logs.t[(logs.src == 6) & (logs.t < 20.0)]
    assert 64 * 10 * 0.8 < early.size < 64 * 10 * 1.2     # rate 0.5 on [0, 20)
    analyse_edges(logs, so, "edges from 0, oracle", start=0.0).check()


def test_poisson_and_sig_controllers_pass():
    so = graphs.readme()
    rates = np.repeat([0.0, 0.5, 4.0, 9.5], 10)
    us = seeds(len(rates), 13)
    for law in ("engine", "ref"):
        run = O.engine_run if law == "engine" else O.ref_run
        out = []
        for u, r in zip(us, rates):
            t, _, s = run(O.Scenario(seeded(so, u), ("poisson", int(u), float(r))))
            out.append((t, s))
        logs = LC.pack(out)
        ctrl = ("poisson", 0, rates)
        LC.check_support(logs, so, ctrl)
        c = LC.controller(logs, so, ctrl)
        fam = LC.Family("poisson ctrl " + law)
        fam.martingale("poisson", c)
        fam.p("poisson uniform", LC.uniform_ks(LC.Proc("p", c.inc[10:], c.n[10:], c.tail[10:]))[1])
        fam.check()
        spw = np.asarray([[1.0, 0.0, 0.5], [2.0, 0.0, 0.0]])
        ctrl = ("sig", 0, spw, 10.0)
        logs = _logs(so, lambda u: ("sig", u, spw, 10.0), seeds(40, 17), law)
        c = LC.controller(logs, so, ctrl)
        fam = LC.Family("sig ctrl " + law)
        fam.fixed_m("sig", c, 100)
        fam.martingale("sig", c)
        fam.check()
        # a wrong period is seen
        bad = LC.controller(logs, so, ("sig", 0, spw, 9.0))
        assert abs(LC.martingale(bad)) > 10.0


# --------------------------------------------------------------------------- wrong laws are rejected
@pytest.mark.parametrize("key,factor", [("alpha", 1.05), ("beta", 1.05), ("l_0", 1.05), ("q", 1.10)])
def test_power_hawkes_and_q(bursty_engine, key, factor):
    so, logs = bursty_engine
    fam = analyse_bursty(logs, LC.perturbed(so, **{key: factor}), "c5_small, %s x %g" % (key, factor))
    fam.report()
    assert fam.rejects()
    # ... by the process the parameter belongs to, and by that one alone
    hit = {lab.split()[0] for lab, _ in fam.failures()}
    assert hit == ({"opt"} if key == "q" else {"Hawkes"}), hit


def test_power_piecewise_rate(mixed_engine):
    so, logs = mixed_engine
    fam = _mixed_family(logs, LC.perturbed(so, rates=1.05), "mixed, rates x 1.05")
    fam.report()
    assert fam.rejects()


def test_power_opt_forgets_reset(bursty_engine):
    so, logs = bursty_engine
    c = LC.controller(logs, so, ("opt", 0), reset=False)
    fam = LC.Family("c5_small, no rank reset")
    fam.fixed_m("opt", c, 400)
    fam.martingale("opt", c)
    fam.report()
    assert fam.rejects()


def test_short_replica_is_an_error_not_dropped(bursty_engine):
    so, logs = bursty_engine
    c = LC.controller(logs, so, ("opt", 0))
    with pytest.raises(AssertionError, match="fewer than m"):
        LC.fixed_m(c, int(c.n.min()) + 1)


# --------------------------------------------------------------------------- unit checks
def test_hawkes_recurrence_equals_direct_sum():
    rs = np.random.RandomState(1)
    t = np.sort(rs.uniform(0.0, 30.0, 50))
    for l0, a, b in [(0.7, 1.3, 2.0), (2.0, 50.0, 1e4), (1.0, 0.045, 0.05), (1.5, 0.0, 1.0)]:
        p = LC.hawkes("h", t[None, :], np.asarray([50]), l0, a, b, 0.0, 31.0)
        inc, tail = LC.hawkes_direct(t, l0, a, b, 0.0, 31.0)
        assert np.allclose(p.inc[0], inc, rtol=1e-12, atol=0.0)
        assert np.isclose(p.tail[0], tail, rtol=1e-12, atol=0.0)
        assert np.isclose(p.total[0], inc.sum() + tail, rtol=1e-12)
    # ragged replicas: the padding changes nothing
    tt = np.full((2, 50), np.nan)
    tt[0] = t
    tt[1, :20] = t[:20]
    p = LC.hawkes("h", tt, np.asarray([50, 20]), 0.7, 1.3, 2.0, 0.0, 31.0)
    inc, tail = LC.hawkes_direct(t[:20], 0.7, 1.3, 2.0, 0.0, 31.0)
    assert np.allclose(p.inc[1, :20], inc, rtol=1e-12) and np.isnan(p.inc[1, 20:]).all()
    assert np.isclose(p.tail[1], tail, rtol=1e-12)


def test_piecewise_integral_by_hand():
    ct, rt = [20.0, 50.0, 50.5, 120.0], [3.0, 0.0, 40.0, 0.5]
    # before the first change time the rate wraps to the last one (0.5)
    assert LC.pw_rate(np.asarray([0.0, 10.0, 20.0, 49.9, 50.0, 50.25, 50.5, 119.0, 120.0, 200.0]), ct, rt).tolist() \
        == [0.5, 0.5, 3.0, 3.0, 0.0, 0.0, 40.0, 40.0, 0.5, 0.5]
    x = np.asarray([0.0, 10.0, 20.0, 30.0, 50.0, 50.25, 51.0, 120.0, 200.0])
    want = [0.0, 5.0, 10.0, 40.0, 100.0, 100.0, 120.0, 2880.0, 2920.0]
    assert np.allclose(LC.pw_integral(x, ct, rt, 0.0), want, rtol=1e-14, atol=0.0)
    # a start time inside the first segment
    assert np.isclose(LC.pw_integral(np.asarray([60.0]), ct, rt, 25.0)[0], 3.0 * 25 + 40.0 * 9.5)
    times = np.asarray([[10.0, 30.0, 51.0, np.nan]])
    p = LC.pwconst("p", times, np.asarray([3]), ct, rt, 0.0, 200.0)
    assert np.allclose(p.inc[0, :3], [5.0, 35.0, 80.0]) and np.isclose(p.tail[0], 2800.0)
    assert np.isclose(p.total[0], 2920.0)


def test_controller_compensator_by_hand():
    """Two followers (w = sqrt(s / q) = 1 and 2), a duplicated edge counting twice, the
    opening post at t = 0 not a point, ranks reset at an own post."""
    so = dict(src_id=1, end_time=10.0, q=0.25, s=np.asarray([0.25, 1.0]), sink_ids=[5, 6, 7],
              other_sources=[], edge_list=[(1, 5), (1, 6), (2, 5), (3, 6), (3, 6), (4, 7)])
    t = np.asarray([0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 7.0])
    s = np.asarray([1, 2, 3, 4, 1, 2, 1])
    c = LC.controller(LC.pack([(t, s)]), so, ("opt", 0))
    # u = 1 on [1, 2), 1 + 2 * 2 = 5 on [2, 4) (source 4 reaches no follower); after the
    # post at 4: 0 until 5, then 1
    assert c.n[0] == 2 and np.allclose(c.inc[0], [1.0 + 10.0, 2.0]) and np.isclose(c.tail[0], 0.0)
    nr = LC.controller(LC.pack([(t, s)]), so, ("opt", 0), reset=False)
    assert np.allclose(nr.inc[0], [11.0, 5.0 + 6.0 * 2]) and np.isclose(nr.tail[0], 18.0)
    # piecewise significance: period 4, two segments; follower 5 only, s = (0.25, 0) -> w = (1, 0)
    so2 = dict(so, edge_list=[(1, 5), (2, 5)])
    t2, s2 = np.asarray([0.0, 1.0, 9.0]), np.asarray([1, 2, 1])
    c = LC.controller(LC.pack([(t2, s2)]), so2, ("sig", 0, np.asarray([[0.25, 0.0]]), 4.0))
    # r = 1 from t = 1: w = 1 on [1, 2), [4, 6), [8, 9)
    assert np.allclose(c.inc[0], [4.0]) and np.isclose(c.tail[0], 0.0)


def test_poisson_m_and_family_bound():
    m = LC.poisson_m(200.0, 512)
    from scipy import stats
    assert 512 * stats.poisson.cdf(m - 1, 200.0) < 1e-9 <= 512 * stats.poisson.cdf(m, 200.0)
    fam = LC.Family("f", level=1e-3)
    for k in range(9):
        fam.p("ok %d" % k, 0.5)
    fam.p("bad", 0.9e-4)
    assert fam.bound == 1e-4 and fam.rejects() and fam.failures() == [("bad", 0.9e-4)]
    with pytest.raises(AssertionError):
        fam.check()

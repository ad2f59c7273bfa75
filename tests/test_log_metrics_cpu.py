"""CPU side of rq_log_metrics (no GPU): the host checker tests/log_metrics_ref.py pinned to
the reference (tests/golden/log_metrics.npz: the reference's own time_in_top_k /
average_rank / int_r_2 / num_tweets_of on worlds with several rows per (t, sink)) and to
the oracle's Appendix-B metrics on the host-expanded rows of random tie-heavy logs; the
ABI entry's argument checks, which come before any HIP call."""
import ctypes as C

import numpy as np
import pytest

from tests import log_metrics_ref as LR

WORLDS = ("game5", "thirds", "wide", "places")


def world(f, name):
    return dict(src_id=int(f[name + "_world"][0]), end_time=float(f[name + "_world"][1]),
                sinks=[int(x) for x in f[name + "_sinks"]],
                edges=[tuple(int(v) for v in e) for e in f[name + "_edges"]],
                t=f[name + "_t"], src=f[name + "_src"])


@pytest.mark.parametrize("name", WORLDS)
def test_checker_equals_the_reference(golden, name):
    f = golden("log_metrics.npz")
    assert [str(n) for n in f["names"]] == list(WORLDS)
    Ks = [int(k) for k in f["Ks"]]
    w = world(f, name)
    got = LR.play(w["t"], w["src"], w["edges"], w["src_id"], w["end_time"], Ks)
    assert LR.same_bits(got["metrics"], f[name + "_metrics"]), (got["metrics"], f[name + "_metrics"])
    assert np.array_equal(got["counts"][:2], f[name + "_posts"])
    assert got["status"] == LR.ST_TIE


def test_fixture_worlds_hold_what_they_are_for(golden):
    f = golden("log_metrics.npz")
    Ks = [int(k) for k in f["Ks"]]
    got = {n: LR.play(*(world(f, n)[k] for k in ("t", "src", "edges", "src_id", "end_time")), Ks) for n in WORLDS}
    # game5: three Opts on sink 1 at start_time
    w = world(f, "game5")
    first = [int(s) for t, s in zip(w["t"], w["src"]) if t == w["t"][0]]
    assert sum(1 for s in first if (s, 1) in w["edges"]) == 3
    # thirds: >= 12 sinks, the lowest followed only by a source without an event, thirds
    # live over many rows, and a zero column in front of the pivot columns changes the bits
    w = world(f, "thirds")
    assert len(w["sinks"]) >= 12 and got["thirds"]["counts"][3] == len(w["sinks"]) - 1
    low = [s for s, x in w["edges"] if x == min(w["sinks"])]
    assert len(low) == 1 and low[0] not in set(int(s) for s in w["src"])
    assert 3 in got["thirds"]["dens"] and got["thirds"]["frac_rows"] >= 20
    shifted = LR.play(w["t"], w["src"], w["edges"], w["src_id"], w["end_time"], Ks, lead_zeros=1)
    assert not LR.same_bits(shifted["metrics"], got["thirds"]["metrics"])
    # wide: >= 130 seen sinks with thirds live
    assert got["wide"]["counts"][3] >= 130 and 3 in got["wide"]["dens"] and got["wide"]["frac_rows"] >= 20
    # places: the controlled source first, in the middle and last of a tie group
    w = world(f, "places")
    where = set()
    for tt in np.unique(w["t"]):
        grp = [int(s) for t, s in zip(w["t"], w["src"]) if t == tt]
        if len(grp) > 1 and w["src_id"] in grp:
            k = grp.index(w["src_id"])
            where.add("first" if k == 0 else ("last" if k == len(grp) - 1 else "middle"))
    assert where == {"first", "middle", "last"}


def random_log(rng, n_src, n_sinks, n_ev, ctrl):
    """A tie-heavy log on a random graph: times drawn from a few values, sources in any
    order (several posts of one source at one time included); some sources have no edge."""
    sinks = list(range(50, 50 + n_sinks))
    srcs = list(range(1, n_src + 1))
    edges = []
    for s in srcs[:-1]:   # the last source has no edge
        for x in rng.choice(sinks, size=rng.randint(1, n_sinks + 1), replace=False):
            edges.append((s, int(x)))
    t = np.sort(rng.choice(np.arange(1, max(2, n_ev // 3)) * 0.375, size=n_ev))
    src = rng.choice(srcs, size=n_ev)
    return sinks, edges, t, src


@pytest.mark.parametrize("seed", range(8))
def test_checker_equals_the_oracle_on_tie_heavy_logs(seed):
    from oracle import oracle as O
    rng = np.random.RandomState(100 + seed)
    n_sinks = [3, 7, 9, 12, 20, 40, 130, 150][seed]
    ctrl = 2
    sinks, edges, t, src = random_log(rng, 6, n_sinks, 60 + 25 * seed, ctrl)
    Ks = (1, 2, 4)
    end = float(t[-1]) + 1.25
    got = LR.play(t, src, edges, ctrl, end, Ks)
    rt, rs, rx, re_ = LR.expand(t, src, edges)
    top, avg, r2, cnt = O.metrics_df(rt, rs, rx, re_, ctrl, end, Ks)
    assert got["status"] == LR.ST_TIE
    assert LR.same_bits(got["metrics"], np.asarray(list(top) + [avg, r2])), (got["metrics"], top, avg, r2)
    assert np.array_equal(got["counts"], cnt), (got["counts"], cnt)


def test_abi_symbols_and_argument_checks():
    """Exported without an ABI version change; bad arguments are refused before any HIP
    call (so this runs without a GPU)."""
    from redqueen_amd import _lib as L
    lib = L.lib()
    for fn in ("rq_log_metrics", "rq_log_metrics_workspace"):
        assert fn in L.EXPORTED and hasattr(lib, fn), fn
    assert lib.rq_abi_version() == 6
    k = np.asarray([1], dtype=np.int32)
    n = C.c_size_t()
    assert lib.rq_log_metrics_workspace(None, 1, 1, 1, C.byref(n)) == L.RQ_EINVAL
    assert lib.rq_log_metrics(None, None, None, None, 1, 1, k.ctypes.data_as(L._pi32), 1, None, None, None,
                              None, 0, None) == L.RQ_EINVAL
    assert L.LOG_METRICS_MAX_SINKS >= 4096
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rq.h")).read()
    assert re.search(r"#define RQ_LOG_METRICS_MAX_SINKS\s+%d\b" % L.LOG_METRICS_MAX_SINKS, src)

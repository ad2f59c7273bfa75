"""What the tests of rq_log_metrics_of share (tests/test_log_sources_cpu.py,
tests/test_gpu_log_sources.py): the OWN-scope edge filter and the fixture's key names.
The checker itself is tests/log_metrics_ref.play, handed the tracked source as ``ctrl`` and,
in scope "own", the edge list filtered here.
"""
import numpy as np

from tests import log_metrics_ref as LR

SCOPES = ("df", "own")
WORLDS = ("game5", "thirds", "wide", "places")


def followers_of(edges, c):
    """The sinks of source c's edges, ascending."""
    return sorted({int(x) for s, x in edges if int(s) == int(c)})


def own_edges(edges, c):
    """The edges whose sink is a follower of c (scope "own"): the dataframe of a log on
    these edges is the log's dataframe with the rows of other sinks removed."""
    fol = set(followers_of(edges, c))
    return [(int(s), int(x)) for s, x in edges if int(x) in fol]


def scope_edges(edges, c, scope):
    assert scope in SCOPES
    return [(int(s), int(x)) for s, x in edges] if scope == "df" else own_edges(edges, c)


def play(t, src, edges, c, end_time, Ks, scope):
    """rq_log_metrics_of's contract for tracked source c on one replica's log."""
    return LR.play(t, src, scope_edges(edges, c, scope), c, end_time, Ks)


def sources(edges, extra=()):
    """Every source id of an edge list (and ``extra``: sources without edges), ascending."""
    return sorted({int(s) for s, _x in edges} | {int(s) for s in extra})


def key(name, scope, what):
    return "%s_%s_%s" % (name, scope, what)


def world(f, name):
    """A world of tests/golden/log_metrics.npz as plain Python."""
    return dict(src_id=int(f[name + "_world"][0]), end_time=float(f[name + "_world"][1]),
                sinks=[int(x) for x in f[name + "_sinks"]],
                edges=[tuple(int(v) for v in e) for e in f[name + "_edges"]],
                t=np.asarray(f[name + "_t"], dtype=np.float64), src=np.asarray(f[name + "_src"], dtype=np.int64))

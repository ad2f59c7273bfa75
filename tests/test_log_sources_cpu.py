"""CPU side of rq_log_metrics_of (no GPU): the host checker handed any source as the
tracked one, in both scopes, pinned to the reference (tests/golden/log_sources.npz: the
reference's own time_in_top_k(df, K, src_id=c) / average_rank / int_r_2 / num_tweets_of on
the log's dataframe and on df[df.sink_id.isin(followers of c)]); the OWN-scope edge filter
the GPU tests use; the entry's argument checks that need no graph; the HIP-free validation
of src_ids (tests/host/log_of_check.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import log_metrics_ref as LR
from tests import log_sources_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("scope", SR.SCOPES)
@pytest.mark.parametrize("name", SR.WORLDS)
def test_checker_equals_the_reference_for_every_source(golden, name, scope):
    f, fs = golden("log_metrics.npz"), golden("log_sources.npz")
    assert [str(n) for n in fs["names"]] == list(SR.WORLDS) and [str(s) for s in fs["scopes"]] == list(SR.SCOPES)
    Ks = [int(k) for k in fs["Ks"]]
    w = SR.world(f, name)
    srcs = [int(s) for s in fs[name + "_srcs"]]
    assert srcs == SR.sources(w["edges"], w["src"])
    met, posts, empty = (fs[SR.key(name, scope, k)] for k in ("metrics", "posts", "empty"))
    for k, c in enumerate(srcs):
        got = SR.play(w["t"], w["src"], w["edges"], c, w["end_time"], Ks, scope)
        if empty[k]:
            assert got["status"] == LR.ST_EMPTY and np.isnan(got["metrics"]).all() and not got["counts"].any()
            assert np.isnan(met[k]).all()
            continue
        assert LR.same_bits(got["metrics"], met[k]), (c, got["metrics"], met[k])
        assert np.array_equal(got["counts"][:2], posts[k]), (c, got["counts"], posts[k])
        if c == w["src_id"] and scope == "df":   # the controlled source: log_metrics.npz's own values
            assert LR.same_bits(met[k], f[name + "_metrics"])


def test_fixture_holds_what_it_is_for(golden):
    f, fs = golden("log_metrics.npz"), golden("log_sources.npz")
    n_case = n_empty = n_differ = 0
    for name in SR.WORLDS:
        n_empty += int(fs[SR.key(name, "own", "empty")].sum()) + int(fs[SR.key(name, "df", "empty")].sum())
        n_case += 2 * len(fs[name + "_srcs"])
        n_differ += int((~np.all(np.isclose(fs[SR.key(name, "own", "metrics")], fs[SR.key(name, "df", "metrics")],
                                            equal_nan=True), axis=1)).sum())
    assert n_case == 48 and n_empty == 1 and n_differ >= 10   # the scopes are different questions
    # thirds: source 9 never posts and nobody else reaches its follower -- EMPTY in scope own
    # only; in scope df it is defined with no event of its own
    w = SR.world(f, "thirds")
    k = [int(s) for s in fs["thirds_srcs"]].index(9)
    assert fs["thirds_own_empty"][k] == 1 and fs["thirds_df_empty"][k] == 0 and fs["thirds_df_posts"][k][0] == 0
    assert SR.followers_of(w["edges"], 9) == [min(w["sinks"])]


@pytest.mark.parametrize("seed", range(4))
def test_own_edges_give_the_filtered_rows(seed):
    """The log's rows on own_edges(edges, c) are its rows on edges with the other sinks'
    rows removed, event ids kept."""
    from tests.test_log_metrics_cpu import random_log
    rng = np.random.RandomState(300 + seed)
    _sinks, edges, t, src = random_log(rng, 6, [3, 9, 40, 130][seed], 80, 2)
    rt, rs, rx, re_ = LR.expand(t, src, edges)
    for c in range(1, 7):
        fol = SR.followers_of(edges, c)
        keep = np.isin(rx, fol)
        sub = SR.own_edges(edges, c)
        assert sorted(set(sub)) == sorted(sub) and {x for _s, x in sub} == set(fol)
        got = LR.expand(t, src, sub)
        for a, b in zip(got, (rt[keep], rs[keep], rx[keep], re_[keep])):
            assert np.array_equal(a, b), c
        ref = LR.play(t, src, sub, c, 50.0, (1, 2))
        if not fol:   # the last source has no edge
            assert c == 6 and ref["status"] == LR.ST_EMPTY
        else:
            assert ref["counts"][0] == int((src == c).sum())
            assert ref["counts"][0] + ref["counts"][1] == len(set(re_[keep].tolist()))
            assert ref["counts"][3] == len(set(rx[keep].tolist()))
    assert SR.scope_edges(edges, 1, "df") == [(int(s), int(x)) for s, x in edges]


def test_abi_symbols_and_argument_checks():
    """Exported without an ABI version change; what needs no graph is refused before any
    HIP call (so this runs without a GPU)."""
    from redqueen_amd import _lib as L
    lib = L.lib()
    for fn in ("rq_log_metrics_of", "rq_log_metrics_of_workspace"):
        assert fn in L.EXPORTED and fn in L.OPTIONAL and L.has(fn), fn
    assert lib.rq_abi_version() == 6
    k = np.asarray([1], dtype=np.int32)
    ids = np.asarray([1], dtype=np.int64)
    n = C.c_size_t()
    assert lib.rq_log_metrics_of_workspace(None, 1, 1, 1, 1, C.byref(n)) == L.RQ_EINVAL
    assert lib.rq_log_metrics_of(None, ids.ctypes.data_as(L._pi64), 1, L.LOG_OF_DF, None, None, None, 1, 1,
                                 k.ctypes.data_as(L._pi32), 1, None, None, None, None, 0, None) == L.RQ_EINVAL
    src = open(os.path.join(ROOT, "include", "rq.h")).read()
    import re
    for name, v in (("RQ_LOG_OF_DF", L.LOG_OF_DF), ("RQ_LOG_OF_OWN", L.LOG_OF_OWN),
                    ("RQ_LOG_OF_MAX_SRC", L.LOG_OF_MAX_SRC)):
        assert re.search(r"#define %s\s+%d\b" % (name, v), src), name


def test_sources_frame():
    from redqueen_amd import batch
    from redqueen_amd._lib import ST_EMPTY, ST_TIE
    rng = np.random.RandomState(4)
    R, P, Ks = 5, 3, (1, 2)
    met = rng.rand(R, P, 4)
    cnt = rng.randint(0, 50, size=(R, P, 4))
    sta = np.zeros((R, P), dtype=np.int32)
    sta[1, 0] = ST_TIE
    sta[2, 1] = ST_EMPTY
    met[2, 1] = np.nan
    sta[:, 2] = ST_EMPTY
    met[:, 2] = np.nan
    frame, summ = batch.sources_frame([7, 3, 9], Ks, met, cnt, sta)
    assert list(frame.columns) == ["replica", "src_id", "top_1", "top_2", "avg_rank", "r_2", "num_events",
                                   "other_events", "status"]
    assert len(frame) == R * P and list(frame.src_id[:P]) == [7, 3, 9] and list(frame.replica[:P]) == [0] * P
    assert np.array_equal(frame.avg_rank.values.reshape(R, P), met[:, :, 2], equal_nan=True)
    assert np.array_equal(frame.num_events.values.reshape(R, P), cnt[:, :, 0])
    assert list(summ.src_id) == [7, 3, 9] and list(summ.n) == [5, 4, 0] and list(summ.n_empty) == [0, 1, 5]
    ok = [0, 1, 3, 4]
    m1, s1 = batch._mean_sem(met[ok, 1, 0])
    assert summ.top_1[1] == m1 and summ.top_1_se[1] == s1 and np.isnan(summ.avg_rank[2])
    assert summ.num_events[0] == batch._mean_sem(cnt[:, 0, 0].astype(np.float64))[0]


def test_tracked_sources_without_a_gpu(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no C++ compiler")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall"]
    exe = str(tmp_path / "log_of_check")
    cc = subprocess.run([cxx] + flags + ["-o", exe, os.path.join(ROOT, "redqueen_amd", "csrc", "rq_topo.cpp"),
                                         os.path.join(ROOT, "tests", "host", "log_of_check.cpp")],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr

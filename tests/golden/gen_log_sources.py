#!/usr/bin/env python
"""Generate tests/golden/log_sources.npz from the REFERENCE (build container only; the
reference never travels to the GPU box):

    MPLBACKEND=Agg python tests/golden/gen_log_sources.py

For the four worlds of tests/golden/log_metrics.npz (their logs and edge lists are read
from that file) and for EVERY source c of each world the fixture holds the reference's own
values for src_id = c -- time_in_top_k for K = 1, 2, 3, average_rank, int_r_2, num_tweets_of
and the number of distinct event ids of the other sources -- in two scopes:

  df    on the log's whole dataframe (the pivot runs over every sink the df holds)
  own   on df[df.sink_id.isin(followers of c)], the feeds an Opt tracks its rank on

Keys: <world>_srcs [P]; <world>_<scope>_metrics [P, 5] (NaN for an empty dataframe),
<world>_<scope>_posts [P, 2] and <world>_<scope>_empty [P] (1: the dataframe has no row).
Every value is asserted bit-equal to the host checker (tests/log_metrics_ref.play with c as
the tracked source and, in scope own, the edge list filtered the same way).
"""
import os
import sys
import types
import warnings

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "_shim"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")
os.environ.setdefault("MPLBACKEND", "Agg")

import redqueen.utils as U  # noqa: E402
from tests import log_metrics_ref as LR  # noqa: E402
from tests import log_sources_ref as SR  # noqa: E402

KS = [1, 2, 3]


def main():
    f = np.load(os.path.join(HERE, "log_metrics.npz"))
    assert [int(k) for k in f["Ks"]] == KS
    rec = {"Ks": np.asarray(KS, dtype=np.int32), "names": np.asarray(SR.WORLDS),
           "scopes": np.asarray(SR.SCOPES)}
    n_eq = n_case = n_empty = n_tie = 0
    for name in SR.WORLDS:
        w = SR.world(f, name)
        rt, rs, rx, re_ = LR.expand(w["t"], w["src"], w["edges"])
        df = pd.DataFrame({"event_id": re_, "t": rt, "src_id": rs, "sink_id": rx})
        srcs = SR.sources(w["edges"], w["src"])
        rec[name + "_srcs"] = np.asarray(srcs, dtype=np.int64)
        for scope in SR.SCOPES:
            met = np.full((len(srcs), len(KS) + 2), np.nan)
            posts = np.zeros((len(srcs), 2), dtype=np.int64)
            empty = np.zeros(len(srcs), dtype=np.int8)
            for k, c in enumerate(srcs):
                d = df if scope == "df" else df[df.sink_id.isin(SR.followers_of(w["edges"], c))]
                got = SR.play(w["t"], w["src"], w["edges"], c, w["end_time"], KS, scope)
                if len(d) == 0:
                    empty[k] = 1
                    n_empty += 1
                    assert got["status"] == LR.ST_EMPTY and np.isnan(got["metrics"]).all(), (name, scope, c)
                    continue
                so = types.SimpleNamespace(src_id=c, end_time=w["end_time"])
                vals = [U.time_in_top_k(df=d, K=K, src_id=c, end_time=w["end_time"]) for K in KS]
                vals += [U.average_rank(d, src_id=c, end_time=w["end_time"]), U.int_r_2(d, so)]
                met[k] = vals
                posts[k] = [int(U.num_tweets_of(d, broadcaster_id=c)), int(d.event_id[d.src_id != c].nunique())]
                n_case += 1
                ok = (LR.same_bits(got["metrics"], met[k]) and np.array_equal(got["counts"][:2], posts[k]) and
                      got["counts"][3] == d.sink_id.nunique() and got["counts"][2] == d.t.nunique())
                assert ok, (name, scope, c, got, met[k], posts[k])
                n_eq += 1
                n_tie += got["status"] == LR.ST_TIE
            rec[SR.key(name, scope, "metrics")] = met
            rec[SR.key(name, scope, "posts")] = posts
            rec[SR.key(name, scope, "empty")] = empty
        print(name, "sources", srcs)
    print("checker == reference: %d/%d non-empty cases (%d with ties), %d empty" % (n_eq, n_case, n_tie, n_empty))
    out = os.path.join(HERE, "log_sources.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

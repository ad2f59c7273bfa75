#!/usr/bin/env python
"""Generate tests/golden/unsorted.npz from the REFERENCE (build container only; the
reference never travels to the GPU box):

    MPLBACKEND=Agg python tests/golden/gen_unsorted.py

Dataframes whose rows are not in time order (tests/unsorted_cases.py golden_frames: a
concat of two runs over overlapping sink sets, shuffles without and with duplicate
cells, a frame concatenated with itself, a reversal, -0.0 and +0.0 times, one sink of
600 shuffled rows, negative times with extreme sink ids and repeated negative event
ids, a long frame with its halves swapped) and the reference's OWN values on them
(MPLBACKEND/_shim as gen_log_metrics.py): time_in_top_k for K = 1, 2, 5, average_rank,
int_r_2, the two event_id.nunique() counts, t.nunique() and sink_id.nunique().  The
file holds data only.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "_shim"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
warnings.filterwarnings("ignore")
os.environ.setdefault("MPLBACKEND", "Agg")

import redqueen.utils as U  # noqa: E402
from tests import replay_cases as RC  # noqa: E402
from tests import unsorted_cases as UC  # noqa: E402


class _Opts(object):
    def __init__(self, end):
        self.src_id = RC.SRC
        self.end_time = end


def main():
    frames = UC.golden_frames()
    rec = {"Ks": np.asarray(UC.KS_GOLDEN, dtype=np.int32), "names": np.asarray(list(frames))}
    for name, df in frames.items():
        end = UC.golden_end(df)
        so = _Opts(end)
        vals = [U.time_in_top_k(df, K, src_id=RC.SRC, end_time=end) for K in UC.KS_GOLDEN]
        vals += [U.average_rank(df, src_id=RC.SRC, end_time=end), U.int_r_2(df, so)]
        own = df.src_id == RC.SRC
        assert int(U.num_tweets_of(df, broadcaster_id=RC.SRC)) == int(df.event_id[own].nunique())
        rec[name + "_t"] = df.t.values.astype(np.float64)
        rec[name + "_src"] = df.src_id.values.astype(np.int64)
        rec[name + "_sink"] = df.sink_id.values.astype(np.int64)
        rec[name + "_eid"] = df.event_id.values.astype(np.int64)
        rec[name + "_end"] = np.float64(end)
        rec[name + "_metrics"] = np.asarray(vals, dtype=np.float64)
        rec[name + "_counts"] = np.asarray([df.event_id[own].nunique(), df.event_id[~own].nunique(),
                                            df.t.nunique(), df.sink_id.nunique()], dtype=np.int64)
        print(name, "rows", len(df), "unsorted", UC.is_unsorted(df), "dup cells", RC.has_dup_cell(df),
              rec[name + "_metrics"], rec[name + "_counts"])
    out = os.path.join(HERE, "unsorted.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

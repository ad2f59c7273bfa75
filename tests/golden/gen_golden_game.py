"""Generates tests/golden/dist_game.npz: the reference's own ensemble of world W5
(tests/game_ref.py w5(): RedQueen 1 against Poisson2 2, Hawkes 3 and the Opt broadcasters 4
and 5 among the other sources), for tests/test_gpu_game.py.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/gen_golden_game.py [N]

It imports MPI-SWS/RedQueen the way gen_golden.py does.  Replica r runs world
randomize_other_sources(r) with create_manager_with_opt(seed=r), so replicas r and r + 99
share streams (tests/ensemble.py clusters them).  Per replica: the posts of sources 1..5 and
source 1's time in the top 1, average rank and int r^2.  N = 10000 takes ~70 s on 16 cores.
"""
import multiprocessing as mp
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "_shim"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
warnings.filterwarnings("ignore")
os.environ.setdefault("MPLBACKEND", "Agg")

from redqueen.opt_model import SimOpts  # noqa: E402
import redqueen.utils as U  # noqa: E402

from game_ref import w5  # noqa: E402  (plain data, shared with the tests)

COLS = ["posts1", "posts2", "posts3", "posts4", "posts5", "top1", "avg", "r2"]


def _worker(r):
    d = w5()
    so = SimOpts(**dict(d, s=np.asarray(d["s"])))
    m = so.randomize_other_sources(r).create_manager_with_opt(seed=r)
    m.run_dynamic()
    df = m.state.get_dataframe()
    ev = df.groupby("event_id", sort=True).first()
    assert list(zip(ev.t.values[:3], ev.src_id.values[:3])) == [(0.0, 1), (0.0, 4), (0.0, 5)]
    posts = [int((ev.src_id.values == k).sum()) for k in range(1, 6)]
    return np.asarray(posts + [U.time_in_top_k(df=df, K=1, sim_opts=so), U.average_rank(df, sim_opts=so),
                               U.int_r_2(df, so)], dtype=np.float64)


def main(n):
    with mp.Pool(min(32, os.cpu_count())) as pool:
        res = np.asarray(pool.map(_worker, range(n), chunksize=16))
    np.savez_compressed(os.path.join(HERE, "dist_game.npz"), data=res, cols=np.asarray(COLS))
    print(res.shape, res.mean(0))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 10000)

"""The stream generator's staging and its last partial chunk (rq_gen_streams: arrivals are
staged 16 at a time and stored as whole 64-byte halves; the tail of a stream is the chunk
that is not full) against the engine oracle's event log of the same seeds.

The event log of a merged-stream run holds every arrival of every stream, so stream j of
replica i is the log's events of source j: its length is the stream's slen, its times the
stream's first slen arrivals.  Worlds (found with the CPU oracle, which asserts them here):

  tails     Poisson at rate 2.4, Poisson2 at 0.2 and Poisson at rate 0 over 10 time units,
            300 randomized replicas from seed 5: the first source's streams are 10 to 38
            arrivals long and take every length mod 16 (16 and 32, whole chunks, among
            them), the second is empty in some replicas, the third in all.
  overflow  a supercritical Hawkes source (l_0 2, alpha 3.5, beta 1) over 4 time units, 64
            replicas from seed 5: from ten arrivals to several times the stream's capacity
            (11,920 = the planner's bound, a multiple of 16).  A stream that reaches it is
            cut there and its replica flagged RQ_ST_STREAM_OVERFLOW; up to the time of its
            last kept arrival the replica is the oracle's.

Bar: bit-exact times and sources, and bit-exact metrics of the fast sweep on the same batch.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TAILS = dict(src_id=1, end_time=10.0, s=np.asarray([1.0, 1.0]), q=1.0, sink_ids=[10, 11],
             other_sources=[("Poisson", {"src_id": 2, "seed": 1, "rate": 2.4}),
                            ("Poisson2", {"src_id": 3, "seed": 2, "rate": 0.2}),
                            ("Poisson", {"src_id": 4, "seed": 3, "rate": 0.0})],
             edge_list=[(1, 10), (1, 11), (2, 10), (3, 11), (4, 10)])
OVERFLOW = dict(src_id=1, end_time=4.0, s=np.asarray([1.0]), q=100.0, sink_ids=[10],
                other_sources=[("Hawkes", {"src_id": 2, "seed": 1, "l_0": 2.0, "alpha": 3.5, "beta": 1.0}),
                               ("Poisson", {"src_id": 3, "seed": 2, "rate": 1.0})],
                edge_list=[(1, 10), (2, 10), (3, 10)])
HAWKES_CAP = 11920   # ceil((m + 8 m + 32)), m = 40 l_0 T + 1000, up to a multiple of 16
ST_STREAM_OVERFLOW = 2


def _ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from redqueen_amd import engine
    from oracle import oracle as O
    return torch, engine, O


def _graph(engine, so):
    return engine.Graph(so["src_id"], so["other_sources"], so["sink_ids"], so["edge_list"],
                        so["end_time"])


def _seeded(so, u):
    """randomize_other_sources(u): other source idx gets seed u + 99 idx."""
    return dict(so, other_sources=[(n, dict(x, seed=(u + 99 * i) & 0xFFFFFFFF)) if "seed" in x else (n, x)
                                   for i, (n, x) in enumerate(so["other_sources"])])


def test_every_tail_length():
    torch, engine, O = _ctx()
    so, R, seed0 = TAILS, 300, 5
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=R, ctrl_seed=seed0, world_seed=seed0, randomize=True, Ks=(1,))
    assert g.run("opt", plan_only=True, **kw)["variant"] >= 20   # merged streams: rq_gen_streams feeds it
    log = g.run("opt", event_log=True, **kw)
    fast = g.run("opt", **kw)
    assert int(log.status.max().item()) == 0 and int(fast.status.max().item()) == 0
    lens = np.zeros((R, 3), dtype=np.int64)
    for i in range(R):
        u = seed0 + i
        t_o, _, s_o = O.engine_run(O.Scenario(_seeded(so, u), ("opt", u)), cap=1 << 14)
        t, s = log.events(i)
        assert np.array_equal(s, s_o) and np.array_equal(t, t_o), i
        for k, sid in enumerate((2, 3, 4)):
            lens[i, k] = int((s == sid).sum())   # the stream's slen
            assert np.array_equal(t[s == sid], t_o[s_o == sid]), (i, sid)
    assert sorted(set(lens[:, 0] % 16)) == list(range(16))
    assert (lens[:, 0] == 16).any() and (lens[:, 0] == 32).any()   # whole chunks, no tail
    assert (lens[:, 1] == 0).any() and (lens[:, 1] > 0).any()
    assert not lens[:, 2].any()                                       # the rate-0 source
    assert torch.equal(fast.counts, log.counts)
    for i in (0, 1, 7, 150, R - 1, int(np.argmax(lens[:, 0])), int(np.argmin(lens[:, 0]))):
        u = seed0 + i
        (top, avg, r2, cnt), _ = O.engine_metrics(O.Scenario(_seeded(so, u), ("opt", u)), (1,))
        assert np.array_equal(fast.metrics[i].cpu().numpy(), np.asarray(list(top) + [avg, r2])), i
        c = fast.counts[i].cpu().numpy()
        assert c[0] == cnt[0] and c[1] == cnt[1] and c[3] == cnt[2], (i, c, cnt)


def test_stream_at_its_capacity():
    torch, engine, O = _ctx()
    so, R, seed0 = OVERFLOW, 64, 5
    g = _graph(engine, so)
    kw = dict(q=so["q"], s=so["s"], n_rep=R, ctrl_seed=seed0, world_seed=seed0, randomize=True, Ks=(1,))
    assert g.run("opt", plan_only=True, **kw)["variant"] >= 20
    log = g.run("opt", event_log=True, check=False, **kw)
    fast = g.run("opt", check=False, **kw)
    st = log.status.cpu().numpy()
    assert np.array_equal((fast.status.cpu().numpy() & ST_STREAM_OVERFLOW) != 0, (st & ST_STREAM_OVERFLOW) != 0)
    n_over = n_fit = 0
    for i in range(R):
        u = seed0 + i
        t_o, _, s_o = O.engine_run(O.Scenario(_seeded(so, u), ("opt", u), max_events=60000), cap=1 << 17)
        n_o = int((s_o == 2).sum())   # the oracle's stream (cut by its max_events far above the capacity)
        t, s = log.events(i)
        n = int((s == 2).sum())
        over = bool(st[i] & ST_STREAM_OVERFLOW)
        assert over == (n_o > HAWKES_CAP), (i, n_o, st[i])
        if not over:
            n_fit += 1
            assert st[i] == 0 and n == n_o
            assert np.array_equal(s, s_o) and np.array_equal(t, t_o), i
            if i % 8 == 0:
                (top, avg, r2, cnt), _ = O.engine_metrics(O.Scenario(_seeded(so, u), ("opt", u)), (1,))
                assert np.array_equal(fast.metrics[i].cpu().numpy(), np.asarray(list(top) + [avg, r2])), i
            continue
        n_over += 1
        # the stream holds its first HAWKES_CAP arrivals; the log shows them unless the
        # replica's rows or log ran out first (then a prefix of them)
        assert n <= HAWKES_CAP and (n == HAWKES_CAP or st[i] & 1), (i, n, st[i])
        assert np.array_equal(t[s == 2], t_o[s_o == 2][:n]), i
        if n:
            m = int(np.searchsorted(t_o, t[s == 2][-1], side="right"))   # the oracle's events up to there
            k = int(np.searchsorted(t, t[s == 2][-1], side="right"))
            assert k == m and np.array_equal(t[:k], t_o[:m]) and np.array_equal(s[:k], s_o[:m]), i
    assert n_over >= 8 and n_fit >= 8, (n_over, n_fit)

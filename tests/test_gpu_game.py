"""Competing RedQueen broadcasters on the GPU (rq_log_game, engine.Graph with ('Opt', kw)
among the other sources):
  a. the kernel's logs bit for bit against tests/game_ref.py, fed the GPU's own exogenous
     logs, at every edge of the kernel (window and output-line boundaries, ties at the start
     time, a post at exactly end_time, max_events, a short output, batch independence, the
     global-table path);
  b. the whole run against the existing engine: the game's posts handed back as dynamic
     RealData streams to the sequential sweep must give the same log, metrics and counts;
  c. the law of every player's posts by time rescaling (tests/lawcheck.py);
  d. the ensemble against the reference's own (tests/golden/dist_game.npz);
  e. the facade (Manager.run_dynamic, create_manager_for_wall, batch.run_grid, refusals)."""
import numpy as np
import pytest

import ensemble as E
import game_ref as G
import lawcheck as LC

pytestmark = pytest.mark.gpu
STRIDE = 100003


def _ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from redqueen_amd import engine
    return torch, engine


def _graph(engine, so, **kw):
    return engine.Graph(so["src_id"], so["other_sources"], so["sink_ids"], so["edge_list"],
                        so["end_time"], **kw)


# ------------------------------------------------------------------ worlds
def small_world(n_players, q=1.0, end_time=10.0, dup=False):
    """Poisson 10, Poisson2 11 and Hawkes 12 on sinks 1..4 (~ 230 exogenous events) and
    n_players Opts 20, 21, ...; Opt k follows sinks 1 + k % 4 and 1 + (k + 1) % 4.  The
    controlled slot (src_id 1) has no edge: the runs are create_manager_for_wall's."""
    others = [("Poisson", {"src_id": 10, "seed": 1, "rate": 10.0}),
              ("Poisson2", {"src_id": 11, "seed": 2, "rate": 10.0}),
              ("Hawkes", {"src_id": 12, "seed": 3, "l_0": 2.0, "alpha": 1.0, "beta": 4.0})]
    edges = [(10, 1), (10, 2), (11, 3), (11, 2), (12, 3), (12, 4)]
    if dup:
        edges.append((11, 3))   # a duplicated wall edge: its term counts twice
    for k in range(n_players):
        others.append(("Opt", {"src_id": 20 + k, "seed": 100 + k, "q": q, "s": [1.0, 0.5]}))
        edges += [(20 + k, 1 + k % 4), (20 + k, 1 + (k + 1) % 4)]
    return dict(src_id=1, q=1.0, s=[], end_time=end_time, sink_ids=[1, 2, 3, 4], other_sources=others,
                edge_list=edges)


def players_of(g):
    """[(src_id, q, s over the sorted followers)] of a graph's Opts, other_sources order."""
    return [(p["src_id"], p["q"], g._player_s(p["src_id"], p["s"])) for p in g.players]


def as_ref(players):
    return [{"src_id": a, "q": b, "s": list(c)} for a, b, c in players]


# ------------------------------------------------------------------ plumbing
def exo_of(torch, g, R, seed, ctrl="wall", **kw):
    """The exogenous logs of R replicas as host arrays (t [R, cap], j [R, cap], n [R])."""
    res = g._run(ctrl, n_rep=R, world_seed=seed, randomize=True, event_log=True, check=True,
                 stream=torch.cuda.current_stream(), **kw)
    return res.ev_t.cpu().numpy(), res.ev_src.cpu().numpy(), res.counts[:, 2].cpu().numpy().copy()


def launch(torch, g, players, seeds, t, j, n, max_events=None, out_cap=None):
    """rq_log_game on host logs; everything back on the host."""
    R = len(n)
    dev = torch.device("cuda", torch.cuda.current_device())
    counts = np.zeros((R, 4), dtype=np.int64)
    counts[:, 2] = n
    sd = torch.from_numpy(np.ascontiguousarray(np.asarray(seeds, dtype=np.int64).astype(np.uint32)
                                               .view(np.int32).reshape(R, len(players)))).to(dev)
    cap = int(out_cap) if out_cap is not None else int(t.shape[1]) + 4096
    out = g._game_launch(players, sd, torch.from_numpy(np.ascontiguousarray(t)).to(dev),
                         torch.from_numpy(np.ascontiguousarray(j)).to(dev), torch.from_numpy(counts).to(dev),
                         max_events, cap, torch.cuda.current_stream())
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out]


def ref_play(g, players, seeds_row, t, j, n, **kw):
    static = set(g.static_src_ids) | {g.src_id}
    return G.play(g.stream_src_ids, static, g._edges, as_ref(players), seeds_row, g.src_id,
                  g.start_time, g.end_time, t[:n], j[:n], **kw)


def same_replica(out, i, ref, players):
    """Replica i of a launch against game_ref: log bits, counts, posts, status."""
    ot, oj, cnt, posts, status = out
    rt, rj, rposts, rovf = ref
    m = len(rt)
    assert int(cnt[i, 2]) == m, (i, int(cnt[i, 2]), m)
    assert np.array_equal(ot[i, :m].view(np.int64), np.asarray(rt, dtype=np.float64).view(np.int64)), i
    assert np.array_equal(oj[i, :m], np.asarray(rj, dtype=np.int32)), i
    assert list(posts[i]) == rposts, (i, list(posts[i]), rposts)
    assert bool(status[i] & 1) == rovf, (i, status[i])
    assert int(cnt[i, 3]) == 0


def seeds_for(R, P, c=0):
    return (np.arange(R, dtype=np.int64)[:, None] * STRIDE + 99 * np.arange(P)[None, :] + c) & 0xFFFFFFFF


# ------------------------------------------------------------------ a. bit-exact
EXO_LENGTHS = (0, 1, 63, 64, 65, 129)


@pytest.mark.parametrize("P", [1, 2, 3, 64])
def test_players_and_exogenous_window_boundaries(P):
    """1, 2, 3 and 64 players against exogenous logs that end before, on and after the
    kernel's 64-entry window."""
    torch, engine = _ctx()
    g = _graph(engine, small_world(P, q=1.0 if P < 64 else 400.0))
    assert g.player_ids == [20 + k for k in range(P)]
    t, j, n = exo_of(torch, g, len(EXO_LENGTHS), 5)
    assert n.min() >= 129
    n = np.asarray(EXO_LENGTHS, dtype=np.int64)
    players, seeds = players_of(g), seeds_for(len(n), P, 5)
    me = None if P < 64 else 250
    out = launch(torch, g, players, seeds, t, j, n, max_events=me)
    for i in range(len(n)):
        ref = ref_play(g, players, seeds[i], t[i], j[i], int(n[i]), max_events=me)
        assert ref[0][:P] == [0.0] * P and ref[1][:P] == sorted(ref[1][:P])   # every Opt opens, in id order
        same_replica(out, i, ref, players)
    assert (out[4] == 0).all()


def test_max_events_and_output_line_boundaries():
    """max_events in {0, 1, n_players, 63, 64, 65 (outputs that end on the staged line's last
    entry, one short of it and one past it), a mid value, past the end}."""
    torch, engine = _ctx()
    from redqueen_amd import _lib as L
    g = _graph(engine, small_world(3))
    caps = [0, 1, 3, 63, 64, 65, 150, 10 ** 9]
    t, j, n = exo_of(torch, g, 1, 9)
    players, seeds = players_of(g), seeds_for(1, 3, 9)
    full = ref_play(g, players, seeds[0], t[0], j[0], int(n[0]))
    assert len(full[0]) > 150
    for me in caps:
        out = launch(torch, g, players, seeds, t, j, n, max_events=me)
        ref = ref_play(g, players, seeds[0], t[0], j[0], int(n[0]), max_events=me)
        assert len(ref[0]) == min(me, len(full[0])) and ref[0] == full[0][:len(ref[0])]
        same_replica(out, 0, ref, players)
        assert int(out[4][0]) == (L.ST_EMPTY if me == 0 else 0)
    # the exogenous pass honours max_events too: Graph.run gives the same prefix
    res = g.run("wall", n_rep=1, world_seed=9, randomize=True, event_log=True, max_events=65)
    assert int(res.counts[0, 2]) == 65
    # run()'s wall Opt seeds: u + 99 idx over other_sources (idx 3, 4, 5 here)
    ref = ref_play(g, players, [(9 + 99 * (3 + k)) & 0xFFFFFFFF for k in range(3)], t[0], j[0], int(n[0]),
                   max_events=65)
    assert np.array_equal(res.ev_t[0, :65].cpu().numpy(), np.asarray(ref[0]))
    assert res.player_posts[0].tolist() == ref[2]


def test_short_output_is_flagged_with_an_exact_prefix():
    torch, engine = _ctx()
    g = _graph(engine, small_world(2))
    t, j, n = exo_of(torch, g, 1, 11)
    players, seeds = players_of(g), seeds_for(1, 2, 11)
    full = ref_play(g, players, seeds[0], t[0], j[0], int(n[0]))
    m = len(full[0])
    exact = launch(torch, g, players, seeds, t, j, n, out_cap=m)
    same_replica(exact, 0, full, players)
    assert int(exact[4][0]) == 0
    short = launch(torch, g, players, seeds, t, j, n, out_cap=m - 1)
    same_replica(short, 0, ref_play(g, players, seeds[0], t[0], j[0], int(n[0]), out_cap=m - 1), players)
    assert int(short[4][0]) & 1 and int(short[2][0, 2]) == m - 1
    assert np.array_equal(short[0][0, :m - 1], exact[0][0, :m - 1])
    # Graph.run(check=True) reruns flagged replicas at doubled capacity: the same logs
    kw = dict(n_rep=5, world_seed=11, randomize=True, event_log=True, Ks=(1, 2))
    res = g.run("wall", **kw)
    assert int(res.status.max()) == 0 and g.reruns == 0
    g.GAME_CAP_SQUEEZE = 0.02
    raw = g.run("wall", check=False, **kw)
    assert int((raw.status & 1).sum()) == 5
    sq = g.run("wall", **kw)
    assert g.reruns >= 5 and int(sq.status.max()) == 0
    nn = res.counts[:, 2].cpu().numpy()
    assert torch.equal(sq.counts, res.counts) and torch.equal(sq.metrics, res.metrics)
    assert torch.equal(sq.player_posts, res.player_posts)
    for i in range(5):
        assert torch.equal(sq.ev_t[i, :nn[i]], res.ev_t[i, :nn[i]])
        assert torch.equal(sq.ev_src[i, :nn[i]], res.ev_src[i, :nn[i]])


def test_special_players_and_a_duplicated_wall_edge():
    """A player nobody reaches opens and never posts again; two players with identical
    followers draw from their own seeds; a duplicated wall edge counts twice."""
    torch, engine = _ctx()
    so = small_world(2, dup=True)
    so["sink_ids"] = [1, 2, 3, 4, 5]
    so["other_sources"] += [("Opt", {"src_id": 30, "seed": 7, "q": 1.0, "s": {5: 3.0}}),     # alone on sink 5
                            ("Opt", {"src_id": 31, "seed": 8, "q": 2.0, "s": [1.0, 0.5]})]  # 20's followers
    so["edge_list"] += [(30, 5), (31, 1), (31, 2)]
    g = _graph(engine, so)
    players = players_of(g)
    assert [p[0] for p in players] == [20, 21, 30, 31]
    R = 4
    t, j, n = exo_of(torch, g, R, 13)
    seeds = seeds_for(R, 4, 13)
    seeds[:, 3] = seeds[:, 0]   # 31 shares 20's seed: the draws still differ by q
    out = launch(torch, g, players, seeds, t, j, n)
    for i in range(R):
        ref = ref_play(g, players, seeds[i], t[i], j[i], int(n[i]))
        same_replica(out, i, ref, players)
        assert ref[2][2] == 1 and ref[2][0] > 1 and ref[2][3] > 1
    C, _ = G.rate_table(g.stream_src_ids, g._edges, as_ref(players))
    # 21 follows sinks 2 (s = 1) and 3 (s = 0.5) at q = 1; 11's edges by sink id: 2, 3, 3
    assert C[1][list(g.stream_src_ids).index(11)] == ((0.0 + 1.0) + np.sqrt(0.5)) + np.sqrt(0.5)


def test_ties_at_start_time():
    """A static RealData time at start_time plays after every opening post, a dynamic one
    among them by src_id."""
    torch, engine = _ctx()
    so = dict(src_id=1, q=1.0, s=[], end_time=4.0, sink_ids=[1, 2],
              other_sources=[("Opt", {"src_id": 2, "seed": 1, "q": 1.0, "s": 1.0}),
                             ("RealData", {"src_id": 3, "times": [0.0, 2.0], "dynamic": True}),
                             ("Opt", {"src_id": 5, "seed": 2, "q": 1.0, "s": 1.0}),
                             ("RealData", {"src_id": 7, "times": [0.0, 1.5]})],
              edge_list=[(2, 1), (3, 1), (3, 2), (5, 2), (7, 1), (7, 2)])
    g = _graph(engine, so)
    t, j, n = exo_of(torch, g, 1, 0)
    assert int(n[0]) == 4
    players, seeds = players_of(g), seeds_for(1, 2, 3)
    out = launch(torch, g, players, seeds, t, j, n)
    ref = ref_play(g, players, seeds[0], t[0], j[0], int(n[0]))
    same_replica(out, 0, ref, players)
    ids = [int(g.stream_src_ids[k]) for k in out[1][0, :4]]
    assert ids == [2, 3, 5, 7] and (out[0][0, :4] == 0.0).all()


def test_a_post_at_exactly_end_time_is_played():
    torch, engine = _ctx()
    so = small_world(2)
    g = _graph(engine, so)
    t, j, n = exo_of(torch, g, 1, 17)
    players, seeds = players_of(g), seeds_for(1, 2, 17)
    full = ref_play(g, players, seeds[0], t[0], j[0], int(n[0]))
    pj = [list(g.stream_src_ids).index(p[0]) for p in players]
    # the last post of a player in the run's first half: end the world exactly there
    k = max(i for i in range(len(full[0]) // 2) if full[1][i] in pj and full[0][i] > 0.0)
    t_end = full[0][k]
    keep = int(np.searchsorted(t[0, :n[0]], t_end, side="right"))
    for end, played in ((t_end, True), (np.nextafter(t_end, 0.0), False)):
        g2 = _graph(engine, dict(so, end_time=float(end)))
        assert list(g2.stream_src_ids) == list(g.stream_src_ids)
        nk = np.asarray([min(keep, int(np.searchsorted(t[0, :n[0]], end, side="right")))])
        out = launch(torch, g2, players, seeds, t, j, nk)
        ref = ref_play(g2, players, seeds[0], t[0], j[0], int(nk[0]))
        same_replica(out, 0, ref, players)
        m = int(out[2][0, 2])
        assert (out[0][0, :m] == t_end).any() == played
        assert out[0][0, :m].max() <= end and m >= k


def test_a_replica_alone_in_a_batch_and_in_a_permuted_batch():
    torch, engine = _ctx()
    g = _graph(engine, small_world(3))
    R = 9
    t, j, n = exo_of(torch, g, R, 21)
    players, seeds = players_of(g), seeds_for(R, 3, 21)
    batch = launch(torch, g, players, seeds, t, j, n)
    perm = np.asarray([4, 8, 0, 3, 7, 2, 6, 1, 5])
    shuf = launch(torch, g, players, seeds[perm], t[perm], j[perm], n[perm])
    same_replica(batch, 0, ref_play(g, players, seeds[0], t[0], j[0], int(n[0])), players)
    for k, i in enumerate(perm):
        m = int(batch[2][i, 2])
        assert np.array_equal(batch[2][i], shuf[2][k]) and np.array_equal(batch[3][i], shuf[3][k])
        assert np.array_equal(batch[0][i, :m], shuf[0][k, :m]) and np.array_equal(batch[1][i, :m], shuf[1][k, :m])
    for i in (0, 5, 8):
        one = launch(torch, g, players, seeds[i:i + 1], t[i:i + 1], j[i:i + 1], n[i:i + 1])
        m = int(batch[2][i, 2])
        assert int(one[2][0, 2]) == m and np.array_equal(one[0][0, :m], batch[0][i, :m])
        assert np.array_equal(one[1][0, :m], batch[1][i, :m]) and np.array_equal(one[3][0], batch[3][i])


@pytest.mark.parametrize("n_wall,P", [(536, 64), (2998, 2)])
def test_wide_graphs_global_and_lds_tables(n_wall, P):
    """601 streams x 64 players: the inverse table (300 KiB) is read from global memory;
    3001 streams x 2 players: 47 KiB, in LDS."""
    torch, engine = _ctx()
    from redqueen_amd import _lib as L
    so = small_world(P, q=400.0 if P == 64 else 1.0, end_time=4.0)
    for k in range(n_wall - 3):
        so["other_sources"].append(("Poisson", {"src_id": 1000 + k, "seed": k, "rate": 20.0 / n_wall}))
        so["edge_list"].append((1000 + k, 1 + k % 4))
    g = _graph(engine, so)
    assert g.n_streams == n_wall + P + 1
    assert L.lib().rq_log_game_table_in_lds(g._h, P) == (0 if P == 64 else 1)
    R = 2
    t, j, n = exo_of(torch, g, R, 23)
    players, seeds = players_of(g), seeds_for(R, P, 23)
    out = launch(torch, g, players, seeds, t, j, n, max_events=200)
    for i in range(R):
        same_replica(out, i, ref_play(g, players, seeds[i], t[i], j[i], int(n[i]), max_events=200), players)


def test_w5_run_matches_game_ref():
    """Graph.run end to end on W5 (the controlled RedQueen is the third player, seeded by
    ctrl_seed; wall Opts by u + 99 idx): the log, the posts and the counts."""
    torch, engine = _ctx()
    so = G.w5()
    g = _graph(engine, so)
    R = 6
    u = torch.arange(R, dtype=torch.int64) * STRIDE + 3
    res = g.run("opt", q=so["q"], s=so["s"], n_rep=R, ctrl_seed=u, world_seed=u, randomize=True,
                Ks=(1, 2), event_log=True)
    assert res.player_ids == [4, 5, 1] and g.player_ids == [4, 5]
    t, j, n = exo_of(torch, g, R, u)
    players = players_of(g) + [(1, so["q"], np.asarray(so["s"]))]
    un = u.numpy()
    for i in range(R):
        sd = [(un[i] + 99 * 2) & 0xFFFFFFFF, (un[i] + 99 * 3) & 0xFFFFFFFF, un[i] & 0xFFFFFFFF]
        rt, rj, posts, _ = ref_play(g, players, sd, t[i], j[i], int(n[i]))
        m = len(rt)
        assert int(res.counts[i, 2]) == m and res.player_posts[i].tolist() == posts
        assert np.array_equal(res.ev_t[i, :m].cpu().numpy(), np.asarray(rt))
        assert np.array_equal(res.ev_src[i, :m].cpu().numpy(), np.asarray(rj, dtype=np.int32))
        ids = g.stream_src_ids[np.asarray(rj)]
        assert list(zip(rt[:3], ids[:3])) == [(0.0, 1), (0.0, 4), (0.0, 5)]
        assert int(res.counts[i, 0]) == posts[2] and int(res.counts[i, 1]) == m - posts[2]


# ------------------------------------------------------------------ b. through the engine
def test_game_log_replayed_by_the_sequential_sweep():
    """W5 with a Poisson controlled source: the game's posts of 4 and 5 as dynamic RealData
    streams of the plain replay graph on the exact sequential sweep give the same event
    log bit for bit, and the same metrics and counts."""
    torch, engine = _ctx()
    so = G.w5()
    g = _graph(engine, so)
    R, Ks = 32, (1, 2)
    u = torch.arange(R, dtype=torch.int64) * STRIDE + 29
    kw = dict(n_rep=R, ctrl_seed=u, world_seed=u, randomize=True, ctrl_rate=[2.5], Ks=Ks, event_log=True)
    game = g.run("poisson", **kw)
    plain = dict(so, other_sources=[(k, v) if k != "Opt" else
                                    ("RealData", {"src_id": v["src_id"], "times": [], "dynamic": True})
                                    for k, v in so["other_sources"]])
    gp = _graph(engine, plain)
    assert list(gp.stream_src_ids) == list(g.stream_src_ids)
    n = game.counts[:, 2].cpu().numpy()
    et, ej = game.ev_t.cpu().numpy(), game.ev_src.cpu().numpy()
    sid = g.stream_src_ids
    times, off, caps = [], [0], [0, 0]
    for i in range(R):
        for k, c in enumerate((4, 5)):
            x = et[i, :n[i]][sid[ej[i, :n[i]]] == c]
            assert x.size == int(game.player_posts[i, k])
            times.append(x)
            off.append(off[-1] + x.size)
            caps[k] = max(caps[k], x.size)
    td = torch.from_numpy(np.concatenate(times + [np.zeros(1)])).cuda()
    od = torch.from_numpy(np.asarray(off, dtype=np.int64)).cuda()
    seq = gp.run("poisson", sweep_mode=2, rd_streams=([4, 5], td, od, caps), **kw)
    assert torch.equal(seq.counts[:, :3], game.counts[:, :3]), (seq.counts[:4], game.counts[:4])
    for i in range(R):
        assert torch.equal(seq.ev_t[i, :n[i]], game.ev_t[i, :n[i]]), i
        assert torch.equal(seq.ev_src[i, :n[i]], game.ev_src[i, :n[i]]), i
    assert torch.equal(seq.metrics, game.metrics), (seq.metrics - game.metrics).abs().max()
    assert torch.equal(seq.counts, game.counts)


# ------------------------------------------------------------------ c. the law
def _logs(res):
    n = res.counts[:, 2].cpu().numpy()
    N = int(n.max())
    idx = res.ev_src[:, :N].cpu().numpy().astype(np.int64)
    pad = np.arange(N)[None, :] >= n[:, None]
    src = res.graph.stream_src_ids[np.where(pad, 0, idx)]
    return LC.from_padded(res.ev_t[:, :N].cpu().numpy(), src, n)


def _family(name, so, players, logs, q_scale=1.0):
    fam = LC.Family(name)
    for p in players:
        view = dict(src_id=p["src_id"], q=p["q"] * q_scale, s=p["s"], edge_list=so["edge_list"],
                    end_time=so["end_time"])
        c = LC.controller(logs, view, ("opt", 0), name="opt %d" % p["src_id"])
        fam.fixed_m(c.name, c, 10)   # asserts that every replica reaches m = 10
        fam.martingale(c.name, c)
    return fam


def test_law_of_every_player():
    """2000 replicas of W5: each of 1, 4 and 5 posts with its own u_c(t); q x 1.25 is rejected."""
    torch, engine = _ctx()
    so = G.w5()
    R = 2000
    u = torch.from_numpy(np.arange(R, dtype=np.int64) * STRIDE + 31)
    res = _graph(engine, so).run("opt", q=so["q"], s=so["s"], n_rep=R, ctrl_seed=u, world_seed=u,
                                 randomize=True, Ks=(1,), event_log=True, check=True)
    assert int((res.status & ~4).abs().max().item()) == 0
    logs = _logs(res)
    players = G.w5_players(so)
    _family("game W5", so, players, logs).check()
    for p in players:
        wrong = _family("q x 1.25, player %d" % p["src_id"], so, [p], logs, q_scale=1.25)
        wrong.report()
        assert wrong.rejects()


# ------------------------------------------------------------------ d. the reference's ensemble
def test_w5_ensemble_vs_reference(golden):
    """10,000 engine replicas (seeds u = r, as the fixture's) against the reference's own."""
    torch, engine = _ctx()
    d = golden("dist_game.npz")
    assert d["data"].shape[0] >= 10000
    ref = {str(c): d["data"][:, i] for i, c in enumerate(d["cols"])}
    so = G.w5()
    g = _graph(engine, so)
    R = 10000
    u = torch.arange(R, dtype=torch.int64)
    res = g.run("opt", q=so["q"], s=so["s"], n_rep=R, ctrl_seed=u, world_seed=u, randomize=True,
                Ks=(1,), event_log=True)
    assert int((res.status & ~4).abs().max().item()) == 0
    n = res.counts[:, 2].cpu().numpy()
    ids = torch.from_numpy(g.stream_src_ids).cuda()[res.ev_src.long().clamp(0, g.n_streams - 1)]
    live = torch.arange(res.ev_src.shape[1], device="cuda")[None, :] < torch.from_numpy(n).cuda()[:, None]
    eng = {"posts%d" % k: ((ids == k) & live).sum(1).double().cpu().numpy() for k in range(1, 6)}
    assert np.array_equal(eng["posts4"], res.player_posts[:, 0].double().cpu().numpy())
    assert np.array_equal(eng["posts1"], res.counts[:, 0].double().cpu().numpy())
    eng.update(top1=res.metrics[:, 0].cpu().numpy(), avg=res.metrics[:, 1].cpu().numpy(),
               r2=res.metrics[:, 2].cpu().numpy())
    E.compare("gpu_game_w5", eng, ref, alpha=0.01, clusters=99)


# ------------------------------------------------------------------ e. the facade
def test_manager_run_dynamic_and_utils():
    torch, engine = _ctx()
    from redqueen_amd import utils as U
    from redqueen_amd.opt_model import SimOpts
    so = SimOpts(**G.w5())
    m = so.create_manager_with_opt(seed=7)
    m.run_dynamic()
    df = m.state.get_dataframe()
    ev = df.groupby("event_id", sort=True).first()
    assert list(zip(ev.t.values[:3], ev.src_id.values[:3])) == [(0.0, 1), (0.0, 4), (0.0, 5)]
    assert set(df.src_id.unique()) == {1, 2, 3, 4, 5}
    assert U.time_in_top_k(df, K=1, sim_opts=so) == float(m.result.metrics[0, 0])
    assert U.average_rank(df, sim_opts=so) == float(m.result.metrics[0, 1])
    assert m.result.player_ids == [4, 5, 1]
    # max_events is honoured
    m2 = so.create_manager_with_opt(seed=7)
    m2.run_dynamic(max_events=40)
    assert int(m2.result.counts[0, 2]) == 40
    assert np.array_equal(m2.result.ev_t[0, :40].cpu().numpy(), m.result.ev_t[0, :40].cpu().numpy())


def test_create_manager_for_wall_plays_the_opts_against_each_other():
    torch, engine = _ctx()
    from redqueen_amd.opt_model import SimOpts
    so = SimOpts(**G.w5())
    m = so.create_manager_for_wall()
    m.run_dynamic()
    df = m.state.get_dataframe()
    ev = df.groupby("event_id", sort=True).first()
    assert list(zip(ev.t.values[:2], ev.src_id.values[:2])) == [(0.0, 4), (0.0, 5)]
    assert set(df.src_id.unique()) == {2, 3, 4, 5}
    assert m.result.player_ids == [4, 5] and (m.result.player_posts[0] > 1).all()


def test_run_grid_and_refusals():
    torch, engine = _ctx()
    from redqueen_amd import batch
    from redqueen_amd.opt_model import Poisson2, SimOpts
    d = G.w5()
    df = batch.run_grid(SimOpts(**d), qs=[0.25, 4.0], seeds=range(8), Ks=(1,))
    assert len(df) == 16 and sorted(df.q.unique()) == [0.25, 4.0]
    assert np.isfinite(df.top_1.values).all() and (df.events > 0).all()
    assert df[df.q == 0.25].num_events.sum() > df[df.q == 4.0].num_events.sum()
    # a dict s of an Opt is part of the graph cache's key
    d2 = dict(d, other_sources=d["other_sources"][:3] + [("Opt", {"src_id": 5, "seed": 4, "s": {102: 9.0}, "q": 2.0})])
    assert batch._key(SimOpts(**d2)) != batch._key(SimOpts(**dict(
        d, other_sources=d["other_sources"][:3] + [("Opt", {"src_id": 5, "seed": 4, "s": {102: 1.0}, "q": 2.0})])))
    g = _graph(engine, d)
    with pytest.raises(NotImplementedError):
        g.run("sig", q=1.0, s_pw=np.ones((3, 2)), period=5.0)
    with pytest.raises(NotImplementedError):
        g.run("opt", q=1.0, s=d["s"], n_rep=4, rep_idx=[1, 2])
    with pytest.raises(NotImplementedError):
        g.run("opt", q=1.0, s=d["s"], n_rep=4, sweep_mode=2)

    class Every(Poisson2):   # a registered static plugin: its own times
        _rq_kind = None

        def initialize(self):
            pass

        def get_all_times(self):
            return np.arange(1.0, 19.0)
    gp = _graph(engine, dict(d, other_sources=d["other_sources"] + [(Every, {"src_id": 9, "seed": 1})],
                             edge_list=d["edge_list"] + [(9, 101)]))
    with pytest.raises(NotImplementedError):
        gp.run("opt", q=1.0, s=d["s"])

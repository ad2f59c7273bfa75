"""tests/game_ref.py -- the host restatement of rq_log_game the GPU tests compare against --
checked on its own, without a GPU: its Philox against Random123's known answers, its log
against libm, and the law of the logs it plays (tests/lawcheck.py): every RedQueen
broadcaster of world W5 must post with intensity u_c(t) = sum_f sqrt(s_cf / q_c) r_cf(t)."""
import math
import struct

import numpy as np

import game_ref as G
import lawcheck as LC


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 at 10 rounds."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, out in kat:
        assert G.philox4x32_10(ctr, key) == out


def _ulps(a, b):
    ia, ib = (struct.unpack("<q", struct.pack("<d", x))[0] for x in (a, b))
    return abs(ia - ib)


def test_rq_log_within_one_ulp():
    rng = np.random.default_rng(7)
    # the arguments the draws give (1 - u, u a 53-bit uniform) and twenty decades around them
    xs = np.concatenate([1.0 - rng.random(5000), np.exp(rng.uniform(-700.0, 700.0, 5000))])
    worst = max(_ulps(G.rq_log(float(x)), math.log(float(x))) for x in xs)
    assert worst <= 1, worst
    assert G.rq_log(1.0) == 0.0 and G.uniform53(0xFFFFFFFF, 0xFFFFFFFF) < 1.0
    assert G.uniform53(0, 0) == 0.0 and G.std_exponential(0.0) == 0.0


def test_rate_table_by_hand():
    so = G.w5()
    C, inv = G.rate_table([3, 4, 5, 1, 2], so["edge_list"], G.w5_players(so))
    # player 1 follows 101, 102, 103 at weight 1; 4 follows 101 (2 / 0.5) and 103 (0.5 / 0.5);
    # 5 follows 102 at sqrt(1 / 2)
    assert C[0] == [2.0, 2.0, 1.0, 0.0, 2.0]
    assert C[1] == [1.0, 0.0, 0.0, 2.0 + 1.0, 2.0]
    r = math.sqrt(0.5)
    assert C[2] == [r, 0.0, 0.0, r, r]
    assert inv[1][1] == 0.0 and inv[2][0] == 1.0 / r
    # a duplicated wall edge adds its term again, in ascending sink id
    C2, _ = G.rate_table([2, 4], [(4, 101), (4, 103), (2, 103), (2, 101), (2, 103)],
                         [{"src_id": 4, "q": 0.5, "s": [2.0, 0.5]}])
    assert C2[0][0] == (0.0 + 2.0) + 1.0 + 1.0 and C2[0][1] == 0.0


R_LAW = 200
STRIDE = 100003


def _w5_logs():
    """R_LAW replicas of W5 from game_ref, the exogenous sources 2 and 3 as numpy Poisson
    arrivals (the players' law conditions on the wall, whatever it is)."""
    so = G.w5()
    players = G.w5_players(so)
    stream_ids = [3, 4, 5, 1, 2]          # dynamic by src_id, then static by src_id
    rng = np.random.default_rng(20)
    logs = []
    for r in range(R_LAW):
        parts = []
        for j, rate in ((4, 3.0), (0, 2.0)):
            n = rng.poisson(rate * so["end_time"])
            parts.append((np.sort(rng.uniform(0.0, so["end_time"], n)), np.full(n, j)))
        t = np.concatenate([p[0] for p in parts])
        j = np.concatenate([p[1] for p in parts])
        o = np.lexsort((j, t))
        seeds = [STRIDE * r + 5, STRIDE * r + 5 + 99 * 2, STRIDE * r + 5 + 99 * 3]
        ot, oj, posts, ovf = G.play(stream_ids, {2}, so["edge_list"], players, seeds, 1, 0.0,
                                    so["end_time"], t[o], j[o])
        assert not ovf and posts == [oj.count(3), oj.count(1), oj.count(2)]
        assert list(zip(ot[:3], oj[:3])) == [(0.0, 3), (0.0, 1), (0.0, 2)]   # 1, 4, 5 open in id order
        assert all(b >= a for a, b in zip(ot, ot[1:])) and ot[-1] <= so["end_time"]
        logs.append((np.asarray(ot), np.asarray([stream_ids[k] for k in oj])))
    return so, players, LC.pack(logs)


def _family(name, so, players, logs, q_scale=1.0):
    fam = LC.Family(name)
    for p in players:
        view = dict(src_id=p["src_id"], q=p["q"] * q_scale, s=p["s"], edge_list=so["edge_list"],
                    end_time=so["end_time"])
        c = LC.controller(logs, view, ("opt", 0), name="opt %d" % p["src_id"])
        fam.fixed_m(c.name, c, 10)
        fam.martingale(c.name, c)
    return fam


def test_every_player_posts_by_its_law_and_a_wrong_q_is_rejected():
    so, players, logs = _w5_logs()
    _family("game_ref W5", so, players, logs).check()
    for p in players:   # the wrong law q x 1.25, each player on its own
        wrong = _family("q x 1.25, player %d" % p["src_id"], so, [p], logs, q_scale=1.25)
        wrong.report()
        assert wrong.rejects()

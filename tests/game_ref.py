"""Host restatement of rq_log_game (include/rq.h): Philox4x32-10, rq_uniform53, rq_log, the
players' rate table and the play rule, in Python ints and IEEE doubles (Python floats: every
+ - * / rounds once, nothing is contracted).  Shares no code with librq or oracle/."""
import math
import struct

M32 = 0xFFFFFFFF
INF = float("inf")
SRC_OPT = 6


def w5():
    """The world of the game tests: RedQueen 1 against Poisson2 2, Hawkes 3 and the Opts 4
    and 5 on three sinks, T = 20."""
    return dict(
        src_id=1, q=1.0, s=[1.0, 1.0, 1.0], end_time=20.0, sink_ids=[101, 102, 103],
        other_sources=[("Poisson2", {"src_id": 2, "seed": 1, "rate": 3.0}),
                       ("Hawkes", {"src_id": 3, "seed": 2, "l_0": 2.0, "alpha": 1.0, "beta": 4.0}),
                       ("Opt", {"src_id": 4, "seed": 3, "s": [2.0, 0.5], "q": 0.5}),
                       ("Opt", {"src_id": 5, "seed": 4, "s": 1.0, "q": 2.0})],
        edge_list=[(1, 101), (1, 102), (1, 103), (2, 101), (2, 102), (3, 102), (3, 103), (4, 101),
                   (4, 103), (5, 102)])


def w5_players(so=None):
    """[{src_id, q, s}] of W5's three RedQueen broadcasters: 1, 4, 5."""
    so = so or w5()
    out = [{"src_id": so["src_id"], "q": so["q"], "s": so["s"]}]
    out += [{"src_id": kw["src_id"], "q": kw["q"], "s": kw["s"]}
            for kind, kw in so["other_sources"] if kind == "Opt"]
    return out


# ------------------------------------------------------------------ Philox4x32-10
def philox4x32_10(ctr, key):
    """Salmon et al., SC'11: ctr 4 x uint32, key 2 x uint32 -> 4 x uint32."""
    c0, c1, c2, c3 = (int(x) & M32 for x in ctr)
    k0, k1 = (int(x) & M32 for x in key)
    for _ in range(10):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def uniform53(a, b):
    """numpy's legacy random_sample(): 53 bits of two words, in [0, 1)."""
    return (float(a >> 5) * 67108864.0 + float(b >> 6)) / 9007199254740992.0


# ------------------------------------------------------------------ rq_log
def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _dbl(u):
    return struct.unpack("<d", struct.pack("<Q", u & 0xFFFFFFFFFFFFFFFF))[0]


def rq_log(x):
    """The engine's natural log (fdlibm's reduction and series) for finite x > 0."""
    ln2_hi = 6.93147180369123816490e-01
    ln2_lo = 1.90821492927058770002e-10
    Lg1, Lg2, Lg3, Lg4 = 6.666666666666735130e-01, 3.999999999940941908e-01, \
        2.857142874366239149e-01, 2.222219843214978396e-01
    Lg5, Lg6, Lg7 = 1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01
    if not x > 0.0:
        return -INF if x == 0.0 else float("nan")
    ux = _bits(x)
    if (ux >> 52) >= 0x7FF:
        return x + x
    k = 0
    if (ux >> 52) == 0:
        x = x * 18014398509481984.0
        ux = _bits(x)
        k = -54
    hx = ux >> 32
    k += (hx >> 20) - 1023
    hx &= 0x000FFFFF
    i = (hx + 0x95F64) & 0x100000
    um = ((hx | (i ^ 0x3FF00000)) << 32) | (ux & M32)
    k += i >> 20
    f = _dbl(um) - 1.0
    dk = float(k)
    s = f / (2.0 + f)
    z = s * s
    w = z * z
    t1 = w * (Lg2 + w * (Lg4 + w * Lg6))
    t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)))
    R = t2 + t1
    hfsq = 0.5 * f * f
    if f == 0.0:
        return dk * ln2_hi + dk * ln2_lo
    return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f)


def std_exponential(u):
    return -rq_log(1.0 - u)


def kind_salt(kind, ctrl):
    return 0x52510000 | kind | (0x100 if ctrl else 0)


def draw(seed, ctrl, e):
    """The Exp(1) draw of a player (seed, is it the controlled source) at output event e."""
    w = philox4x32_10((e & M32, (e >> 32) & M32, 0, 0), (seed, kind_salt(SRC_OPT, ctrl)))
    return std_exponential(uniform53(w[0], w[1]))


# ------------------------------------------------------------------ the rate table
def followers_of(src_id, edges):
    return sorted({int(x) for a, x in edges if int(a) == int(src_id)})


def s_vector(s, followers):
    """s as the reference's Opt takes it: scalar, array over the sorted followers, dict."""
    if isinstance(s, dict):
        return [float(s[x]) for x in followers]
    try:
        v = [float(x) for x in s]
    except TypeError:
        return [float(s)] * len(followers)
    if len(v) == 1:
        v = v * len(followers)
    assert len(v) == len(followers)
    return v


def rate_table(stream_ids, edges, players):
    """C[c][j] over the streams in ``stream_ids`` order for players [{src_id, q, s}, ...]
    (s over the player's sorted followers), and inv = 1 / C (0 where C is 0).  The terms
    add one by one in ascending sink id, a duplicated edge again."""
    C, inv = [], []
    sinks_of = {}
    for a, b in edges:
        sinks_of.setdefault(int(a), []).append(int(b))
    for v in sinks_of.values():
        v.sort()
    for p in players:
        fol = followers_of(p["src_id"], edges)
        sv = s_vector(p["s"], fol)
        w = {x: math.sqrt(sv[k] / float(p["q"])) for k, x in enumerate(fol)}
        row = []
        for j in stream_ids:
            c = 0.0
            if int(j) != int(p["src_id"]):
                for x in sinks_of.get(int(j), ()):
                    if x in w:
                        c = c + w[x]
            row.append(c)
        C.append(row)
        inv.append([1.0 / c if c > 0.0 else 0.0 for c in row])
    return C, inv


# ------------------------------------------------------------------ the play rule
def play(stream_ids, static_ids, edges, players, seeds, ctrl_src_id, start, end, exo_t, exo_j,
         max_events=None, out_cap=None):
    """The completed log of one replica.  stream_ids: src_id per stream index;
    static_ids: src_ids of the static streams; players: [{src_id, q, s}] in seed order;
    exo_t / exo_j: the exogenous log (times, stream indices).
    Returns (t, j, posts per player, overflow)."""
    stream_ids = [int(x) for x in stream_ids]
    P = len(players)
    _C, inv = rate_table(stream_ids, edges, players)
    pj = [stream_ids.index(int(p["src_id"])) for p in players]
    order = sorted(range(P), key=lambda c: int(players[c]["src_id"]))
    T = [float(start)] * P
    posts = [0] * P
    out_t, out_j = [], []
    k, n = 0, len(exo_t)
    while True:
        e = len(out_t)
        if max_events is not None and e >= max_events:
            break
        cm = None
        for c in order:   # least (T, src_id)
            if cm is None or T[c] < T[cm]:
                cm = c
        due = T[cm] <= end
        if k < n:
            te, je = float(exo_t[k]), int(exo_j[k])
            player = False
            if due and T[cm] <= te:
                first = stream_ids[je] in static_ids or int(players[cm]["src_id"]) < stream_ids[je]
                player = T[cm] < te or first
        else:
            if not due:
                break
            player = True
        if out_cap is not None and e >= out_cap:
            return out_t, out_j, posts, True
        if player:
            t, j = T[cm], pj[cm]
            posts[cm] += 1
        else:
            t, j = te, je
            k += 1
        for c in range(P):
            if pj[c] == j:
                T[c] = INF
            elif inv[c][j] > 0.0:
                x = draw(int(seeds[c]), int(players[c]["src_id"]) == int(ctrl_src_id), e)
                cand = t + x * inv[c][j]
                if cand < T[c]:
                    T[c] = cand
        out_t.append(t)
        out_j.append(j)
    return out_t, out_j, posts, False

"""Law checks by time rescaling (test helper, like ensemble.py; not a conftest).

For a point process with conditional intensity lambda(t), the compensator increments
between consecutive points, Lambda(t_i) - Lambda(t_{i-1}), are iid Exp(1) (the
time-rescaling theorem).  This module rebuilds every compensator from the event log
``(t, src_id)`` and the USER-VISIBLE parameters alone -- ``l_0 / alpha / beta``,
``rate``, ``change_times / rates``, ``q / s``, ``s_pw / period`` and the edge list -- in
float64 numpy.  It shares nothing with the engine, its generators, its math functions
or the oracle: an error both of those make identically is still an error here.

Censoring at ``end_time`` is handled exactly, never ignored:

* fixed-m: the first m increments of every (replica, process), m chosen so that every
  replica reaches it (asserted, never silently dropped) -> KS against Exp(1), a z-test
  of the mean (sigma = 1 / sqrt(N)) and a lag-1 correlation of 1 - exp(-x) (independence);
* count martingale: z = sum(N(T) - Lambda(T)) / sqrt(sum Lambda(T)), Lambda(T) including
  the censored tail -- exact in mean for every kind, sees the end-of-horizon edge;
* sparse Poisson kinds: Lambda(t_i) / Lambda(T) against Uniform(0, 1), exact given N.

All arrays are over replicas; loops run over the event index only.
"""
import numpy as np
from scipy import stats


# --------------------------------------------------------------------------- logs
class Logs:
    """Event logs of R replicas, padded: ``t`` [R, N] (padding +inf), ``src`` [R, N]
    source ids (padding -1), ``n`` [R] events per replica."""

    def __init__(self, t, src, n):
        self.t = np.asarray(t, dtype=np.float64)
        self.src = np.asarray(src, dtype=np.int64)
        self.n = np.asarray(n, dtype=np.int64)
        self.R = self.t.shape[0]

    def subset(self, rows):
        return Logs(self.t[rows], self.src[rows], self.n[rows])


def pack(logs):
    """[(t, src_id) per replica] -> Logs."""
    R = len(logs)
    n = np.asarray([len(t) for t, _ in logs], dtype=np.int64)
    N = int(n.max()) if R else 0
    T = np.full((R, N), np.inf)
    S = np.full((R, N), -1, dtype=np.int64)
    for r, (t, s) in enumerate(logs):
        T[r, :n[r]] = t
        S[r, :n[r]] = s
    return Logs(T, S, n)


def from_padded(t, src, n):
    """Arrays [R, cap] whose row r holds n[r] events (the rest is garbage) -> Logs."""
    n = np.asarray(n, dtype=np.int64)
    N = int(n.max()) if n.size else 0
    pad = np.arange(N)[None, :] >= n[:, None]
    T = np.array(t[:, :N], dtype=np.float64)
    S = np.array(src[:, :N], dtype=np.int64)
    T[pad] = np.inf
    S[pad] = -1
    return Logs(T, S, n)


def source_times(logs, src_id):
    """Arrival times of one source: (times [R, K] padded with NaN, n [R])."""
    mask = logs.src == src_id
    n = mask.sum(1)
    K = int(n.max()) if n.size else 0
    out = np.full((logs.R, K), np.nan)
    pos = np.cumsum(mask, 1) - 1
    rows, cols = np.nonzero(mask)
    out[rows, pos[rows, cols]] = logs.t[rows, cols]
    return out, n


# --------------------------------------------------------------------------- compensators
class Proc:
    """One process over R replicas: ``inc`` [R, K] compensator increments between
    consecutive points (the first from start_time; NaN past n), ``n`` [R] points,
    ``tail`` [R] the censored increment from the last point to end_time."""

    def __init__(self, name, inc, n, tail):
        self.name, self.inc, self.n, self.tail = name, inc, np.asarray(n, dtype=np.int64), tail

    @property
    def total(self):
        """Lambda(T) per replica."""
        return np.nansum(self.inc, 1) + self.tail


def _from_cumulative(name, times, n, lam, start, end):
    """A process whose compensator Lambda(t) is a closed form ``lam``."""
    L = lam(times)
    L0 = lam(np.full(times.shape[0], float(start)))
    inc = np.diff(np.concatenate([L0[:, None], L], 1), axis=1)
    last = np.where(n > 0, np.nanmax(np.concatenate([L0[:, None], L], 1), 1), L0)
    tail = lam(np.full(times.shape[0], float(end))) - last
    return Proc(name, inc, n, tail)


def poisson(name, times, n, rate, start, end):
    """Lambda(t) = rate (t - start); ``rate`` a scalar or per replica [R]."""
    rate = np.asarray(rate, dtype=np.float64)

    def lam(t):
        return (rate[:, None] if (rate.ndim and t.ndim == 2) else rate) * (t - start)
    return _from_cumulative(name, times, n, lam, start, end)


def pw_rate(t, change_times, rates):
    """rates[bisect_right(change_times, t) - 1]; index -1 (t before the first change
    time) wraps to the last rate, as the reference's Python indexing does."""
    ct = np.asarray(change_times, dtype=np.float64)
    return np.asarray(rates, dtype=np.float64)[np.searchsorted(ct, t, side="right") - 1]


def pw_integral(t, change_times, rates, start):
    """Integral of pw_rate over [start, t]."""
    ct = np.asarray(change_times, dtype=np.float64)
    rt = np.asarray(rates, dtype=np.float64)
    lo = np.concatenate([[-np.inf], ct])
    hi = np.concatenate([ct, [np.inf]])
    val = np.concatenate([[rt[-1]], rt])
    t = np.asarray(t, dtype=np.float64)
    out = np.zeros_like(t)
    for a, b, v in zip(lo, hi, val):
        out = out + v * np.clip(np.minimum(t, b) - max(a, start), 0.0, None)
    return out


def pwconst(name, times, n, change_times, rates, start, end):
    return _from_cumulative(name, times, n,
                            lambda t: pw_integral(t, change_times, rates, start), start, end)


def hawkes(name, times, n, l_0, alpha, beta, start, end):
    """lambda(t) = l_0 + sum_i alpha exp(-beta (t - t_i)).  With eta the excitation just
    after the previous arrival, the increment over a gap d is
    l_0 d - (eta / beta) expm1(-beta d), and eta <- eta exp(-beta d) + alpha."""
    R, K = times.shape
    inc = np.full((R, K), np.nan)
    eta = np.zeros(R)
    tau = np.full(R, float(start))

    def step(d):
        if beta > 0.0:
            return l_0 * d - (eta / beta) * np.expm1(-beta * d)
        return (l_0 + eta) * d
    for k in range(K):
        ok = k < n
        d = np.where(ok, times[:, k] - tau, 0.0)
        inc[:, k] = np.where(ok, step(d), np.nan)
        eta = np.where(ok, eta * np.exp(-beta * d) + alpha, eta)
        tau = np.where(ok, times[:, k], tau)
    return Proc(name, inc, n, step(end - tau))


def hawkes_direct(times, l_0, alpha, beta, start, end):
    """O(n^2) compensator of ONE stream: over every gap (a, b], the integral of each
    earlier arrival's kernel summed directly (the unit check of the recurrence).
    Returns (increments [n], tail)."""
    t = np.asarray(times, dtype=np.float64)
    pts = np.concatenate([[start], t, [end]])
    inc = np.empty(len(pts) - 1)
    for k in range(len(pts) - 1):
        a, b = pts[k], pts[k + 1]
        past = t[:k]                       # arrivals at or before a
        inc[k] = l_0 * (b - a) + np.sum((alpha / beta) * np.exp(-beta * (a - past))
                                        * -np.expm1(-beta * (b - a)))
    return inc[:-1], inc[-1]


def followers_of(sim_opts):
    return sorted(e[1] for e in sim_opts["edge_list"] if e[0] == sim_opts["src_id"])


def _s_rows(sim_opts, fol, R):
    s = sim_opts["s"]
    if isinstance(s, dict):
        s = [s[f] for f in fol]
    s = np.asarray(s, dtype=np.float64)
    if s.ndim == 2:
        return s
    return np.broadcast_to(np.ones(len(fol)) * s, (R, len(fol)))


def controller(logs, sim_opts, ctrl, start=0.0, reset=True, name="ctrl"):
    """The controlled source's posts.  ``ctrl`` as oracle.Scenario takes it:
    ("opt", seed): u(t) = sum_f sqrt(s_f / q) r_f(t), q and s from ``sim_opts`` (a scalar
        / a row over the sorted followers, or per replica [R] / [R, F]);
    ("sig", seed, s_pw, period): the same with s_f(t) = s_pw[f][segment of t mod period];
    ("poisson", seed, rate): rate a scalar or [R].
    r_f(t): posts since the controlled source's last post (0 at ``start``) by OTHER
    sources with an edge to follower f, a duplicated edge counting twice -- rebuilt from
    the log and the edge list.  The post at t = start itself (the controller opens with
    one) is not a point of the process.  ``reset=False`` forgets to reset the ranks at an
    own post (a deliberately wrong law, for the power tests)."""
    own = sim_opts["src_id"]
    end = float(sim_opts["end_time"])
    R = logs.R
    kind = ctrl[0]
    if kind == "poisson":
        times, n = source_times(logs, own)
        return poisson(name, times, n, np.broadcast_to(np.asarray(ctrl[2], dtype=np.float64), (R,)),
                       start, end)
    fol = followers_of(sim_opts)
    F = len(fol)
    q = np.broadcast_to(np.asarray(sim_opts["q"], dtype=np.float64), (R,))
    ids = np.asarray(sorted({e[0] for e in sim_opts["edge_list"] if e[0] != own}), dtype=np.int64)
    # A[j, f]: edges from other source ids[j] to follower fol[f]; last row: no effect
    A = np.zeros((len(ids) + 1, F))
    for a, b in sim_opts["edge_list"]:
        if a != own and b in fol:
            A[np.searchsorted(ids, a), fol.index(b)] += 1.0
    j = np.full(logs.src.shape, len(ids), dtype=np.int64)
    for i, sid in enumerate(ids):
        j[logs.src == sid] = i
    if kind == "opt":
        w = np.sqrt(_s_rows(sim_opts, fol, R) / q[:, None])            # [R, F]

        def W(t):
            return w * t[:, None]
    elif kind == "sig":
        spw = np.atleast_2d(np.asarray(ctrl[2], dtype=np.float64))      # [F, S]
        T = float(ctrl[3])
        S = spw.shape[1]
        seg = T / S
        w = np.sqrt(spw[None, :, :] / q[:, None, None])                 # [R, F, S]
        cw = np.concatenate([np.zeros((R, F, 1)), np.cumsum(w, 2)], 2) * seg
        rows = np.arange(R)

        def W(t):
            per = np.floor(t / T)
            ph = t - per * T
            k = np.minimum((S * ph / T).astype(np.int64), S - 1)
            return (per[:, None] * cw[:, :, S] + cw[rows, :, k]
                    + w[rows, :, k] * (ph - k * seg)[:, None])
    else:
        raise ValueError(kind)
    N = logs.t.shape[1]
    t = np.minimum(logs.t, end)
    is_own = logs.src == own
    cnt_all = is_own.sum(1)
    inc = np.full((R, int(cnt_all.max()) if R else 0), np.nan)
    cnt = np.zeros(R, dtype=np.int64)
    r = np.zeros((R, F))
    acc = np.zeros(R)
    t_prev = np.full(R, float(start))
    W_prev = W(t_prev)
    for k in range(N):
        tk = t[:, k]
        Wk = W(tk)
        acc = acc + (r * (Wk - W_prev)).sum(1)
        o = is_own[:, k]
        if o.any():
            # the opening post at t = start is not a point of the process
            rec = o & ~((cnt == 0) & (tk == start))
            rr = np.flatnonzero(rec)
            inc[rr, cnt[rr]] = acc[rr]
            cnt[rr] += 1
            acc[o] = 0.0
            if reset:
                r[o] = 0.0
        r = r + A[j[:, k]]
        W_prev = Wk
    tail = acc + (r * (W(np.full(R, end)) - W_prev)).sum(1)
    return Proc(name, inc[:, :int(cnt.max()) if R else 0], cnt, tail)


def world(logs, sim_opts, start=0.0):
    """{src_id: Proc} of every Poisson / Poisson2 / Hawkes / PiecewiseConst source of
    ``sim_opts["other_sources"]`` (the reference's defaults for missing parameters)."""
    end = float(sim_opts["end_time"])
    out = {}
    for kind, kw in sim_opts["other_sources"]:
        sid = kw["src_id"]
        times, n = source_times(logs, sid)
        label = "%s#%d" % (kind, sid)
        if kind in ("Poisson", "Poisson2"):
            out[sid] = poisson(label, times, n, kw.get("rate", 1.0), start, end)
        elif kind == "Hawkes":
            out[sid] = hawkes(label, times, n, kw.get("l_0", 1.0), kw.get("alpha", 1.0),
                              kw.get("beta", 10.0), start, end)
        elif kind == "PiecewiseConst":
            out[sid] = pwconst(label, times, n, kw["change_times"], kw["rates"], start, end)
    return out


def perturbed(sim_opts, src_ids=None, **scale):
    """A copy of ``sim_opts`` with parameters scaled (alpha=1.05, rates=1.05, q=1.1 ...):
    the deliberately wrong laws of the power tests.  ``src_ids``: only these sources."""
    so = dict(sim_opts)
    if "q" in scale:
        so["q"] = np.asarray(so["q"], dtype=np.float64) * scale.pop("q")
    defaults = {"Hawkes": {"l_0": 1.0, "alpha": 1.0, "beta": 10.0}, "Poisson": {"rate": 1.0},
                "Poisson2": {"rate": 1.0}}
    others = []
    for kind, kw in so["other_sources"]:
        kw = dict(defaults.get(kind, {}), **kw)
        if src_ids is None or kw["src_id"] in src_ids:
            for key, f in scale.items():
                if key in kw:
                    v = np.asarray(kw[key], dtype=np.float64) * f
                    kw[key] = v.tolist() if v.ndim else float(v)
        others.append((kind, kw))
    so["other_sources"] = others
    return so


# --------------------------------------------------------------------------- statistics
def poisson_m(mu, n_streams, tail=1e-9):
    """The largest m with n_streams * P(Poisson(mu) < m) < tail: every one of n_streams
    independent streams of mean count mu reaches m arrivals."""
    m = int(stats.poisson.ppf(tail / n_streams, mu))
    while m > 0 and n_streams * stats.poisson.cdf(m - 1, mu) >= tail:
        m -= 1
    return m


def p_of_z(z):
    return float(2.0 * stats.norm.sf(abs(z)))


def fixed_m(procs, m):
    """The first m increments of every replica of every process in ``procs`` pooled:
    dict(N, ks_p, mean_z, lag1_z).  Every replica must have reached m."""
    if isinstance(procs, Proc):
        procs = [procs]
    rows = []
    for p in procs:
        short = np.flatnonzero(p.n < m)
        assert short.size == 0, "%s: replicas %s have fewer than m = %d points (min %d)" % (
            p.name, short[:8], m, int(p.n.min()))
        rows.append(p.inc[:, :m])
    x = np.concatenate(rows, 0)
    assert np.isfinite(x).all() and (x >= 0.0).all(), "a negative or non-finite increment"
    N = x.size
    v = -np.expm1(-x) - 0.5                       # uniform(-1/2, 1/2) under the law
    pairs = v[:, :-1] * v[:, 1:]                  # mean 0, variance 1 / 144, uncorrelated
    return dict(N=N, ks_p=float(stats.kstest(x.ravel(), "expon").pvalue),
                mean_z=float((x.mean() - 1.0) * np.sqrt(N)),
                lag1_z=float(12.0 * pairs.sum() / np.sqrt(pairs.size)) if pairs.size else 0.0)


def martingale(procs):
    """z = sum (N(T) - Lambda(T)) / sqrt(sum Lambda(T)) over the replicas of ``procs``."""
    if isinstance(procs, Proc):
        procs = [procs]
    num = sum(float((p.n - p.total).sum()) for p in procs)
    den = sum(float(p.total.sum()) for p in procs)
    return num / np.sqrt(den) if den > 0.0 else (0.0 if num == 0.0 else np.inf)


def uniform_ks(proc):
    """Poisson kinds, exact given N: Lambda(t_i) / Lambda(T) against Uniform(0, 1), the
    points of all replicas pooled.  Returns (n points, p)."""
    L = np.cumsum(np.nan_to_num(proc.inc), 1)
    ok = np.arange(L.shape[1])[None, :] < proc.n[:, None]
    u = (L / proc.total[:, None])[ok]
    if u.size == 0:
        return 0, 1.0
    return int(u.size), float(stats.kstest(u, "uniform").pvalue)


class Family:
    """The statistics one test asserts, held together to a false-alarm level (Bonferroni)."""

    def __init__(self, name, level=1e-3):
        self.name, self.level, self.items = name, level, []

    def p(self, label, p, shown=None):
        self.items.append((label, float(p), shown))

    def z(self, label, z):
        self.p(label, p_of_z(z), "z = %+.2f" % z)

    def fixed_m(self, label, procs, m):
        f = fixed_m(procs, m)
        self.p(label + " KS", f["ks_p"], "N = %d" % f["N"])
        self.z(label + " mean", f["mean_z"])
        self.z(label + " lag-1", f["lag1_z"])
        return f

    def martingale(self, label, procs):
        z = martingale(procs)
        self.z(label + " count", z)
        return z

    @property
    def bound(self):
        return self.level / max(1, len(self.items))

    def failures(self):
        return [(lab, p) for lab, p, _ in self.items if not p >= self.bound]

    def rejects(self):
        return bool(self.failures())

    def report(self):
        print("%s: %d statistics, per-test bound p >= %.3g" % (self.name, len(self.items), self.bound))
        for lab, p, shown in self.items:
            print("  %-34s p = %-10.3g %s%s" % (lab, p, shown or "", "" if p >= self.bound else "   <-- REJECT"))

    def check(self):
        self.report()
        bad = self.failures()
        assert not bad, "%s: law rejected at family level %g: %s" % (self.name, self.level, bad)


# --------------------------------------------------------------------------- deterministic
def check_support(logs, sim_opts, ctrl=None, start=0.0):
    """No arrival outside [start, end]; none inside a zero-rate PiecewiseConst segment;
    none from an l_0 = 0 Hawkes source, a rate-0 Poisson source or a rate-0 controller."""
    end = float(sim_opts["end_time"])
    real = logs.src >= 0
    t = logs.t[real]
    assert t.size == int(logs.n.sum())
    assert (t >= start).all() and (t <= end).all(), "an arrival outside [start, end]"
    assert (logs.t[:, 1:] >= logs.t[:, :-1])[real[:, 1:]].all(), "log not in time order"
    for kind, kw in sim_opts["other_sources"]:
        mine = logs.t[logs.src == kw["src_id"]]
        if kind == "PiecewiseConst":
            dead = pw_rate(mine, kw["change_times"], kw["rates"]) <= 0.0
            assert not dead.any(), "%d arrivals in a zero-rate segment: %s" % (dead.sum(), mine[dead][:5])
        elif kind == "Hawkes" and kw.get("l_0", 1.0) == 0.0:
            assert mine.size == 0, "arrivals from an l_0 = 0 Hawkes source"
        elif kind in ("Poisson", "Poisson2") and kw.get("rate", 1.0) == 0.0:
            assert mine.size == 0, "arrivals from a rate-0 source"
    if ctrl is not None and ctrl[0] == "poisson":
        rate = np.broadcast_to(np.asarray(ctrl[2], dtype=np.float64), (logs.R,))
        posts = (logs.src == sim_opts["src_id"]).sum(1)
        assert (posts[rate == 0.0] == 0).all(), "posts from a rate-0 controller"

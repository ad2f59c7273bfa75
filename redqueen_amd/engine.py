"""Engine front-end: a device-resident graph + batched runs through librq.so.

``Graph`` is the compiled form of a SimOpts (opt_model.py:755-967): other
sources, sinks and edge list are validated like ``Manager.__init__``
(opt_model.py:145-181) and uploaded once.  ``Graph.run`` enqueues one batch
(seeds x grid points) on the current torch stream and returns torch tensors;
torch is only the device-memory / stream plumbing.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L

KIND_BY_NAME = {"Poisson": L.SRC_POISSON, "Poisson2": L.SRC_POISSON2, "Hawkes": L.SRC_HAWKES,
                "PiecewiseConst": L.SRC_PWCONST, "RealData": L.SRC_REALDATA, "Opt": L.SRC_OPT}
CTRL_BY_NAME = {"opt": L.SRC_OPT, "poisson": L.SRC_POISSON2, "pwconst": L.SRC_PWCONST,
                "times": L.SRC_REALDATA, "wall": L.SRC_NONE, "sig": L.SRC_OPTPW}


def _arr(x, dt):
    return np.ascontiguousarray(np.asarray(x, dtype=dt))


def _source_class(name):
    """The class behind an other_sources entry: a built-in name, a name registered
    with SimOpts.registerSource (opt_model.py:768-771), or a callable."""
    if isinstance(name, str):
        if name in KIND_BY_NAME:
            return None
        from .opt_model import SimOpts
        cls = SimOpts.broadcasters.get(name)
        if cls is None:
            raise ValueError("Unknown type of broadcaster: {}".format(name))
        return cls
    return name


def _source_kind(name):
    if isinstance(name, str) and name in KIND_BY_NAME:
        return KIND_BY_NAME[name]
    cls = _source_class(name)
    kind = getattr(cls, "_rq_kind", None)
    return L.SRC_REALDATA if kind is None else kind   # a plugin: its times as RealData


class Graph:
    """Compiled network.  ``other_sources``: list of (name-or-class, kwargs)."""

    def __init__(self, src_id, other_sources, sink_ids, edge_list, end_time, start_time=0.0,
                 ctrl_a=None, ctrl_b=None):
        self._keep = []
        srcs = []
        self.has_realdata = False
        # registered static plugin broadcasters: (position in other_sources, class, kwargs)
        self.plugins = []
        # src_ids of the static wall sources (run_dynamic plays their times only when
        # strictly earlier than the dynamic sources' next event, opt_model.py:289-290)
        self.static_src_ids = set()
        # ('Opt', kw) entries of other_sources (opt_model.py:761): the players of the game
        self.players = []
        for idx, (name, kw) in enumerate(other_sources):
            kind = _source_kind(name)
            cls = _source_class(name)
            dyn_plugin = False
            if cls is not None and getattr(cls, "_rq_kind", None) is None:
                # graph-level times: the instance its own kwargs make (the seed as given);
                # randomized batches replace them per replica (run(randomize=True)).  A
                # dynamic plugin must be self-driven: every run checks it (_verify_dynamic)
                from .opt_model import source_times
                inst = cls(**kw)
                dyn = bool(getattr(inst, "is_dynamic", True))
                self.plugins.append((idx, cls, dict(kw), int(kw["src_id"]), dyn))
                dyn_plugin = dyn
                kw = {"src_id": kw["src_id"],
                      "times": source_times(inst, float(start_time), sink_ids, edge_list,
                                            float(end_time))}
            self.has_realdata = self.has_realdata or kind == L.SRC_REALDATA
            # a dynamic broadcaster replayed from its times (a dynamic plugin, or RealData
            # kwargs dynamic=True): equal times order it as a dynamic source
            dyn_rd = kind == L.SRC_REALDATA and (bool(kw.get("dynamic")) or dyn_plugin)
            if kind in (L.SRC_POISSON2, L.SRC_PWCONST) or (kind == L.SRC_REALDATA and not dyn_rd):
                self.static_src_ids.add(int(kw["src_id"]))
            if kind == L.SRC_OPT:
                # a competing RedQueen broadcaster: a player of the game (_run_game).  In the
                # graph it is a replay stream -- a dynamic RealData source without times --
                # so the stream order, and with it every log entry, is the reference's
                self.players.append({"idx": idx, "src_id": int(kw["src_id"]),
                                     "seed": kw.get("seed"), "q": float(kw.get("q", 1.0)),
                                     "s": kw.get("s", 1.0)})
                kind, dyn_rd, kw = L.SRC_REALDATA, True, {"src_id": kw["src_id"], "times": []}
            d = L.SourceDesc()
            d.kind = kind
            d.src_id = int(kw["src_id"])
            d.seed = int(kw.get("seed", 0)) & 0xFFFFFFFF
            d.flags = L.SRCF_DYNAMIC if dyn_rd else 0
            if kind in (L.SRC_POISSON, L.SRC_POISSON2):
                d.p0 = float(kw.get("rate", 1.0))
            elif kind == L.SRC_HAWKES:
                d.p0 = float(kw.get("l_0", 1.0))
                d.p1 = float(kw.get("alpha", 1.0))
                d.p2 = float(kw.get("beta", 10.0))
            elif kind == L.SRC_PWCONST:
                a = _arr(kw["change_times"], np.float64)
                b = _arr(kw["rates"], np.float64)
                if a.size != b.size:
                    raise ValueError("change_times and rates differ in length")
                self._keep += [a, b]
                d.n_arr = a.size
                d.a = a.ctypes.data_as(L._pd)
                d.b = b.ctypes.data_as(L._pd)
            elif kind == L.SRC_REALDATA:
                a = _arr(kw["times"], np.float64)
                self._keep.append(a)
                d.n_arr = a.size
                d.a = a.ctypes.data_as(L._pd)
            srcs.append(d)
        self.src_id = int(src_id)
        self.end_time = float(end_time)
        self.start_time = float(start_time)
        self.sink_ids = _arr(sink_ids, np.int64)
        edges = list(edge_list)
        self._edges = edges
        self.edge_src = _arr([e[0] for e in edges], np.int64)
        self.edge_sink = _arr([e[1] for e in edges], np.int64)
        arr = (L.SourceDesc * max(1, len(srcs)))(*srcs)
        gd = L.GraphDesc()
        gd.n_sources = len(srcs)
        gd.sources = arr
        gd.n_sinks = self.sink_ids.size
        gd.sink_ids = self.sink_ids.ctypes.data_as(L._pi64)
        gd.n_edges = len(edges)
        gd.edge_src = self.edge_src.ctypes.data_as(L._pi64)
        gd.edge_sink = self.edge_sink.ctypes.data_as(L._pi64)
        gd.ctrl_src_id = self.src_id
        gd.start_time = self.start_time
        gd.end_time = self.end_time
        if ctrl_a is not None:
            ca = _arr(ctrl_a, np.float64)
            self._keep.append(ca)
            gd.ctrl_n_arr = ca.size
            gd.ctrl_a = ca.ctypes.data_as(L._pd)
            if ctrl_b is not None:
                cb = _arr(ctrl_b, np.float64)
                self._keep.append(cb)
                gd.ctrl_b = cb.ctypes.data_as(L._pd)
        h = C.c_void_p()
        L.check("rq_graph_build", L.lib().rq_graph_build(C.byref(gd), C.byref(h)))
        self._h = h
        info = np.zeros(8, dtype=np.int64)
        L.lib().rq_graph_info(h, info.ctypes.data_as(L._pi64))
        self.n_streams, self.n_sinks, self.n_followers, self.n_edges, self.ctrl_idx = (
            int(v) for v in info[:5])
        self.stream_src_ids = np.zeros(self.n_streams, dtype=np.int64)
        L.lib().rq_graph_source_ids(h, self.stream_src_ids.ctypes.data_as(L._pi64))
        self.followers = np.zeros(max(1, self.n_followers), dtype=np.int64)[:self.n_followers]
        if self.n_followers:
            L.lib().rq_graph_followers(h, self.followers.ctypes.data_as(L._pi64))
        # one workspace per caller stream: batches enqueued on different streams may run
        # at the same time and must not share buffers
        self._wss = {}
        self._cap_scale = {}   # _cap_key(...) -> cap_scale an overflow rerun needed (reset_capacity_memo)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                L.lib().rq_graph_free(h)
            except Exception:
                pass

    def workspace_bytes(self, stream=None):
        """Bytes of the workspace held for ``stream`` (default: the current stream)."""
        use = stream or torch.cuda.current_stream()
        ws = self._wss.get(use.cuda_stream)
        return 0 if ws is None else ws.numel()

    def release_workspaces(self):
        """Drop every stream's workspace (the caching allocator keeps the blocks)."""
        self._wss.clear()

    # ------------------------------------------------------------------
    def s_matrix(self, s, n_grid=1):
        """s as in SimOpts (scalar, vector over sorted followers, or dict sink->s)."""
        F = self.n_followers
        if isinstance(s, dict):
            row = np.asarray([s[int(x)] for x in self.followers], dtype=np.float64)
        else:
            row = np.ones(F, dtype=np.float64) * np.asarray(s, dtype=np.float64)
        return np.ascontiguousarray(np.tile(row, (n_grid, 1)))

    def run(self, *args, stream=None, **kw):
        """Enqueue one batch on ``stream`` (default: the current torch stream).  Every
        tensor the batch reads or writes is allocated with that stream current, so
        the caching allocator, the library and the status check all agree on it.
        With a dynamic plugin among the sources, the batch's replicas (all of a batch of
        <= 64, else a seeded sample of 64) are checked to be self-driven (_verify_dynamic);
        when one reacts to other sources' events the whole batch is replayed to the
        reactive fixed point (_run_reactive) before the result is returned.
        A graph with Opt broadcasters among its other sources runs as a game (_run_game)."""
        from .opt_model import PluginReacts
        use = stream or torch.cuda.current_stream()
        if self.players:   # Opt broadcasters among the other sources: the game
            with torch.cuda.stream(use):
                return self._run_game(*args, stream=use, **kw)
        with torch.cuda.stream(use):
            res = self._run(*args, stream=use, **kw)
            if any(p[4] for p in self.plugins) and not kw.get("plan_only"):
                try:
                    self._verify_dynamic(args, dict(kw, stream=use), res)
                except PluginReacts:
                    res = self._run_reactive(args, dict(kw, stream=use), res)
            return res

    def _run(self, ctrl="opt", q=1.0, s=None, n_rep=1, ctrl_seed=0, world_seed=0,
            randomize=False, seed_mod=0, ctrl_rate=None, Ks=(1,), max_events=None,
            event_log=False, cap_scale=1.0, chunk=0, stream=None, check=True, sweep_mode=0, replica0=0, n_local=0,
            plan_only=False, s_pw=None, period=None, rep_lo=0, rep_cnt=0, rd_override=None,
            rd_streams=None, rep_idx=None):
        """Enqueue one batch.  ``q``: scalar or [n_grid]; ``s``: per grid point
        row(s) over the sorted followers ([n_grid, F]) or anything ``s_matrix``
        takes.  Seeds: int base (seed + replica id) or a device uint32 tensor.
        ``ctrl="sig"`` (OptPWSignificance): ``s_pw`` [F, S] or [n_grid, F, S] over the
        sorted followers and ``period`` T.
        ``rep_lo`` / ``rep_cnt``: run only replicas [rep_lo, rep_lo + rep_cnt) of every grid
        point (a balanced multi-GPU shard, rq_batch_desc.rep_lo); ``replica0`` / ``n_local``
        then index that n_grid x rep_cnt space, and so do the outputs.
        ``rd_streams = (src_ids, times, off, caps)``: per-replica times of the graph's
        RealData sources ``src_ids`` (declared with no times) already on the device --
        replica i (global id) plays times[off[i * n + k] .. off[i * n + k + 1]) for source
        k, sorted, within [start_time, end_time]; ``caps[k]`` >= any replica's count
        (rq_batch_desc.rd_*, read in place: no host pass per replica).
        ``rep_idx``: run exactly these global replica ids (rq_batch_desc.rep_idx; replica0,
        n_local and the rep_lo / rep_cnt window are then ignored); output k = rep_idx[k]."""
        dev = torch.device("cuda", torch.cuda.current_device())
        ck = CTRL_BY_NAME[ctrl] if isinstance(ctrl, str) else int(ctrl)
        qv = _arr(np.atleast_1d(q), np.float64)
        n_grid = qv.size
        if ck == L.SRC_OPT:
            if s is None:
                raise ValueError("s required for the RedQueen broadcaster")
            sm = np.asarray(s, dtype=np.float64) if (isinstance(s, np.ndarray) and s.ndim == 2) \
                else self.s_matrix(s, n_grid)
            sm = np.ascontiguousarray(sm, dtype=np.float64)
            if sm.shape != (n_grid, self.n_followers):
                raise ValueError("s must be [n_grid, n_followers]")
        else:
            sm = np.zeros((n_grid, max(1, self.n_followers)))
        spw = None
        if ck == L.SRC_OPTPW:
            if s_pw is None or period is None:
                raise ValueError("s_pw and period required for OptPWSignificance")
            spw = np.asarray(s_pw, dtype=np.float64)
            if spw.ndim == 2:
                spw = np.broadcast_to(spw, (n_grid,) + spw.shape)
            spw = np.ascontiguousarray(spw)
            if spw.ndim != 3 or spw.shape[:2] != (n_grid, self.n_followers) or spw.shape[2] < 1:
                raise ValueError("s_pw must be [n_grid, n_followers, n_segments]")
        R_all = n_grid * int(n_rep)
        cnt = int(rep_cnt) if rep_cnt else int(n_rep)
        lo = int(rep_lo) if rep_cnt else 0
        R = int(n_local) if n_local else n_grid * cnt - int(replica0)
        # global replica ids of this call's outputs (rq_global_replica)
        sp = np.arange(int(replica0), int(replica0) + R, dtype=np.int64)
        gids = sp if cnt == int(n_rep) else (sp // cnt) * int(n_rep) + lo + sp % cnt
        if rep_idx is not None:
            gids = _arr(rep_idx, np.int64)
            R, replica0, n_local, lo, rep_cnt = gids.size, 0, gids.size, 0, 0
            if R < 1 or gids.min() < 0 or gids.max() >= R_all:
                raise ValueError("rep_idx: global ids in [0, n_grid * n_rep) expected")
        Ks = _arr(Ks, np.int32)
        if not 1 <= Ks.size <= L.MAX_K:
            raise ValueError("1..%d K values per run" % L.MAX_K)
        b = L.BatchDesc()
        b.ctrl_kind = ck
        b.n_grid = n_grid
        b.q = qv.ctypes.data_as(L._pd)
        b.s = sm.ctypes.data_as(L._pd)
        b.n_rep = int(n_rep)
        keep = []
        if torch.is_tensor(ctrl_seed):
            cs = ctrl_seed.to(device=dev, dtype=torch.int32).contiguous()
            keep.append(cs)
            b.ctrl_seed = cs.data_ptr()
        else:
            b.ctrl_seed0 = int(ctrl_seed) & 0xFFFFFFFF
        b.randomize_world = int(bool(randomize))
        if torch.is_tensor(world_seed):
            ws_ = world_seed.to(device=dev, dtype=torch.int32).contiguous()
            keep.append(ws_)
            b.world_seed = ws_.data_ptr()
        else:
            b.world_seed0 = int(world_seed) & 0xFFFFFFFF
        b.seed_mod = int(seed_mod)
        if rd_streams is not None:
            if self.plugins:
                raise ValueError("rd_streams and registered plugin broadcasters are exclusive")
            sids, td, to, caps = rd_streams
            sid = _arr(sids, np.int64)
            cap = _arr(caps, np.int64)
            if not (torch.is_tensor(td) and torch.is_tensor(to) and td.dtype == torch.float64 and
                    to.dtype == torch.int64 and td.is_cuda and to.is_cuda and to.is_contiguous()
                    and td.is_contiguous() and to.numel() == R_all * sid.size + 1
                    and cap.size == sid.size and 1 <= sid.size <= L.MAX_RD):
                raise ValueError("rd_streams: (src_ids[n], device f64 times, device i64 "
                                 "off[n_grid * n_rep * n + 1], caps[n]) expected")
            keep += [sid, cap, td, to]
            b.n_rd = sid.size
            b.rd_src_id = sid.ctypes.data_as(L._pi64)
            b.rd_cap = cap.ctypes.data_as(L._pi64)
            b.rd_times = td.data_ptr()
            b.rd_off = to.data_ptr()
        elif self.plugins and (randomize or rd_override is not None):
            self._plugin_streams(b, keep, dev, R_all, gids, world_seed, int(seed_mod), rd_override)
        if ck == L.SRC_POISSON2:
            if ctrl_rate is None:
                raise ValueError("ctrl_rate required for a Poisson controlled source")
            cr = torch.as_tensor(ctrl_rate, dtype=torch.float64, device=dev).reshape(-1)
            if cr.numel() == 1:
                cr = cr.expand(R_all)
            cr = cr.contiguous()
            keep.append(cr)
            b.ctrl_rate = cr.data_ptr()
            b.ctrl_rate_max = float(cr.max().item()) if cr.numel() else 0.0
        b.Ks = Ks.ctypes.data_as(L._pi32)
        b.nK = Ks.size
        b.max_events = -1 if max_events is None or max_events == float("inf") else int(max_events)
        b.flags = L.RUN_EVENT_LOG if event_log else 0
        b.cap_scale = float(cap_scale)
        b.chunk = int(chunk)
        b.sweep_mode = int(sweep_mode)
        b.replica0 = int(replica0)
        b.n_local = int(n_local)
        b.rep_lo = lo
        b.rep_cnt = int(rep_cnt)
        if rep_idx is not None:
            keep.append(gids)
            b.rep_idx = gids.ctypes.data_as(L._pi64)
        if spw is not None:
            b.n_seg = spw.shape[2]
            b.period = float(period)
            b.s_pw = spw.ctypes.data_as(L._pd)
        lib = L.lib()
        if plan_only:
            b.ws_budget = self._ws_budget(dev)
            info = (C.c_int64 * 11)()
            L.check("rq_plan_info_n", lib.rq_plan_info_n(self._h, C.byref(b), info, 11))
            keys = ("variant", "sources_per_lane", "ring_depth", "waves_per_block",
                    "blocks_per_cu", "columns_in_lds", "lds_bytes_per_block", "chunk", "sweep_scan",
                    "sweep_blk", "sweep_rows16")
            return dict(zip(keys, (int(v) for v in info)))
        return self._run_loop(lib, b, keep, dev, R, Ks, n_grid, n_rep, ck, event_log,
                              gids, check, stream)

    # ------------------------------------------------------------------ the game
    @property
    def player_ids(self):
        """src_ids of the Opt broadcasters among the other sources (the game's players
        besides a RedQueen controlled source), in other_sources order."""
        return [p["src_id"] for p in self.players]

    def _player_s(self, src_id, s):
        """s over the sorted followers of ``src_id`` as the reference's Opt takes it
        (opt_model.py:507-513): a dict by sink id, or a scalar / array times ones."""
        fol = sorted({int(e[1]) for e in self._edges if int(e[0]) == int(src_id)})
        if isinstance(s, dict):
            return np.asarray([s[x] for x in fol], dtype=np.float64)
        return np.ascontiguousarray(np.ones(len(fol), dtype=np.float64) * np.asarray(s, dtype=np.float64))

    GAME_REPLAY_ROWS = 1 << 26   # dataframe rows per expand + replay chunk (40 B a row)
    GAME_CAP_SQUEEZE = 1.0       # scales the output-log capacity down; tests only (overflow reruns)
    # stage 3 of a game: "log" = rq_log_metrics on the completed log (a graph or a log capacity
    # it refuses takes the other route), "replay" = rq_log_expand + rq_metrics_replay_batch; the
    # same bits, C3 with 10,000 replicas in 45-52 ms against 3,053-3,920 ms (profiles/game_c3_logmetrics.json)
    GAME_METRICS = "log"
    # whether "log" may take rq_log_metrics_slim where rq_log_metrics refuses the graph (more than
    # LOG_METRICS_MAX_SINKS sinks) instead of the replay route: C5's graph with end_time 10 and 64
    # replicas in 25.2-25.5 ms against 209.0-215.7 ms, the same bits (profiles/log_metrics_slim.json,
    # DESIGN section 33)
    GAME_METRICS_SLIM = True
    game_metrics_route = None    # the route stage 3 of the last game took: "log", "log-slim" or "replay"

    def _game_launch(self, players, seeds, ev_t, ev_src, counts, max_events, out_cap, use):
        """One rq_log_game: ``players`` [(src_id, q, s array)], ``seeds`` device int32
        [R, P] (uint32 bits), the exogenous logs.  Returns (out_t, out_src, out_counts,
        player_posts, status) device tensors."""
        lib = L.lib()
        dev = ev_t.device
        R = int(counts.shape[0])
        P = len(players)
        arr = (L.GamePlayer * max(1, P))()
        keep = []
        for c, (sid, q, s) in enumerate(players):
            sv = _arr(s, np.float64)
            keep.append(sv)
            arr[c].src_id, arr[c].q, arr[c].n_s = int(sid), float(q), int(sv.size)
            arr[c].s = sv.ctypes.data_as(L._pd)
        nbytes = C.c_size_t()
        L.check("rq_log_game_workspace", lib.rq_log_game_workspace(self._h, P, C.byref(nbytes)))
        ws = torch.empty(max(256, nbytes.value), dtype=torch.uint8, device=dev)
        out_t = torch.empty((R, out_cap), dtype=torch.float64, device=dev)
        out_src = torch.empty((R, out_cap), dtype=torch.int32, device=dev)
        out_counts = torch.empty((R, 4), dtype=torch.int64, device=dev)
        posts = torch.empty((R, P), dtype=torch.int64, device=dev)
        status = torch.empty(R, dtype=torch.int32, device=dev)
        ev_cap = int(ev_t.shape[1])
        if ev_cap == 0:   # an empty world: nothing is read, but the pointers must be real
            ev_t = torch.zeros((R, 1), dtype=torch.float64, device=dev)
            ev_src = torch.zeros((R, 1), dtype=torch.int32, device=dev)
        me = -1 if max_events is None or max_events == float("inf") else int(max_events)
        L.check("rq_log_game", lib.rq_log_game(
            self._h, arr, P, seeds.data_ptr(), ev_t.data_ptr(), ev_src.data_ptr(), counts.data_ptr(),
            R, ev_cap, me, out_t.data_ptr(), out_src.data_ptr(), int(out_cap), out_counts.data_ptr(),
            posts.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), use.cuda_stream))
        return out_t, out_src, out_counts, posts, status

    def _run_game(self, ctrl="opt", q=1.0, s=None, n_rep=1, ctrl_seed=0, world_seed=0,
                  randomize=False, seed_mod=0, ctrl_rate=None, Ks=(1,), max_events=None,
                  event_log=False, cap_scale=1.0, chunk=0, stream=None, check=True, sweep_mode=0,
                  replica0=0, n_local=0, plan_only=False, s_pw=None, period=None, rep_lo=0,
                  rep_cnt=0, rd_override=None, rd_streams=None, rep_idx=None):
        """A batch of a graph with Opt broadcasters among its other sources.  The sources
        no Opt influences are played by the ordinary path with their event log (ctrl
        "wall" when the controlled source is RedQueen, which then is one more player, seeded
        by ``ctrl_seed``); rq_log_game plays the Opts against that log, one launch per grid
        point; metrics and counts come from the completed log, pandas-exact on the
        start-time ties every game has: by rq_log_metrics (``GAME_METRICS`` "log"; a graph or
        a log capacity above 2^20 events, which it refuses, takes the other route -- with
        ``GAME_METRICS_SLIM``, a graph of up to LOG_METRICS_SLIM_MAX_SINKS sinks goes to
        rq_log_metrics_slim instead) or by rq_log_expand + rq_metrics_replay_batch ("replay"),
        the same bits; ``self.game_metrics_route`` names the route taken ("log", "log-slim",
        "replay").  With ``check`` replicas whose output log overflowed are rerun at doubled capacity
        (``self.reruns``).  The result carries ``player_posts`` [R, P] and ``player_ids``.
        With ``self.game_timing`` set, ``self.game_ms`` holds the device milliseconds of the
        three stages (exogenous pass, game launches and reruns, and under the key "replay"
        the metrics of the completed log on either route)."""
        from .utils import replay_columns
        ck = CTRL_BY_NAME[ctrl] if isinstance(ctrl, str) else int(ctrl)
        if ck == L.SRC_OPTPW:
            raise NotImplementedError("OptPWSignificance against Opt broadcasters among the other sources")
        if self.plugins:
            raise NotImplementedError("registered plugin broadcasters beside Opt broadcasters")
        if rd_streams is not None or rd_override is not None:
            raise NotImplementedError("rd_streams in a run with Opt broadcasters among the other sources")
        if rep_idx is not None or replica0 or n_local or rep_lo or rep_cnt:
            raise NotImplementedError("replica sharding (rep_idx / replica0 / n_local / rep_lo / rep_cnt) "
                                      "of a run with Opt broadcasters among the other sources")
        if int(sweep_mode) != 0:
            raise NotImplementedError("sweep_mode != 0 in a run with Opt broadcasters among the other sources")
        if plan_only:
            raise NotImplementedError("plan_only in a run with Opt broadcasters among the other sources")
        use = stream
        dev = torch.device("cuda", torch.cuda.current_device())
        qv = _arr(np.atleast_1d(q), np.float64)
        n_grid, n_rep = qv.size, int(n_rep)
        R = n_grid * n_rep
        Ks = _arr(Ks, np.int32)
        if not 1 <= Ks.size <= L.MAX_K:
            raise ValueError("1..%d K values per run" % L.MAX_K)
        sm = None
        if ck == L.SRC_OPT:
            if s is None:
                raise ValueError("s required for the RedQueen broadcaster")
            sm = np.asarray(s, dtype=np.float64) if (isinstance(s, np.ndarray) and s.ndim == 2) \
                else self.s_matrix(s, n_grid)
            if sm.shape != (n_grid, self.n_followers):
                raise ValueError("s must be [n_grid, n_followers]")
        # stage times for scripts/bench_game.py (game_timing): device events around the stages
        marks = []

        def mark():
            if getattr(self, "game_timing", False):
                ev = torch.cuda.Event(enable_timing=True)
                ev.record(use)
                marks.append(ev)
        mark()
        # 1. the exogenous world: global replica ids 0 .. R - 1, seeds as in any batch
        exo_kw = dict(n_rep=R, world_seed=world_seed, randomize=randomize, seed_mod=seed_mod,
                      Ks=Ks, max_events=max_events, event_log=True, cap_scale=cap_scale,
                      chunk=chunk, stream=use, check=True)
        if ck == L.SRC_OPT:
            exo = self._run("wall", **exo_kw)
        else:
            rate = ctrl_rate
            if ck == L.SRC_POISSON2 and ctrl_rate is not None:
                rate = torch.as_tensor(ctrl_rate, dtype=torch.float64, device=dev).reshape(-1)
            exo = self._run(ctrl, ctrl_seed=ctrl_seed, ctrl_rate=rate, **exo_kw)
        reruns = int(getattr(self, "reruns", 0))
        mark()
        # 2. the players and their seeds (uint32 arithmetic, as the kernels' seeds wrap)
        ids = np.arange(R, dtype=np.int64)
        kk = ids % int(seed_mod) if int(seed_mod) > 0 else ids
        u = (world_seed.to(torch.int64).cpu().numpy() if torch.is_tensor(world_seed)
             else int(world_seed) + kk) & 0xFFFFFFFF
        cols = []
        for p in self.players:
            if randomize:
                cols.append((u + 99 * p["idx"]) & 0xFFFFFFFF)
            else:
                cols.append(np.full(R, int(p["seed"] or 0) & 0xFFFFFFFF, dtype=np.int64))
        wall = [(p["src_id"], p["q"], self._player_s(p["src_id"], p["s"])) for p in self.players]
        if ck == L.SRC_OPT:
            cols.append((ctrl_seed.to(torch.int64).cpu().numpy() if torch.is_tensor(ctrl_seed)
                         else int(ctrl_seed) + kk) & 0xFFFFFFFF)
        seeds = torch.from_numpy(np.ascontiguousarray(
            np.stack(cols, axis=1).astype(np.uint32).view(np.int32))).to(dev)
        P = len(cols)
        ev_cap = int(exo.ev_t.shape[1])
        out_cap = max(1, int((2 * ev_cap + 64 * P) * self.GAME_CAP_SQUEEZE))
        if max_events is not None and max_events != float("inf"):
            out_cap = max(1, min(out_cap, int(max_events)))
        parts = []
        mark()
        for g in range(n_grid):
            players = list(wall)
            if ck == L.SRC_OPT:
                players.append((self.src_id, float(qv[g]), sm[g]))
            lo, hi = g * n_rep, (g + 1) * n_rep
            parts.append(self._game_launch(players, seeds[lo:hi], exo.ev_t[lo:hi], exo.ev_src[lo:hi],
                                           exo.counts[lo:hi], max_events, out_cap, use))
        out_t, out_src, out_counts, posts, status = (torch.cat([p[k] for p in parts]) for k in range(5))
        # overflowed output logs again, alone, at doubled capacity
        while check:
            use.synchronize()
            flagged = np.flatnonzero(status.cpu().numpy() & L.ST_ROWS_OVERFLOW)
            if not flagged.size:
                break
            if out_cap > (1 << 28):
                raise L.RQError("rq_log_game", L.RQ_EOVERFLOW)
            out_cap *= 2
            at = torch.from_numpy(flagged).to(dev)
            t2 = torch.empty((R, out_cap), dtype=out_t.dtype, device=dev)
            s2 = torch.empty((R, out_cap), dtype=out_src.dtype, device=dev)
            t2[:, :out_t.shape[1]] = out_t
            s2[:, :out_src.shape[1]] = out_src
            out_t, out_src = t2, s2
            for g in np.unique(flagged // n_rep):
                pick = flagged[flagged // n_rep == g]
                pk = torch.from_numpy(pick).to(dev)
                players = list(wall)
                if ck == L.SRC_OPT:
                    players.append((self.src_id, float(qv[g]), sm[g]))
                r = self._game_launch(players, seeds[pk].contiguous(), exo.ev_t[pk].contiguous(),
                                      exo.ev_src[pk].contiguous(), exo.counts[pk].contiguous(),
                                      max_events, out_cap, use)
                out_t[pk], out_src[pk] = r[0], r[1]
                out_counts[pk], posts[pk], status[pk] = r[2], r[3], r[4]
            reruns += int(at.numel())
        self.reruns = reruns
        mark()
        # 3. metrics and counts of the completed log: straight from it, or its dataframe rows
        # through the replay
        metrics = torch.empty((R, Ks.size + 2), dtype=torch.float64, device=dev)
        counts = out_counts.clone()
        res = BatchResult(self, metrics, counts, status, out_t, out_src, Ks, n_grid, n_rep)
        if self.GAME_METRICS not in ("log", "replay"):
            raise ValueError("Graph.GAME_METRICS: 'log' or 'replay' expected")
        lm = None
        if self.GAME_METRICS == "log":   # straight from the log, where graph and capacity are supported
            try:
                lm = BatchResult(self, None, out_counts, None, out_t, out_src, Ks, n_grid, n_rep)._log_metrics(
                    Ks, use, None if self.GAME_METRICS_SLIM else False)
            except L.RQError as e:
                if e.code != L.RQ_EUNSUPPORTED:
                    raise
        self.game_metrics_route = "replay" if lm is None else ("log-slim" if lm.slim else "log")
        lo = 0
        if lm is not None:
            metrics.copy_(lm.metrics)
            # a batch in which no event has an edge keeps the game kernel's counts, as the
            # other route's empty chunk does
            if bool((lm.counts[:, 3] > 0).any().item()):
                counts[:, 0], counts[:, 1], counts[:, 3] = lm.counts[:, 0], lm.counts[:, 1], lm.counts[:, 2]
            lo = R
        else:
            row_all = torch.empty(R + 1, dtype=torch.int64, device=dev)
            L.check("rq_log_rows", L.lib().rq_log_rows(self._h, out_src.data_ptr(), out_counts.data_ptr(), R,
                                                       int(out_src.shape[1]), row_all.data_ptr(), use.cuda_stream))
            ra = row_all.cpu().numpy()
        while lo < R:   # replica chunks of at most GAME_REPLAY_ROWS dataframe rows (one at least)
            hi = int(np.searchsorted(ra, ra[lo] + self.GAME_REPLAY_ROWS, side="right")) - 1
            hi = min(R, max(hi, lo + 1))
            sub = BatchResult(self, metrics[lo:hi], out_counts[lo:hi], status[lo:hi], out_t[lo:hi],
                              out_src[lo:hi], Ks, 1, hi - lo)
            ro, c = sub._log_columns(use)
            if int(ro[-1]) == 0:   # no event of the chunk has an edge: empty dataframes
                metrics[lo:hi] = float("nan")
                lo = hi
                continue
            off = torch.from_numpy(np.ascontiguousarray(ro)).to(dev)
            m, cn = replay_columns(c["t"], c["src_id"], c["sink_id"], c["event_id"], off, self.src_id,
                                   self.end_time, Ks)
            metrics[lo:hi] = m
            counts[lo:hi, 0], counts[lo:hi, 1], counts[lo:hi, 3] = cn[:, 0], cn[:, 1], cn[:, 2]
            lo = hi
        mark()
        if marks:
            marks[-1].synchronize()
            self.game_ms = {"exogenous": marks[0].elapsed_time(marks[1]), "game": marks[2].elapsed_time(marks[3]),
                            "replay": marks[3].elapsed_time(marks[4])}
        if not event_log:
            res.ev_t = res.ev_src = None
        res.player_posts = posts
        res.player_ids = [p[0] for p in wall] + ([self.src_id] if ck == L.SRC_OPT else [])
        res.replica0 = 0
        res.global_ids = ids
        return res

    def _launch(self, lib, b, dev, R, Ks, n_grid, n_rep, event_log, use):
        """One rq_run_batch of R output replicas on stream ``use``.  The outputs (and the
        event log) are allocated first, so the workspace budget is what is left after them."""
        sk = use.cuda_stream
        metrics = torch.empty((R, Ks.size + 2), dtype=torch.float64, device=dev)
        counts = torch.empty((R, 4), dtype=torch.int64, device=dev)
        status = torch.empty(R, dtype=torch.int32, device=dev)
        out = L.Outputs()
        out.metrics, out.counts, out.status = metrics.data_ptr(), counts.data_ptr(), status.data_ptr()
        ev_t = ev_src = None
        if event_log:
            cap = C.c_int64()
            L.check("rq_event_capacity", lib.rq_event_capacity(self._h, C.byref(b), C.byref(cap)))
            ev_t = torch.empty((R, cap.value), dtype=torch.float64, device=dev)
            ev_src = torch.empty((R, cap.value), dtype=torch.int32, device=dev)
            out.ev_t, out.ev_src, out.ev_cap = ev_t.data_ptr(), ev_src.data_ptr(), cap.value
        nbytes = C.c_size_t()
        b.ws_budget = self._ws_budget(dev, sk)
        L.check("rq_workspace_size", lib.rq_workspace_size(self._h, C.byref(b), C.byref(nbytes)))
        ws = self._wss.get(sk)
        if ws is None or ws.numel() < nbytes.value:
            self._wss[sk] = ws = None
            ws = self._wss[sk] = torch.empty(max(256, nbytes.value), dtype=torch.uint8, device=dev)
        L.check("rq_run_batch", lib.rq_run_batch(self._h, C.byref(b), C.byref(out),
                                                 ws.data_ptr(), ws.numel(), sk))
        return BatchResult(self, metrics, counts, status, ev_t, ev_src, Ks, n_grid, int(n_rep))

    # an overflow memo is kept only when at least this share of a batch overflowed (a
    # few flagged replicas rerun alone, cheaply; a batch mostly over capacity would pay a
    # second pass every call)
    CAP_MEMO_SHARE = 1.0 / 16

    def _cap_key(self, b, ck):
        """Capacity-relevant inputs of a run: controller kind, max_events set, sweep
        mode, and the octave of the controller's rate parameter (RedQueen: the q range;
        Poisson: the largest rate) -- an overflow at one q says nothing about another."""
        qk = None
        if ck in (L.SRC_OPT, L.SRC_OPTPW) and b.n_grid > 0:
            qs = np.ctypeslib.as_array(b.q, shape=(b.n_grid,))
            qk = (int(np.floor(np.log2(max(qs.min(), 1e-300)))), int(np.floor(np.log2(max(qs.max(), 1e-300)))))
        elif ck == L.SRC_POISSON2:
            qk = int(np.floor(np.log2(max(b.ctrl_rate_max, 1e-300))))
        return (ck, b.max_events >= 0, int(b.sweep_mode), qk)

    def reset_capacity_memo(self):
        """Forget the capacity scales earlier overflow reruns of this graph remembered."""
        self._cap_scale.clear()

    def _run_loop(self, lib, b, keep, dev, R, Ks, n_grid, n_rep, ck, event_log, gids,
                  check, use):
        """The batch, then -- with ``check`` -- only its flagged replicas again
        (rq_batch_desc.rep_idx: the same global ids, so the same seeds and inputs): an
        overflowed one (RQ_ST_*_OVERFLOW) at doubled capacities, a tie-flagged one of a
        fast sweep (RQ_ST_TIE: equal event times) on the exact sequential sweep; their
        rows replace the flagged rows.  ``self.reruns`` counts the replicas rerun."""
        key = self._cap_key(b, ck)
        b.cap_scale = max(b.cap_scale, self._cap_scale.get(key, 1.0))
        res = self._launch(lib, b, dev, R, Ks, n_grid, n_rep, event_log, use)
        res.replica0 = int(gids[0]) if len(gids) else 0
        res.global_ids = gids
        self.reruns = 0
        if not check:
            return res
        gids = np.asarray(gids, dtype=np.int64)
        # per output replica: the sweep mode it last ran with, and whether that run was the
        # exact sequential sweep (from the library's own plan: rq_plan_info variant 1 / 4)
        mode = np.full(R, int(b.sweep_mode), dtype=np.int64)
        seq = np.full(R, b.sweep_mode == 2 or self._plan_variant(lib, b) % 10 in (1, 4))
        scale = np.full(R, float(b.cap_scale))
        while True:
            use.synchronize()
            st = res.status.cpu().numpy()
            if (st & L.ST_UNORDERED).any():
                raise NotImplementedError(
                    "more than 2048 arrivals at one time in a sequential run over > 2048 sources "
                    "(RQ_ST_UNORDERED): their play order is not the reference's")
            ovf = (st & (L.ST_ROWS_OVERFLOW | L.ST_STREAM_OVERFLOW)) != 0
            tie = ((st & L.ST_TIE) != 0) & ~seq & ~ovf
            if not ovf.any() and not tie.any():
                return res
            if ovf.any():
                if scale[ovf].max() > 64:
                    raise L.RQError("rq_run_batch", L.RQ_EOVERFLOW)
                scale[ovf] *= 2.0
                if ovf.sum() >= self.CAP_MEMO_SHARE * R:
                    self._cap_scale[key] = max(self._cap_scale.get(key, 1.0), float(scale[ovf].max()))
            # equal event times in a fast tiled sweep: those replicas on the exact sequential sweep
            mode[tie] = 2
            seq[tie] = True
            # one rerun per (sweep mode, capacity scale) group of flagged replicas
            flagged = np.flatnonzero(ovf | tie)
            for m_, s_ in sorted({(int(mode[k]), float(scale[k])) for k in flagged}):
                pick = flagged[(mode[flagged] == m_) & (scale[flagged] == s_)]
                self._rerun_into(lib, b, dev, res, pick, gids[pick], s_, m_, Ks, n_grid, n_rep,
                                 event_log, use)
                self.reruns += int(pick.size)

    def _rerun_into(self, lib, b, dev, res, pick, ids, scale, mode, Ks, n_grid, n_rep, event_log, use):
        """Rerun global replicas ``ids`` (outputs ``pick`` of ``res``) and scatter them in."""
        sub = L.BatchDesc.from_buffer_copy(b)
        idx = np.ascontiguousarray(ids, dtype=np.int64)
        sub.rep_idx = idx.ctypes.data_as(L._pi64)
        sub.replica0, sub.n_local, sub.rep_lo, sub.rep_cnt = 0, int(idx.size), 0, 0
        sub.cap_scale = float(scale)
        sub.sweep_mode = int(mode)
        sub.chunk = 0
        r = self._launch(lib, sub, dev, int(idx.size), Ks, n_grid, n_rep, event_log, use)
        _scatter(res, pick, r, dev, event_log)

    def _ws_budget(self, dev, sk=None):
        """The workspace's device-memory budget (rq_batch_desc.ws_budget): 0.9 x what this
        process can get -- the device's free memory, torch's cached (reserved, unallocated)
        blocks and the stream's own workspace, which the next one replaces."""
        if not torch.cuda.is_available():
            return 0   # plan queries without a device: the library's default
        free, _total = torch.cuda.mem_get_info(dev)
        cached = torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
        ws = self._wss.get(sk if sk is not None else torch.cuda.current_stream().cuda_stream)
        held = ws.numel() if ws is not None else 0
        return int(0.9 * (free + cached + held))

    def _plugin_streams(self, b, keep, dev, R_all, gids, world_seed, seed_mod, override=None):
        """Per-replica times of the registered plugin broadcasters of a randomized
        batch: replica i's instance gets seed u_i + 99 idx (randomize_other_sources,
        opt_model.py:795-804) and the host runs its initialize() / get_all_times() (or a
        self-driven dynamic plugin's schedule); ``override``: {global id: [times per
        plugin]} instead (the reactive fixed point).  The times reach the kernels as
        per-replica RealData streams (rq_batch_desc.rd_*)."""
        wseed = world_seed.to(torch.int64).cpu().numpy() if torch.is_tensor(world_seed) else None
        nrd = len(self.plugins)
        if nrd > L.MAX_RD:
            raise NotImplementedError("more than %d plugin broadcasters" % L.MAX_RD)
        counts = np.zeros((R_all, nrd), dtype=np.int64)
        chunks = []
        # rd_off is a prefix over the global ids: each id once, in increasing order, whatever
        # the order (or repeats) of a caller's rep_idx
        for i in np.unique(np.asarray(gids, dtype=np.int64)):
            i = int(i)
            ts = override[i] if override is not None else \
                [self._plugin_source_times(inst)
                 for inst in self._plugin_instances(i, wseed, world_seed, seed_mod)]
            for c, t in enumerate(ts):
                t = np.asarray(t, dtype=np.float64)
                counts[i, c] = t.size
                chunks.append(t)
        off = np.concatenate([[0], np.cumsum(counts.ravel())]).astype(np.int64)
        times = np.concatenate(chunks) if chunks else np.zeros(0)
        td = torch.from_numpy(np.ascontiguousarray(np.concatenate([times, [0.0]]))).to(dev)
        to = torch.from_numpy(off).to(dev)
        sid = _arr([p[3] for p in self.plugins], np.int64)
        cap = _arr(counts.max(0) if R_all else np.zeros(nrd), np.int64)
        keep += [td, to, sid, cap]
        b.n_rd = nrd
        b.rd_src_id = sid.ctypes.data_as(L._pi64)
        b.rd_cap = cap.ctypes.data_as(L._pi64)
        b.rd_times = td.data_ptr()
        b.rd_off = to.data_ptr()

    def _plugin_instances(self, i, wseed, world_seed, seed_mod):
        """Fresh instances of the registered plugins for global replica i of a
        randomized batch: seed u_i + 99 idx (randomize_other_sources, opt_model.py:795-804)."""
        k = i % seed_mod if seed_mod > 0 else i
        u = int(wseed[i]) if wseed is not None else int(world_seed) + k
        return [cls(**dict(kw, seed=(u + 99 * idx) & 0xFFFFFFFF))
                for idx, cls, kw, _sid, _dyn in self.plugins]

    def _plugin_source_times(self, inst):
        from .opt_model import source_times
        return source_times(inst, self.start_time, self.sink_ids, self._edges, self.end_time)

    VERIFY_ALL = 64   # dynamic-plugin check: every replica of a batch this small, else a sample

    def _verify_dynamic(self, args, kw, res):
        """A dynamic plugin is played from its own schedule: check that it is self-driven
        -- rerun replicas with their event log and feed a fresh copy of each dynamic plugin
        the whole event sequence in play order (opt_model.verify_dynamic_plugin), which
        raises when its schedule reacts to another source's event.  Every replica of a
        batch of <= 64 (one probe batch), else 64 replicas drawn with a seed fixed by the
        batch (one probe run each): a plugin that reacts only in some replicas is caught
        whenever one of them is probed.  Cost: one event-logged run of the probed replicas
        plus a host replay of their events through the plugin (~10-50 ms per replica)."""
        from .opt_model import verify_dynamic_plugin
        gids = np.asarray(res.global_ids, dtype=np.int64)
        R = len(gids)
        if not R:
            return
        base = dict(kw)
        r0 = int(base.get("replica0", 0))
        base.update(event_log=True, check=True)
        if R <= self.VERIFY_ALL:
            probes = [(np.arange(R), self._run(*args, **dict(base, replica0=r0, n_local=R)))]
        else:
            rng = np.random.default_rng([0x52510000, R, int(gids[0])])
            pick = np.sort(rng.choice(R, self.VERIFY_ALL, replace=False))
            probes = [(np.asarray([j]), self._run(*args, **dict(base, replica0=r0 + int(j), n_local=1)))
                      for j in pick]
        ws = kw.get("world_seed", 0)
        wseed = ws.to(torch.int64).cpu().numpy() if torch.is_tensor(ws) else None
        me = kw.get("max_events")
        me = None if me is None or me == float("inf") else int(me)
        for idx, probe in probes:
            for k, j in enumerate(idx):
                t_ev, s_ev = probe.events(k)
                i = int(gids[j])
                if kw.get("randomize"):
                    make = lambda: self._plugin_instances(i, wseed, ws, int(kw.get("seed_mod", 0)))  # noqa: E731
                else:
                    make = lambda: [cls(**kw_) for _idx, cls, kw_, _sid, _dyn in self.plugins]  # noqa: E731
                for fresh, gen, p in zip(make(), make(), self.plugins):
                    if not p[4]:
                        continue
                    times = self._plugin_source_times(gen)
                    verify_dynamic_plugin(fresh, self.start_time, self.sink_ids, self._edges,
                                          self.end_time, t_ev, s_ev, times, max_events=me)

    def _run_reactive(self, args, kw, res):
        """A batch whose dynamic plugins react to other sources' events, played to the
        fixed point of run_dynamic's loop: every replica's plugin times are recomputed
        from its run's other events (opt_model.reactive_plugin_times, a fresh plugin
        instance per replica) and ONLY the replicas whose times moved are replayed with
        them (per-replica RealData streams, a replica list: rq_batch_desc.rep_idx), until
        no replica's times move; events before a plugin event whose time changed never
        change (every source sees only earlier events), so each rerun fixes at least one
        more plugin event of every replica still moving.  Each replica's result is the
        probe in which its times reproduced themselves (no extra final run).  At most
        max(REACTIVE_MAX_ITERATIONS, 2 x the most plugin events of a replica + 16) reruns,
        else NotImplementedError.  Cost per rerun: one event-logged run of the moving
        replicas and a host pass over their events."""
        from .opt_model import REACTIVE_MAX_ITERATIONS, reactive_plugin_times
        gids = np.asarray(res.global_ids, dtype=np.int64)
        ws = kw.get("world_seed", 0)
        wseed = ws.to(torch.int64).cpu().numpy() if torch.is_tensor(ws) else None
        rand = bool(kw.get("randomize"))
        sm = int(kw.get("seed_mod", 0))
        me = kw.get("max_events")
        me = None if me is None or me == float("inf") else int(me)
        ctrl = args[0] if args else kw.get("ctrl", "opt")
        ck = CTRL_BY_NAME[ctrl] if isinstance(ctrl, str) else int(ctrl)
        static_ids = set(self.static_src_ids)
        if ck in (L.SRC_POISSON2, L.SRC_PWCONST, L.SRC_REALDATA):
            static_ids.add(self.src_id)   # a static controlled source (Poisson2 / PWConst / RealData)

        def make(i):
            if rand:
                return self._plugin_instances(i, wseed, ws, sm)
            return [cls(**kw_) for _idx, cls, kw_, _sid, _dyn in self.plugins]
        times = {int(i): [self._plugin_source_times(inst) for inst in make(int(i))] for i in gids}
        probe_kw = dict(kw, event_log=True, check=True)
        dev = torch.device("cuda", torch.cuda.current_device())
        out = None
        moving = np.arange(len(gids))
        n_max = max((len(t) for ts in times.values() for t in ts), default=0)
        cap_it = max(REACTIVE_MAX_ITERATIONS, 2 * n_max + 16)
        self.reactive_replayed = 0
        for it in range(cap_it + 1):
            pk = dict(probe_kw, rd_override=times)
            if out is not None:   # only the replicas still moving
                pk["rep_idx"] = gids[moving]
            probe = self._run(*args, **pk)
            if out is None:
                out = probe
            else:
                _scatter(out, moving, probe, dev, True)
            self.reactive_replayed += len(moving)
            nxt = []
            for kl, k in enumerate(moving):
                i = int(gids[k])
                t_ev, s_ev = probe.events(kl)
                insts, cur = make(i), times[i]
                new = list(cur)
                for c, p in enumerate(self.plugins):
                    if p[4]:
                        new[c] = reactive_plugin_times(insts[c], self.start_time, self.sink_ids,
                                                       self._edges, self.end_time, t_ev, s_ev,
                                                       max_events=me, static_ids=static_ids)
                if any(not np.array_equal(a_, b_) for a_, b_ in zip(new, cur)):
                    times[i] = new
                    nxt.append(k)
            if not nxt:
                break
            if it == cap_it:
                raise NotImplementedError("reactive dynamic broadcasters: no fixed point after %d "
                                          "reruns" % cap_it)
            moving = np.asarray(nxt, dtype=np.int64)
        self.reactive_reruns = it
        if not kw.get("event_log"):
            out.ev_t = out.ev_src = None
        out.global_ids = gids
        out.replica0 = int(gids[0]) if len(gids) else 0
        return out

    def _plan_variant(self, lib, b):
        info = (C.c_int64 * 8)()
        L.check("rq_plan_info", lib.rq_plan_info(self._h, C.byref(b), info))
        return int(info[0])


def _log_edges(what, graph, edges, bins, default_bins):
    """The time-bin edges of a log metric as float64: ``edges``, or ``bins`` equal bins over
    the graph's [start_time, end_time].  With neither, ``default_bins`` bins; None demands
    one of the two."""
    if default_bins is None and (edges is None) == (bins is None):
        raise ValueError(what + ": give either edges or bins")
    if edges is not None and bins is not None:
        raise ValueError(what + ": give edges or bins, not both")
    if edges is None:
        n = default_bins if bins is None else int(bins)
        if n < 1:
            raise ValueError(what + ": bins >= 1 expected")
        span = graph.end_time - graph.start_time
        e = np.asarray([graph.start_time + span * k / n for k in range(n)] + [graph.end_time],
                       dtype=np.float64)
    else:
        e = _arr(edges, np.float64).reshape(-1)
    if e.size < 2 or not np.all(np.isfinite(e)) or not np.all(e[1:] > e[:-1]):
        raise ValueError(what + ": edges must be finite and strictly increasing")
    return e


class BatchResult:
    """Per-replica outputs (torch tensors on the device), replica i = g * n_rep + r."""

    def __init__(self, graph, metrics, counts, status, ev_t, ev_src, Ks, n_grid, n_rep):
        self.graph = graph
        self.metrics, self.counts, self.status = metrics, counts, status
        self.ev_t, self.ev_src = ev_t, ev_src
        self.Ks = list(int(k) for k in Ks)
        self.n_grid, self.n_rep = n_grid, n_rep

    def top_k(self, k):
        return self.metrics[:, self.Ks.index(k)]

    @property
    def avg_rank(self):
        return self.metrics[:, len(self.Ks)]

    @property
    def r_2(self):
        return self.metrics[:, len(self.Ks) + 1]

    @property
    def num_events(self):
        return self.counts[:, 0]

    @property
    def world_events(self):
        return self.counts[:, 1]

    @property
    def n_events(self):
        return self.counts[:, 2]

    def log_columns(self, stream=None):
        """The reference dataframe rows of every replica's event log, expanded on the
        GPU (rq_log_rows + rq_log_expand; State.get_dataframe, opt_model.py:85-97).
        Returns (row_off [R+1] host int64, {event_id, time_delta, src_id, t, sink_id}
        device tensors); replica i owns rows [row_off[i], row_off[i+1])."""
        if self.ev_t is None:
            raise ValueError("run with event_log=True to export the event log")
        use = stream or torch.cuda.current_stream()
        with torch.cuda.stream(use):
            return self._log_columns(use)

    def _log_columns(self, use):
        dev = self.ev_t.device
        R, cap = self.ev_t.shape
        st = use.cuda_stream
        row_off = torch.empty(R + 1, dtype=torch.int64, device=dev)
        lib = L.lib()
        L.check("rq_log_rows", lib.rq_log_rows(self.graph._h, self.ev_src.data_ptr(),
                                               self.counts.data_ptr(), R, cap,
                                               row_off.data_ptr(), st))
        ro = row_off.cpu().numpy()
        n = int(ro[-1])
        cols = {"event_id": torch.empty(n, dtype=torch.int64, device=dev),
                "time_delta": torch.empty(n, dtype=torch.float64, device=dev),
                "src_id": torch.empty(n, dtype=torch.int64, device=dev),
                "t": torch.empty(n, dtype=torch.float64, device=dev),
                "sink_id": torch.empty(n, dtype=torch.int64, device=dev)}
        if n:
            L.check("rq_log_expand", lib.rq_log_expand(
                self.graph._h, self.ev_t.data_ptr(), self.ev_src.data_ptr(),
                self.counts.data_ptr(), R, cap, row_off.data_ptr(),
                *(cols[k].data_ptr() for k in ("event_id", "time_delta", "src_id", "t", "sink_id")),
                st))
        return ro, cols

    def dataframe(self, i=None):
        """State.get_dataframe() of replica i, or of all replicas with a leading
        'replica' column (i=None); rows expanded on the GPU."""
        import pandas as pd
        ro, cols = self.log_columns()
        host = {k: v.cpu().numpy() for k, v in cols.items()}
        if i is not None:
            a, b = int(ro[i]), int(ro[i + 1])
            return pd.DataFrame({k: host[k][a:b] for k in
                                 ("event_id", "time_delta", "src_id", "t", "sink_id")})
        gids = getattr(self, "global_ids", None)
        if gids is None:
            gids = np.arange(len(ro) - 1, dtype=np.int64) + getattr(self, "replica0", 0)
        rep = np.repeat(np.asarray(gids, dtype=np.int64), np.diff(ro))
        return pd.DataFrame(dict(replica=rep, **host))

    def _log_graph(self):
        """The graph of timeline / followers / rank_hist, which need the event logs."""
        if self.ev_t is None:
            raise ValueError("run with event_log=True to export the event log")
        return self.graph

    def _log_ks(self, Ks):
        """The K values of a log metric as int32: ``Ks``, default the result's own."""
        ks = _arr(self.Ks if Ks is None else Ks, np.int32).reshape(-1)
        if not 1 <= ks.size <= L.MAX_K or ks.min() < 1:
            raise ValueError("1..%d K values >= 1" % L.MAX_K)
        return ks

    def timeline(self, edges=None, bins=None, Ks=None, wall=False, stream=None):
        """The metrics split over time bins, straight from the event logs
        (rq_log_timeline): ``edges`` [n_bins + 1], strictly increasing and finite, or
        ``bins`` = n equal bins over the graph's [start_time, end_time].  ``Ks``: default
        the result's own; ``wall``: also the wall rows per (sink, bin).  Returns a
        ``Timeline`` of device tensors; needs event_log=True."""
        g = self._log_graph()
        e = _log_edges("timeline", g, edges, bins, None)
        ks = self._log_ks(Ks)
        use = stream or torch.cuda.current_stream()
        with torch.cuda.stream(use):
            dev = self.ev_t.device
            R, cap = self.ev_t.shape
            nb = e.size - 1
            ed = torch.from_numpy(e).to(dev)
            metrics = torch.empty((R, nb, ks.size + 2), dtype=torch.float64, device=dev)
            posts = torch.empty((R, nb, 2), dtype=torch.int64, device=dev)
            status = torch.empty(R, dtype=torch.int32, device=dev)
            wp = torch.empty((R, g.n_sinks, nb), dtype=torch.int32, device=dev) if wall else None
            L.check("rq_log_timeline", L.lib().rq_log_timeline(
                g._h, self.ev_t.data_ptr(), self.ev_src.data_ptr(), self.counts.data_ptr(), R, cap,
                ed.data_ptr(), nb, ks.ctypes.data_as(L._pi32), ks.size, metrics.data_ptr(),
                posts.data_ptr(), wp.data_ptr() if wall else None, status.data_ptr(),
                use.cuda_stream))
        return Timeline(e, ed, [int(k) for k in ks], metrics, posts, status, wp,
                        np.sort(g.sink_ids))

    def followers(self, Ks=None, rows=False, stream=None, tiled=None):
        """The metrics split over the followers, straight from the event logs
        (rq_log_followers): per (replica, sink) the integrals of I(r <= K-1), r and r^2
        over the sink's seen span, its first-row time and, with ``rows``, its own / wall
        row counts; per replica int_r_2_true.  ``Ks``: default the result's own.
        ``tiled``: None takes rq_log_followers while the graph's sinks fit its limit
        (rq_log_followers_max_sinks) and the sink-tiled rq_log_followers_tiled (up to
        FOLLOWERS_TILED_MAX_SINKS sinks, the same bits) past it; True / False force the
        tiled / the plain entry.  Returns a ``Followers`` of device tensors; needs
        event_log=True."""
        g = self._log_graph()
        ks = self._log_ks(Ks)
        lib = L.lib()
        if tiled is None:
            tiled = g.n_sinks > lib.rq_log_followers_max_sinks(ks.size, 1 if rows else 0)
        use = stream or torch.cuda.current_stream()
        with torch.cuda.stream(use):
            dev = self.ev_t.device
            R, cap = self.ev_t.shape
            ws = None
            if tiled:   # refused graphs are refused before anything is allocated
                nb = C.c_size_t()
                L.check("rq_log_followers_tiled_workspace",
                        lib.rq_log_followers_tiled_workspace(g._h, R, C.byref(nb)))
                ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
            vals = torch.empty((R, g.n_sinks, ks.size + 2), dtype=torch.float64, device=dev)
            first_t = torch.empty((R, g.n_sinks), dtype=torch.float64, device=dev)
            rw = torch.empty((R, g.n_sinks, 2), dtype=torch.int32, device=dev) if rows else None
            r2 = torch.empty(R, dtype=torch.float64, device=dev)
            status = torch.empty(R, dtype=torch.int32, device=dev)
            if tiled:
                L.check("rq_log_followers_tiled", lib.rq_log_followers_tiled(
                    g._h, self.ev_t.data_ptr(), self.ev_src.data_ptr(), self.counts.data_ptr(), R, cap,
                    ks.ctypes.data_as(L._pi32), ks.size, vals.data_ptr(), first_t.data_ptr(),
                    rw.data_ptr() if rows else None, r2.data_ptr(), status.data_ptr(),
                    ws.data_ptr(), nb.value, use.cuda_stream))   # ws: allocated on `use`, reused there only
            else:
                L.check("rq_log_followers", lib.rq_log_followers(
                    g._h, self.ev_t.data_ptr(), self.ev_src.data_ptr(), self.counts.data_ptr(), R, cap,
                    ks.ctypes.data_as(L._pi32), ks.size, vals.data_ptr(), first_t.data_ptr(),
                    rw.data_ptr() if rows else None, r2.data_ptr(), status.data_ptr(), use.cuda_stream))
        return Followers([int(k) for k in ks], vals, first_t, rw, r2, status, np.sort(g.sink_ids))

    def rank_hist(self, ranks=64, edges=None, bins=None, stream=None):
        """The rank distribution over time bins, straight from the event logs
        (rq_log_rank_hist): per (replica, bin) the seen sink-time at rank 0 .. ranks - 1
        and, in a last cell, at rank >= ``ranks`` (the tail), each as a share of the seen
        sinks.  ``edges`` / ``bins`` as in timeline(); with neither, one bin over the
        graph's [start_time, end_time].  1 <= ranks <= RANK_HIST_MAX_RANKS.  Returns a
        ``RankHist`` of device tensors; needs event_log=True."""
        g = self._log_graph()
        e = _log_edges("rank_hist", g, edges, bins, 1)
        nr = int(ranks)
        if not 1 <= nr <= L.RANK_HIST_MAX_RANKS:
            raise ValueError("rank_hist: 1 <= ranks <= %d expected" % L.RANK_HIST_MAX_RANKS)
        use = stream or torch.cuda.current_stream()
        with torch.cuda.stream(use):
            dev = self.ev_t.device
            R, cap = self.ev_t.shape
            nb = e.size - 1
            ed = torch.from_numpy(e).to(dev)
            hist = torch.empty((R, nb, nr + 1), dtype=torch.float64, device=dev)
            n_seen = torch.empty(R, dtype=torch.int32, device=dev)
            max_rank = torch.empty(R, dtype=torch.int32, device=dev)
            status = torch.empty(R, dtype=torch.int32, device=dev)
            L.check("rq_log_rank_hist", L.lib().rq_log_rank_hist(
                g._h, self.ev_t.data_ptr(), self.ev_src.data_ptr(), self.counts.data_ptr(), R, cap,
                ed.data_ptr(), nb, nr, hist.data_ptr(), n_seen.data_ptr(), max_rank.data_ptr(),
                status.data_ptr(), use.cuda_stream))
        return RankHist(e, nr, hist, n_seen, max_rank, status)

    LOG_METRICS_WS_BYTES = 1 << 31   # workspace budget of one rq_log_metrics call

    def _lm_entry(self, slim, nK, of=False):
        """(name, workspace query, entry, slim) of log_metrics' / source_metrics' ABI entry.
        ``slim`` False: the 16-byte cells; True: the 8-byte cells (rq_log_metrics_slim,
        rq_log_metrics_of_slim); None: the 16-byte entry, and the slim one where the 16-byte
        one answers RQ_EUNSUPPORTED and the slim one does not."""
        lib = L.lib()
        base = "rq_log_metrics_of" if of else "rq_log_metrics"
        plain = (base, getattr(lib, base + "_workspace"), getattr(lib, base), False)
        if slim is False:
            return plain
        if not all(L.has(fn) for fn in L.OPTIONAL_SLIM):
            if slim:
                raise L.RQError(base + "_slim", L.RQ_EUNSUPPORTED)
            return plain
        thin = (base + "_slim", getattr(lib, base + "_slim_workspace"), getattr(lib, base + "_slim"), True)
        if slim:
            return thin
        R, cap = self.ev_t.shape
        nb = C.c_size_t()
        args = (self.graph._h,) + ((1,) if of else ()) + (max(1, R), max(1, cap), nK, C.byref(nb))
        if plain[1](*args) == L.RQ_EUNSUPPORTED and thin[1](*args) == L.RQ_OK:
            return thin
        return plain

    def log_metrics(self, Ks=None, stream=None, slim=None):
        """The whole-horizon metrics and counts straight from the event logs, exact on
        equal times (rq_log_metrics): what rq_metrics_replay_batch gives on the logs'
        dataframe rows, bit for bit, without a dataframe.  ``Ks``: default the result's
        own.  Returns a ``LogMetrics`` of device tensors: ``metrics`` [R, nK + 2],
        ``counts`` [R, 4] (own events, other events, pivot rows, pivot columns) and
        ``status`` [R] (ST_TIE is informational, ST_EMPTY replicas are NaN).  Replicas go
        in chunks that keep the workspace within LOG_METRICS_WS_BYTES.  ``slim``: the cell
        layout.  None (default): rq_log_metrics, and rq_log_metrics_slim -- 8-byte cells,
        the same bits, a larger workspace -- for the graphs only the latter takes (more
        than LOG_METRICS_MAX_SINKS and up to LOG_METRICS_SLIM_MAX_SINKS sinks); False /
        True: that entry, whatever the graph (``.slim`` of the result says which ran).
        Raises RQError(RQ_EUNSUPPORTED) for a graph with duplicate edges or more sinks than
        the entry takes, and for logs with room for more than 2^20 events per
        replica (``ev_t.shape[1]``; ``utils.replay_columns`` over ``log_columns()`` takes
        those); needs event_log=True."""
        self._log_graph()
        ks = self._log_ks(Ks)
        use = stream or torch.cuda.current_stream()
        with torch.cuda.stream(use):
            return self._log_metrics(ks, use, slim)

    def _log_metrics(self, ks, use, slim=None):
        g = self.graph
        name, query, entry, thin = self._lm_entry(slim, ks.size)
        wname = name + "_workspace"
        dev = self.ev_t.device
        R, cap = self.ev_t.shape
        metrics = torch.empty((R, ks.size + 2), dtype=torch.float64, device=dev)
        counts = torch.empty((R, 4), dtype=torch.int64, device=dev)
        status = torch.empty(R, dtype=torch.int32, device=dev)
        nb = C.c_size_t()
        if R == 0 or cap == 0:   # nothing to play: every replica is empty
            L.check(wname, query(g._h, 1, 1, ks.size, C.byref(nb)))
            metrics.fill_(float("nan"))
            counts.zero_()
            status.fill_(L.ST_EMPTY)
            return LogMetrics([int(k) for k in ks], metrics, counts, status, thin)
        # the whole batch in one launch if its workspace (which stops growing at a fixed
        # number of blocks) fits the budget, else as many replicas a call as fit it
        chunk = R
        L.check(wname, query(g._h, R, cap, ks.size, C.byref(nb)))
        if nb.value > self.LOG_METRICS_WS_BYTES:
            L.check(wname, query(g._h, 1, cap, ks.size, C.byref(nb)))
            chunk = max(1, min(R, self.LOG_METRICS_WS_BYTES // nb.value))
            L.check(wname, query(g._h, chunk, cap, ks.size, C.byref(nb)))
        ws = torch.empty(max(256, nb.value), dtype=torch.uint8, device=dev)
        for lo in range(0, R, chunk):
            n = min(chunk, R - lo)
            L.check(name, entry(
                g._h, self.ev_t[lo:].data_ptr(), self.ev_src[lo:].data_ptr(), self.counts[lo:].data_ptr(),
                n, cap, ks.ctypes.data_as(L._pi32), ks.size, metrics[lo:].data_ptr(),
                counts[lo:].data_ptr(), status[lo:].data_ptr(), ws.data_ptr(), ws.numel(),
                use.cuda_stream))   # ws: allocated on `use`, reused there only
        return LogMetrics([int(k) for k in ks], metrics, counts, status, thin)

    def source_metrics(self, src_ids=None, scope="own", Ks=None, stream=None, slim=None):
        """log_metrics for any sources of the graph (rq_log_metrics_of): the reference's
        time_in_top_k(df, K, src_id=c), average_rank(df, src_id=c) and int_r_2 for every
        c of ``src_ids`` -- default the result's ``player_ids`` when it has them, else
        every source of the graph.  ``scope`` "df": on the replica's whole dataframe;
        "own": on df[df.sink_id.isin(followers of c)], the feeds an Opt tracks its rank
        on.  Returns a ``SourceMetrics`` of device tensors: ``metrics`` [R, P, nK + 2],
        ``counts`` [R, P, 4] (c's events with a row, the others', pivot rows, pivot
        columns) and ``status`` [R, P].  Sources go in chunks of LOG_OF_MAX_SRC, replicas
        in chunks that keep the workspace within LOG_METRICS_WS_BYTES.  ``slim``: as
        log_metrics' (rq_log_metrics_of_slim).  Raises as log_metrics does; needs
        event_log=True."""
        g = self._log_graph()
        ks = self._log_ks(Ks)
        if scope not in ("df", "own"):
            raise ValueError('source_metrics: scope "df" or "own" expected')
        if src_ids is None:
            src_ids = getattr(self, "player_ids", None) or g.stream_src_ids
        ids = _arr(src_ids, np.int64).reshape(-1)
        known = set(int(s) for s in g.stream_src_ids)
        if ids.size < 1 or len(set(ids.tolist())) != ids.size or not set(ids.tolist()) <= known:
            raise ValueError("source_metrics: distinct sources of the graph expected")
        if not all(L.has(fn) for fn in L.OPTIONAL):
            raise L.RQError("rq_log_metrics_of", L.RQ_EUNSUPPORTED)
        use = stream or torch.cuda.current_stream()
        with torch.cuda.stream(use):
            return self._source_metrics(ids, L.LOG_OF_OWN if scope == "own" else L.LOG_OF_DF, ks, use, slim)

    def _source_metrics(self, ids, scope, ks, use, slim=None):
        g = self.graph
        name, query, entry, thin = self._lm_entry(slim, ks.size, of=True)
        wname = name + "_workspace"
        dev = self.ev_t.device
        R, cap = self.ev_t.shape
        P, nK = ids.size, ks.size
        nb = C.c_size_t()
        out = SourceMetrics([int(s) for s in ids], [int(k) for k in ks],
                            torch.empty((R, P, nK + 2), dtype=torch.float64, device=dev),
                            torch.empty((R, P, 4), dtype=torch.int64, device=dev),
                            torch.empty((R, P), dtype=torch.int32, device=dev), thin)
        if R == 0 or cap == 0:   # nothing to play: every (replica, source) is empty
            L.check(wname, query(g._h, 1, 1, 1, nK, C.byref(nb)))
            out.metrics.fill_(float("nan"))
            out.counts.zero_()
            out.status.fill_(L.ST_EMPTY)
            return out
        ws = None
        for p0 in range(0, P, L.LOG_OF_MAX_SRC):
            sub = np.ascontiguousarray(ids[p0:p0 + L.LOG_OF_MAX_SRC])
            n_src = sub.size
            # the whole batch in one launch if its workspace (which stops growing at a fixed
            # number of blocks) fits the budget, else as many replicas a call as fit it
            chunk = R
            L.check(wname, query(g._h, n_src, R, cap, nK, C.byref(nb)))
            if nb.value > self.LOG_METRICS_WS_BYTES:
                L.check(wname, query(g._h, 1, 1, cap, nK, C.byref(nb)))
                chunk = max(1, min(R, self.LOG_METRICS_WS_BYTES // nb.value // n_src))
                L.check(wname, query(g._h, n_src, chunk, cap, nK, C.byref(nb)))
            if ws is None or ws.numel() < nb.value:
                ws = torch.empty(max(256, nb.value), dtype=torch.uint8, device=dev)
            whole = n_src == P
            for lo in range(0, R, chunk):
                n = min(chunk, R - lo)
                # a chunk of the sources writes its own [n, n_src, ...] block, copied into place
                m, c, s = ((out.metrics[lo:], out.counts[lo:], out.status[lo:]) if whole else
                           (torch.empty((n, n_src, nK + 2), dtype=torch.float64, device=dev),
                            torch.empty((n, n_src, 4), dtype=torch.int64, device=dev),
                            torch.empty((n, n_src), dtype=torch.int32, device=dev)))
                L.check(name, entry(
                    g._h, sub.ctypes.data_as(L._pi64), n_src, scope, self.ev_t[lo:].data_ptr(),
                    self.ev_src[lo:].data_ptr(), self.counts[lo:].data_ptr(), n, cap,
                    ks.ctypes.data_as(L._pi32), nK, m.data_ptr(), c.data_ptr(), s.data_ptr(),
                    ws.data_ptr(), ws.numel(), use.cuda_stream))   # ws: allocated on `use`, reused there only
                if not whole:
                    out.metrics[lo:lo + n, p0:p0 + n_src] = m
                    out.counts[lo:lo + n, p0:p0 + n_src] = c
                    out.status[lo:lo + n, p0:p0 + n_src] = s
        return out

    def player_metrics(self, scope="own", Ks=None, stream=None, slim=None):
        """source_metrics of the game's players (``player_ids``, in their order): how
        visible every competing Opt ended up, on its own followers' feeds (scope "own") or
        on the whole dataframe ("df"); ``slim`` as source_metrics'.  ValueError for a
        result without players."""
        ids = getattr(self, "player_ids", None)
        if not ids:
            raise ValueError("player_metrics: the result of a game (Opt broadcasters among the sources) expected")
        return self.source_metrics(ids, scope=scope, Ks=Ks, stream=stream, slim=slim)

    def events(self, i):
        """(t, src_id) numpy arrays of replica i (needs event_log=True)."""
        n = int(self.counts[i, 2].item())
        t = self.ev_t[i, :n].cpu().numpy()
        s = self.graph.stream_src_ids[self.ev_src[i, :n].cpu().numpy()]
        return t, s


class LogMetrics:
    """BatchResult.log_metrics' outputs: ``metrics`` [R, nK + 2] (top_K..., avg_rank,
    r_2), ``counts`` [R, 4] (the controlled source's events with an edge, the others',
    pivot rows, pivot columns) and ``status`` [R] (0, ST_TIE: informational, or ST_EMPTY:
    metrics NaN), device tensors; ``slim``: the 8-byte-cell entry computed them."""

    def __init__(self, Ks, metrics, counts, status, slim=False):
        self.Ks, self.metrics, self.counts, self.status, self.slim = Ks, metrics, counts, status, slim

    def top_k(self, k):
        return self.metrics[:, self.Ks.index(k)]

    @property
    def avg_rank(self):
        return self.metrics[:, len(self.Ks)]

    @property
    def r_2(self):
        return self.metrics[:, len(self.Ks) + 1]


class SourceMetrics:
    """BatchResult.source_metrics' outputs for the sources ``src_ids`` [P]: ``metrics``
    [R, P, nK + 2] (top_K..., avg_rank, r_2), ``counts`` [R, P, 4] (the source's events
    with a row, the other sources', pivot rows, pivot columns) and ``status`` [R, P] (0,
    ST_TIE: informational, or ST_EMPTY: metrics NaN), device tensors; ``slim``: the
    8-byte-cell entry computed them."""

    def __init__(self, src_ids, Ks, metrics, counts, status, slim=False):
        self.src_ids, self.Ks, self.slim = src_ids, Ks, slim
        self.metrics, self.counts, self.status = metrics, counts, status

    def top_k(self, k):
        return self.metrics[:, :, self.Ks.index(k)]

    @property
    def avg_rank(self):
        return self.metrics[:, :, len(self.Ks)]

    @property
    def r_2(self):
        return self.metrics[:, :, len(self.Ks) + 1]


class Timeline:
    """BatchResult.timeline's outputs: ``metrics`` [R, n_bins, nK + 2] (top_K...,
    avg_rank, r_2: each bin's share of BatchResult.metrics), ``posts`` [R, n_bins, 2]
    (own, other), ``status`` [R] (0, ST_TIE or ST_EMPTY: metrics NaN) and ``wall_posts``
    [R, n_sinks, n_bins] or None, device tensors; ``edges`` (host float64) and
    ``sink_ids``, the sink of every wall_posts row (ascending ids)."""

    def __init__(self, edges, edges_dev, Ks, metrics, posts, status, wall_posts, sink_ids):
        self.edges, self._edges_dev, self.Ks = edges, edges_dev, Ks
        self.metrics, self.posts, self.status, self.wall_posts = metrics, posts, status, wall_posts
        self.sink_ids = sink_ids

    def top_k(self, k):
        return self.metrics[:, :, self.Ks.index(k)]

    @property
    def avg_rank(self):
        return self.metrics[:, :, len(self.Ks)]

    @property
    def r_2(self):
        return self.metrics[:, :, len(self.Ks) + 1]

    def wall_intensities(self):
        """wall_posts per unit time: [R, n_sinks, n_bins] float64 (needs wall=True)."""
        if self.wall_posts is None:
            raise ValueError("timeline(wall=True) needed for wall intensities")
        width = self._edges_dev[1:] - self._edges_dev[:-1]
        return self.wall_posts.to(torch.float64) / width


class RankHist:
    """BatchResult.rank_hist's outputs: ``hist`` [R, n_bins, ranks + 1] (the seen
    sink-time at rank 0 .. ranks - 1 and, last, at rank >= ranks, over the replica's seen
    sinks S: top_K is the sum of the first K cells), ``n_seen`` [R] (S), ``max_rank`` [R]
    (the largest rank of the replica, -1 without a row: ranks > max_rank leaves the tail
    empty) and ``status`` [R] (0, ST_TIE or ST_EMPTY: hist NaN), tensors on the run's
    device; ``edges`` (host float64) and ``ranks``."""

    def __init__(self, edges, ranks, hist, n_seen, max_rank, status):
        self.edges, self.ranks = edges, int(ranks)
        self.hist, self.n_seen, self.max_rank, self.status = hist, n_seen, max_rank, status

    def top_k(self, k):
        """Time in the top k per (replica, bin), [R, n_bins]: 1 <= k <= ranks."""
        k = int(k)
        if not 1 <= k <= self.ranks:
            raise ValueError("top_k: 1 <= k <= %d (the histogram's ranks) expected" % self.ranks)
        return self.hist[:, :, :k].sum(-1)

    @property
    def tail(self):
        """The seen sink-time at rank >= ranks, [R, n_bins]."""
        return self.hist[:, :, self.ranks]

    def cdf(self):
        """The cumulative share of the bin's seen sink-time at rank <= rho (the last
        cell, the tail included, is 1), [R, n_bins, ranks + 1]; NaN where the bin's
        total is 0."""
        c = self.hist.cumsum(-1)
        tot = c[:, :, -1:]
        return torch.where(tot > 0, c / tot, torch.full_like(c, float("nan")))

    def quantile(self, p):
        """The smallest rho whose cdf >= p (0 < p <= 1), int64 [R, n_bins]: ``ranks``
        means "in the tail"; -1 where the cdf is NaN."""
        p = float(p)
        if not 0.0 < p <= 1.0:
            raise ValueError("quantile: 0 < p <= 1 expected")
        c = self.cdf()
        q = (c < p).sum(-1)
        return torch.where(torch.isnan(c[:, :, -1]), torch.full_like(q, -1), q)


class Followers:
    """BatchResult.followers' outputs: ``vals`` [R, n_sinks, nK + 2] (top_K..., the
    integrals of r and of r^2 over every sink's seen span; 0 for a sink without a row),
    ``first_t`` [R, n_sinks] (NaN without a row), ``rows`` [R, n_sinks, 2] (own, wall) or
    None, ``r_2_true`` [R] (utils.int_r_2_true) and ``status`` [R] (0, ST_TIE or ST_EMPTY:
    vals and r_2_true NaN), device tensors; ``Ks`` and ``sink_ids``, the sink of every
    column (ascending ids)."""

    def __init__(self, Ks, vals, first_t, rows, r_2_true, status, sink_ids):
        self.Ks, self.vals, self.first_t, self.rows = Ks, vals, first_t, rows
        self.r_2_true, self.status, self.sink_ids = r_2_true, status, sink_ids

    def top_k(self, k):
        return self.vals[:, :, self.Ks.index(k)]

    @property
    def rank_int(self):
        return self.vals[:, :, len(self.Ks)]

    @property
    def rank_sq_int(self):
        return self.vals[:, :, len(self.Ks) + 1]

    def _per_sink(self, s):
        """s per column of sink_ids: a scalar, a dict by sink id (a sink it does not
        name weighs 0: Opt's s names the controlled source's followers only) or an array
        in sink_ids order (host float64)."""
        n = len(self.sink_ids)
        if isinstance(s, dict):
            return np.asarray([float(s.get(int(x), 0.0)) for x in self.sink_ids], dtype=np.float64)
        v = np.asarray(s, dtype=np.float64)
        if v.ndim == 0:
            return np.full(n, float(v))
        if v.shape != (n,):
            raise ValueError("s: a scalar, a dict by sink id or %d values expected" % n)
        return v

    def loss(self, s):
        """0.5 * sum_x s_x * rank_sq_int[:, x]: the significance-weighted quadratic cost
        of every replica over each follower's seen span, [R]."""
        w = torch.from_numpy(self._per_sink(s)).to(self.vals.device)
        return 0.5 * (self.rank_sq_int * w).sum(1)

    def u_int(self, s, q):
        """sum_x sqrt(s_x / q) * rank_int[:, x], [R]."""
        w = torch.from_numpy(np.sqrt(self._per_sink(s) / float(q))).to(self.vals.device)
        return (self.rank_int * w).sum(1)


def expected_events(graph_kw):
    """Rough expected event count of a world (for sizing benchmarks)."""
    span = graph_kw["end_time"] - graph_kw.get("start_time", 0.0)
    tot = 0.0
    for name, kw in graph_kw["other_sources"]:
        if name in ("Poisson", "Poisson2"):
            tot += kw.get("rate", 1.0) * span
        elif name == "Hawkes":
            br = kw.get("alpha", 1.0) / kw.get("beta", 10.0)
            tot += kw.get("l_0", 1.0) * span / max(1e-9, 1 - br)
    return tot if math.isfinite(tot) else 0.0


def _scatter(res, pick, r, dev, event_log):
    """Rows of BatchResult ``r`` into outputs ``pick`` of ``res`` (event logs widened to
    the larger capacity when ``event_log``)."""
    at = torch.from_numpy(np.asarray(pick, dtype=np.int64)).to(dev)
    res.metrics.index_copy_(0, at, r.metrics)
    res.counts.index_copy_(0, at, r.counts)
    res.status.index_copy_(0, at, r.status)
    if event_log:
        cap, cap2 = res.ev_t.shape[1], r.ev_t.shape[1]
        if cap2 > cap:   # a larger event capacity: widen every replica's log row
            t2 = torch.empty((res.ev_t.shape[0], cap2), dtype=res.ev_t.dtype, device=dev)
            s2 = torch.empty((res.ev_src.shape[0], cap2), dtype=res.ev_src.dtype, device=dev)
            t2[:, :cap] = res.ev_t
            s2[:, :cap] = res.ev_src
            res.ev_t, res.ev_src = t2, s2
        res.ev_t[at, :cap2] = r.ev_t
        res.ev_src[at, :cap2] = r.ev_src

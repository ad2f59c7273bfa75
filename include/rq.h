/*
 * rq.h -- C ABI of librq.so, the MI355X (gfx950) RedQueen Monte-Carlo engine.
 *
 * The reference (MPI-SWS/RedQueen) is pure Python with no FFI; these entry
 * points replace the following in-process Python calls (file:line into the
 * reference):
 *
 *   rq_graph_build      SimOpts(**kw)                      opt_model.py:773-780
 *                       + Manager.__init__ validation       opt_model.py:145-181
 *                       + Broadcaster.init_state sink lists opt_model.py:340-344
 *   rq_run_batch        SimOpts.create_manager_with_opt     opt_model.py:806-811
 *                       / _with_poisson :821-837 / _for_wall :886-891
 *                       / _with_times :893-898 / _with_piecewise_const :839-848
 *                       -> Manager.run_dynamic              opt_model.py:241-314
 *                       -> State.get_dataframe              opt_model.py:85-97
 *                       -> utils.time_in_top_k / average_rank / int_r_2 /
 *                          num_tweets_of                    utils.py:84-121,170-176
 *                       over a seeds x q x s grid, i.e. the loops of
 *                       utils.calc_q_capacity_iter          utils.py:447-470 and
 *                       opt_runs.worker_opt/worker_poisson  opt_runs.py:51-126
 *                       with opt_runs.add_perf's fields     opt_runs.py:41-48
 *   rq_metrics_replay   utils.time_in_top_k(df, K, ...)     utils.py:84-98
 *   (_batch: many dfs)  utils.average_rank(df, ...)         utils.py:101-114
 *                       utils.int_r_2(df, ...)              utils.py:117-121
 *                       utils.num_tweets_of(df, ...)        utils.py:170-176
 *                       on dataframes in the reference's row layout (raw sink ids).
 *   rq_oracle_dp        utils.oracle_ranking(df, sim_opts)  utils.py:181-245
 *                       (batched over walls / q values: the loops of
 *                       find_opt_oracle :260-340 and opt_runs.worker_oracle
 *                       opt_runs.py:129-155)
 *   rq_rank_table       utils.rank_of_src_in_df(df, src)    utils.py:38-56
 *   rq_u_int            utils.u_int_opt(df, ...)            utils.py:59-81
 *   rq_log_rows /       State.get_dataframe()               opt_model.py:85-97
 *   rq_log_expand       for every replica of an RQ_RUN_EVENT_LOG batch at once
 *   rq_log_timeline     utils.rank_of_src_in_df + time_in_top_k / average_rank /
 *                       int_r_2 split over time bins         utils.py:38-56, :84-121
 *                       and the posts per (sink, segment) opt_runs.py:69-84 counts,
 *                       for every replica of an RQ_RUN_EVENT_LOG batch at once
 *   rq_log_followers    utils.rank_of_src_in_df + the same integrals per sink column
 *                       and int_r_2_true                     utils.py:38-56, :84-128
 *                       for every replica of an RQ_RUN_EVENT_LOG batch at once
 *   rq_log_followers_tiled  the same, sink-tiled: graphs of up to 40,960 sinks
 *   rq_log_rank_hist    utils.rank_of_src_in_df + time_in_top_k for every K at once:
 *                       the seen sink-time per rank value and time bin
 *                       utils.py:38-56, :84-98 (opt_runs.py:31-33's Ks curve)
 *                       for every replica of an RQ_RUN_EVENT_LOG batch at once
 *   rq_log_metrics      utils.rank_of_src_in_df + time_in_top_k / average_rank /
 *                       int_r_2 / num_tweets_of over the whole horizon, exact on
 *                       equal times                          utils.py:38-56, :84-121, :170-176
 *                       for every replica of a batch of event logs at once
 *   rq_log_metrics_of   the same with src_id = any source of the graph, on the df or on
 *                       df[df.sink_id.isin(its followers)], several sources in one call
 *   rq_log_metrics_slim, rq_log_metrics_of_slim   the two above for graphs of up to 19,400
 *                       sinks (8-byte pivot cells), the same bits
 *   rq_log_game        Opt broadcasters among SimOpts.other_sources  opt_model.py:761,
 *                       each Opt.get_next_interval :502-544 in run_dynamic's loop :271-309
 *
 * Conventions
 *   - every function returns 0 (RQ_OK) or a negative rq_status; no C++
 *     exception crosses the ABI; rq_strerror() names a code.
 *   - rq_graph_t handles are immutable after build and may be shared by threads.
 *   - rq_run_batch / rq_metrics_replay are stream-ordered and asynchronous:
 *     they enqueue work on `hip_stream` (a hipStream_t, NULL = default stream)
 *     and never touch caller memory on the host side.  The caller owns every
 *     device buffer (workspace and outputs) and must keep them alive until the
 *     stream has passed the work.  rq_run_batch stages its per-run parameter
 *     tables through a ring of 4 pinned host buffers owned by the graph handle:
 *     the ring is allocated (hipHostMalloc) on the first call and when a larger
 *     table is needed, and a call waits (hipEventSynchronize) for the copy
 *     issued by the call 4 earlier on the same graph before reusing its slot --
 *     so a warm-up call keeps allocation out of timed regions, and a caller
 *     issuing many batches back to back runs at most 4 copies ahead.
 *     rq_metrics_replay never allocates or waits.  One device per process; the
 *     caller selects it.
 *   - "device pointer" = memory allocated on the current HIP device
 *     (e.g. torch.empty(..., device="cuda").data_ptr()).
 */
#ifndef RQ_H
#define RQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RQ_ABI_VERSION 6
#define RQ_MAX_K 4 /* at most 4 K values (perf_opts.Ks, opt_runs.py:31-38) per run */

typedef enum {
    RQ_OK = 0,
    RQ_EINVAL = -1,       /* bad argument / reference would raise (assert, ValueError, KeyError) */
    RQ_EOVERFLOW = -2,    /* a capacity was too small (see per-replica status bits)    */
    RQ_EHIP = -3,         /* a HIP runtime call failed                                   */
    RQ_ENOMEM = -4,       /* host or device allocation failed                            */
    RQ_EUNSORTED = -5,    /* replay: df 't' column is not non-decreasing                 */
    RQ_EUNSUPPORTED = -6  /* valid for the reference, not supported by this engine       */
} rq_status;

/* broadcaster kinds (SimOpts.broadcasters, opt_model.py:758-766) */
typedef enum {
    RQ_SRC_NONE = 0,      /* controlled slot only: create_manager_for_wall          */
    RQ_SRC_POISSON = 1,   /* Poisson        opt_model.py:424-433 (dynamic)          */
    RQ_SRC_POISSON2 = 2,  /* Poisson2       opt_model.py:381-421 (static)           */
    RQ_SRC_HAWKES = 3,    /* Hawkes         opt_model.py:458-490                    */
    RQ_SRC_PWCONST = 4,   /* PiecewiseConst opt_model.py:626-689                    */
    RQ_SRC_REALDATA = 5,  /* RealData       opt_model.py:711-750                    */
    RQ_SRC_OPT = 6,       /* Opt = RedQueen opt_model.py:493-544 (controlled only)  */
    RQ_SRC_OPTPW = 7      /* OptPWSignificance opt_model.py:547-623 (controlled only) */
} rq_src_kind;

typedef struct rq_source_desc {
    int32_t kind;        /* rq_src_kind                                                   */
    int32_t n_arr;       /* PWCONST: #segments; REALDATA: #times                           */
    int64_t src_id;
    uint32_t seed;       /* kwargs['seed'] (RandomState seed, opt_model.py:329)            */
    uint32_t flags;      /* RQ_SRCF_* (ABI v6; was reserved, 0)                            */
    double p0, p1, p2;   /* POISSON/POISSON2: rate; HAWKES: l_0, alpha, beta               */
    const double* a;     /* host: PWCONST change_times[n_arr]; REALDATA times[n_arr]       */
    const double* b;     /* host: PWCONST rates[n_arr]                                     */
} rq_source_desc;
/* rq_source_desc.flags: RQ_SRCF_DYNAMIC on an RQ_SRC_REALDATA source = its times are a
   DYNAMIC broadcaster's (a registered plugin with is_dynamic, opt_model.py:259-260,
   replayed from its times): at an equal time it plays before every static source and
   among the dynamic ones (the controller included) in src_id order
   (opt_model.py:279-281, :289-290), like the built-in Poisson / Hawkes. */
#define RQ_SRCF_DYNAMIC 1

typedef struct rq_graph_desc {
    int32_t n_sources;                /* SimOpts.other_sources, in list order          */
    const rq_source_desc* sources;    /* host                                           */
    int32_t n_sinks;
    const int64_t* sink_ids;          /* host, SimOpts.sink_ids                          */
    int64_t n_edges;
    const int64_t* edge_src;          /* host, SimOpts.edge_list in list order           */
    const int64_t* edge_sink;
    int64_t ctrl_src_id;              /* SimOpts.src_id                                  */
    double start_time;                /* Manager start_time (0 in every reference call)  */
    double end_time;                  /* SimOpts.end_time                                */
    /* controlled broadcaster parameters used by RQ_SRC_PWCONST / RQ_SRC_REALDATA runs */
    int32_t ctrl_n_arr;
    const double* ctrl_a;             /* host: change_times or event_times               */
    const double* ctrl_b;             /* host: rates                                     */
} rq_graph_desc;

typedef struct rq_graph* rq_graph_t;

/* status bits written per replica into rq_outputs.status */
#define RQ_ST_ROWS_OVERFLOW 1    /* metric-row / event-log capacity exceeded: rerun with larger cap_scale */
#define RQ_ST_STREAM_OVERFLOW 2  /* a source's arrival stream exceeded its capacity: rerun      */
/* A replica flagged with either overflow bit ran TRUNCATED: its metrics and counts cover
   only the events that fit and are not the reference's.  Every other replica of the batch
   is exact.  The library never reruns by itself: the Python Graph.run(check=True) reruns
   the batch with doubled cap_scale (and remembers the scale for the graph's later runs);
   check=False hands the flagged rows back as they are, for the caller to mask or rerun. */
#define RQ_ST_TIE 4              /* events at equal times shared a pivot row.  Exact (pivot cells
                                    averaged like pandas) in the sequential sweep -- sweep_mode 2,
                                    a multigraph, repeated graph-level RealData times; the fast
                                    tiled sweep keeps the last row, so for a replica flagged
                                    here avg-rank / r^2 may differ: rerun it with sweep_mode 2
                                    (alone: rep_idx; Graph.run(check=True) does) */
#define RQ_ST_EMPTY 8            /* no event reached any sink: the reference's df is empty      */
#define RQ_ST_UNORDERED 16       /* a sequential run over > 2048 sources (merged streams) met more
                                    than 2048 arrivals at ONE time (replayed data only): their
                                    order is not the reference's, the replica is not played    */

#define RQ_RUN_EVENT_LOG 1       /* also write the (t, source) event log (for get_dataframe)    */

typedef struct rq_batch_desc {
    int32_t ctrl_kind;           /* RQ_SRC_OPT / OPTPW / POISSON2 / PWCONST / REALDATA / NONE   */
    int32_t n_grid;              /* grid points                                                  */
    const double* q;             /* host [n_grid] (OPT)                                          */
    const double* s;             /* host [n_grid * n_followers], sorted-follower order (OPT)     */
    int64_t n_rep;               /* replicas per grid point; replica id i = g * n_rep + r        */
    const uint32_t* ctrl_seed;   /* device [n_grid*n_rep] or NULL: ctrl_seed0 + k(i)             */
    uint32_t ctrl_seed0;
    int32_t randomize_world;     /* 1: world seeds = u_i + 99*idx (randomize_other_sources,      */
                                 /*    opt_model.py:795-804); 0: the graph's fixed seeds         */
    const uint32_t* world_seed;  /* device [n_grid*n_rep] u_i, or NULL: world_seed0 + k(i)       */
    uint32_t world_seed0;
    int64_t seed_mod;            /* k(i) = i % seed_mod if > 0 else i; seed_mod = n_rep gives    */
                                 /* every grid point the same seeds (calc_q_capacity_iter)       */
    const double* ctrl_rate;     /* device [n_grid*n_rep] Poisson2 rate (RQ_SRC_POISSON2)        */
    double ctrl_rate_max;        /* host: max of ctrl_rate, sizes the stream capacity            */
    const int32_t* Ks;           /* host [nK], nK <= RQ_MAX_K                                     */
    int32_t nK;
    int64_t max_events;          /* run_dynamic(max_events); < 0 = unbounded                     */
    int32_t flags;               /* RQ_RUN_EVENT_LOG                                              */
    double cap_scale;            /* >= 1: multiplies every auto-sized capacity                   */
    int64_t chunk;               /* replicas per launch (0 = library default: the batch in an   */
                                 /* even number of chunks of <= 131072, pipelined on two streams */
                                 /* within the workspace budget, ws_budget below)               */
    int64_t replica0;            /* this call runs global replicas [replica0, replica0+n_local):  */
    int64_t n_local;             /* a shard of the grid (0 = all n_grid*n_rep); outputs are      */
                                 /* indexed locally, seeds and grid point use the global id     */
    int32_t sweep_mode;          /* 0 auto: a fast tiled sweep unless the run needs the exact
                                    sequential one (a multigraph; the graph's own RealData
                                    times repeat a time); max_events cuts the fast sweeps'
                                    tiles, per-replica RealData streams play on them (a replica
                                    meeting equal times is flagged RQ_ST_TIE); the fast sweeps
                                    write the event log themselves.
                                    The fast sweeps play MERGED streams: rq_gen_classes writes
                                    every source's arrivals, rq_merge_streams merges them into
                                    one (t, stream) sequence per replica, and the sweep plays it
                                    in tiles of 64 entries (the fused sweep for <= 64 sources,
                                    the general sweep above);
                                    1 fast whenever max_events allows; 2 force the sequential
                                    sweep; 3 as 0 but never a K=1 sink-bit variant (per-sink
                                    ranks); 4 / 5 as 0 / 1 on the general sweep instead of the
                                    fused one; 6 as 4 with the general sweep merging the
                                    per-source streams itself (register windows, the round-2
                                    kernel); 7 as 0 with the fused sweep generating its arrivals
                                    in-kernel (LDS rings, the round-2 kernel).  Every variant
                                    gives the same bits; 6 and 7 are kept for A/B checks      */
    /* RQ_SRC_OPTPW (create_manager_with_significance, opt_model.py:850-884): the follower
       significance s_pw[g][f][k] over n_seg equal segments of time_period, rows in the
       order of rq_graph_followers (sorted follower ids), q from q[g] */
    int32_t n_seg;
    double period;
    const double* s_pw;          /* host [n_grid][n_followers][n_seg]                            */
    /* Per-replica times of RealData sources -- the static broadcasters a user registers
       with SimOpts.registerSource (opt_model.py:768-771): the host runs their
       initialize() / get_all_times() (:336-338, :391-394) once per replica (seeded as
       randomize_other_sources gives them) and hands the times over here.  Source k is the
       graph's RealData source rd_src_id[k] (declared with no times); replica i (global id)
       plays rd_times[rd_off[i * n_rd + k] .. rd_off[i * n_rd + k + 1]), sorted and within
       [start_time, end_time].  n_rd = 0: every RealData source plays its graph times. */
    int32_t n_rd;                /* <= RQ_MAX_RD                                                 */
    const int64_t* rd_src_id;    /* host [n_rd]                                                  */
    const int64_t* rd_cap;       /* host [n_rd]: the most times any replica gives source k       */
    const double* rd_times;      /* device                                                       */
    const int64_t* rd_off;       /* device [n_grid * n_rep * n_rd + 1]                           */
    /* Per-grid-point replica window (ABI v4): this call's replica space is the
       n_grid x rep_cnt grid of global ids i = g * n_rep + rep_lo + rr, rr < rep_cnt,
       flattened as g * rep_cnt + rr; replica0 / n_local then select a contiguous part
       of THAT space and outputs are indexed by it.  A multi-GPU shard that takes the
       same replica window of every grid point sees every grid point (every q), so
       shards cost the same however the work per replica varies with q.
       rep_cnt = 0: the whole grid (rep_lo = 0, rep_cnt = n_rep). */
    int64_t rep_lo;
    int64_t rep_cnt;
    /* Device-memory budget of the workspace (ABI v5), bytes.  With the library's chunking
       (chunk = 0) the plan takes smaller chunks (an even count when pipelined) until the
       buffer sets in flight fit it; RQ_ENOMEM when one replica does not.  0: the library's
       default -- rq_workspace_size / rq_plan_info / rq_event_capacity take 0.9 x the
       device's free memory (hipMemGetInfo), rq_run_batch the workspace_bytes it is handed
       (so a workspace sized by rq_workspace_size always fits; the chunking, never the
       results, may differ).  A caller that frees or reuses memory of its own (a caching
       allocator) passes its reclaimable total here so both calls plan alike.  The
       environment variable RQ_WS_BUDGET_GB caps either. */
    int64_t ws_budget;
    /* Replica list (ABI v6): host [n_local] global ids (i = g * n_rep + r, each in
       [0, n_grid * n_rep)); the call runs exactly these replicas, output k = replica
       rep_idx[k] -- seeds, grid point and per-replica inputs (ctrl_seed, world_seed,
       ctrl_rate, rd_*) come from the global id as in the full batch, so a replica gives
       the same bits alone as inside its batch.  Requires replica0 = 0, rep_cnt = 0 and
       n_local > 0.  The caller reruns only a batch's flagged replicas with it (an
       RQ_ST_*_OVERFLOW replica at a larger cap_scale, an RQ_ST_TIE one on the exact
       sequential sweep, sweep_mode 2).  NULL: the replica space above. */
    const int64_t* rep_idx;
} rq_batch_desc;
#define RQ_MAX_RD 64

typedef struct rq_outputs {
    double* metrics;   /* device [R][nK + 2]: top_K..., avg_rank, r_2  (R = n_local or n_grid*rep_cnt) */
    int64_t* counts;   /* device [R][4]: num_events (own posts that reached a sink = the   */
                       /* reference 'capacity'), world_events, n_events (all), pivot rows   */
    int32_t* status;   /* device [R]: RQ_ST_* bits                                            */
    double* ev_t;      /* device [R][ev_cap] event times   (RQ_RUN_EVENT_LOG)                */
    int32_t* ev_src;   /* device [R][ev_cap] source index  (rq_graph_source_ids order)       */
    int64_t ev_cap;
} rq_outputs;

int rq_abi_version(void);
const char* rq_strerror(int code);

int rq_graph_build(const rq_graph_desc* desc, rq_graph_t* out);
int rq_graph_free(rq_graph_t g);
/* info[0] n_streams, [1] n_sinks, [2] n_followers, [3] n_edges, [4] ctrl stream index or -1 */
int rq_graph_info(rq_graph_t g, int64_t* info);
/* src_id of every stream index (the ev_src values); ids[n_streams], host */
int rq_graph_source_ids(rq_graph_t g, int64_t* ids);
/* sink ids in follower order (the order of rq_batch_desc.s), host */
int rq_graph_followers(rq_graph_t g, int64_t* ids);

/* bytes of device workspace rq_run_batch needs for this graph/batch */
int rq_workspace_size(rq_graph_t g, const rq_batch_desc* b, size_t* bytes);
/* suggested per-replica event-log capacity for RQ_RUN_EVENT_LOG */
int rq_event_capacity(rq_graph_t g, const rq_batch_desc* b, int64_t* cap);
/* how rq_run_batch will run this batch (diagnostics / occupancy reporting):
 * info[0] sweep variant (0 fast tiled, 1 sequential exact, 2 fast tiled on K=1 sink
 * bitsets, 3 fast tiled on K=1 per-wave LDS sink bits, 4 sequential exact with the
 * per-sink state in global memory; +10 fused), [1] sources per lane,
 * [2] arrival-ring depth W, [3] waves per block, [4] blocks per CU (runtime occupancy,
 * 0 without a device), [5] sink columns in LDS (1) or global (0), [6] dynamic LDS
 * bytes per block, [7] replicas per chunk */
int rq_plan_info(rq_graph_t g, const rq_batch_desc* b, int64_t* info);
/* the first n entries of the same list, which continues: [8] the sweep integrates each
 * replica's rows itself and the chunk launches no scan kernel (1; the merged fused sweep
 * without event log or max_events, RQ_SWEEP_SCAN=0 in the environment turns it off) or the
 * scan kernel runs after the sweep (0); [9] the merged fused sweep on K=1 sink bitsets
 * counts a tile's top-1 sets with its events blocked four to a lane (1; graphs of at least
 * 385 sinks, RQ_PHASEC_BLK=0 in the environment turns it off) or one event per lane (0);
 * [10] the sweep of [8] keeps a replica's pivot rows as 16-byte records (1; one K, at most
 * 65535 sinks and sinks x merged entries per replica below 2^32, RQ_ROWS_PACKED=0 in the
 * environment turns it off) or in four arrays (0).
 * Entries past the last defined one are not written. */
int rq_plan_info_n(rq_graph_t g, const rq_batch_desc* b, int64_t* info, int n);

int rq_run_batch(rq_graph_t g, const rq_batch_desc* b, const rq_outputs* out,
                 void* workspace, size_t workspace_bytes, void* hip_stream);

/* Metrics of dataframes in the reference's row layout (State.get_dataframe,
 * opt_model.py:85-97): one row per (event, sink) in df order, 't' non-decreasing
 * within a dataframe, sink ids RAW (any int64; the pivot columns -- the sorted
 * unique sink ids of each dataframe -- are built on the device).  Replaces
 *   utils.time_in_top_k(df, K, src_id, end_time)      utils.py:84-98
 *   utils.average_rank(df, src_id, end_time)           utils.py:101-114
 *   utils.int_r_2(df, sim_opts)                        utils.py:117-121
 *   utils.num_tweets_of(df, src_id) (+ world events)   utils.py:170-176, opt_runs.py:41-48
 * with the reference's arithmetic bit for bit (rank_of_src_in_df utils.py:38-56:
 * per-sink rank scan, pivot mean of duplicate (t, sink) rows, ffill; numpy's
 * pairwise sums).
 *   t, src, sink, event_id : device [n_rows] (event_id may be NULL)
 *   out                    : device [n_df][nK + 2]  top_K..., avg_rank, r_2 (NaN on error)
 *   counts                 : device [n_df][4]       num_tweets_of(src_id), world events
 *                            (-1 without event ids or if event_id decreases), pivot rows
 *                            (0: empty df; RQ_EUNSORTED: 't' decreases; RQ_EOVERFLOW: the df
 *                            needs the RQ_REPLAY_LARGE workspace; RQ_EINVAL: its df_off range
 *                            is malformed -- negative, decreasing, past n_rows or >= 2^31 rows),
 *                            unique sinks
 * Workspace: rq_replay_workspace_size; the small one serves dataframes with <= 3071
 * unique sinks (the per-sink state lives in LDS), RQ_REPLAY_LARGE any width.
 * RQ_REPLAY_CHUNKED adds room (~32 B per row + 192 KB per dataframe) for spreading ONE
 * long dataframe over many workgroups (chunks of 4096 rows; <= 4096 unique sinks), which
 * the call uses for up to 64 dataframes averaging >= 8192 rows (a batch of many
 * dataframes runs one workgroup per dataframe).
 * Per dataframe: < 2^31 rows. */
#define RQ_REPLAY_LARGE 1
#define RQ_REPLAY_CHUNKED 2
int rq_replay_workspace_size(int64_t n_rows, int64_t n_df, int32_t nK, int32_t flags, size_t* bytes);
int rq_metrics_replay(const double* t, const int64_t* src, const int64_t* sink,
                      const int64_t* event_id, int64_t n_rows, int64_t src_id, double end_time,
                      const int32_t* Ks, int32_t nK, double* out, int64_t* counts,
                      void* workspace, size_t workspace_bytes, void* hip_stream);
/* Many dataframes at once (the replicas of a batch, the reference's loop of
 * utils calls over opt_runs worker outputs): dataframe d owns rows
 * [df_off[d], df_off[d + 1]) of the concatenated columns; df_off device [n_df + 1],
 * n_rows = df_off[n_df]. */
int rq_metrics_replay_batch(const double* t, const int64_t* src, const int64_t* sink,
                            const int64_t* event_id, const int64_t* df_off, int64_t n_df,
                            int64_t n_rows, int64_t src_id, double end_time, const int32_t* Ks,
                            int32_t nK, double* out, int64_t* counts, void* workspace,
                            size_t workspace_bytes, void* hip_stream);
/* The same on dataframes in ANY row order, as the reference's functions take them
 * (utils.py:41: the is_sorted assertion is commented out): a concat of two runs, a
 * shuffle, re-appended rows.  Ranks are taken per sink in DATAFRAME order, the pivot is
 * on the sorted unique t with the mean of duplicate (t, sink) rows, and the two event
 * counts are distinct-id counts whatever the order of the ids -- sorting the rows by t
 * first gives other numbers.  Arguments, outputs and per-dataframe statuses are those of
 * rq_metrics_replay_batch (df_off NULL: one dataframe of n_rows rows), except that a
 * dataframe whose 't' decreases is evaluated instead of flagged RQ_EUNSORTED, with any
 * number of unique sinks; its event counts do not need increasing ids.  A dataframe in
 * time order takes the tiers of rq_metrics_replay_batch for `flags` and returns its bits.
 * Still RQ_EUNSORTED (NaN metrics): a dataframe whose 't' decreases AND holds a NaN (the
 * reference drops such rows in its pivot).
 * Workspace: rq_replay_unsorted_workspace_size = the replay workspace for `flags`
 * followed by the sort area (64 B per row).  One workgroup sorts one unsorted dataframe.
 * No ABI version change: detect the entries by symbol. */
int rq_replay_unsorted_workspace_size(int64_t n_rows, int64_t n_df, int32_t nK, int32_t flags, size_t* bytes);
int rq_metrics_replay_unsorted(const double* t, const int64_t* src, const int64_t* sink,
                               const int64_t* event_id, const int64_t* df_off /* NULL: one df */,
                               int64_t n_df, int64_t n_rows, int64_t src_id, double end_time,
                               const int32_t* Ks, int32_t nK, double* out, int64_t* counts,
                               void* workspace, size_t workspace_bytes, void* hip_stream);

/* Offline oracle (utils.oracle_ranking) for n_inst single-follower walls at once.
 * Instance i: n_i wall events, w_i[0..n_i+2) = np.diff([0, 0, event_times..., end_time])
 * (utils.py:207), q_i, s_i.  Device arrays: w (instances concatenated), w_off[n_inst+1]
 * (prefix of n_i + 2), q[n_inst], s[n_inst], out_off[n_inst+1] (prefix of n_i + 1).
 * Outputs (device): cost[i] = J[0, 0]; events / ranks [out_off[i] .. + n_i + 1) = the
 * oracle_df 'events' and 'ranks' columns.  n_max >= every n_i (<= 1e6, the reference's
 * own limit); workspace: rq_oracle_workspace_size (n_inst (n_max+1)^2 / 8 bytes of
 * decision bits). */
int rq_oracle_workspace_size(int32_t n_inst, int64_t n_max, size_t* bytes);
int rq_oracle_dp(const double* w, const int64_t* w_off, const double* q, const double* s,
                 int32_t n_inst, int64_t n_max, double* cost, int32_t* events, int32_t* ranks,
                 const int64_t* out_off, void* workspace, size_t workspace_bytes, void* hip_stream);

/* rank_of_src_in_df: table[n_t][n_cols] (device) of the rank of src_id in every sink's
 * feed at every unique t (index[n_t], device); cells = mean of the (t, sink) ranks, then
 * forward-filled per column when fill != 0 (NaN before a sink's first row / without fill).
 * Rows in df order, t non-decreasing; n_t = number of unique t.  err (device int32[1]):
 * 0 ok, bit 0 t not sorted, bit 1 n_t wrong. */
int rq_rank_table(const double* t, const int64_t* src, const int32_t* sink_col, int64_t n_rows,
                  int32_t n_cols, int64_t src_id, int32_t fill, int64_t n_t, double* table,
                  double* index, int32_t* err, void* hip_stream);

/* u_int_opt from a filled rank table: sum_k (sum_f table[k, fcol[f]] * wts[f]) * dt_k with
 * dt_k = index[k+1] - index[k] (end_time - index[n_t-1] last), numpy pairwise sum.
 * wts = sqrt(s / q) per follower (device), fcol their table columns (device).
 * out: device double[1]; workspace >= n_t * 8 bytes. */
int rq_u_int(const double* table, const double* index, int64_t n_t, int32_t n_cols,
             const int32_t* fcol, const double* wts, int32_t n_f, double end_time, double* out,
             void* workspace, size_t workspace_bytes, void* hip_stream);

/* Dataframe rows of a batch's event logs (State.get_dataframe, opt_model.py:85-97):
 * one row per (event, sink of an edge of the event's source), event order then
 * edge-list order.  ev_t / ev_src / counts are rq_run_batch's outputs (RQ_RUN_EVENT_LOG,
 * counts[i][2] = events of replica i), ev_cap their row stride.
 * rq_log_rows writes row_off[n_rep + 1] (device): replica i owns rows
 * [row_off[i], row_off[i+1]).  rq_log_expand then fills the five reference columns
 * (device, row_off[n_rep] rows each): event_id (100 + event index), time_delta, src_id,
 * t, sink_id.  time_delta follows the reference's accumulated State.time
 * (opt_model.py:68, :304): time_delta_k = t_k - time_{k-1}, time_k = time_{k-1} +
 * time_delta_k, time_{-1} = start_time -- which differs from t_k - t_{k-1} in the last
 * bit wherever the running sum has rounded. */
int rq_log_rows(rq_graph_t g, const int32_t* ev_src, const int64_t* counts, int64_t n_rep,
                int64_t ev_cap, int64_t* row_off, void* hip_stream);
int rq_log_expand(rq_graph_t g, const double* ev_t, const int32_t* ev_src, const int64_t* counts,
                  int64_t n_rep, int64_t ev_cap, const int64_t* row_off, int64_t* event_id,
                  double* time_delta, int64_t* src_id, double* t, int64_t* sink_id,
                  void* hip_stream);

/* Time-resolved metrics of a batch's event logs: the integrals rq_outputs.metrics holds
 * over the whole horizon, split over n_bins time bins [edges[b], edges[b+1]), straight
 * from the compact log (no dataframe rows are written).  ev_t / ev_src / counts are
 * rq_run_batch's outputs (RQ_RUN_EVENT_LOG) or any arrays in that layout, ev_cap their row
 * stride; replica i plays its first min(counts[i][2], ev_cap) events and reads nothing
 * past them.
 *   Events play in log order.  An event of stream j at t gives every sink x of j's edges
 * one row: rank_x = 0 if j is the controlled stream, else rank_x + 1 (1 for a sink without
 * a row so far) -- rank_of_src_in_df's steps_to, utils.py:43-46.  The pivot row at t is
 * nvalid (sinks with a row so far), sumR (the sum of their ranks) and c_K (those with
 * rank <= K-1); it holds until the next event that has an edge, the last one until the
 * graph's end_time.  With S = the sinks seen by the end of the replica (the df's pivot
 * columns), the integrands are c_K / S, m = sumR / nvalid and m^2, and
 *   metrics[i][b][.] = sum over rows of f_row * |[t_row, t_next) n [edges[b], edges[b+1])|
 * in the field order of rq_outputs.metrics (top_K..., avg_rank, r_2).  Time before the
 * first row contributes nothing, a bin no row overlaps is exactly 0.0, the bins need not
 * cover the horizon; over bins that do, the fields sum to rq_outputs.metrics up to
 * rounding (the order of summation differs: <= (rows + 8) ulp).
 *   posts[i][b] = events with at least one edge and edges[b] <= t < edges[b+1]: [0] the
 * controlled stream's, [1] every other stream's (over covering bins they sum to
 * counts[i][0] and counts[i][1]).  wall_posts[i][x][b] (optional) = rows of sink x from
 * the other streams under the same bin rule; x indexes the graph's sinks in ascending
 * sink-id order (the pivot's column order).
 *   status[i]: 0; RQ_ST_TIE when some sink got two rows at one t (pandas' fractional
 * pivot mean: not computed, the replica's metrics are NaN; equal times on disjoint sinks
 * are exact and not flagged); RQ_ST_EMPTY when no event had an edge (metrics NaN).  posts
 * and wall_posts of a flagged replica are valid, and no replica's output depends on its
 * neighbours or on the launch: one wavefront plays a replica and writes each of its
 * output elements once (wall_posts included: no zeroing pass, no atomics).
 *   edges: device [n_bins + 1], strictly increasing and finite (the caller's contract; a
 * bin with edges[b+1] <= edges[b] is empty, and nothing is accessed out of bounds
 * whatever edges holds).  Ks: host, 1 <= nK <= RQ_MAX_K, K >= 1.  Enqueues on hip_stream
 * only: no allocation, no synchronisation, no workspace.
 *   RQ_EUNSUPPORTED: a graph with duplicate edges (one sink, several rows per event), or
 * with more than RQ_TIMELINE_MAX_SINKS sinks (the per-sink state -- 8 bytes, 12 with
 * wall_posts -- lives in one workgroup's LDS).
 *   Added without an ABI version change (RQ_ABI_VERSION stays 6: no existing layout or
 * entry changed); a caller detects the function by its symbol. */
#define RQ_TIMELINE_MAX_SINKS 12288
int rq_log_timeline(rq_graph_t g, const double* ev_t, const int32_t* ev_src,
                    const int64_t* counts, int64_t n_rep, int64_t ev_cap,
                    const double* edges, int32_t n_bins,      /* device [n_bins + 1] */
                    const int32_t* Ks, int32_t nK,            /* host, 1 <= nK <= 4, K >= 1 */
                    double* metrics,      /* device [n_rep][n_bins][nK + 2] */
                    int64_t* posts,       /* device [n_rep][n_bins][2]: own, other */
                    int32_t* wall_posts,  /* device [n_rep][n_sinks][n_bins] or NULL */
                    int32_t* status,      /* device [n_rep] */
                    void* hip_stream);

/* Per-follower metrics of a batch's event logs: the other axis of rank_of_src_in_df's
 * pivot table (utils.py:38-56) -- one value per sink column where rq_log_timeline gives one
 * per time bin -- and int_r_2_true (utils.py:84-128 are the integrals over that table).
 * Logs, counts and ev_cap as for rq_log_timeline; the rank rule is the same.  Sink x (the
 * graph's sinks in ascending sink-id order) holds rank_x from each of its rows to its next
 * row, the last rank until the graph's end_time; over that seen span
 *   vals[i][x][.] = int I(rank_x <= K-1) dt for every K, int rank_x dt, int rank_x^2 dt,
 * each summed sequentially in time order from 0.0 as acc = acc + f(rank) * (t_next - t_row)
 * with every product rounded (no contraction), an interval of non-positive length adding
 * nothing: a host loop in the same order gives the same bits.  0.0 for a sink without a
 * row.  first_t[i][x] = the time of x's first row (NaN without one); rows[i][x] (optional)
 * = x's rows from the controlled stream and from every other stream.
 *   r2_true[i] = int_r_2_true: with nvalid the sinks seen so far and sumR2 the exact integer
 * sum of their rank^2 after the last event of a time t_row, summed over the distinct times
 * in order as acc = acc + ((double)sumR2 / (double)nvalid) * (t_next - t_row), the last
 * row until end_time.
 *   status[i]: 0; RQ_ST_TIE when some sink got two rows at one t (vals and r2_true NaN;
 * equal times on disjoint sinks are exact and not flagged); RQ_ST_EMPTY when no event had an
 * edge (vals and r2_true NaN).  first_t and rows of a flagged replica are valid.  An event
 * with a stream index outside the graph gives no row; counts[i][2] is clamped to
 * [0, ev_cap].  One wavefront plays a replica and writes each of its output elements once
 * (no zeroing pass, no atomics): no replica's bits depend on its neighbours or the launch.
 *   Ks: host, 1 <= nK <= RQ_MAX_K, K >= 1; ev_cap <= 2^24 (rank^2 < 2^48, sumR2 in int64),
 * else RQ_EINVAL.  Enqueues on hip_stream only: no allocation, no synchronisation, no
 * workspace.
 *   RQ_EUNSUPPORTED: a graph with duplicate edges, or with more sinks than
 * rq_log_followers_max_sinks(nK, rows != NULL): the per-sink state -- 12 + 8 (nK + 2) bytes,
 * 8 more with rows -- lives in one workgroup's 160 KiB of LDS (4551 sinks at nK = 1).
 *   Added without an ABI version change (RQ_ABI_VERSION stays 6); a caller detects the
 * functions by their symbols. */
int rq_log_followers(rq_graph_t g, const double* ev_t, const int32_t* ev_src,
                     const int64_t* counts, int64_t n_rep, int64_t ev_cap,
                     const int32_t* Ks, int32_t nK,  /* host, 1 <= nK <= 4, K >= 1 */
                     double* vals,         /* device [n_rep][n_sinks][nK + 2] */
                     double* first_t,      /* device [n_rep][n_sinks] */
                     int32_t* rows,        /* device [n_rep][n_sinks][2]: own, wall; or NULL */
                     double* r2_true,      /* device [n_rep] */
                     int32_t* status,      /* device [n_rep] */
                     void* hip_stream);
int32_t rq_log_followers_max_sinks(int32_t nK, int32_t with_rows);   /* 0 for a bad nK */

/* rq_log_followers past its sink limit: the same outputs -- shapes, layout, meaning and bits
 * -- for a graph of 1 <= n_sinks <= RQ_FOLLOWERS_TILED_MAX_SINKS sinks.  The sink columns are
 * cut into tiles of rq_log_followers_tile_sinks() columns (tile i owns columns [i TS,
 * min((i + 1) TS, n_sinks)); a graph of at most TS sinks is one tile).  One wavefront per
 * (replica, tile) replays the replica's whole log against a CSR of the tile's edges and
 * keeps the state of its own sinks in LDS; a second kernel, one wavefront per replica with
 * every sink's rank in LDS (4 bytes a sink: 40,960 sinks fill one workgroup's 160 KiB),
 * gives r2_true and status and overwrites vals with NaN for a TIE / EMPTY replica.  Both
 * are enqueued in order on hip_stream.
 *   Exactness: a sink's sums see only that sink's rows, in time order from 0.0 under
 * rq_log_followers' rule, so vals, first_t and rows do not depend on the tiling; r2_true is
 * rq_log_followers' loop over the whole graph.  Every finite output equals
 * rq_log_followers' bit for bit where both entries run, NaN where it has NaN, integers
 * equal; no replica's output depends on its neighbours or on the launch.  Every element is
 * written once, but for vals of a TIE / EMPTY replica (the tile's value, then NaN, in
 * stream order).
 *   workspace: device, rq_log_followers_tiled_workspace bytes = one int32 flag per
 * (replica, tile), 4 n_rep ceil(n_sinks / TS) rounded up to 256; contents on entry do not
 * matter, no zeroing is needed.  Enqueues on hip_stream only: no allocation, no
 * synchronisation.
 *   RQ_EINVAL, before any HIP call: rq_log_followers' cases, a null workspace or one smaller
 * than the query's size, n_rep * tiles > INT32_MAX.  RQ_EUNSUPPORTED: a graph with
 * duplicate edges, or with more than RQ_FOLLOWERS_TILED_MAX_SINKS sinks -- above that
 * int_r_2_true would need the ranks of a replica outside LDS, which is not built.  A refused
 * call launches nothing.
 *   Added without an ABI version change (RQ_ABI_VERSION stays 6); a caller detects the
 * functions by their symbols. */
#define RQ_FOLLOWERS_TILED_MAX_SINKS 40960   /* the r2 pass: 4 B per sink in 160 KiB */
int32_t rq_log_followers_tile_sinks(void);   /* TS */
int rq_log_followers_tiled_workspace(rq_graph_t g, int64_t n_rep, size_t* bytes);
int rq_log_followers_tiled(rq_graph_t g, const double* ev_t, const int32_t* ev_src,
                           const int64_t* counts, int64_t n_rep, int64_t ev_cap,
                           const int32_t* Ks, int32_t nK,  /* host, 1 <= nK <= 4, K >= 1 */
                           double* vals,         /* device [n_rep][n_sinks][nK + 2] */
                           double* first_t,      /* device [n_rep][n_sinks] */
                           int32_t* rows,        /* device [n_rep][n_sinks][2]: own, wall; or NULL */
                           double* r2_true,      /* device [n_rep] */
                           int32_t* status,      /* device [n_rep] */
                           void* workspace, size_t workspace_bytes, void* hip_stream);

/* The rank distribution of a batch's event logs: the third axis of rank_of_src_in_df's
 * pivot table (utils.py:38-56), the rank value itself -- per time bin, how long the seen
 * sinks sat at rank 0, 1, 2, ...  utils.time_in_top_k (utils.py:84-98) is the sum of the
 * first K cells, so one call gives top_K for every K <= n_ranks (rq_log_timeline: at most
 * RQ_MAX_K per call) and the distribution avg_rank and r_2 are moments of.
 *   Logs, counts, ev_cap, the rank rule, the time-bin rule, RQ_ST_TIE / RQ_ST_EMPTY and the
 * clamping of counts[i][2] to [0, ev_cap] are rq_log_timeline's; an event whose stream
 * index is outside the graph gives no row.  After the last event at a time t_row, cnt_rho
 * is the number of seen sinks whose rank equals rho, for rho < n_ranks, and cnt_{n_ranks}
 * is the tail: the seen sinks at rank >= n_ranks; sum over rho of cnt_rho = nvalid.  The
 * row holds until the next event that has an edge, the last one until the graph's
 * end_time.  With S = the sinks seen by the end of the replica,
 *   hist[i][b][rho] = ( sum over pivot rows of
 *                       (double)cnt_rho * |[t_row, t_next) n [edges[b], edges[b+1])| ) / (double)S
 * each (b, rho) cell summed sequentially in time order from 0.0 as
 * acc = acc + (double)cnt * len with the product rounded on its own (no contraction), an
 * overlap of non-positive length adding nothing, and one division by S at the end: a host
 * loop in that order gives the same bits (adding or skipping a term whose cnt is 0 does
 * not change them).  Time before the first row contributes nothing and a bin no row
 * overlaps is exactly 0.0.  Over the rank cells hist sums to the share of int nvalid dt / S
 * that falls in the bin, and over rho < K to rq_log_timeline's top_K field, both up to
 * rounding (the order of summation differs).
 *   n_seen[i] = S.  max_rank[i] = the largest rank any row gave any sink (-1 for an EMPTY
 * replica): a caller picks n_ranks > max_rank for an empty tail.  Both are valid for a TIE
 * replica; hist is NaN for TIE and EMPTY.  No replica's output depends on its neighbours or
 * on the launch: one wavefront plays a replica and writes each of its output elements once
 * (no global atomics, no zeroing pass; the counts cnt are integers, so the order in which
 * an event's sinks update them does not matter).
 *   edges: device [n_bins + 1], strictly increasing and finite (the caller's contract, as
 * for rq_log_timeline).  Enqueues on hip_stream only: no allocation, no synchronisation, no
 * workspace; n_rep = 0 enqueues nothing.
 *   RQ_EINVAL, before any HIP call: a null pointer, n_rep < 0 (or > INT32_MAX), ev_cap < 0,
 * n_bins < 1, n_ranks outside 1..RQ_RANK_HIST_MAX_RANKS.  RQ_EUNSUPPORTED: a graph with
 * duplicate edges, or with more than RQ_TIMELINE_MAX_SINKS sinks (the per-sink state, 8
 * bytes, lives in one workgroup's LDS: 96 KiB at that limit, plus at most 1 KiB of counts).
 *   Added without an ABI version change (RQ_ABI_VERSION stays 6); a caller detects the
 * function by its symbol. */
#define RQ_RANK_HIST_MAX_RANKS 255
int rq_log_rank_hist(rq_graph_t g, const double* ev_t, const int32_t* ev_src,
                     const int64_t* counts, int64_t n_rep, int64_t ev_cap,
                     const double* edges, int32_t n_bins,   /* device [n_bins + 1] */
                     int32_t n_ranks,                       /* 1..RQ_RANK_HIST_MAX_RANKS */
                     double* hist,        /* device [n_rep][n_bins][n_ranks + 1] */
                     int32_t* n_seen,     /* device [n_rep]: S */
                     int32_t* max_rank,   /* device [n_rep] */
                     int32_t* status,     /* device [n_rep] */
                     void* hip_stream);

/* Whole-horizon metrics of a batch's event logs, exact on equal times: time_in_top_k,
 * average_rank and int_r_2 (utils.py:84-121) over rank_of_src_in_df's pivot table
 * (utils.py:38-56) and num_tweets_of's counts (utils.py:170-176), bit for bit what
 * rq_metrics_replay_batch gives on the logs' dataframe rows (rq_log_expand), without
 * writing a row.  Logs, counts[i][2] clamping, stream indices outside the graph, the rank
 * rule and Ks are rq_log_timeline's.
 *   A t-group is the maximal run of consecutive events with equal t.  Its pivot row is
 * made when some event of it has an edge.  The group's cell of a sink x it touches is
 * (double)(sum of the ranks of x's rows in the group) / (double)(their number) -- pandas'
 * pivot mean; an untouched sink keeps its cell (ffill), while its rank runs on from the
 * last rank.  The row holds nvalid (sinks with a cell), c_K (cells <= K-1) and rowsum: the
 * exact integer sum while every cell is integral, else numpy's pairwise sum over the
 * replica's pivot columns -- the S sinks that get a row anywhere in the replica, in
 * ascending sink id, a column without a cell yet counting 0.  (A graph sink the replica
 * never reaches is no column: a zero there would shift numpy's tree and the rounding.)
 *   metrics[i] = numpy's sums (8192-row chunks, pairwise inside) of ((double)c_K / S) * dt,
 * m * dt and (m * m) * dt over the rows, m = rowsum / (double)nvalid, dt to the next row,
 * the last to the graph's end_time; every product rounded.  out_counts[i] is the replay's
 * layout: [0] the controlled stream's events with an edge, [1] the other streams', [2]
 * pivot rows, [3] S.
 *   status[i]: 0; RQ_ST_TIE when some sink got two rows in one t-group (informational: the
 * values are exact, as in the sequential sweep); RQ_ST_EMPTY when no event had an edge
 * (metrics NaN, counts 0).  No replica's output depends on its neighbours or on the
 * launch; every output element is written once (no atomics on outputs, no zeroing pass).
 *   workspace: device, 8-byte aligned, at least rq_log_metrics_workspace's bytes: a block's
 * pivot rows before the same wave integrates them.  It grows with ev_cap and with n_rep up
 * to 4096 replicas.  Non-decreasing t is the caller's contract; nothing is accessed out of
 * bounds whatever the arrays hold.  Enqueues on hip_stream only.
 *   RQ_EINVAL: a null pointer, n_rep < 1 (or > INT32_MAX), ev_cap < 1, bad nK or K, a
 * workspace too small or misaligned.  RQ_EUNSUPPORTED, nothing launched (the workspace query
 * answers the same): ev_cap > 2^20 (a sink's rows in one t-group are counted in 24 bits and
 * their ranks summed in 40; rq_log_expand + rq_metrics_replay_batch take such logs), a graph with
 * duplicate edges, or with more than RQ_LOG_METRICS_MAX_SINKS sinks.  A sink's state is 16
 * bytes of the workgroup's 160 KiB LDS (rank, t-group tag, and the group's row count and
 * rank sum packed in 64 bits -- one 128-bit LDS read and write per row); beside it stand
 * 4,784 bytes of summation scratch and 6 bytes per 32 sinks of column index, which leaves
 * room for 9,825 sinks: the limit is 9,800.  (The pass that finds a replica's columns
 * keeps one bit per stream in the same LDS; a graph of more than ~1.2 million streams is
 * refused too.)
 *   Added without an ABI version change (RQ_ABI_VERSION stays 6); a caller detects the
 * functions by their symbols. */
#define RQ_LOG_METRICS_MAX_SINKS 9800
int rq_log_metrics_workspace(rq_graph_t g, int64_t n_rep, int64_t ev_cap, int32_t nK, size_t* bytes);
int rq_log_metrics(rq_graph_t g, const double* ev_t, const int32_t* ev_src,
                   const int64_t* counts, int64_t n_rep, int64_t ev_cap,
                   const int32_t* Ks, int32_t nK,   /* host, 1 <= nK <= 4, K >= 1 */
                   double* metrics,       /* device [n_rep][nK + 2]: top_K..., avg_rank, r_2 */
                   int64_t* out_counts,   /* device [n_rep][4] */
                   int32_t* status,       /* device [n_rep] */
                   void* workspace, size_t workspace_bytes, void* hip_stream);

/* rq_log_metrics for any source of the graph, several in one call: the reference's
 * time_in_top_k(df, K, src_id=c), average_rank(df, src_id=c) and int_r_2 for src_id = c
 * (utils.py:84-121 take any src_id), on the log's dataframe (scope RQ_LOG_OF_DF) or on
 * df[df.sink_id.isin(followers of c)] (scope RQ_LOG_OF_OWN: the feeds an Opt tracks its
 * rank on, opt_model.py:505).
 *   For the tracked source c = src_ids[k] the outputs at [i][k] -- metrics [nK + 2],
 * out_counts [4], status -- are rq_log_metrics' outputs for replica i with two changes:
 *   1. "the controlled stream" is read as "stream c";
 *   2. in scope RQ_LOG_OF_OWN the graph's edges are restricted to those whose sink is a
 *      follower of c, i.e. a sink of one of c's edges.  An event with no edge into c's
 *      followers then gives no row: it is not counted and makes no pivot row (inside a
 *      t-group whose other events reach them it adds nothing).  The pivot columns are the
 *      followers of c that get a row anywhere in the replica, and status is RQ_ST_EMPTY
 *      (metrics NaN, counts 0) when no event reaches them -- always for a c without edges.
 * Everything else is rq_log_metrics' word for word: t-groups; pandas' pivot mean on ties;
 * the exact integer rowsum, or numpy's pairwise sum over the replica's own columns in
 * ascending sink id; numpy's 8192-row chunked sums; out_counts = [c's events with a row,
 * the other streams' with a row, pivot rows, S]; RQ_ST_TIE as informational; the clamping
 * of counts[i][2]; stream indices outside the graph.  No replica's and no source's output
 * depends on its neighbours, on the order of src_ids or on the launch; every output element
 * is stored once.
 *   So: scope RQ_LOG_OF_DF with src_ids = { ctrl_src_id } equals rq_log_metrics bit for
 * bit; the values for c in scope DF equal rq_metrics_replay_batch(..., src_id = c, ...) on
 * the rq_log_expand rows, and in scope OWN on those rows with the rows of other sinks
 * removed.
 *   src_ids: host [n_src], any order, each a stream of the graph (rq_graph_source_ids; the
 * controlled one is allowed).  The tracked stream indices travel in the kernel's arguments:
 * no staging, no allocation; the call only enqueues on hip_stream.  workspace: as
 * rq_log_metrics', rq_log_metrics_of_workspace bytes (a block's pivot rows; it grows with
 * ev_cap and with n_rep * n_src up to 4096 blocks -- a block plays its (replica, source)
 * items one after the other).
 *   RQ_EINVAL, before any HIP call: a null pointer, n_src outside 1..RQ_LOG_OF_MAX_SRC, an
 * id that is no stream of the graph or is named twice, a scope other than the two, and
 * rq_log_metrics' own cases.  RQ_EUNSUPPORTED exactly where rq_log_metrics returns it
 * (duplicate edges, more than RQ_LOG_METRICS_MAX_SINKS sinks, ev_cap > 2^20); the workspace
 * query answers the same.  A refused call launches nothing.
 *   Added without an ABI version change (RQ_ABI_VERSION stays 6); a caller detects the
 * functions by their symbols. */
#define RQ_LOG_OF_DF  0   /* pivot columns: every sink the replica's log reaches (the df's) */
#define RQ_LOG_OF_OWN 1   /* pivot columns: the tracked source's own followers only */
#define RQ_LOG_OF_MAX_SRC 64
int rq_log_metrics_of_workspace(rq_graph_t g, int32_t n_src, int64_t n_rep, int64_t ev_cap,
                                int32_t nK, size_t* bytes);
int rq_log_metrics_of(rq_graph_t g, const int64_t* src_ids /* host [n_src] */, int32_t n_src,
                      int32_t scope, const double* ev_t, const int32_t* ev_src,
                      const int64_t* counts, int64_t n_rep, int64_t ev_cap,
                      const int32_t* Ks, int32_t nK,
                      double* metrics,      /* device [n_rep][n_src][nK + 2] */
                      int64_t* out_counts,  /* device [n_rep][n_src][4] */
                      int32_t* status,      /* device [n_rep][n_src] */
                      void* workspace, size_t workspace_bytes, void* hip_stream);

/* rq_log_metrics for graphs of up to RQ_LOG_METRICS_SLIM_MAX_SINKS sinks: the same
 * time_in_top_k / average_rank / int_r_2 over rank_of_src_in_df's pivot table (utils.py:84-121,
 * utils.py:38-56) and num_tweets_of's counts (utils.py:170-176), the same arguments, the same
 * outputs bit for bit, the same validation order and statuses.  Two things differ:
 *   1. a sink's state is 8 bytes of LDS, not 16: rank (i32), the tag of its last t-group + 1
 *      (21 bits) and one bit that says the group has several rows of this sink.  While a group
 *      has one row of a sink its row count is 1 and its rank sum is the rank, so nothing more
 *      is kept; the 64-bit (rank sum << 24 | row count) of a group with several rows lives in
 *      the workspace, one word per sink and block, written on the sink's second row in a
 *      t-group and read only where the bit is set.  Every quotient and comparison gets the
 *      operands rq_log_metrics gives it.  4,784 + 8 n + 6 ceil(n / 32) bytes fit the
 *      workgroup's 160 KiB up to n = 19,426: the limit is 19,400;
 *   2. rq_log_metrics_slim_workspace's bytes are rq_log_metrics_workspace's plus, per block,
 *      8 * n_sinks rounded up to 16.
 * RQ_EUNSUPPORTED, nothing launched, the workspace query answering the same: ev_cap > 2^20,
 * duplicate edges, more than RQ_LOG_METRICS_SLIM_MAX_SINKS sinks.  After an event with a tie
 * a block waits for its workspace stores before the next event.  rq_log_metrics and
 * rq_log_metrics_of stay as they are, their limit included.
 *   Added without an ABI version change (RQ_ABI_VERSION stays 6); a caller detects the
 * functions by their symbols. */
#define RQ_LOG_METRICS_SLIM_MAX_SINKS 19400
int rq_log_metrics_slim_workspace(rq_graph_t g, int64_t n_rep, int64_t ev_cap, int32_t nK, size_t* bytes);
int rq_log_metrics_slim(rq_graph_t g, const double* ev_t, const int32_t* ev_src,
                        const int64_t* counts, int64_t n_rep, int64_t ev_cap,
                        const int32_t* Ks, int32_t nK,   /* host, 1 <= nK <= 4, K >= 1 */
                        double* metrics,       /* device [n_rep][nK + 2]: top_K..., avg_rank, r_2 */
                        int64_t* out_counts,   /* device [n_rep][4] */
                        int32_t* status,       /* device [n_rep] */
                        void* workspace, size_t workspace_bytes, void* hip_stream);

/* rq_log_metrics_of on the 8-byte cells of rq_log_metrics_slim: time_in_top_k(df, K, src_id=c),
 * average_rank(df, src_id=c) and int_r_2 for any sources c (utils.py:84-121 take any src_id),
 * on the log's dataframe or on the rows of c's followers (opt_model.py:505).  Arguments,
 * outputs (bit for bit), validation order, statuses, the number of blocks and their shares of
 * the (replica, source) items are rq_log_metrics_of's; the sink limit and the workspace
 * (rq_log_metrics_of_workspace's bytes plus 8 * n_sinks rounded up to 16 per block) are
 * rq_log_metrics_slim's.  In scope RQ_LOG_OF_OWN the follower bits are built where the cells
 * will be, as there.
 *   Added without an ABI version change (RQ_ABI_VERSION stays 6); a caller detects the
 * functions by their symbols. */
int rq_log_metrics_of_slim_workspace(rq_graph_t g, int32_t n_src, int64_t n_rep, int64_t ev_cap,
                                     int32_t nK, size_t* bytes);
int rq_log_metrics_of_slim(rq_graph_t g, const int64_t* src_ids /* host [n_src] */, int32_t n_src,
                           int32_t scope, const double* ev_t, const int32_t* ev_src,
                           const int64_t* counts, int64_t n_rep, int64_t ev_cap,
                           const int32_t* Ks, int32_t nK,
                           double* metrics,      /* device [n_rep][n_src][nK + 2] */
                           int64_t* out_counts,  /* device [n_rep][n_src][4] */
                           int32_t* status,      /* device [n_rep][n_src] */
                           void* workspace, size_t workspace_bytes, void* hip_stream);

/* Competing RedQueen broadcasters (Opt among SimOpts.other_sources, opt_model.py:493-544,
 * :761): several Opts -- the PLAYERS -- post against each other and against an exogenous
 * world in one run_dynamic loop (opt_model.py:271-309).  The sources no Opt influences
 * (Poisson, Poisson2, Hawkes, PiecewiseConst, RealData, a static controlled source) are
 * played first by rq_run_batch with RQ_RUN_EVENT_LOG; rq_log_game plays the players against
 * that log and writes the completed log in the same layout, which every rq_log_* entry reads.
 *   g is the REPLAY graph: every player is an RQ_SRC_REALDATA source flagged
 * RQ_SRCF_DYNAMIC and declared with no times, or the controlled slot (else RQ_EINVAL).
 * players: host [n_players], any order, distinct src_ids; player c has q > 0 and s[n_s] >= 0
 * over its followers -- the distinct sinks of its edges in ascending sink id, n_s of them.
 *   Rates.  C[c][j] = sum over stream j's edges (j, x), x a follower of c, of
 * sqrt(s_c[x] / q_c), the terms added one by one from 0.0 in ascending sink id (a duplicated
 * edge adds its term again); C[c][c] = 0; inv[c][j] = 1.0 / C[c][j], 0 where C is 0.
 *   Play.  Every player's pending time T_c starts at the graph's start_time.  The pending
 * post (T, c) of the player with the least (T, src_id) plays before the next exogenous entry
 * (t, j) when T < t, or T == t and j is a static stream or src_id(c) < src_id(j)
 * (opt_model.py:279-290); a post with T > end_time is never played; when the exogenous log is
 * exhausted the players go on among themselves; play stops after max_events events (< 0:
 * unbounded).  When event number e (0-based in the output) of stream j plays at time t:
 * T_j = +inf if j is a player, and every other player c with inv[c][j] > 0 takes
 * x = rq_std_exponential(rq_uniform53(w0, w1)), w = Philox4x32-10 of counter
 * (lo32 e, hi32 e, 0, 0) under key (seeds[i][c], 0x52510006 | 0x100 if c is the controlled
 * source), and sets T_c = min(T_c, t + x * inv[c][j]), product and sum each rounded.
 *   seeds: device uint32 [n_rep][n_players], column c = players[c].  ev_t / ev_src / counts /
 * ev_cap: the exogenous logs, rq_run_batch's layout (replica i plays its first
 * min(counts[i][2], ev_cap) entries).  Outputs (device): out_t / out_src [n_rep][out_cap];
 * out_counts [n_rep][4] with rq_outputs.counts' meaning (field 3 is 0); player_posts
 * [n_rep][n_players] int64; status [n_rep]: RQ_ST_ROWS_OVERFLOW when an event was due with
 * out_cap events written (the out_cap events written are the run's first: rerun with more),
 * RQ_ST_EMPTY when no played event had an edge.  One wavefront plays a replica (lane c =
 * the player with the c-th smallest src_id): no replica's bits depend on its neighbours,
 * the launch or the batch.
 *   workspace: device, rq_log_game_workspace bytes (the transposed inverse table
 * [n_streams][n_players] and 4 bytes per stream); the call stages them through the graph's
 * pinned ring exactly as rq_run_batch stages its tables (see Conventions), and otherwise only
 * enqueues on hip_stream.  The table is read from LDS when rq_log_game_table_in_lds, else
 * from global memory (any graph size).
 *   RQ_EINVAL: a null pointer, n_rep < 1 (or > INT32_MAX), ev_cap < 0, out_cap < 1, a short
 * workspace, or a player that is no stream of the graph / not a replay stream / named twice /
 * with a duplicated follower edge / without followers / with n_s wrong / q <= 0 / an s < 0.
 * RQ_EUNSUPPORTED: more than RQ_GAME_MAX_PLAYERS players.  A refused call launches nothing.
 *   Added without an ABI version change (RQ_ABI_VERSION stays 6); a caller detects the
 * functions by their symbols. */
#define RQ_GAME_MAX_PLAYERS 64
typedef struct rq_game_player {
    int64_t src_id;
    double q;
    const double* s;   /* host [n_s], ascending follower sink id */
    int32_t n_s;
} rq_game_player;
int rq_log_game_workspace(rq_graph_t g, int32_t n_players, size_t* bytes);
int32_t rq_log_game_table_in_lds(rq_graph_t g, int32_t n_players);   /* 1 LDS, 0 global */
int rq_log_game(rq_graph_t g, const rq_game_player* players, int32_t n_players,
                const uint32_t* seeds,                        /* device [n_rep][n_players] */
                const double* ev_t, const int32_t* ev_src, const int64_t* counts,
                int64_t n_rep, int64_t ev_cap, int64_t max_events,
                double* out_t, int32_t* out_src, int64_t out_cap,
                int64_t* out_counts,                          /* device [n_rep][4] */
                int64_t* player_posts,                        /* device [n_rep][n_players] */
                int32_t* status,                              /* device [n_rep] */
                void* workspace, size_t workspace_bytes, void* hip_stream);

/* Per-kernel timing for benchmarks: rq_timing(1) starts recording HIP events
 * around every kernel this library launches (on the caller's stream);
 * rq_timing_read() waits for them and returns, per kernel class
 * [0 stream generation, 1 sweep, 2 scan, 3 replay, 4 merge], the summed milliseconds
 * and the number of launches, then clears the record.  rq_timing(0) stops. */
int rq_timing(int enable);
int rq_timing_read(double* ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* RQ_H */

// rq_internal.h -- kernel argument blocks shared by rq_kernels.hip and rq_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <tuple>

#include "../../include/rq.h"
#include "rq_host.h"   // the planner's constants, SweepInst and the three device queries
#include "rq_log_walk.h"

// global replica id of position s of a call's replica space (rq_batch_desc.rep_lo /
// rep_cnt): the n_grid x rep_cnt window of every grid point's n_rep replicas
__host__ __device__ __forceinline__ int64_t rq_global_replica(int64_t s, int64_t n_rep, int64_t rep_lo,
                                                               int64_t rep_cnt)
{
    return rep_cnt == n_rep ? s : (s / rep_cnt) * n_rep + rep_lo + s % rep_cnt;
}

struct GenArgs {
    int64_t n_chunk, chunk0, rep0;   // local replica = chunk0 + rl, space position = rep0 + local
    int64_t n_rep, rep_lo, rep_cnt;  // global id = rq_global_replica(rep0 + local, ...)
    const int64_t* rep_idx;          // rq_batch_desc.rep_idx (device copy): global id = rep_idx[local]
    int n_str, ctrl_idx, ctrl_stream_kind, randomize;
    int64_t seed_mod;
    const uint32_t* ctrl_seed;
    uint32_t ctrl_seed0;
    const uint32_t* world_seed;
    uint32_t world_seed0;
    const double* ctrl_rate;
    const int* kind;
    const int* orig_idx;
    const uint32_t* seed;
    const double *p0, *p1, *p2;
    const int *arr_off, *arr_n;
    const double *arr_a, *arr_b;
    const int64_t* st_off;
    const int* cap;
    int64_t capsum;
    double start, end;
    double* streams;
    int* slen;                       // [n_str][slen_stride]: lane-coalesced stores
    int64_t slen_stride;             // >= n_chunk (the chunk buffers' replica capacity)
    int32_t* status;
    // per-replica RealData times (rq_batch_desc.rd_*): stream j -> source k or -1
    const int* rd_k;
    int n_rd;
    const double* rd_times;
    const int64_t* rd_off;
    // rq_launch_gen only: the graph's streams by generator class (GraphTopo.gen_cls: H, P, G;
    // the controlled slot is not in it), cls_n streams each.  Null (RQ_GEN_SPLIT=0):
    // rq_gen_streams for every stream.
    const int* cls;
    int cls_n[3];
};

// global id of a call's local replica: the replica list (rq_batch_desc.rep_idx) or the
// replica space position rep0 + local
__host__ __device__ __forceinline__ int64_t rq_replica_of(const GenArgs& a, int64_t local)
{
    return a.rep_idx ? a.rep_idx[local] : rq_global_replica(a.rep0 + local, a.n_rep, a.rep_lo, a.rep_cnt);
}

struct SweepArgs {
    int64_t n_chunk, chunk0, n_rep, rep0;
    int wpb, n_str, n_sinks, n_sinks_pad, ctrl_idx, ctrl_kind, n_fol;
    int Ks[RQ_MAX_K];
    int64_t ctrl_src_id;
    int64_t seed_mod;
    const uint32_t* ctrl_seed;
    uint32_t ctrl_seed0;
    const int64_t* src_id;     // [n_str]
    const double* inv_c;       // [n_grid][n_str]
    const double* pw_c;        // OptPWSignificance: [n_grid][n_str][n_seg] (else null)
    const double* pw_max;      // [n_grid][n_str]
    int n_seg;
    double period;
    const int* csr_ptr;        // [n_str + 1]
    const int* csr_col;        // sink columns, edge-list order per source
    const int* outdeg_f;       // [n_str] edges into the controlled source's followers
    const int* cbf_g;          // [n_str] the controller posts first at an equal time (GT instances)
    const int* fol;            // [n_fol] follower columns
    const int64_t* st_off;
    int64_t capsum;
    const double* streams;
    const int* slen;           // [n_str][slen_stride]
    int64_t slen_stride;
    double start, end;
    int64_t max_events;
    int64_t cap_rows;
    double* rows_t;
    double* rows_sum;
    uint32_t* rows_valid;
    uint32_t* rows_cnt;
    int* sall;
    int64_t* counts;
    int32_t* status;
    double* ev_t;
    int32_t* ev_src;
    int64_t ev_cap;
    int n_csr;
    const uint32_t* masks;   // [n_str][nw] sink bitsets (BITS variant)
    int nw, mstride;         // words per bitset; LDS row stride in words (odd: bank spread)
    const uint32_t* fbits;   // follower set as a sink bitset [nwl] (BL variant)
    int nwl;                 // BL: words per per-wave T / V bitset = ceil(n_sinks / 32)
    size_t lds_fbits;        // BL: the follower bitset's place in the block's shared LDS
    size_t lds_skip;         // BL + MRG: per-wave stream stamps / first-lane table (0: no skipping)
    size_t lds_etab;         // fused sweep: rq_exp's table (64 x u64) in the block's shared LDS
    int dbg;                 // profiling: 1 skip phase C, 2 skip sink updates, 3 skip phase B
    unsigned long long* clk; // RQ_PHASE_CLOCK builds only: per-phase s_memtime sums [8]
    double tile_target;      // fused sweep: arrivals a tile aims at (the cut adapts to it)
    int fw_hmin;             // fused sweep: a ring showing fewer arrivals forces refill passes (1..H)
    size_t lds_invc;         // general sweep, one grid point: 1/c_j [n_str] in the block's shared LDS
    int invc_shared;         //   (else each wave loads its replica's grid point at the start of its wave region)
    int fw_thr;              // fused sweep: opportunistic refill passes while >= fw_thr rings are below W
    int fw_hfill;            // fused sweep: a forced refill run ends once every ring shows >= fw_hfill
    int* wq;                 // fused sweep: replica work queue (zeroed per launch; null = one replica per wave)
    double* metrics;         // SweepInst.scan: [R][nK + 2], written by the sweep's own scan (else unused)
    int col_in_lds, win;    // general sweep: CSR copied to LDS; arrival-ring depth
    size_t lds_col, lds_ptr, lds_odf, lds_cbf, lds_wave, lds_wave_stride, lds_rank_off, lds_win_off, lds_x_off, lds_mask,
        lds_total, lds_stage_off;
    GenArgs gen;             // fused sweep: arrival generation parameters
    // duplicate edges: stream j's CSR row is layers of distinct sinks, ending at
    // lay_end[lay_ptr[j] .. lay_ptr[j+1]) (null: one layer per row, a simple graph)
    const int* lay_ptr;
    const int* lay_end;
    // LOG sweep with the per-sink state in global memory (more sinks than LDS holds):
    // gs_slots wave slots of gs_stride bytes (rank int + gtag/gcnt/gsum per sink)
    char* gs;
    int64_t gs_stride;
    int gs_slots;
    // general fast sweep on merged streams (rq_merge_streams): replica rl's arrivals of
    // every source in play order, mrg_t / mrg_j [rl * mrg_stride + k], k < mrg_len[rl]
    const double* mrg_t;
    const uint16_t* mrg_j;
    const uint8_t* mrg_jh;     // > 65535 streams: bits 16-23 of each entry's stream (else null)
    const int* mrg_len;
    int64_t mrg_stride;        // entries per replica of mrg_t / mrg_j
    // longest-first play order of the chunk's replicas (rq_order_replicas over mrg_len):
    // the wave slots and the work queue take chunk replica order[q] for queue position q
    // (null: q itself).  Outputs stay indexed by replica, so no result bit depends on it.
    const int* order;
};

// rq_merge_streams: one block per replica merges its pre-generated per-source streams
// into the (t, stream) sequence the sweep plays -- time order, equal times in stream
// order, a source's equal times in stream order (the windowed sweep's stage rank)
struct MergeArgs {
    int64_t n_chunk, chunk0;
    int n_str;
    int64_t capsum;
    const int64_t* st_off;
    const double* streams;
    const int* slen;        // [n_str][slen_stride]
    int64_t slen_stride;
    double end;
    double* out_t;          // [C][mrg_stride]
    uint16_t* out_j;        // [C][mrg_stride] the stream (a group-local one at a two-level merge's first level)
    uint8_t* out_jh;        // > 65535 streams: bits 16-23 of the stream (else null)
    int* out_len;           // [C]
    int64_t mrg_stride;     // capacity per replica: past it the replica is flagged RQ_ST_STREAM_OVERFLOW
    int32_t* status;        // RQ_ST_TIE (strict_ties: RQ_ST_UNORDERED) when > RQ_MG_CAP arrivals share one time
    int strict_ties;        // the sequential sweep plays this sequence: no exact rerun behind it
    // two-level merge (> RQ_MG_B sources): the first level merges group g's streams
    // [g RQ_MG_B, (g + 1) RQ_MG_B) of replica rl (grid y = group) into out_* at
    // [(rl n_grp + g) mrg_stride]; the second level (sub-merge) takes those n_grp
    // sequences -- sub_t / sub_j / sub_len, sub_stride entries each -- as its streams
    const double* sub_t;
    const uint16_t* sub_j;
    const int* sub_len;
    int n_grp;
    int64_t sub_stride;
    // streams per first-level group: RQ_MG_B, or 64 (one-wave blocks) up to 64 groups of
    // them -- the second level then has more streams walking (a lane per group) per round
    int grp_sz;
    unsigned long long* clk;   // RQ_PHASE_CLOCK builds only: per-phase s_memtime sums [8]
};
// wall events per branch-free batch of the merged-stream K = 1 sink-bit sweep: C5 sweep
// per 4096 replicas on one stream (same box, round 5) 4: 139.0, 5: 136.1, 6: 135.0 ms;
// the pipelined 8192-replica step 382.6 / 372.0 / 374.5 ms (gpurun_out/abc5)
// merged-stream sweeps: a tile's rows are stored at the top of the next tile, ahead of
// its prefetch loads (RowStage::flush_pend); 0 = at the end of their own tile (A/B)
#ifndef RQ_MRG_DEFER
#define RQ_MRG_DEFER 1
#endif
#ifndef RQ_MRG_BLB
#define RQ_MRG_BLB 5
#endif

struct ScanArgs {
    int64_t n_chunk, chunk0;
    const int64_t* nrows;   // number of pivot rows of replica rl at nrows[(chunk0+rl)*nrows_stride]
    int64_t nrows_stride;
    const int* sall;        // sink columns S of replica rl (chunk-relative)
    int64_t row_stride;
    const double* rows_t;
    const double* rows_sum;
    const uint32_t* rows_valid;
    const uint32_t* rows_cnt;
    double end;
    double* metrics;
    int* wq;                // replica work queue (zeroed before the launch; null = one replica per wave)
};

// SweepInst (rq_host.h) names the sweep template instance a plan selects; the launches
// below and the occupancy queries (rq_sweep_blocks_per_cu / rq_fw_blocks_per_cu, declared
// there too) resolve it to the kernel in one place per kernel file.
using SweepKernel = void (*)(SweepArgs);

hipError_t rq_launch_gen(const GenArgs& a, hipStream_t s);
// hipErrorInvalidValue for a combination without an instance (bits with gt; fused: pw
// with merged streams, without uint16 columns or at W != 16)
hipError_t rq_launch_sweep(const SweepArgs& a, const SweepInst& i, hipStream_t s);
hipError_t rq_launch_scan(const ScanArgs& a, int nK, hipStream_t s);
hipError_t rq_launch_merge(const MergeArgs& a, hipStream_t s);
// > RQ_MG_B sources: level 1 over n_grp groups (a.n_str streams, grid C x n_grp), then
// the second level over the groups' sequences (a.sub_*, a.n_grp "streams")
hipError_t rq_launch_merge_groups(const MergeArgs& a, hipStream_t s);
hipError_t rq_launch_merge_sub(const MergeArgs& a, hipStream_t s);
// longest-first order of n <= 65536 replicas by len (descending; ties in any order)
hipError_t rq_launch_order(const int* len, int64_t n, int* order, hipStream_t s);
// the fused pair of rq_launch_sweep (SweepInst.fused); rows16_bytes: what the caller has at
// a.rows_t for the 16-byte row records of a SweepInst.pk instance
hipError_t rq_launch_sweep_fw(const SweepArgs& a, const SweepInst& i, hipStream_t s, size_t rows16_bytes = 0);

// Blocks per CU a kernel reaches at `threads` threads and `lds` bytes of dynamic LDS
// (the runtime's occupancy: VGPR, SGPR and LDS limits), cached per (kernel, threads,
// lds).  rq_run_batch may be called from several threads at once (rq.h), so the cache
// is mutex-guarded; 0 when the query fails (no device).
template <class K>
int rq_occupancy(K kernel, int threads, size_t lds)
{
    static std::mutex mu;
    static std::map<std::tuple<const void*, int, size_t>, int> cache;
    const auto key = std::make_tuple(reinterpret_cast<const void*>(kernel), threads, lds);
    std::lock_guard<std::mutex> lock(mu);
    const auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, threads, lds) != hipSuccess) nb = 0;
    cache.emplace(key, nb);
    return nb;
}

// ---- dataframe replay (rq_replay.hip) ----
// per-dataframe status, in the workspace
struct RpInfo {
    int64_t n_piv;            // pivot rows (unique t)
    int64_t n_own, n_world;   // distinct event ids of the source / of the others
    int32_t S;                // unique sink ids (pivot columns)
    int32_t flags;            // RP_*
};
#define RP_FALLBACK 1    // a duplicate (t, sink) pivot cell: the sequential replay owns the df
#define RP_UNSORTED 2    // 't' decreases
#define RP_GLOBAL 4      // more unique sinks than the LDS table: needs the global-table pass
#define RP_EIDBAD 8      // event_id decreases: the event counts are unknown
#define RP_BIG 16        // needs the large workspace (or exceeds it)
#define RP_EMPTYDF 32    // no rows
#define RP_BADOFF 64     // df_off[d] .. df_off[d + 1] is not a valid row range (< 2^31 rows)
#define RP_MID 256       // more unique sinks than the small LDS table: the full-table pass takes it
#define RP_SORTED 512    // the sort route (rq_replay_sort.hip) evaluated an unsorted df: its rows, dense
                         // columns and ranks stand in t order in the sort area (RpArgs::us_*)
#define RP_CSKIP 128     // chunked mode: the df is not chunkable (> RC_S sinks, the INT64_MIN id):
                         // the one-workgroup path (rq_rp_fast) takes it
enum { RP_PHASE_FAST = 0, RP_PHASE_GLOBAL = 1, RP_PHASE_KEYS = 2, RP_PHASE_SEQ = 3, RP_PHASE_SCAN = 4,
       RP_PHASE_CHUNK = 5, RP_PHASE_SMALL = 6, RP_PHASE_SEQ_GIVEN = 7 };
// chunked replay (one dataframe over many workgroups): rows per chunk, most unique sinks
// per dataframe, hash slots per dataframe
#define RC_L 4096
#define RC_S 4096
#define RC_HT 8192
struct RcCarry {     // one chunk's effect on one sink (rq_rc_sum)
    int n;           // rows of the sink in the chunk
    int after;       // rows after its last own row in the chunk (-1: no own row)
    double last_t;   // t of its last row in the chunk
};
struct RcState {     // a sink's state entering a chunk (rq_rc_scan)
    int r;           // rank of its last row (-1: no row yet, a NaN cell)
    int pad;
    double last_t;   // t of its last row
};

struct RpArgs {
    const double* t;
    const int64_t* src;
    const int64_t* sink;
    const int64_t* eid;       // may be null
    const int64_t* df_off;    // device [n_df + 1], or null: one dataframe of n_rows rows
    int64_t n_df, n_rows;
    int64_t src_id;
    double end;
    int Ks[RQ_MAX_K];
    int nK;
    RpInfo* info;             // [n_df]
    // pivot rows of dataframe d at rows [df_off[d], ...): dt, cell sum, #valid, #<=K-1
    double* rows_dt;
    double* rows_sum;
    uint32_t* rows_valid;
    uint32_t* rows_cnt;       // [row][nK]
    int64_t* keys;            // [n_rows]: sorted unique sink ids of fallback dataframes
    // large workspace only (null otherwise): per-df hash tables, slots [4 r0, 4 r1)
    uint64_t* gkeys;          // [4 n_rows]
    void* gstate;             // [4 n_rows] x 16 B
    double* metrics;          // [n_df][nK + 2]
    int64_t* counts;          // [n_df][4]
    // chunked mode (RP_PHASE_CHUNK; null otherwise): per df chunk prefix [n_df + 1], hash
    // tables [n_df][RC_HT], per chunk the group base, carries / entering states [chunk][RC_S]
    int chunked;
    int first_tier;         // 0: the small-table pass runs first (RP_PHASE_SMALL), 1: the full-table pass
    int64_t max_chunks;
    int64_t* cbase;
    uint64_t* ht_keys;
    int* ht_dense;
    int* gstart;              // [chunk] t-group starts in the chunk
    int64_t* gbase;           // [chunk] t-groups started before the chunk (within its df)
    RcCarry* carry;
    RcState* state;
    unsigned long long* clk;  // RQ_PHASE_CLOCK builds only: rq_rp_fast per-phase s_memtime sums [8]
    // sort route (rq_metrics_replay_unsorted; null otherwise).  us_scratch: RP_US_SCRATCH bytes per
    // row, dataframe d's at byte RP_US_SCRATCH * df_off[d]: the radix sort's key / payload
    // ping-pong and per-row column / rank, later the given-rank rq_rp_seq's per-sink state.
    // The rest [n_rows], dataframe d's rows in (t, dataframe index) order at df_off[d]:
    // t, dense column, rank, previous rank of the sink (-1: none), pivot row.
    char* us_scratch;
    double* us_t;
    int* us_col;
    int* us_rank;
    int* us_prev;
    int* us_g;
};
#define RP_US_SCRATCH 40
hipError_t rq_launch_rp(const RpArgs& a, int phase, hipStream_t s);
// the unsorted route for the dataframes rq_rp_fast flagged RP_UNSORTED (rq_replay_sort.hip)
hipError_t rq_launch_rp_sort(const RpArgs& a, hipStream_t s);

// ---- analysis kernels (rq_analysis.hip) ----
struct OracleArgs {
    const double* w;          // device, concatenated per instance: w[n_i + 2]
    const int64_t* w_off;     // device [n_inst + 1]
    const double* q;          // device [n_inst]
    const double* s;          // device [n_inst]
    int n_inst;
    int64_t n_max;
    double* cost;             // device [n_inst]
    int32_t* events;          // device, concatenated [n_i + 1]
    int32_t* ranks;           // device, concatenated [n_i + 1]
    const int64_t* out_off;   // device [n_inst + 1]
    uint64_t* bits;           // workspace [n_inst][bits_stride]
    int64_t bits_stride;
    double* gcol;             // workspace [n_inst][2][n_max + 2] (global-column mode)
};
hipError_t rq_launch_oracle_dp(const OracleArgs& a, bool lds, hipStream_t s);

struct RankTableArgs {
    const double* t;
    const int64_t* src;
    const int32_t* col;
    int64_t n_rows;
    int n_cols;
    int64_t src_id;
    int fill;
    int64_t n_t;
    double* table;            // [n_t][n_cols]
    double* index;            // [n_t]
    int32_t* err;             // [1]: 1 unsorted t, 2 n_t mismatch
};
hipError_t rq_launch_rank_table(const RankTableArgs& a, hipStream_t s);

struct UIntArgs {
    const double* table;
    const double* index;
    int64_t n_t;
    int n_cols;
    const int32_t* fcol;
    const double* wts;
    int n_f;
    double end;
    double* x;                // workspace [n_t]
    double* out;              // [1]
};
hipError_t rq_launch_u_int(const UIntArgs& a, hipStream_t s);

struct LogArgs {
    const double* ev_t;       // [n_rep][ev_cap]
    const int32_t* ev_src;    // [n_rep][ev_cap] stream indices
    const int64_t* counts;    // [n_rep][4], [2] = events
    int64_t n_rep, ev_cap;
    const int* csr_ptr;       // [n_str + 1]
    const int* csr_col;       // sink columns, edge-list order per stream
    int n_str;
    const int64_t* src_ids;   // [n_str]
    const int64_t* sink_ids;  // [n_sinks] sorted
    double start;
    int64_t* row_off;         // [n_rep + 1]
    int64_t* event_id;
    double* time_delta;
    int64_t* src_id;
    double* t;
    int64_t* sink_id;
};
hipError_t rq_launch_log_rows(const LogArgs& a, hipStream_t s);
hipError_t rq_launch_log_expand(const LogArgs& a, hipStream_t s);

// ---- the log kernels: each args block starts with the LogView of rq_log_walk.h ----
// ---- time-resolved metrics from event logs (rq_timeline.hip) ----
struct TimelineArgs {
    LogView log;
    const double* edges;      // [n_bins + 1]
    int n_bins;
    int Ks[RQ_MAX_K];
    int nK;
    double* metrics;          // [n_rep][n_bins][nK + 2]
    int64_t* posts;           // [n_rep][n_bins][2]
    int32_t* wall_posts;      // [n_rep][n_sinks][n_bins] or null
    int32_t* status;          // [n_rep]
};
hipError_t rq_launch_timeline(const TimelineArgs& a, hipStream_t s);

// ---- per-follower metrics from event logs (rq_followers.hip) ----
// LDS bytes of one sink's state: tlast f64 + acc[nK + 2] f64 + rank i32 (+ rows[2] i32)
inline int rq_followers_sink_bytes(int nK, bool with_rows) { return 12 + 8 * (nK + 2) + (with_rows ? 8 : 0); }
constexpr int RQ_FOLLOWERS_LDS_BYTES = 160 * 1024;   // one workgroup's LDS on gfx950
struct FollowersArgs {
    LogView log;
    int Ks[RQ_MAX_K];
    int nK;
    double* vals;             // [n_rep][n_sinks][nK + 2]
    double* first_t;          // [n_rep][n_sinks]
    int32_t* rows;            // [n_rep][n_sinks][2] or null
    double* r2_true;          // [n_rep]
    int32_t* status;          // [n_rep]
};
hipError_t rq_launch_followers(const FollowersArgs& a, hipStream_t s);

// ---- the same past the LDS sink limit: sink tiles + an r2 pass (rq_followers.hip) ----
struct FollowersTiledArgs {
    FollowersArgs f;          // f.log: the graph's full CSR (the r2 pass)
    const int* tile_ptr;      // [n_tiles][n_str + 1] into tile_col (GraphTopo)
    const int* tile_col;      // [n_edges]
    int n_tiles;
    int32_t* flags;           // [n_rep][n_tiles] workspace; bit 0: a sink of the tile got two rows at one t
};
hipError_t rq_launch_followers_tiled(const FollowersTiledArgs& a, hipStream_t s);

// ---- rank distribution from event logs (rq_rank_hist.hip) ----
struct RankHistArgs {
    LogView log;
    const double* edges;      // [n_bins + 1]
    int n_bins;
    int n_ranks;              // 1..RQ_RANK_HIST_MAX_RANKS; cell n_ranks is the tail
    double* hist;             // [n_rep][n_bins][n_ranks + 1]
    int32_t* n_seen;          // [n_rep]
    int32_t* max_rank;        // [n_rep]
    int32_t* status;          // [n_rep]
};
hipError_t rq_launch_rank_hist(const RankHistArgs& a, hipStream_t s);

// ---- whole-horizon metrics from event logs, exact on ties (rq_log_metrics.hip) ----
constexpr int RQ_LM_NL = 66;                // leaf capacity of the scan's LDS layout (as RQ_FWS_NL)
constexpr size_t RQ_LM_SCRATCH_BYTES = 4784;   // 8 * npsum_lds_doubles<RQ_MAX_K + 2, 66>() >= wave_npsum<1>'s 4128
constexpr int RQ_LM_CELL_BYTES = 16;        // one pivot column's state
constexpr size_t RQ_LM_LDS_BYTES = 160 * 1024;   // one workgroup's LDS on gfx950
// blocks of a launch, each with its own rows in the workspace.  Blocks stride over the
// replicas, so fewer would do, but the stride is static: at 2048 the C3 game's 10,000 logs
// took 59-68 ms against 45-51 ms at 4096 (more, shorter blocks even out)
constexpr int RQ_LM_SLOTS = 4096;
constexpr int64_t RQ_LM_MAX_EV_CAP = 1 << 20;   // a column's rows in a t-group in 24 bits, their rank sum in 40
// bytes of the per-column state: the cells, or the stream bits the first step keeps there
inline size_t rq_log_metrics_state_bytes(int n_sinks, int n_str)
{
    const size_t cells = (size_t)n_sinks * RQ_LM_CELL_BYTES;
    const size_t sbits = (((size_t)n_str + 31) / 32 * 4 + 15) / 16 * 16;
    return cells > sbits ? cells : sbits;
}
// scratch + state + one bit per sink + a uint16 per word of those bits
inline size_t rq_log_metrics_lds_bytes(int n_sinks, int n_str)
{
    const size_t W = ((size_t)n_sinks + 31) / 32;
    return RQ_LM_SCRATCH_BYTES + rq_log_metrics_state_bytes(n_sinks, n_str) + 4 * W + (2 * W + 3) / 4 * 4;
}
// one block's rows: t f64, rowsum f64, nvalid u32, c_K u32 x nK for up to ev_cap rows
inline size_t rq_log_metrics_slot_bytes(int64_t ev_cap, int nK)
{
    return ((size_t)ev_cap * (20 + 4 * (size_t)nK) + 15) / 16 * 16;
}
// The slim entries (rq_log_metrics_slim, rq_log_metrics_of_slim): a column's state is 8 bytes
// of LDS -- rank, tag and one bit "several rows in the tag's t-group" -- and the 64-bit
// sum << 24 | count of such a group lives in the block's slot of the workspace, one word per
// column behind the slot's rows (rq_log_metrics.hip).
constexpr int RQ_LM_SLIM_CELL_BYTES = 8;
inline size_t rq_log_metrics_slim_state_bytes(int n_sinks, int n_str)
{
    const size_t cells = (size_t)n_sinks * RQ_LM_SLIM_CELL_BYTES;
    const size_t sbits = (((size_t)n_str + 31) / 32 * 4 + 15) / 16 * 16;
    return cells > sbits ? cells : sbits;
}
constexpr size_t rq_log_metrics_slim_cells_lds_bytes(size_t n_sinks)   // the formula while the cells outgrow the stream bits
{
    return RQ_LM_SCRATCH_BYTES + n_sinks * RQ_LM_SLIM_CELL_BYTES + 4 * ((n_sinks + 31) / 32) +
           (2 * ((n_sinks + 31) / 32) + 3) / 4 * 4;
}
inline size_t rq_log_metrics_slim_lds_bytes(int n_sinks, int n_str)
{
    const size_t W = ((size_t)n_sinks + 31) / 32;
    return RQ_LM_SCRATCH_BYTES + rq_log_metrics_slim_state_bytes(n_sinks, n_str) + 4 * W + (2 * W + 3) / 4 * 4;
}
static_assert(rq_log_metrics_slim_cells_lds_bytes(RQ_LOG_METRICS_SLIM_MAX_SINKS) <= RQ_LM_LDS_BYTES,
              "RQ_LOG_METRICS_SLIM_MAX_SINKS sinks of 8-byte cells fit one workgroup's LDS");
// the spill words of a slot: one per graph sink (a replica has at most that many columns)
inline size_t rq_log_metrics_spill_bytes(int n_sinks) { return ((size_t)n_sinks * 8 + 15) / 16 * 16; }
inline size_t rq_log_metrics_slim_slot_bytes(int64_t ev_cap, int nK, int n_sinks)
{
    return rq_log_metrics_slot_bytes(ev_cap, nK) + rq_log_metrics_spill_bytes(n_sinks);
}
struct LogMetricsArgs {
    LogView log;
    int Ks[RQ_MAX_K];
    int nK;
    int n_slots;              // blocks; block b plays replicas b, b + n_slots, ...
    size_t state_bytes;       // rq_log_metrics_state_bytes / rq_log_metrics_slim_state_bytes
    size_t slot_bytes;        // rq_log_metrics_slot_bytes / rq_log_metrics_slim_slot_bytes
    size_t spill_off;         // slim: the spill words' offset in a slot (rq_log_metrics_slot_bytes); else 0
    char* rows;               // workspace [n_slots][slot_bytes]
    double* metrics;          // [n_rep][nK + 2]
    int64_t* out_counts;      // [n_rep][4]
    int32_t* status;          // [n_rep]
};
// slim: the 8-byte cells (state_bytes, slot_bytes and spill_off sized for them)
hipError_t rq_launch_log_metrics(const LogMetricsArgs& a, hipStream_t s, bool slim = false);

// rq_log_metrics_of: the same play for n_src tracked streams.  The work items (replica,
// tracked source) are dealt to m.n_slots blocks in contiguous ranges, so a block plays, per
// replica it meets, a run of consecutive tracked sources in its slot; while n_rep * n_src <=
// the slot count every run is one source long.  Outputs are indexed [replica][source].
struct LogMetricsOfArgs {
    LogMetricsArgs m;         // m.log.ctrl_idx is not read; m.n_slots = min(n_rep * n_src, slots)
    int trk[RQ_LOG_OF_MAX_SRC];   // stream index of src_ids[k]
    int n_src;
    int scope;                // RQ_LOG_OF_DF / RQ_LOG_OF_OWN
    double taper;             // set by the launch: 1, or RQ_LM_OF_TAPER when the blocks outnumber the resident ones
};
// shares of the work items fall from this many times the mean to 2 minus it (of_first_item)
#ifndef RQ_LM_OF_TAPER
#define RQ_LM_OF_TAPER 1.95
#endif
hipError_t rq_launch_log_metrics_of(const LogMetricsOfArgs& a, hipStream_t s, bool slim = false);

// ---- competing RedQueen broadcasters against an exogenous log (rq_game.hip) ----
struct GameArgs {
    const double* ev_t;       // [n_rep][ev_cap] the exogenous logs
    const int32_t* ev_src;    // [n_rep][ev_cap]
    const int64_t* counts;    // [n_rep][4], [2] = entries
    int64_t n_rep, ev_cap, max_events;
    int n_str, P, ctrl_lane, ctrl_idx;
    const double* inv;        // [n_str][P] (rqh::GameTables.inv)
    const int* meta;          // [n_str]    (rqh::GameTables.meta)
    int in_lds;               // inv copied to the block's LDS
    const uint32_t* seeds;    // [n_rep][P], column = lane_col
    double start, end;
    double* out_t;            // [n_rep][out_cap]
    int32_t* out_src;         // [n_rep][out_cap]
    int64_t out_cap;
    int64_t* out_counts;      // [n_rep][4]
    int64_t* player_posts;    // [n_rep][P], column = lane_col
    int32_t* status;          // [n_rep]
    const int* lane_stream;   // [P] (device copies of rqh::GameTables' lane tables)
    const int* lane_col;      // [P]
};
hipError_t rq_launch_game(const GameArgs& a, hipStream_t s);

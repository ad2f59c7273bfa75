// rq_host.h -- the host core of librq: graph topology, environment knobs, the planner and
// the controller tables.  Pure host arithmetic: this header, rq_topo.cpp and rq_plan.cpp
// build with any C++17 compiler and no ROCm include path (tests/host/plan_check.cpp does).
// rq_internal.h includes it, so the kernels and rq_api.cpp share the constants and
// SweepInst below.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/rq.h"

// ---- constants the planner and the kernels share ----
#define RQ_MAX_STREAMS 2048   // 512 per fast instance (8 per lane); LOG instances 16 / 32 per lane
#define RQ_NPSUM1_LDS 516   // doubles of wave_npsum<1> scratch (== rq::npsum_lds_doubles<1>())
// threads per block of the merged-stream sweep instances (1024: <= 128 VGPRs)
#ifndef RQ_MRG_LB
#define RQ_MRG_LB 1024
#endif
#define RQ_MG_B 512         // merge block: one source per thread (the fast general sweep: <= 512)
// merged entries carry the stream as u16 (+ a u8 of its high bits past 65535 streams);
// the two-level merge takes up to RQ_MG_B groups of RQ_MG_B streams
#define RQ_MAX_STREAMS_MRG (RQ_MG_B * RQ_MG_B)

// The sweep template instance a plan selects, one field per template axis.  The planner
// builds it from a Plan (sweep_inst: its candidates, rq_plan_info and the launch alike);
// each kernel file resolves it to the kernel in one place (sweep_kernel / fw_kernel), which
// the launch and the occupancy query share.  The flags name the kernels' template
// parameters (the rq_kernels and rq_sweep_fw kernel files).
struct SweepInst {
    bool fused;   // rq_sweep_fw / rq_sweep_fwm (<= 64 sources), else the general rq_sweep
    int nK;       // K variants (1..RQ_MAX_K)
    bool col16;   // sink columns in LDS as uint16, else read from global memory as int
    bool log;     // the sequential sweep (event log, max_events, duplicate edges, ties)
    bool gs;      // log: the per-sink state in global memory (SweepArgs.gs)
    bool bits;    // K = 1 on per-stream sink bitsets
    bool bl;      // K = 1 on per-wave LDS sink bits (general sweep)
    bool mrg;     // plays the merged streams of rq_merge_streams; else:
    int spl;      //   general: sources per lane, 1 / 2 / 4 / 8 (log: 1 / 8 / 16 / 32)
    int W;        //   fused: depth of the generated arrival rings, 32 / 16 / 8 (the general
                  //   instances fix theirs: a window of 4; log: rings of 8, 4 at 32 per lane)
    bool gt;      // mrg, general: the per-stream tables in global memory
    bool pw;      // fused: the OptPWSignificance controller
    bool pair;    // fused, mrg: the RedQueen controller's draws by call pairs (one Philox call per
                  //   lane every other tile, both of its draws used), else a call per draw
    bool scan;    // fused, mrg: the wave that swept a replica integrates its rows itself (rq_scan's
                  //   sums, written to SweepArgs.metrics; no rq_scan launch for the chunk)
    bool blk;     // fused, mrg, bits: phase C with the tile's events blocked four to a lane
                  //   (BlkFlags) once every sink has a row, else one event per lane throughout
    bool pk;      // fused, mrg, scan, nK == 1: the replica's pivot rows as 16-byte records {t, sumR u32,
                  //   cnt u16, valid u16} in the bytes of rows_t / rows_sum, else the four row arrays
};
// SweepInst.blk: lane 16 b + g scans events 4g .. 4g + 3 over the RQ_BLK_CB words of column
// block b.  An even number of words per block (two columns per trip, 8-byte reads), so the
// four blocks cover nw rounded up to 8 words; the pad words hold zero masks and zero F.  A
// mask row is the four blocks plus 4 words: rows stay 16-byte aligned and start on 16 banks.
// A tile pays the staging, the flags and the transposed sum of the counts whatever nw is
// (about 85 VALU in the gfx950 code) and 65 per trip of two columns, where the word loop pays
// 33 per trip of two words: 85 + 65 ceil(nw / 8) against 16.5 nw + 10 is the shorter one at 13
// to 16 words and from 17 on.
#define RQ_BLK_CB(nw) ((((nw) + 7) >> 3) << 1)
#define RQ_BLK_MSTRIDE(nw) (4 * RQ_BLK_CB(nw) + 4)
#define RQ_BLK_MIN_NW 13
// SweepInst.scan: the per-wave LDS of the sweep's scan, aliased on the wave's sweep area
// (dead after the tile loop, initialised again at the top of each replica); the layout of
// rq::npsum_lds_doubles<nK + 2, RQ_FWS_NL>() -- 66 leaf slots, a block of 8192 rows has <= 65
#define RQ_FWS_NL 66
#define RQ_FWS_LDS_BYTES(nK) ((size_t)8 * (((nK) + 2 + 3) * RQ_FWS_NL + 4))

// The sink-tiled follower kernels (rq_followers.hip): sink columns per tile.  A tile's
// per-sink state -- 12 + 8 (nK + 2) bytes, 8 more with row counts -- lives in one workgroup's
// 160 KiB of LDS whatever nK and the counts, so TS <= 2409; 2048 is the measured choice
// (-DRQ_FOLLOWERS_TILE_SINKS=... builds the other for the A/B).
#ifndef RQ_FOLLOWERS_TILE_SINKS
#define RQ_FOLLOWERS_TILE_SINKS 2048
#endif
static_assert(RQ_FOLLOWERS_TILE_SINKS >= 1 &&
                  (long long)RQ_FOLLOWERS_TILE_SINKS * (12 + 8 * (RQ_MAX_K + 2) + 8) <= 160 * 1024,
              "a tile of every nK / rows variant must fit one workgroup's LDS");

// ---- the planner's three questions to the device ----
// Defined next to the kernels (the rq_kernels and rq_sweep_fw files); a program that links the
// host core without them supplies its own.
// blocks of 64 * wpb threads per CU the instance reaches with `lds` bytes of dynamic LDS
// (rq_occupancy); <= 0: no instance or no device -- the planner takes the LDS bound
int rq_sweep_blocks_per_cu(const SweepInst& i, int wpb, size_t lds);
// the fused pair of rq_sweep_blocks_per_cu (SweepInst.fused)
int rq_fw_blocks_per_cu(const SweepInst& i, int wpb, size_t lds);
int rq_cu_count();   // CUs of the current device (256 on MI355X when the query fails)

namespace rqh {

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// SweepInst.pk: whether a 16-byte row record holds every row of a replica.  One K; valid and
// cnt count sinks (16 bits each); sumR, the sum of the sinks' ranks, grows by at most n_sinks per
// wall event and a replica plays at most mrg_stride merged entries (32 bits).
inline bool rows16_fits(int nK, int n_sinks, int64_t mrg_stride)
{
    // both factors bounded first: the product stays below 2^48, no wrap
    return nK == 1 && n_sinks >= 0 && n_sinks <= 65535 && mrg_stride >= 0 && mrg_stride < ((int64_t)1 << 32) &&
           (uint64_t)n_sinks * (uint64_t)mrg_stride < ((uint64_t)1 << 32);
}

// sink tiles of a graph of n_sinks sinks, and the workspace of rq_log_followers_tiled on it:
// one int32 flag per (replica, tile), rounded up to 256 bytes
inline int followers_tiles(int n_sinks) { return (n_sinks + RQ_FOLLOWERS_TILE_SINKS - 1) / RQ_FOLLOWERS_TILE_SINKS; }
inline size_t followers_tiled_ws_bytes(int n_sinks, int64_t n_rep)
{
    return align_up((size_t)4 * (size_t)n_rep * (size_t)followers_tiles(n_sinks), 256);
}

// ---- environment knobs ----
// Everything a plan or a launch depends on besides its arguments.  read_knobs() reads the
// environment once per ABI call (tests and bench.py flip knobs between runs of one process);
// the planner and the run loop take the struct and never call getenv themselves.
template <class T>
struct Knob {   // a knob whose unset default depends on the plan or the call
    bool set = false;
    T v{};
};
struct Knobs {
    // -- the planner (make_plan and the workspace budget) --
    // RQ_WS_BUDGET_GB: caps the workspace budget, GiB (include/rq.h documents it for users)
    Knob<double> ws_budget_gb;
    // RQ_CAP_SQUEEZE: scales the merged-sequence / pivot-row capacities down, clamped to
    // [0.01, 1]; tests only (test_gpu_engine, test_gpu_reruns, test_gpu_sweep_scan: undersized
    // capacities exercise the overflow reruns)
    double cap_squeeze = 1.0;
    // RQ_MG_GRP: streams per first-level merge group, 64 or RQ_MG_B; A/B (scripts/dev/ab_grp.sh)
    Knob<int> mg_grp;
    // RQ_MRG=0: the general fast sweep merges the per-source streams itself; A/B only
    bool mrg = true;
    // RQ_G_COLLDS: force the general sweep's column placement (1 LDS, 0 global); tuning only
    Knob<int> g_collds;
    // RQ_G_W: only this ring depth for the general sweep (0: any); tuning only
    int g_w = 0;
    // RQ_SKIP=0: no played-stream skipping in the K = 1 sink-bit sweep; A/B, test_gpu_graphs
    bool skip = true;
    // RQ_FWM=0: the fused sweep generates its arrivals in-kernel; A/B only
    bool fwm = true;
    // RQ_CTRL_DRAWS=0: a Philox call per controller draw instead of call pairs; A/B and
    // tests (test_gpu_ctrl_draws, test_gpu_draws_ahead, test_gpu_sweep_scan)
    bool ctrl_draws = true;
    // RQ_SWEEP_SCAN=0: the scan kernel instead of the sweep's own scan; A/B, test_gpu_sweep_scan
    bool sweep_scan = true;
    // RQ_ROWS_PACKED=0: the scanning merged fused sweep keeps its rows in the four row arrays
    // instead of 16-byte records; A/B, test_gpu_rows_packed
    bool rows_packed = true;
    // RQ_GEN_SPLIT=0: rq_gen_streams for every stream instead of rq_gen_classes' body per
    // class of source kinds; A/B, test_gpu_gen_split
    bool gen_split = true;
    // RQ_PHASEC_BLK=0: the merged sink-bit sweep keeps one event per lane in phase C (the word
    // loop); A/B, test_gpu_phase_c_blocked
    bool phasec_blk = true;
    // RQ_FW_W: only this ring depth for the fused sweep (0: any); tuning (scripts/gpu_envab.sh)
    // and test_gpu_policy
    int fw_w = 0;
    // RQ_PIPE: streams of the pipelined chunk loop, clamped to 1..3; bench.py sets 1 for its
    // per-kernel times; A/B (scripts/bench_paths.py, scripts/gpu_ab_env.sh, scripts/dev/ab5.sh,
    // ab_c5.sh)
    int pipe = 2;
    // RQ_PIPE_CHUNK: replicas per pipelined chunk, at least 64; A/B only
    Knob<int64_t> pipe_chunk;
    // RQ_ORDER=1: longest-first replica order for the sweep; A/B and test_gpu_merge
    bool order = false;

    // -- rq_run_batch (the sweep's launch arguments) --
    // RQ_SWEEP_DBG: SweepArgs.dbg, skips sweep phases; profiling only (scripts/gpu_dbg.sh,
    // gpu_breakdown.sh, c5_phase.py)
    int sweep_dbg = 0;
    // RQ_FW_TILE: arrivals a fused tile aims at; tuning and test_gpu_policy
    double fw_tile = 58.0;   // measured on C3: 40 -> 895k, 48 -> 943k, 58 -> 964k, 62 -> 956k replicas/s
    // RQ_FW_HMIN / RQ_FW_THR / RQ_FW_HFILL: the fused sweep's refill policy (clamped against
    // the plan where they are used); tuning and test_gpu_policy
    Knob<int> fw_hmin, fw_thr, fw_hfill;
    // RQ_FW_STATIC: nonzero = no replica work queue (one replica per wave); read once per
    // process; A/B only (scripts/c5_rate.py)
    int fw_static = 0;
    // RQ_CLK_MERGE: RQ_PHASE_CLOCK builds only, the merge's phase clocks instead of the
    // sweep's (scripts/dev/merge_clock.py)
    bool clk_merge = false;

    // -- rp_run (dataframe replay) --
    // RQ_RP_CHUNK: force the chunked replay on (nonzero) or off (0); A/B, test_gpu_replay_chunked,
    // scripts/bench_paths.py, redqueen_amd/utils.py's docs
    Knob<int> rp_chunk;
    // RQ_RP_SMALL=0: no small-table first tier for one K; A/B only
    bool rp_small = true;
    // RQ_CLK_REPLAY: RQ_PHASE_CLOCK builds only, rq_rp_fast's phase clocks (scripts/dev/replay_clock.py)
    bool clk_replay = false;

    // -- rq_log_metrics_of --
    // RQ_LM_OF_SLOTS: blocks (workspace slots) of a launch, clamped to 1..4096 (the default);
    // tests only (test_gpu_log_sources: tiny batches past the slot count, where a block plays
    // runs of sources)
    int lm_of_slots = 4096;
};
Knobs read_knobs();

// ---- graph topology: the host half of an rq_graph ----
struct GraphTopo {
    int n_str = 0, ctrl_idx = -1, n_sinks = 0, n_fol = 0;
    int64_t n_edges = 0, ctrl_src_id = 0;
    double start = 0.0, end = 0.0;
    // per stream (dynamic sources by src_id, then static ones by src_id); the controlled
    // slot has kind RQ_SRC_NONE
    std::vector<int64_t> src_id;
    std::vector<int> kind, orig_idx, arr_off, arr_n;
    std::vector<int> is_static;   // 1: a static source (equal times play after the dynamic ones)
    std::vector<uint32_t> seed;
    std::vector<double> p0, p1, p2, arr_a, arr_b;
    std::vector<int> csr_ptr, csr_col, outdeg_f, fol;
    std::vector<int64_t> fol_ids;
    std::vector<int64_t> sink_ids;   // sorted: the sink column -> sink id map
    std::vector<int> csr_col_el;     // sink columns in edge-list order for every stream
    std::vector<int> col_to_fol;     // sink column -> follower position or -1
    // duplicate (source, sink) edges (a multigraph, opt_model.py:169-175 accepts them): the
    // sweep's CSR row of a source holds its distinct sinks first (layer 0), then the 2nd
    // occurrences (layer 1), ...; every layer has distinct sinks.  lay_end[lay_ptr[j] ..
    // lay_ptr[j+1]) are the CSR ends of stream j's layers.  multi: some row has > 1 layer.
    bool multi = false, ctrl_dup = false;
    // two of the graph's own RealData times are equal -- among the wall sources
    // (rd_ties), or with the controlled slot's replayed times too (rd_ties_ctrl, runs with
    // an RQ_SRC_REALDATA controller): every replica meets that tie, so such runs go to the
    // exact sequential sweep directly
    bool rd_ties = false, rd_ties_ctrl = false;
    std::vector<int> lay_ptr, lay_end;
    // per-stream sink bitsets (32 sinks per word) for the K=1 bitset sweep, n_sinks <= 2048
    int nw = 0;
    std::vector<uint32_t> masks;
    std::vector<uint32_t> fbits;   // follower set as a sink bitset (BL sweep)
    // the controller posts before a wall event at the same time when that source is static
    // or has a larger src_id (opt_model.py:279-281, :289-290): the sweeps' per-stream flag,
    // in global memory for the GT instances (the others build it in LDS)
    std::vector<int> cbf;
    // the streams but the controlled slot by generator class -- gen_n[0] Hawkes, gen_n[1]
    // Poisson / Poisson2, gen_n[2] others -- for rq_gen_classes' body per class
    std::vector<int> gen_cls;
    int gen_n[3] = {0, 0, 0};
    // the CSR cut into sink tiles of RQ_FOLLOWERS_TILE_SINKS columns (tile i owns columns
    // [i TS, min((i + 1) TS, n_sinks))), for graphs without duplicate edges and with at most
    // RQ_FOLLOWERS_TILED_MAX_SINKS sinks (n_tiles == 0 otherwise): tile_ptr[n_tiles][n_str + 1]
    // indexes tile_col[n_edges], laid out tile-major, and stream j's entry of tile i is the
    // columns of j's row that fall in the tile (global column indices, the row's order).  So
    // csr_ptr = tile_ptr + i (n_str + 1), csr_col = tile_col is a CSR of the tile's edges.
    int n_tiles = 0;
    std::vector<int> tile_ptr, tile_col;
    // controlled-slot arrays (PiecewiseConst / RealData controlled runs)
    int ctrl_arr_off = 0, ctrl_arr_n = 0;
};
// validate the network and fill *g (rq_graph_build up to its uploads); RQ_OK or the
// rq_status rq_graph_build returns for this description
int topo_build(const rq_graph_desc* d, GraphTopo* g);

// ---- the plan of one rq_run_batch call ----
struct Plan {
    int nK = 1, spl = 1, wpb = 4, n_sinks_pad = 0;
    int64_t R = 0, chunk = 0, capsum = 0, cap_rows = 0;
    int64_t rep_lo = 0, rep_cnt = 0;   // per-grid-point replica window (rq_batch_desc.rep_lo/rep_cnt)
    std::vector<int> cap;
    std::vector<int64_t> st_off;
    std::vector<int> rd_k;   // stream -> per-replica RealData source k (rq_batch_desc.rd_*) or -1
    // sequential (event log / max_events) sweep variant; K=1 sink-bitset variant
    bool log = false, bits = false;
    // K=1 on per-wave LDS sink bits for graphs past the bitset variant (> 64 sources)
    bool bl = false;
    size_t g_fb = 0, g_etab = 0, g_inv = 0, g_skip = 0;
    bool g_inv_sh = false;   // general sweep: 1/c_j in the block's shared LDS (one grid point)
    bool gs = false;         // LOG sweep: per-sink state in global memory, gs_slots wave slots
    int64_t gs_slots = 0, gs_stride = 0;
    // fused windowed sweep (n_str <= 64): arrivals generated in-kernel, window depth fw_h
    bool fw = false;
    int fw_h = 8, mstride = 1;
    // general fast sweep on merged streams (rq_merge_streams; sweep_mode 6: the windowed
    // per-source merge inside the sweep instead)
    bool mrg = false;
    // the sequential sweep over > RQ_MAX_STREAMS sources: it plays the merged sequence
    // too (its own per-lane rings hold <= 32 sources per lane)
    bool lmrg = false;
    // merged streams with the per-stream tables (CSR starts, follower out-degrees, tie
    // flags, 1/c_j) in global memory: graphs whose tables do not fit LDS (the GT instances;
    // the sequential ones on merged streams always)
    bool gt = false;
    size_t off_mt = 0, off_mj = 0, off_mjh = 0, off_mlen = 0;
    int64_t mrg_stride = 0;   // merged entries per replica (capacity)
    int n_grp = 1;            // > RQ_MG_B sources: groups of the two-level merge
    int grp_sz = RQ_MG_B;     //   streams per group (64 up to 64 groups: MergeArgs.grp_sz)
    int64_t sub_stride = 0;   //   entries per (replica, group) of the first level
    size_t off_sub_t = 0, off_sub_j = 0, off_sub_len = 0;
    // the fused sweep's phases B / C on merged streams (rq_gen_streams + rq_merge_streams
    // instead of in-kernel generation; sweep_mode 7: the in-kernel generating sweep)
    bool fwm = false;
    // fwm with the RedQueen controller: its Exp(1) draws by call pairs (SweepInst.pair;
    // RQ_CTRL_DRAWS=0 keeps a Philox call per draw)
    bool pair = false;
    // fwm without event log or max_events: each wave integrates the rows of the replica it
    // swept (SweepInst.scan), the chunk launches no rq_scan; RQ_SWEEP_SCAN=0 keeps the kernel
    bool scan = false;
    // scan at one K where a 16-byte record holds every row (rows16_fits with this plan's
    // mrg_stride, so a rerun with doubled capacities decides again): the sweep writes and reads
    // records in the bytes of off_rt .. off_rv (SweepInst.pk); RQ_ROWS_PACKED=0 keeps the arrays
    bool rows16 = false;
    // fwm on sink bits with at least RQ_BLK_MIN_NW words: phase C event-blocked (SweepInst.blk),
    // mask rows of RQ_BLK_MSTRIDE words; RQ_PHASEC_BLK=0 keeps the word loop and its stride
    bool blk = false;
    // general sweep LDS layout
    int gwpb = 4, gwin = 16, gcol_lds = 1, gcol16 = 0;
    size_t g_col = 0, g_ptr = 0, g_odf = 0, g_cbf = 0, g_wave = 0, g_wave_stride = 0, g_rank_off = 0,
           g_win_off = 0, g_x_off = 0, g_total = 0, g_stage_off = 0;
    size_t tables_bytes = 0;
    // resident sweep waves per CU of the chosen instance (the persistent grid's slots)
    int wpc = 0;
    // pipelined chunks (merged-stream sweeps): nbuf buffer sets, chunk k on stream k % nbuf
    // with set k % nbuf, so chunk k+1's generation / merge and chunk k-1's scan fill the
    // wave slots chunk k's sweep tail leaves (rq_run_batch); off_set0 + set * set_stride
    // is a set's base, the per-chunk offsets below are relative to it
    int nbuf = 1;
    bool order = false;   // longest-first replica order for the sweep (rq_order_replicas)
    size_t off_set0 = 0, set_stride = 0, off_ord = 0;
    size_t off_pwc = 0, off_pwmax = 0;
    size_t off_invc = 0, off_streams = 0, off_slen = 0, off_rt = 0, off_rs = 0, off_rv = 0,
           off_rc = 0, off_sall = 0, off_wq = 0, off_stoff = 0, off_cap = 0, off_rdk = 0, off_repidx = 0, off_gs = 0,
           total = 0;
};

// The plan of batch b on graph g within `budget` bytes of workspace (<= 0: no budget); the
// only device facts it uses are the three queries above.  RQ_OK or the rq_status the ABI
// call returns.
int make_plan(const GraphTopo& g, const rq_batch_desc* b, const Knobs& kn, double budget, Plan* p);
// the instance a finished plan runs
SweepInst sweep_inst(const Plan& p, int ctrl_kind);
// the nine values of rq_plan_info_n (include/rq.h)
void plan_info(const Plan& p, int ctrl_kind, int64_t info[9]);

// ---- the controller's per-run tables ----
struct CtrlTables {
    std::vector<double> invc;         // [n_grid][n_str] 1 / c_j (RedQueen; else zeros)
    std::vector<double> pwc, pwmax;   // OptPWSignificance: [n_grid][n_str][n_seg], [n_grid][n_str]
};
CtrlTables ctrl_tables(const GraphTopo& g, const rq_batch_desc* b);

// ---- the players' rate tables of rq_log_game (include/rq.h) ----
// Lane c of the game kernel is the player with the c-th smallest src_id, so the lowest lane
// among equal pending times is the reference's tie winner.
struct GameTables {
    int P = 0;                      // players
    int ctrl_lane = -1;             // the lane of the controlled source, if it plays
    std::vector<int> lane_stream;   // [P] the lane's stream index
    std::vector<int> lane_col;      // [P] the lane's position in the caller's players[] (seed column)
    std::vector<double> C;          // [P][n_str] by lane
    std::vector<double> inv;        // [n_str][P] transposed: 1 / C, 0 where C is 0
    // per stream: bits 0-7 = the lanes [0, k) whose post plays before an entry of this stream
    // at an equal time (P for a static stream, else the players of smaller src_id);
    // bit 8 = the stream has an edge
    std::vector<int> meta;
};
#define RQ_GAME_META_EDGE 256
// LDS bytes the transposed table may take (4 waves a block share it; 64 KiB leaves two blocks a CU)
#define RQ_GAME_LDS_TABLE_BYTES (64 * 1024)
inline size_t game_table_bytes(int n_str, int P) { return (size_t)n_str * (size_t)P * sizeof(double); }
inline bool game_table_in_lds(int n_str, int P) { return game_table_bytes(n_str, P) <= RQ_GAME_LDS_TABLE_BYTES; }
// workspace of rq_log_game: [inv | meta | lane_stream | lane_col], each rounded up to 256 bytes
inline size_t game_ws_off_meta(int n_str, int P) { return align_up(game_table_bytes(n_str, P), 256); }
inline size_t game_ws_off_lanes(int n_str, int P)
{
    return game_ws_off_meta(n_str, P) + align_up((size_t)n_str * sizeof(int), 256);
}
inline size_t game_ws_bytes(int n_str, int P)
{
    return game_ws_off_lanes(n_str, P) + 2 * align_up((size_t)RQ_GAME_MAX_PLAYERS * sizeof(int), 256);
}
// RQ_OK, or the rq_status rq_log_game returns for these players on this graph
int game_tables(const GraphTopo& g, const rq_game_player* players, int n_players, GameTables* out);

// ---- the tracked sources of rq_log_metrics_of (include/rq.h) ----
// trk[k] = the stream index of src_ids[k]; RQ_EINVAL for n_src outside 1..RQ_LOG_OF_MAX_SRC,
// an id that is no stream of the graph or an id named twice (trk is then unspecified)
int log_of_streams(const GraphTopo& g, const int64_t* src_ids, int n_src, int* trk);
// blocks (= workspace slots) of a launch over n_rep * n_src work items
inline int64_t log_of_blocks(int64_t n_rep, int n_src, int slots)
{
    const int64_t items = n_rep * (int64_t)n_src;
    return items < slots ? items : slots;
}

}  // namespace rqh

// rq_sweep_fw.hip -- the fused windowed sweep (<= 64 sources: arrivals generated
// in-kernel) and its launch wrappers, called by the C ABI in rq_api.cpp.  The
// general sweep, the stream generator and the scan are in rq_kernels.hip.
//
// Kernel role (reference file:line it replaces): Manager.run_dynamic
// opt_model.py:241-314 with every broadcaster's get_next_interval (Poisson :424-433,
// Poisson2 :396-405, Hawkes :466-490, PiecewiseConst :642-663, RealData :722-750,
// Opt :502-544, OptPWSignificance :547-623) + State.apply_event :61-83 + the per-row
// part of rank_of_src_in_df utils.py:38-56.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rq_device.h"
#include "rq_internal.h"
#include "rq_sweep_core.h"
#include "rq_gen.h"
#include "rq_scan_rows.h"
#include <type_traits>
#include <cstdlib>

#pragma clang fp contract(off)

using namespace rq;

// ============================================================================
// fused windowed sweep (n_str <= 64).  Lane j owns stream j and GENERATES its
//     arrivals (SrcGen) into an LDS ring -- no stream buffer, no generator
//     kernel.  A tile is every pending arrival earlier than a cut tau, found from
//     the next H arrivals of each ring held in registers (a ring's unseen
//     arrivals are >= its H-th, so tau <= min over rings of the H-th keeps the
//     tile complete); tau adapts so a tile holds <= 64 arrivals.  The tile is
//     staged in source order and rank-sorted into (t, stream) order -- the
//     reference's (time, src_id) order (opt_model.py:279-281).  Phase B is the
//     same controller; phase C for K = 1 runs lane-parallel over the tile's
//     events: per sink-bitset word, segmented prefix ORs (segments start at the
//     posts) give each event's top-1 set, plain prefix ORs its valid set.
// ============================================================================
// MRG: the arrivals come pre-generated (rq_gen_streams) and merged into the replica's
// (t, stream) sequence (rq_merge_streams): a tile is its next 64 entries, loaded one tile
// ahead, and phase A (refill passes, window cut, rank sort) disappears
// PAIR (MRG, RedQueen controller): the controller's draws by call pairs.  Draw d is half
// d & 1 of Philox call d >> 1, and a tile starts at a multiple of 64 draws, so lanes 2k and
// 2k + 1 of controller_tile each run call k and keep one half.  Here every other tile
// each lane runs ONE call and both of its logarithms, and the 128 draws of that tile and
// the next reach their lanes by cross-lane reads: half the Philox calls, the same bits.
// SCAN (MRG): the wave integrates the rows of the replica it has just swept (scan_rows:
// rq_scan's sums, bit for bit) before it takes the next replica, so the chunk needs no
// rq_scan launch.  Producer and consumer of the rows are the same wave: its stores drained
// and a workgroup-scope fence order them, nothing crosses a CU.  The scan's LDS aliases the
// wave's sweep area, which is dead by then and initialised again at the top of a replica.
//
// fws_tu: rows per lane and trip of that scan (TU of wave_npsum_rows; rq_scan runs 16 at
// 176 VGPRs).  The kernel stays at 128 VGPRs and 4 waves per SIMD, and the scan's registers
// come on top of what lives across the replica loop.  At 8 the tile loop of every instance
// spills; at 4 the one-K instances' (sink bits and columns) are free of scratch, at 2 the
// two-K instances' too.  The three- and four-K instances stand at 128 VGPRs without the
// scan and keep a few scratch accesses per tile at any TU, also with the scan as a call
// (DESIGN §15).
// PK (16-byte records, K = 1): a row is four registers until it is used, not six, so the
// budget of 4 array rows holds 6 records per lane.  4, 6 and 8 all compile to the same spill
// count and no further scratch access in the tile loop; 6 and 8 measured alike on the C3 step
// and 4 slightly slower, so 6, the one that fits the old budget.
constexpr int fws_tu(int nk, bool pk = false) { return nk == 1 ? (pk ? 6 : 4) : 2; }
template <int NK, bool PK = false>
__device__ __forceinline__ void fw_scan_rows(int64_t n, double S, double end, const double* Rt, const double* Rs,
                                             const uint32_t* Rv, const uint32_t* Rc, double* lds, double* out)
{
    constexpr int NV = NK + 2;
    static_assert(RQ_FWS_LDS_BYTES(NK) == 8 * (size_t)npsum_lds_doubles<NV, RQ_FWS_NL>(), "the planner's size");
    const int lane = lane_id();
    if (n == 0) {
        if (lane < NV) out[lane] = __builtin_nan("");
        return;
    }
    // every row was stored by this wave: drain its stores, then order them before its
    // loads at workgroup scope (same wave, same CU: no L2 write-back)
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    double res[NV];
    if constexpr (PK)   // Rt: the replica's records
        scan_rows16<fws_tu(NK, true), RQ_FWS_NL>(n, S, end, reinterpret_cast<const uint4*>(Rt), lds, res);
    else
        scan_rows<NK, fws_tu(NK), RQ_FWS_NL>(n, S, end, Rt, Rs, Rv, Rc, lds, res);
    if (lane == 0) {
#pragma unroll
        for (int s = 0; s < NV; ++s) out[s] = res[s];
    }
}
// PK (SCAN, K = 1): the replica's rows as 16-byte records at rows_t (RowStage<1, true>), which
// only this wave reads; the planner admits it where every field fits (Plan.rows16).
template <int NK, class COL, int W, int H, bool BITS, bool PW, bool MRG, bool PAIR = false, bool SCAN = false,
          bool BLK = false, bool PK = false>
__device__ __forceinline__ void sweep_fw_body(SweepArgs a)
{
    static_assert((W & (W - 1)) == 0 && H <= W, "ring");
    static_assert(!SCAN || MRG, "the sweep's own scan: merged instances only");
    static_assert(!BLK || (MRG && BITS), "event-blocked phase C: the merged sink-bit instances only");
    static_assert(!PK || (SCAN && NK == 1), "16-byte rows: the sweep's own rows at one K");
    extern __shared__ double lds_g[];
    char* base = reinterpret_cast<char*>(lds_g);
    const int lane = lane_id();
    const int w = threadIdx.x >> 6;
    int* cptr = reinterpret_cast<int*>(base + a.lds_ptr);
    int* odf = reinterpret_cast<int*>(base + a.lds_odf);
    int* cbf = reinterpret_cast<int*>(base + a.lds_cbf);
    constexpr bool col_lds = sizeof(COL) == 2;
    COL* col_l = reinterpret_cast<COL*>(base + a.lds_col);
    const int* col_g = a.csr_col;
    if (col_lds && !BITS)
        for (int e = threadIdx.x; e < a.n_csr; e += blockDim.x) col_l[e] = (COL)a.csr_col[e];
    uint32_t* msk = reinterpret_cast<uint32_t*>(base + a.lds_mask);
    const int ms = a.mstride;
    if (BITS)   // row n_str stays zero: the mask row of a lane without a wall event
        for (int e = threadIdx.x; e < (a.n_str + 1) * ms; e += blockDim.x) {
            const int jj = e / ms, ww = e - jj * ms;
            msk[e] = (jj < a.n_str && ww < a.nw) ? a.masks[jj * a.nw + ww] : 0u;
        }
    uint64_t* etab = reinterpret_cast<uint64_t*>(base + a.lds_etab);
    for (int e = threadIdx.x; e < RQ_EXP_TAB_N; e += blockDim.x) etab[e] = rq_exp_tab_c[e];
    for (int j = threadIdx.x; j <= a.n_str; j += blockDim.x) cptr[j] = a.csr_ptr[j];
    for (int j = threadIdx.x; j < a.n_str; j += blockDim.x) {
        odf[j] = a.outdeg_f[j];
        // the controller (a dynamic source) posts before a wall event at the same time
        // when that source is static (run_dynamic plays a static time only if it is
        // strictly earlier, opt_model.py:289-290) or has a larger src_id (the sorted
        // (t_delta, src_id) of the dynamic sources, :279-281)
        cbf[j] = a.cbf_g[j];   // the graph's table (static sources, RQ_SRCF_DYNAMIC)
    }
    __syncthreads();   // block-shared tables ready; no block barrier below this line
    char* wb = base + a.lds_wave + (size_t)w * a.lds_wave_stride;
    double* invc = reinterpret_cast<double*>(wb);
    int16_t* rank = reinterpret_cast<int16_t*>(wb + a.lds_rank_off);   // saturating, exact vs K-1
    // BITS: word w of the follower set F (.x) and of the top-1 set T (.y), read by
    // broadcast LDS loads in phase C (T is written back by the tile's last lane)
    uint2* ft = reinterpret_cast<uint2*>(wb + a.lds_rank_off);
    double* ring = reinterpret_cast<double*>(wb + a.lds_win_off) + lane * (W + 1);   // odd stride
    double* st_t = reinterpret_cast<double*>(wb + a.lds_stage_off);
    int* st_j = reinterpret_cast<int*>(st_t + 64);
    // first replica: the wave's static slot; with a work queue (a.wq) the wave then takes
    // replicas nslot, nslot + 1, ... in queue order until the chunk is exhausted (every
    // wave leaves once the counter passes n_chunk)
    const int64_t nslot = (int64_t)gridDim.x * a.wpb;
    for (int64_t qi = (int64_t)blockIdx.x * a.wpb + w; qi < a.n_chunk;) {
    const int64_t rl = a.order ? (int64_t)a.order[qi] : qi;   // longest first (rq_order_replicas)
    const int64_t o = a.chunk0 + rl;
    const int64_t i = rq_replica_of(a.gen, o);
    const int g = (int)(i / a.n_rep);
    for (int j = lane; j < a.n_str; j += 64) invc[j] = a.inv_c[(int64_t)g * a.n_str + j];
    if (!BITS)
        for (int c = lane; c < a.n_sinks; c += 64) rank[c] = -1;   // NaN: no row yet
    wave_lds_sync();

#ifdef RQ_PHASE_CLOCK
    unsigned long long ck[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tk = __builtin_amdgcn_s_memtime();
#define RQ_CLK(q)                                                   \
    do {                                                            \
        const unsigned long long t2 = __builtin_amdgcn_s_memtime(); \
        ck[q] += t2 - tk;                                           \
        tk = t2;                                                    \
    } while (0)
#else
#define RQ_CLK(q) \
    do {          \
    } while (0)
#endif
    // rows stored one tile late (RowStage::flush_pend); 16-byte rows at the end of their own tile
    constexpr bool DEFER = MRG && RQ_MRG_DEFER && !PK;
    SrcGen gen;
    if (lane < a.n_str && !MRG) gen.init(a.gen, lane, i, etab);
    else gen.none();
    int pos = 0, fil = 0;   // arrivals consumed / generated by this lane's source
    // MRG: the replica's merged sequence; lane l holds entry mpos + l of the next tile
    // (entry index of the replica's first entry; opaque at each tile's loads, so no
    // per-lane 64-bit sequence pointers are hoisted out of the tile loop and spilled)
    const int64_t mb = MRG ? rl * a.mrg_stride : 0;
    auto mload = [&](int64_t e, double& t_, int& j_) __attribute__((always_inline)) {
        int64_t x = mb;
        __asm__ volatile("" : "+v"(x));
        t_ = a.mrg_t[x + e];
        j_ = a.mrg_j[x + e];
    };
    const int mlen = MRG ? a.mrg_len[rl] : 0;
    int mpos = 0;
    double nxt_t = RQ_INF;
    int nxt_j = 0;
    if (MRG && lane < mlen) mload(lane, nxt_t, nxt_j);

    const bool opt = a.ctrl_kind == RQ_SRC_OPT || a.ctrl_kind == RQ_SRC_OPTPW;
    // OptPWSignificance only in the PW instances: the thinning loop's registers stay out
    // of the RedQueen controller's allocation
    const double* pwc = PW ? a.pw_c + (size_t)g * a.n_str * a.n_seg : nullptr;
    const double* pwm = PW ? a.pw_max + (size_t)g * a.n_str : nullptr;
    double opt_next = opt ? a.start : RQ_INF;
    const int64_t k = a.seed_mod > 0 ? i % a.seed_mod : i;
    const uint32_t oseed = a.ctrl_seed ? a.ctrl_seed[i] : a.ctrl_seed0 + (uint32_t)k;
    uint64_t ndraw = 0;   // wall events seen so far = the controller's draw index
    double px0 = 0.0, px1 = 0.0;   // PAIR: both draws of this lane's call of the current tile pair
    auto colat = [&](int e) -> int { return col_lds ? (int)col_l[e] : col_g[e]; };
    const int fol0 = cptr[a.ctrl_idx];
    auto folat = [&](int f) -> int { return colat(fol0 + f); };

    Agg<NK> ag;
    ag.init(a.Ks);
    AggB agb;
    if (BITS) {
        agb.init(msk, a.nw, ms, a.ctrl_idx, lane);
        // agb.F = 0 past nw; BLK: the pad words of the four column blocks too
        if (lane < (BLK ? 4 * RQ_BLK_CB(a.nw) : (a.nw + 1) & ~1)) ft[lane] = make_uint2(agb.F, 0u);
    }
    RowStage<NK, PK> rs;
    const int64_t rbase = rl * a.cap_rows;
    rs.init(a.rows_t, a.rows_sum, a.rows_valid, a.rows_cnt, rbase, a.cap_rows);

    int64_t n_events = 0, posts = 0, world = 0;
    int status = 0;
    double span = -1.0;   // adaptive tile width in time (< 0: not estimated yet)
    bool stop = false;
    // A refill pass steps every ring below W once and costs the same however few lanes
    // step; passes taken only while >= thr rings are below W keep the lanes busy, and a
    // ring is forced full only when it shows fewer than fw_hmin arrivals (the cut below
    // is bounded by each ring's last visible arrival, so a short ring only narrows it).
    const int thr = a.fw_thr;
    auto refill_pass = [&]() __attribute__((always_inline)) {
#ifdef RQ_PHASE_CLOCK
        ck[6] += 1;   // refill passes
        ck[7] += __popcll(__ballot(!gen.done && fil - pos < W));   // lanes stepping
#endif
        if (!gen.done && fil - pos < W) {
            double tv;
            if (gen.step(&tv, a.end)) {
                ring[fil & (W - 1)] = tv;
                ++fil;
            }
        }
    };
    for (;;) {
        int n = 0;
        bool act, fin;
        double tt, tx = 0.0;   // tx: the entry's controller draw (PAIR)
        int tj;
        if constexpr (MRG) {
            if (mpos >= mlen) break;   // every arrival played
            n = mlen - mpos < 64 ? mlen - mpos : 64;
            act = lane < n;
            tt = act ? nxt_t : RQ_INF;
            tj = act ? nxt_j : 0;
            mpos += n;
            fin = mpos >= mlen;
            if constexpr (DEFER) rs.flush_pend();   // the last tile's rows, ahead of the loads
            // the next tile's loads stay in flight through phases B and C
            nxt_t = RQ_INF;
            nxt_j = 0;
            if (mpos + lane < mlen) mload(mpos + lane, nxt_t, nxt_j);
            if constexpr (PAIR) {
                // ndraw = 64 x the tile's index (every tile before the last holds 64 entries,
                // a max_events cut ends the replica): an even tile draws calls ndraw / 2 + lane,
                // lane l of it takes draw ndraw + l from lane l / 2, of the next from 32 + l / 2
                const uint32_t tile = (uint32_t)(ndraw >> 6);
                if ((tile & 1u) == 0u) {
                    const uint64_t call = (ndraw >> 1) + (uint64_t)lane;
                    uint32_t w4[4] = {(uint32_t)call, (uint32_t)(call >> 32), 0u, 0u};
                    philox4x32_10(w4, oseed, kind_salt(RQ_SRC_OPT, true));
                    px0 = rq_std_exponential(rq_uniform53(w4[0], w4[1]));
                    px1 = rq_std_exponential(rq_uniform53(w4[2], w4[3]));
                }
                const int srcl = (int)((tile & 1u) << 5) + (lane >> 1);
                const double y0 = __shfl(px0, srcl, 64), y1 = __shfl(px1, srcl, 64);
                tx = (lane & 1) ? y1 : y0;
            }
            RQ_CLK(2);
        } else {
        // ---- A1: opportunistic passes while >= thr rings are below W; if some unfinished
        //      ring shows < hmin arrivals, passes until every ring shows >= hfill ----
        {
            bool hard = __ballot(!gen.done && fil - pos < a.fw_hmin) != 0;
            for (;;) {
                const uint64_t need = __ballot(!gen.done && fil - pos < W);
                if (!need || (!hard && __popcll(need) < thr)) break;
                refill_pass();
                // a forced run lasts until every ring shows >= fw_hfill arrivals
                if (hard) hard = __ballot(!gen.done && fil - pos < a.fw_hfill) != 0;
            }
        }
        RQ_CLK(0);   // A1: ring refills (arrival generation)
        const int avail = fil - pos;
        double v[H];
#pragma unroll
        for (int q = 0; q < H; ++q) v[q] = q < avail ? ring[(pos + q) & (W - 1)] : RQ_INF;
        const bool more = !gen.done || avail > H;        // arrivals past the window exist
        // the last arrival the window shows (avail >= hmin >= 1 for an unfinished ring):
        // this ring's unseen arrivals are >= it, so it bounds the cut
        double vb = v[0];
#pragma unroll
        for (int q = 1; q < H; ++q) vb = q < avail ? v[q] : vb;
        const double tfirst = wave_min_f64(v[0]);
        if (!(tfirst < RQ_INF)) break;                   // everything consumed
        const double tmax = wave_min_f64(more ? vb : RQ_INF);

        // ---- A2: the cut (exclusive): complete below tmax, <= 64 arrivals ----
        int c = 0;
        bool trunc = !(tmax > tfirst);   // a ring's window is all at tfirst: equal-time prefix
        if (!trunc) {
            double cut = tmax;
            if (span > 0.0 && tfirst + span < cut) cut = tfirst + span;
            if (!(cut > tfirst)) cut = next_up(tfirst);
            for (;;) {
                c = 0;
#pragma unroll
                for (int q = 0; q < H; ++q) c += v[q] < cut ? 1 : 0;
                n = (int)wave_sum_u32((uint32_t)c);
                if (n <= 64) break;
                const double nc = tfirst + (cut - tfirst) * 0.5;
                const double lo = next_up(tfirst);
                if (nc > tfirst && nc < cut) {
                    cut = nc < lo ? lo : nc;
                } else if (cut != lo) {
                    cut = lo;
                } else {
                    trunc = true;   // > 64 arrivals share tfirst
                    break;
                }
            }
            if (!trunc) span = (cut - tfirst) * (a.tile_target / (double)(n > 8 ? n : 8));
        }
        if (trunc) {
            // the arrivals equal to tfirst, in stream order, up to the first ring whose
            // window may continue at tfirst, at most 64
            c = 0;
#pragma unroll
            for (int q = 0; q < H; ++q) c += v[q] == tfirst ? 1 : 0;
            const uint64_t bl = __ballot(more && vb == tfirst);
            const int lb = bl ? __ffsll((unsigned long long)bl) - 1 : 64;
            if (lane > lb) c = 0;
        }
        const int off = (int)wave_scan_add((uint32_t)c) - c;
        if (trunc) {
            c = off >= 64 ? 0 : (c < 64 - off ? c : 64 - off);
            n = (int)wave_sum_u32((uint32_t)c);
        }

        RQ_CLK(1);   // window + A2 cut
        // ---- A3: stage in stream order, rank-sort into (t, stream) order ----
#pragma unroll
        for (int q = 0; q < H; ++q)
            if (q < c) {
                st_t[off + q] = v[q];
                st_j[off + q] = lane;
            }
        if (lane >= n) st_t[lane] = RQ_INF;   // the rank loop reads whole blocks of 8
        wave_lds_sync();
        act = lane < n;
        const double ti = act ? st_t[lane] : RQ_INF;
        const int ji = act ? st_j[lane] : 0;
        // rank = #staged arrivals before this one in (t, stream) order (stage_rank:
        // broadcast LDS reads, 8 slots per wait); profiling only: dbg 4 skips it
        const int rnk = a.dbg != 4 ? stage_rank(st_t, n, ti, lane) : lane;
        wave_lds_sync();
        if (act) {
            st_t[rnk] = ti;
            st_j[rnk] = ji;
        }
        wave_lds_sync();
        tt = act ? st_t[lane] : RQ_INF;
        tj = act ? st_j[lane] : 0;
        pos += c;
        fin = !__ballot(!gen.done || pos < fil);
        RQ_CLK(2);   // A3 stage + rank sort
        }   // !MRG

        int e0 = 0, e1 = 0, od = 0;
        if (act) {
            e0 = cptr[tj];
            e1 = cptr[tj + 1];
            od = odf[tj];
        }
        // ---- B: RedQueen controller over the tile ----
        uint64_t ownm = 0;
        double ot = RQ_INF;
        if (opt && a.dbg != 3) controller_tile<PW, PAIR>(n, act, tt, tj, invc, cbf, oseed, ndraw, opt_next, ownm, ot, pwc, pwm, a.n_seg,
                            a.period, tx);

        RQ_CLK(3);   // B controller
        // max_events: the tile keeps the events numbered below it, the replica ends here
        if (a.max_events >= 0 && truncate_tile(a.max_events, n_events, n, act, tt, tj, ownm, ot, opt_next))
            fin = true;
        // ---- C: aggregates after each event ----
        const bool own_b = act && ((ownm >> lane) & 1ull);       // controller post before #lane
        if (a.ev_t) {
            // event log (t, stream): lane q's post (if any) then its arrival, in tile order
            const int64_t pp = n_events + lane + mbcnt64(ownm);
            const int64_t pw = pp + (own_b ? 1 : 0);
            double* Et = a.ev_t + o * a.ev_cap;
            int32_t* Es = a.ev_src + o * a.ev_cap;
            if (own_b && pp < a.ev_cap) {
                Et[pp] = ot;
                Es[pp] = a.ctrl_idx;
            }
            if (act && pw < a.ev_cap) {
                Et[pw] = tt;
                Es[pw] = tj;
            }
            if (n_events + n + __popcll(ownm) > a.ev_cap) status |= RQ_ST_ROWS_OVERFLOW;
        }
        const bool strm_own = act && !opt && tj == a.ctrl_idx;   // controlled stream's arrival
        const bool has_o = own_b && a.n_fol > 0;
        const bool has_w = act && e1 > e0;
        int64_t osum = 0, wsum = 0;
        int oval = 0, wval = 0;
        int ocnt[NK], wcnt[NK];
#pragma unroll
        for (int kq = 0; kq < NK; ++kq) ocnt[kq] = wcnt[kq] = 0;
        if (a.dbg == 1) {
            // profiling only: skip phase C
        } else if (BITS) {
            // segments of the tile start at its own events (posts / own-stream arrivals)
            const bool rst = own_b || strm_own;
            const uint64_t rm = __ballot(rst);
            const bool hasr = mbcnt64_incl(rm) != 0;   // own event at or before #lane
            const bool wl = act && !strm_own;                        // a wall event
            const int deg = wl ? e1 - e0 : 0;
            const int odv = wl ? od : 0;
            SegFlags sf;
            sf.init(rst);
            // sumR / sumF: wall adds deg / odf, an own event drops sumF from sumR
            const int pdeg = (int)wave_scan_add((uint32_t)deg);
            const int64_t sfq = (int64_t)(int)sf.scan_add((uint32_t)odv) + (hasr ? 0 : agb.sumF);
            int64_t dec = 0;
            for (uint64_t b = rm; b; b &= b - 1) {
                const int r = __ffsll((unsigned long long)b) - 1;
                const int64_t D = r == 0 ? agb.sumF : bcast_i64(sfq, r - 1);
                if (lane >= r) dec += D;
            }
            wsum = agb.sumR + pdeg - dec;
            osum = agb.sumR + (pdeg - deg) - dec;
            // sink bitsets, one word at a time, every event of the tile at once; F and T
            // words come from LDS broadcasts, the mask row of a non-wall lane is the zero
            // row n_str, and the tile's last lane stores the new T word
            const bool vfull = agb.nvalid == a.n_sinks;
            const int last = n - 1;
            const uint32_t* mr = msk + (wl ? tj : a.n_str) * ms;
            const bool wlast = lane == last;
            int cw = 0, vw = 0, vo = 0;
            uint32_t nV = agb.V;
            if (BLK && vfull) {
                // event-blocked (BlkFlags): lane 16 b + g takes events 4g .. 4g + 3 for the
                // CB words of column block b.  The events' mask rows (word offsets into msk,
                // the zero row for a lane without a wall event) go through the wave's stage
                // area, which the merged instances do not use otherwise.
                const int CB = RQ_BLK_CB(a.nw);
                // the lane id opaque at each tile, so that what derives from it here is not
                // hoisted out of the tile loop and spilled
                int ln = lane;
                __asm__ volatile("" : "+v"(ln));
                int* st_r = reinterpret_cast<int*>(wb + a.lds_stage_off);
                st_r[ln] = (wl ? tj : a.n_str) * ms;
                wave_lds_sync();
                const int g4 = ln & 15, cb0 = (ln >> 4) * CB;
                const int4 ro = *reinterpret_cast<const int4*>(st_r + 4 * g4);
                BlkFlags bf;
                bf.init(rm, ln);
                auto m0 = lds_opaque(reinterpret_cast<const uint2*>(msk + ro.x + cb0));
                auto m1 = lds_opaque(reinterpret_cast<const uint2*>(msk + ro.y + cb0));
                auto m2 = lds_opaque(reinterpret_cast<const uint2*>(msk + ro.z + cb0));
                auto m3 = lds_opaque(reinterpret_cast<const uint2*>(msk + ro.w + cb0));
                auto fb = lds_opaque(reinterpret_cast<uint4*>(ft + cb0));   // the block's F / T words
                // events past the tile's last have zero masks and start no segment, so the
                // union after the group's fourth event is the union after the last
                const bool wgrp = g4 == (last >> 2);
                uint32_t q0 = 0, q1 = 0, q2 = 0, q3 = 0;
                // one column: F / carried T word f, the four events' mask words; returns the
                // new T word.  Where event 0 is no head, group 0 ORs F & ~T into its mask:
                // the events before the first head then see F & ~u = T & ~(wall union), T <= F
                auto column = [&](uint2 f, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3)
                                  __attribute__((always_inline)) -> uint32_t {
                    w0 |= (f.x & ~f.y) & bf.kc;
                    uint32_t l0, l1, l2, l3, u0, u1, u2, u3;
                    bf.chain(0u, w0, w1, w2, w3, l0, l1, l2, l3);
                    bf.chain(bf.carry(l3), w0, w1, w2, w3, u0, u1, u2, u3);
                    q0 += __popc(f.x & ~u0);
                    q1 += __popc(f.x & ~u1);
                    q2 += __popc(f.x & ~u2);
                    const uint32_t t3 = f.x & ~u3;
                    q3 += __popc(t3);
                    return t3;
                };
                // two columns per trip (CB is even), their chains interleaved
                for (int c = 0; c < CB; c += 2, ++fb, ++m0, ++m1, ++m2, ++m3) {
                    const uint4 f = *fb;
                    const uint2 w0 = *m0, w1 = *m1, w2 = *m2, w3 = *m3;
                    const uint32_t ta = column(make_uint2(f.x, f.y), w0.x, w1.x, w2.x, w3.x);
                    const uint32_t tb = column(make_uint2(f.z, f.w), w0.y, w1.y, w2.y, w3.y);
                    if (wgrp) {
                        fb->y = ta;
                        fb->w = tb;
                    }
                }
                // q_k of lane 16 b + g: block b's part of event 4g + k's count.  Half swap and add:
                // rows 0-1 hold k = 0 (from q0, q1) and k = 2 (from q2, q3), rows 2-3 k = 1 and
                // k = 3, each over blocks b and b + 2; row swap and add: rows 0, 1, 2, 3 hold
                // k = 0, 2, 1, 3 over the four blocks; lane e then fetches event e's count
                const auto s01 = __builtin_amdgcn_permlane32_swap(q0, q1, false, false);
                const auto s23 = __builtin_amdgcn_permlane32_swap(q2, q3, false, false);
                const auto s4 = __builtin_amdgcn_permlane16_swap(s01[0] + s01[1], s23[0] + s23[1], false, false);
                const int src = (((ln & 1) << 1 | ((ln >> 1) & 1)) << 4) | (ln >> 2);
                cw = __builtin_amdgcn_ds_bpermute(src << 2, (int)(s4[0] + s4[1]));
            } else if (vfull) {
                // two words per trip (ft holds an even number of words, the pad word's F
                // and T are zero), their DPP chains interleaved
                for (int ww = 0; ww < a.nw; ww += 2) {
                    const uint2 f0 = ft[ww], f1 = ft[ww + 1];
                    const uint32_t u0 = sf.scan_or_z(mr[ww]);          // wall union since the segment start
                    const uint32_t u1 = sf.scan_or_z(mr[ww + 1]);
                    const uint32_t t0 = (hasr ? f0.x : f0.y) & ~u0;    // top-1 set after #lane
                    const uint32_t t1 = (hasr ? f1.x : f1.y) & ~u1;
                    cw += __popc(t0) + __popc(t1);
                    if (wlast) {
                        ft[ww].y = t0;
                        ft[ww + 1].y = t1;
                    }
                }
            } else {
                for (int ww = 0; ww < a.nw; ++ww) {
                    const uint2 fw2 = ft[ww];
                    const uint32_t m = mr[ww];
                    const uint32_t u = sf.scan_or_z(m);
                    const uint32_t tq = (hasr ? fw2.x : fw2.y) & ~u;
                    cw += __popc(tq);
                    if (wlast) ft[ww].y = tq;
                    const uint32_t Vw = (uint32_t)__builtin_amdgcn_readlane((int)agb.V, ww);
                    const uint32_t x = wave_scan_or(m);
                    const uint32_t vq = Vw | x | (hasr ? fw2.x : 0u);  // valid set after #lane
                    vw += __popc(vq);
                    const uint32_t xe = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x138, 0xF, 0xF, false);
                    vo += __popc(Vw | xe | fw2.x);                     // after the post before #lane
                    nV = (uint32_t)wlane((int)nV, __builtin_amdgcn_readlane((int)vq, last), ww);
                }
            }
            wcnt[0] = cw;
            ocnt[0] = a.n_fol;   // a post puts every follower at rank 0
            wval = vfull ? a.n_sinks : vw;
            oval = vfull ? a.n_sinks : vo;
            if (n > 0) {
                if (!vfull) {
                    agb.V = nV;
                    agb.nvalid = bcast_i(vw, last);
                }
                agb.sumR = bcast_i64(wsum, last);
                agb.sumF = bcast_i64(sfq, last);
            }
        } else {
            for (int q = 0; q < n; ++q) {
                if ((ownm >> q) & 1ull) {
                    ag.own(rank, folat, a.n_fol, lane);
                    if (lane == q) {
                        osum = ag.sumR;
                        oval = ag.nvalid;
#pragma unroll
                        for (int kq = 0; kq < NK; ++kq) ocnt[kq] = ag.cnt[kq];
                    }
                }
                const int jw = bcast_i(tj, q);
                if (!opt && jw == a.ctrl_idx)
                    ag.own(rank, folat, a.n_fol, lane);
                else
                    ag.wall(rank, colat, bcast_i(e0, q), bcast_i(e1, q), bcast_i(od, q), lane);
                if (lane == q) {
                    wsum = ag.sumR;
                    wval = ag.nvalid;
#pragma unroll
                    for (int kq = 0; kq < NK; ++kq) wcnt[kq] = ag.cnt[kq];
                }
            }
        }
        RQ_CLK(4);   // C aggregates
        const uint64_t mo = __ballot(has_o), ma = mo | __ballot(has_w);
        n_events += n + __popcll(ownm);
        posts += __popcll(mo) + __popcll(__ballot(has_w && strm_own));
        world += __popcll(__ballot(has_w && !strm_own));
        if (ma && place_rows<NK, DEFER, PK>(rs, ma, has_o, has_w, ot, tt, osum, oval, ocnt, wsum, wval, wcnt, status))
            stop = true;
        RQ_CLK(5);   // rows
        if (stop || fin) break;
    }
    if constexpr (DEFER) rs.flush_pend();
#ifdef RQ_PHASE_CLOCK
    if (lane == 0 && a.clk)
        for (int q = 0; q < 8; ++q) atomicAdd(&a.clk[q], ck[q]);
#endif
    if (BITS) agb.T = lane < a.nw ? ft[lane].y : 0u;   // the top-1 set back in its lane words
    // the controller's last post after the final arrival (or the tile max_events cut)
    if (!stop && opt && opt_next <= a.end && (a.max_events < 0 || n_events < a.max_events)) {
        if (a.ev_t && lane == 0) {
            if (n_events < a.ev_cap) {
                a.ev_t[o * a.ev_cap + n_events] = opt_next;
                a.ev_src[o * a.ev_cap + n_events] = a.ctrl_idx;
            } else {
                status |= RQ_ST_ROWS_OVERFLOW;
            }
        }
        ++n_events;
        if (BITS) {
            agb.own();
            agb.sync();
            ag.sumR = agb.sumR;
            ag.nvalid = agb.nvalid;
            ag.cnt[0] = agb.cnt[0];
        } else {
            ag.own(rank, folat, a.n_fol, lane);
        }
        if (a.n_fol > 0) {
            ++posts;
            int64_t rr = rs.nrow;
            if (rs.nrow > 0 && opt_next == rs.last_t) {
                status |= RQ_ST_TIE;
                rr = rs.nrow - 1;
            } else if (rs.nrow >= rs.cap) {
                status |= RQ_ST_ROWS_OVERFLOW;
                rr = -1;
            } else {
                ++rs.nrow;
                rs.s0 = rs.nrow;
                rs.last_t = opt_next;
            }
            if (rr >= 0 && lane == 0) {
                rs.write(rr, opt_next, (double)ag.sumR, ag.nvalid, ag.cnt);
            }
        }
    }
    if (BITS) {
        agb.sync();
        ag.nvalid = agb.nvalid;
    }
    if (lane == 0) {
        int64_t* cnto = a.counts + o * 4;
        cnto[0] = posts;
        cnto[1] = world;
        cnto[2] = n_events;
        cnto[3] = rs.nrow;
        a.sall[rl] = ag.nvalid;
        if (rs.nrow == 0) status |= RQ_ST_EMPTY;
        if (status) atomicOr(&a.status[o], status);
    }
    if constexpr (SCAN)   // PK: a record is two doubles of rows_t
        fw_scan_rows<NK, PK>(rs.nrow, (double)ag.nvalid, a.end, a.rows_t + (PK ? 2 : 1) * rbase, a.rows_sum + rbase,
                             a.rows_valid + rbase, a.rows_cnt + rbase * NK, reinterpret_cast<double*>(wb),
                             a.metrics + o * (NK + 2));
    if (!a.wq) break;
    int nx = 0;
    if (lane == 0) nx = atomicAdd(a.wq, 1);
    qi = nslot + __builtin_amdgcn_readfirstlane(nx);
    }   // replica loop
}

template <int NK, class COL, int W, int H, bool BITS, bool PW = false, bool MRG = false>
__global__ __launch_bounds__(1024) void rq_sweep_fw(SweepArgs a)
{
    sweep_fw_body<NK, COL, W, H, BITS, PW, MRG>(a);
}
// the merged-stream instances: no generator state, so a tighter VGPR budget buys waves
// (RQ_FWM_WPE waves per SIMD; the planner picks the block size that fills them)
#ifndef RQ_FWM_WPE
#define RQ_FWM_WPE 4
#endif
template <int NK, class COL, bool BITS, bool PAIR = false, bool SCAN = false, bool BLK = false, bool PK = false>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(RQ_FWM_WPE))) void rq_sweep_fwm(SweepArgs a)
{
    sweep_fw_body<NK, COL, 16, 8, BITS, false, true, PAIR, SCAN, BLK, PK>(a);
}

// ============================================================================
// launch wrappers
// ============================================================================
// ---- the fused instance of a SweepInst: the one list of instances ----
// generated arrivals: rings of W, a register window of H, (W, H) in {(32, 8), (16, 8), (8, 4)}
template <class COL, int W, bool PW = false>
static SweepKernel fw_nk(int nK)
{
    constexpr int H = W > 16 ? 8 : W / 2;
    switch (nK) {
    case 1: return rq_sweep_fw<1, COL, W, H, false, PW>;
    case 2: return rq_sweep_fw<2, COL, W, H, false, PW>;
    case 3: return rq_sweep_fw<3, COL, W, H, false, PW>;
    default: return rq_sweep_fw<4, COL, W, H, false, PW>;
    }
}
template <class COL, bool PAIR, bool SCAN>
static SweepKernel fwm_nk(int nK)
{
    switch (nK) {
    case 1: return rq_sweep_fwm<1, COL, false, PAIR, SCAN>;
    case 2: return rq_sweep_fwm<2, COL, false, PAIR, SCAN>;
    case 3: return rq_sweep_fwm<3, COL, false, PAIR, SCAN>;
    default: return rq_sweep_fwm<4, COL, false, PAIR, SCAN>;
    }
}
// the merged instances: (call pairs) x (the sweep's own scan); the sink-bit ones x (phase C
// event-blocked); the scanning K = 1 ones x (16-byte rows)
template <bool PAIR, bool SCAN>
static SweepKernel fwm_kernel(const SweepInst& i)
{
    if (i.blk && !i.bits) return nullptr;
    if (i.pk) {
        if constexpr (SCAN) {
            if (i.nK != 1) return nullptr;
            if (i.bits)
                return i.blk ? rq_sweep_fwm<1, uint16_t, true, PAIR, true, true, true>
                             : rq_sweep_fwm<1, uint16_t, true, PAIR, true, false, true>;
            // int columns mean more than 65535 sinks, which the record's 16-bit fields exclude
            return i.col16 ? rq_sweep_fwm<1, uint16_t, false, PAIR, true, false, true> : nullptr;
        } else {
            return nullptr;
        }
    }
    if (i.bits)
        return i.blk ? rq_sweep_fwm<1, uint16_t, true, PAIR, SCAN, true> : rq_sweep_fwm<1, uint16_t, true, PAIR, SCAN>;
    return i.col16 ? fwm_nk<uint16_t, PAIR, SCAN>(i.nK) : fwm_nk<int, PAIR, SCAN>(i.nK);
}
// null: no such instance
static SweepKernel fw_kernel(const SweepInst& i)
{
    if (i.mrg) {   // merged streams (RedQueen / Poisson / replayed controllers)
        if (i.pw) return nullptr;
        if (i.pair)   // the RedQueen controller's draws by call pairs
            return i.scan ? fwm_kernel<true, true>(i) : fwm_kernel<true, false>(i);
        return i.scan ? fwm_kernel<false, true>(i) : fwm_kernel<false, false>(i);
    }
    // call pairs, the sweep's own scan, event-blocked phase C, 16-byte rows: the merged instances only
    if (i.pair || i.scan || i.blk || i.pk) return nullptr;
    // OptPWSignificance (PW) instances exist for uint16 columns and W = 16 only (make_plan
    // keeps other PW runs off this path)
    if (i.pw) {
        if (!i.col16 || i.W != 16) return nullptr;
        return i.bits ? rq_sweep_fw<1, uint16_t, 16, 8, true, true> : fw_nk<uint16_t, 16, true>(i.nK);
    }
    if (i.bits)   // 32-deep rings: this K = 1 bitset instance only
        return i.W == 32 ? rq_sweep_fw<1, uint16_t, 32, 8, true>
             : i.W == 16 ? rq_sweep_fw<1, uint16_t, 16, 8, true> : rq_sweep_fw<1, uint16_t, 8, 4, true>;
    if (i.W == 16) return i.col16 ? fw_nk<uint16_t, 16>(i.nK) : fw_nk<int, 16>(i.nK);
    return i.col16 ? fw_nk<uint16_t, 8>(i.nK) : fw_nk<int, 8>(i.nK);
}

// ---- the leaf operations on an instance ----
static int occ_fw_t(SweepKernel k, int wpb, size_t lds)
{
    return rq_occupancy(k, 64 * wpb, lds);
}
static hipError_t launch_fw_t(SweepKernel k, const SweepArgs& a, hipStream_t s)
{
    unsigned blocks = (unsigned)((a.n_chunk + a.wpb - 1) / a.wpb);
    if (a.wq) {
        // persistent grid: every resident wave slot once, the rest from the queue
        const int nb = occ_fw_t(k, a.wpb, a.lds_total);
        const unsigned cap = (unsigned)(nb > 0 ? nb : 1) * (unsigned)rq_cu_count();
        if (cap < blocks) blocks = cap;
    }
    hipLaunchKernelGGL(k, dim3(blocks), dim3(64 * a.wpb), a.lds_total, s, a);
    return hipGetLastError();
}

hipError_t rq_launch_sweep_fw(const SweepArgs& a, const SweepInst& i, hipStream_t s, size_t rows16_bytes)
{
    if (a.n_chunk <= 0) return hipSuccess;
    if (i.pair && a.ctrl_kind != RQ_SRC_OPT) return hipErrorInvalidValue;
    // the sweep's own scan: its LDS inside the wave's area, no event log or max_events cut
    if (i.scan && (!a.metrics || a.ev_t || a.max_events >= 0 || a.lds_wave_stride < RQ_FWS_LDS_BYTES(i.nK)))
        return hipErrorInvalidValue;
    // event-blocked phase C: the planner's row stride (8-byte reads of a block's words)
    if (i.blk && a.mstride != RQ_BLK_MSTRIDE(a.nw)) return hipErrorInvalidValue;
    // 16-byte rows: the records of the launch's replicas, 16 * n_chunk * cap_rows bytes from a
    // 16-byte-aligned rows_t, inside the rows16_bytes the caller has there, and fields that
    // hold every value (rqh::rows16_fits)
    if (i.pk && (!a.rows_t || ((uintptr_t)a.rows_t & 15) != 0 ||
                 (uint64_t)rows16_bytes < (uint64_t)16 * (uint64_t)a.n_chunk * (uint64_t)a.cap_rows ||
                 !rqh::rows16_fits(i.nK, a.n_sinks, a.mrg_stride)))
        return hipErrorInvalidValue;
    const SweepKernel k = fw_kernel(i);
    return k ? launch_fw_t(k, a, s) : hipErrorInvalidValue;
}

int rq_fw_blocks_per_cu(const SweepInst& i, int wpb, size_t lds)
{
    const SweepKernel k = fw_kernel(i);
    return k ? occ_fw_t(k, wpb, lds) : -1;
}

// rq_plan.cpp -- the planner of rq_run_batch (rq_host.h): every sweep instance, LDS
// layout, the chunking and the workspace layout of a batch, and the one reader of the
// environment knobs.  Host arithmetic only; the device is asked through
// rq_sweep_blocks_per_cu, rq_fw_blocks_per_cu and rq_cu_count.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "rq_host.h"
#include "rq_tables.h"

namespace rqh {

Knobs read_knobs()
{
    Knobs k;
    if (const char* e = getenv("RQ_WS_BUDGET_GB")) k.ws_budget_gb = {true, atof(e)};
    if (const char* e = getenv("RQ_CAP_SQUEEZE")) k.cap_squeeze = std::max(0.01, std::min(1.0, atof(e)));
    if (const char* e = getenv("RQ_MG_GRP")) k.mg_grp = {true, atoi(e)};
    if (const char* e = getenv("RQ_MRG")) k.mrg = atoi(e) != 0;
    if (const char* e = getenv("RQ_G_COLLDS")) k.g_collds = {true, atoi(e)};
    if (const char* e = getenv("RQ_G_W")) k.g_w = atoi(e);
    if (const char* e = getenv("RQ_SKIP")) k.skip = atoi(e) != 0;
    if (const char* e = getenv("RQ_FWM")) k.fwm = atoi(e) != 0;
    if (const char* e = getenv("RQ_CTRL_DRAWS")) k.ctrl_draws = atoi(e) != 0;
    if (const char* e = getenv("RQ_SWEEP_SCAN")) k.sweep_scan = atoi(e) != 0;
    if (const char* e = getenv("RQ_ROWS_PACKED")) k.rows_packed = atoi(e) != 0;
    if (const char* e = getenv("RQ_GEN_SPLIT")) k.gen_split = atoi(e) != 0;
    if (const char* e = getenv("RQ_PHASEC_BLK")) k.phasec_blk = atoi(e) != 0;
    if (const char* e = getenv("RQ_FW_W")) k.fw_w = atoi(e);
    if (const char* e = getenv("RQ_PIPE")) k.pipe = std::max(1, std::min(3, atoi(e)));
    if (const char* e = getenv("RQ_PIPE_CHUNK")) k.pipe_chunk = {true, std::max<int64_t>(64, atoll(e))};
    if (const char* e = getenv("RQ_ORDER")) k.order = atoi(e) != 0;
    if (const char* e = getenv("RQ_SWEEP_DBG")) k.sweep_dbg = atoi(e);
    if (const char* e = getenv("RQ_FW_TILE")) k.fw_tile = atof(e);
    if (const char* e = getenv("RQ_FW_HMIN")) k.fw_hmin = {true, atoi(e)};
    if (const char* e = getenv("RQ_FW_THR")) k.fw_thr = {true, atoi(e)};
    if (const char* e = getenv("RQ_FW_HFILL")) k.fw_hfill = {true, atoi(e)};
    static const int fw_static = getenv("RQ_FW_STATIC") ? atoi(getenv("RQ_FW_STATIC")) : 0;
    k.fw_static = fw_static;
    k.clk_merge = getenv("RQ_CLK_MERGE") != nullptr;
    if (const char* e = getenv("RQ_RP_CHUNK")) k.rp_chunk = {true, atoi(e)};
    if (const char* e = getenv("RQ_RP_SMALL")) k.rp_small = atoi(e) != 0;
    k.clk_replay = getenv("RQ_CLK_REPLAY") != nullptr;
    if (const char* e = getenv("RQ_LM_OF_SLOTS")) k.lm_of_slots = std::max(1, std::min(4096, atoi(e)));
    return k;
}

namespace {

constexpr size_t kLdsMax = 160 * 1024;

double stream_mean_var(const GraphTopo* g, int j, int kind, const rq_batch_desc* b, double* var)
{
    const double span = g->end - g->start;
    double m = 0.0;
    *var = 0.0;
    switch (kind) {
    case RQ_SRC_POISSON:
    case RQ_SRC_POISSON2: {
        const double rate = j == g->ctrl_idx ? b->ctrl_rate_max : g->p0[j];
        m = std::max(0.0, rate) * span;
        *var = m;
        break;
    }
    case RQ_SRC_HAWKES: {
        const double l0 = g->p0[j], al = g->p1[j], be = g->p2[j];
        const double br = be > 0.0 ? al / be : 1.0;
        if (br < 0.95) {
            m = l0 * span / (1.0 - br);
            *var = l0 * span / ((1.0 - br) * (1.0 - br) * (1.0 - br));
        } else {
            m = l0 * span * 40.0 + 1000.0;
            *var = m * m;
        }
        break;
    }
    case RQ_SRC_PWCONST: {
        const int off = g->arr_off[j], n = g->arr_n[j];
        for (int k = 0; k < n; ++k) {
            const double lo = std::max(g->arr_a[off + k], g->start);
            const double hi = std::min(k + 1 < n ? g->arr_a[off + k + 1] : g->end, g->end);
            if (hi > lo) m += std::max(0.0, g->arr_b[off + k]) * (hi - lo);
        }
        *var = m;
        break;
    }
    case RQ_SRC_REALDATA:
        m = g->arr_n[j];
        *var = 0.0;
        break;
    default:
        break;
    }
    return m;
}

// The sweep instance of a plan -- or of a candidate the LDS searches of make_plan score:
// what a search is still deciding (sweep kind, ring depth, column placement, GS, GT) comes
// as arguments, the rest from the plan so far.
SweepInst sweep_inst(const Plan& p, int ctrl_kind, bool fused, int W, bool col16, bool gs, bool gt)
{
    SweepInst i{};
    i.fused = fused;
    i.nK = p.nK;
    i.col16 = col16;
    i.log = p.log;
    i.gs = gs;
    i.bits = p.bits;
    i.bl = p.bl;
    i.mrg = fused ? p.fwm : p.mrg;
    i.spl = p.spl;
    i.W = W;
    i.gt = gt;
    i.pw = ctrl_kind == RQ_SRC_OPTPW;   // exactly the runs rq_run_batch gives SweepArgs.pw_c
    i.pair = fused && i.mrg && p.pair;
    i.scan = fused && i.mrg && p.scan;
    i.blk = fused && i.mrg && p.blk;
    i.pk = i.scan && p.rows16;
    return i;
}
int sweep_blocks_per_cu(const SweepInst& i, int wpb, size_t lds)
{
    return i.fused ? rq_fw_blocks_per_cu(i, wpb, lds) : rq_sweep_blocks_per_cu(i, wpb, lds);
}

// the buffer layout of one chunk plan (p->chunk, p->nbuf): offsets and p->total
void plan_layout(const GraphTopo* g, const rq_batch_desc* b, Plan* p);

// make_plan, part 1: the call's arguments, its replica window and per-replica RealData
int plan_args(const GraphTopo* g, const rq_batch_desc* b, Plan* p)
{
    if (!b) return RQ_EINVAL;
    if (b->nK < 1 || b->nK > RQ_MAX_K || !b->Ks) return RQ_EINVAL;
    if (b->n_grid < 1 || b->n_rep < 1) return RQ_EINVAL;
    const int ck = b->ctrl_kind;
    if (ck != RQ_SRC_OPT && ck != RQ_SRC_OPTPW && ck != RQ_SRC_POISSON2 && ck != RQ_SRC_PWCONST &&
        ck != RQ_SRC_REALDATA && ck != RQ_SRC_NONE)
        return RQ_EINVAL;
    if (ck == RQ_SRC_OPT && (!b->q || (g->n_fol > 0 && !b->s))) return RQ_EINVAL;
    if (ck == RQ_SRC_OPTPW &&
        (!b->q || b->n_seg < 1 || b->n_seg > 4096 || !(b->period > 0.0) || (g->n_fol > 0 && !b->s_pw)))
        return RQ_EINVAL;
    if (ck == RQ_SRC_POISSON2 && !b->ctrl_rate) return RQ_EINVAL;
    if ((ck == RQ_SRC_PWCONST) && g->ctrl_arr_n < 1) return RQ_EINVAL;
    p->nK = b->nK;
    // the call's replica space: the [rep_lo, rep_lo + rep_cnt) window of every grid point
    if (b->rep_cnt < 0 || (b->rep_cnt > 0 && (b->rep_lo < 0 || b->rep_lo + b->rep_cnt > b->n_rep)))
        return RQ_EINVAL;
    p->rep_lo = b->rep_cnt > 0 ? b->rep_lo : 0;
    p->rep_cnt = b->rep_cnt > 0 ? b->rep_cnt : b->n_rep;
    const int64_t Rall = (int64_t)b->n_grid * p->rep_cnt;
    if (b->replica0 < 0 || b->n_local < 0 || b->replica0 + b->n_local > Rall) return RQ_EINVAL;
    p->R = b->n_local > 0 ? b->n_local : Rall - b->replica0;
    if (p->R < 1) return RQ_EINVAL;
    // a replica list (ABI v6): n_local global ids of the whole n_grid x n_rep grid
    if (b->rep_idx) {
        if (b->replica0 != 0 || b->rep_cnt != 0 || b->n_local < 1) return RQ_EINVAL;
        const int64_t nall = (int64_t)b->n_grid * b->n_rep;
        for (int64_t k = 0; k < b->n_local; ++k)
            if (b->rep_idx[k] < 0 || b->rep_idx[k] >= nall) return RQ_EINVAL;
    }
    p->chunk = b->chunk > 0 ? std::min<int64_t>(b->chunk, p->R) : std::min<int64_t>(p->R, 16384);
    p->cap.assign(g->n_str, 0);
    p->st_off.assign(g->n_str, 0);
    p->rd_k.assign(g->n_str, -1);
    if (b->n_rd < 0 || b->n_rd > RQ_MAX_RD) return RQ_EINVAL;
    if (b->n_rd > 0) {
        if (!b->rd_src_id || !b->rd_cap || !b->rd_times || !b->rd_off) return RQ_EINVAL;
        for (int k = 0; k < b->n_rd; ++k) {
            int jk = -1;
            for (int j = 0; j < g->n_str; ++j)
                if (g->src_id[j] == b->rd_src_id[k]) jk = j;
            // a RealData wall source of the graph, named once
            if (jk < 0 || jk == g->ctrl_idx || g->kind[jk] != RQ_SRC_REALDATA || p->rd_k[jk] >= 0 ||
                b->rd_cap[k] < 0 || b->rd_cap[k] > ((int64_t)1 << 30))
                return RQ_EINVAL;
            p->rd_k[jk] = k;
        }
    }
    return RQ_OK;
}

// make_plan, part 2: per-stream, merged-sequence and pivot-row capacities
int plan_capacities(const GraphTopo* g, const rq_batch_desc* b, const Knobs& kn, Plan* p)
{
    const int ck = b->ctrl_kind;
    const double scale = b->cap_scale >= 1.0 ? b->cap_scale : 1.0;
    double wall_caps = 0.0, wall_mean = 0.0, wall_var = 0.0;
    int64_t ctrl_cap = 0;
    for (int j = 0; j < g->n_str; ++j) {
        int kind = g->kind[j];
        if (j == g->ctrl_idx)
            kind = (ck == RQ_SRC_OPT || ck == RQ_SRC_OPTPW || ck == RQ_SRC_NONE) ? RQ_SRC_NONE : ck;
        double var;
        const double m = stream_mean_var(g, j, kind, b, &var);
        int64_t c = 0;
        if (kind != RQ_SRC_NONE)
            c = kind == RQ_SRC_REALDATA ? (p->rd_k[j] >= 0 ? b->rd_cap[p->rd_k[j]] : (int64_t)m)
                                        : (int64_t)std::ceil((m + 8.0 * std::sqrt(var) + 32.0) * scale);
        if (c > (int64_t)1 << 30) return RQ_EINVAL;
        c = (c + 15) & ~(int64_t)15;   // whole 128-byte lines: the merge's loads, the generator's stores
        p->cap[j] = (int)c;
        p->st_off[j] = p->capsum;
        p->capsum += c;
        if (j == g->ctrl_idx) {
            ctrl_cap = c;
        } else {
            wall_caps += (double)c;
            if (kind != RQ_SRC_NONE) {
                wall_mean += kind == RQ_SRC_REALDATA ? (double)c : m;
                wall_var += var;
            }
        }
    }
    // the wall events of a replica together: mean + 8 sigma of their SUM (the streams'
    // own 8-sigma capacities add up to far more: C5 769k against 511k); a replica past it
    // is flagged (RQ_ST_STREAM_OVERFLOW / RQ_ST_ROWS_OVERFLOW) and Graph.run(check=True)
    // reruns the batch with doubled capacities
    const double squeeze = kn.cap_squeeze;   // tests only: undersized capacities exercise the overflow reruns
    const double walls_agg = std::ceil((wall_mean + 8.0 * std::sqrt(wall_var) + 32.0) * scale * squeeze);
    const bool opt_ctrl = ck == RQ_SRC_OPT || ck == RQ_SRC_OPTPW;
    // merged sequence per replica: every arrival of every stream (the controlled one too)
    p->mrg_stride = std::min<int64_t>(p->capsum, ((int64_t)walls_agg + ctrl_cap + 64 + 15) & ~(int64_t)15);
    // pivot rows <= events: walls + posts; RedQueen posts at most once per wall event (+1),
    // so the old bound was 2 x the walls; posts are sized max(4096, walls / 4) now (C3: ~180
    // per replica, C5: ~1400; the C4 grid's q = 1e-4 corner: 1816 on 2075 walls)
    double rows = wall_caps + (opt_ctrl ? wall_caps + 1.0 : (double)ctrl_cap) + 8.0;
    rows = std::min(rows, walls_agg + (opt_ctrl ? std::max(4096.0, std::ceil(walls_agg / 4.0)) + 1.0
                                                : (double)ctrl_cap) + 8.0);
    if (b->max_events >= 0) rows = std::min(rows, (double)b->max_events + 1.0);
    // a multiple of 32 rows: replica row bases stay aligned to the scan's 32-row trips
    p->cap_rows = (std::max<int64_t>(64, (int64_t)rows) + 31) & ~(int64_t)31;
    return RQ_OK;
}

// the sweep variant of a make_plan pass, p->log decided: sources per lane, K = 1 sink
// bits, merged streams and the merge's groups
void plan_variant(const GraphTopo* g, const rq_batch_desc* b, const Knobs& kn, Plan* p)
{
    // the sequential sweep owns <= 32 sources per lane; past that it plays the merged
    // (t, stream) sequence of rq_merge_streams like the fast general sweep
    p->lmrg = p->log && g->n_str > RQ_MAX_STREAMS;
    if (p->log) p->spl = g->n_str <= 64 ? 1 : g->n_str <= 512 ? 8 : g->n_str <= 1024 ? 16 : 32;
    p->mstride = g->nw | 1;   // odd row stride: one LDS bank per stream for a given word
    p->bits = !p->log && p->nK == 1 && b->Ks[0] == 1 && g->nw > 0 && b->sweep_mode != 3 &&
              (size_t)g->n_str * p->mstride * 4 <= 64 * 1024;
    if (p->bits) p->spl = g->n_str <= 64 ? 1 : g->n_str <= 128 ? 2 : g->n_str <= 256 ? 4 : 8;
    p->bl = !p->log && !p->bits && p->nK == 1 && b->Ks[0] == 1 && p->spl >= 2 && b->sweep_mode != 3;
    // K = 1 with too many sinks for int16 ranks in LDS (> 24k): per-wave sink BITS, which
    // exist for 2+ sources per lane (lanes past the sources idle)
    if (!p->log && !p->bits && !p->bl && p->nK == 1 && b->Ks[0] == 1 && b->sweep_mode != 3 &&
        2 * (size_t)p->n_sinks_pad > 48 * 1024) {
        p->spl = std::max(p->spl, 2);
        p->bl = true;
    }
    p->gs = false;
    // the fast general sweep plays the merged (t, stream) sequence: the merge kernel reads
    // every stream line once (one source per thread, <= RQ_MG_B sources)
    p->mrg = (!p->log && b->sweep_mode != 6) || p->lmrg;
    // > RQ_MG_B sources: two levels; groups of 64 streams (one-wave first-level blocks) while
    // <= 64 of them cover the graph, so the second level walks up to 64 sequences a round
    // instead of 2-8 (600 sources: 2 groups of <= 512 -> 10 of <= 64)
    p->grp_sz = g->n_str <= 64 * 64 ? 64 : RQ_MG_B;
    if (kn.mg_grp.set)   // A/B only
        p->grp_sz = kn.mg_grp.v == 64 && g->n_str <= 64 * 64 ? 64 : RQ_MG_B;
    p->n_grp = g->n_str > RQ_MG_B ? (g->n_str + p->grp_sz - 1) / p->grp_sz : 1;
    p->mrg = p->lmrg || (p->mrg && kn.mrg);   // A/B only
}

// general sweep: pick (ring depth W, waves per block) for the most waves per CU; false:
// no layout of this variant fits LDS
bool plan_general_lds(const GraphTopo* g, const rq_batch_desc* b, const Knobs& kn, Plan* p)
{
    const int nwl = (g->n_sinks + 31) / 32;
    int best = -1;
    // sink columns live in LDS as uint16 when they fit, else they are read from
    // global memory as int (the kernel's COL type selects the path at compile time)
    // both placements are scored: LDS columns only win at equal waves per CU
    // LOG: the per-sink state in LDS, or (gs) in global memory for more sinks than fit
    // GT (merged streams only): the per-stream tables in global memory -- tried when no
    // layout with them in LDS fits, always for the sequential sweep on merged streams
    for (int gt = p->lmrg ? 1 : 0; gt <= (p->mrg ? 1 : 0) && best < 0; ++gt)
    for (int gs = 0; gs <= (p->log ? 1 : 0); ++gs)
    for (int col_lds = g->n_sinks <= 65535 && !(p->log && p->spl >= 16) && !gt ? 1 : 0; col_lds >= 0; --col_lds) {
        if (gt && p->bits) continue;   // the sink-bitset instances keep their tables in LDS
        if (kn.g_collds.set && kn.g_collds.v != col_lds) continue;   // tuning only: force the column placement
        const int c16 = col_lds;
        // BITS: sink bitsets [n_str][nw] replace the columns (and the per-wave ranks)
        const size_t colb = p->bits ? 4 * (size_t)g->n_str * p->mstride
                                    : (col_lds ? 2 * g->csr_col.size() : 0);
        size_t sh = 0;
        const size_t o_col = sh;  sh = align_up(sh + colb, 16);
        const size_t tabn = gt ? 0 : (size_t)g->n_str;
        const size_t o_ptr = sh;  sh = align_up(sh + 4 * (tabn + (gt ? 0 : 1)), 16);
        const size_t o_odf = sh;  sh = align_up(sh + 4 * tabn, 16);
        const size_t o_cbf = sh;  sh = align_up(sh + 4 * tabn, 16);
        const size_t o_fb = sh;   if (p->bl) sh = align_up(sh + 4 * (size_t)nwl, 16);
        // one grid point: the 1/c_j table once per block instead of once per wave
        const bool inv_sh = b->n_grid == 1 && !gt;
        const size_t o_inv = sh;  if (inv_sh) sh = align_up(sh + 8 * (size_t)g->n_str, 16);
        const int spl = p->spl;
        const int only_w = kn.g_w;   // tuning only
        // LOG: LDS rings of W = 8 per source (4 at 32 sources per lane); the fast sweep:
        // a register window of 4
        for (int W : {8, 4}) {
            if ((p->log ? (spl >= 32 ? 4 : 8) : 4) != W) continue;
            if (only_w && W != only_w) continue;
            const size_t r_off = inv_sh || gt ? 0 : align_up(8 * (size_t)g->n_str, 16);
            const size_t rank_b = p->log ? (gs ? 0 : 4) : (p->bits ? 0 : 2);   // fast: int16 saturating
            const SweepInst inst = sweep_inst(*p, b->ctrl_kind, false, W, c16, gs, gt);
            // BL: two bits per sink (T, V words) in place of the int16 ranks
            const size_t w_off = p->bl ? align_up(r_off + 8 * (size_t)nwl, 16)
                                       : align_up(r_off + rank_b * (size_t)p->n_sinks_pad, 16);
            // LOG: rings of W arrivals for each real source; fast: the tile's staging
            size_t stride = p->log && !p->lmrg ? align_up(w_off + 8 * (size_t)g->n_str * W, 16)
                                               : align_up(w_off + 64 * 12, 16);
            // LOG: per-sink gtag/gcnt/gsum (gs: in global memory) + a wave_npsum<1>
            // scratch (RQ_NPSUM1_LDS doubles)
            const size_t x_off = stride;
            if (p->log) stride = align_up(x_off + (gs ? 0 : 12 * (size_t)p->n_sinks_pad) + 8 * (size_t)RQ_NPSUM1_LDS, 16);
            for (int wpb : {16, 12, 10, 8, 6, 5, 4, 3, 2, 1}) {
                if (p->log && wpb > 4) continue;   // LOG instances: 256-thread blocks
                if (!p->log && !p->mrg && spl >= 4 && wpb > 8) continue;   // 512-thread instances
                if (p->mrg && 64 * wpb > RQ_MRG_LB) continue;
                const size_t tot = sh + wpb * stride;
                if (tot > kLdsMax) continue;
                // resident waves per CU: the runtime's occupancy for this instance
                // (VGPR/SGPR/LDS); without a device, the LDS bound capped at 16
                int blocks = sweep_blocks_per_cu(inst, wpb, tot);
                if (blocks <= 0) blocks = (int)std::min<size_t>(kLdsMax / tot, 16 / wpb);
                const int waves = blocks * wpb;
                // LDS columns skip the global latency; LDS sink state wherever it fits
                const int score = waves * 8 + col_lds * 2 + (gs ? 0 : 100000);
                if (score > best) {
                    best = score;
                    p->wpc = waves;
                    p->gs = gs;
                    p->gs_slots = std::min<int64_t>((int64_t)align_up((size_t)p->chunk, (size_t)wpb),
                                                    (int64_t)blocks * wpb * rq_cu_count());
                    p->gwin = W; p->gwpb = wpb; p->gcol_lds = col_lds; p->gcol16 = c16;
                    p->g_col = o_col; p->g_ptr = o_ptr; p->g_odf = o_odf; p->g_cbf = o_cbf;
                    p->g_wave = sh; p->g_wave_stride = stride; p->g_rank_off = r_off;
                    p->g_win_off = w_off; p->g_x_off = x_off; p->g_total = tot; p->g_fb = o_fb;
                    p->g_inv = o_inv; p->g_inv_sh = inv_sh; p->gt = gt;
                }
            }
        }
    }
    if (best < 0) return false;
    // BL on merged streams: a per-wave stamp (the reset epoch a stream last played in)
    // and first-lane table per stream let a tile skip the events whose stream already
    // played since the last post -- their sinks are out of the top-1 set and valid.
    // Only where it costs no resident waves.
    p->g_skip = 0;
    if (p->bl && p->mrg && !p->gs) {
        const size_t st2 = align_up(p->g_wave_stride + 8 * (size_t)g->n_str, 16);
        const size_t tot2 = p->g_wave + p->gwpb * st2;
        const SweepInst inst = sweep_inst(*p, b->ctrl_kind, false, p->gwin, p->gcol16, p->gs, p->gt);
        int blocks = tot2 <= kLdsMax ? sweep_blocks_per_cu(inst, p->gwpb, tot2) : 0;
        if (tot2 <= kLdsMax && blocks <= 0) blocks = (int)std::min<size_t>(kLdsMax / tot2, 16 / p->gwpb);
        const bool on = blocks * p->gwpb >= p->wpc && kn.skip;   // RQ_SKIP=0: A/B only
        if (on) {
            p->g_skip = p->g_wave_stride;
            p->g_wave_stride = st2;
            p->g_total = tot2;
        }
    }
    return true;
}

// fused windowed sweep: one stream per lane, rings of W arrivals generated in LDS,
// a window of H per ring in registers; (W, H, waves per block) for the most waves per CU
void plan_fused_lds(const GraphTopo* g, const rq_batch_desc* b, const Knobs& kn, Plan* p)
{
    const bool pw = b->ctrl_kind == RQ_SRC_OPTPW;
    p->fw = !p->log && !p->bl && g->n_str <= 64 && b->sweep_mode != 4 && b->sweep_mode != 5 &&
            b->sweep_mode != 6;
    p->fwm = p->fw && !pw && b->sweep_mode != 7;
    p->fwm = p->fwm && kn.fwm;   // A/B only
    p->pair = p->fwm && b->ctrl_kind == RQ_SRC_OPT;
    p->pair = p->pair && kn.ctrl_draws;   // A/B and tests
    p->scan = p->fwm && !(b->flags & RQ_RUN_EVENT_LOG) && b->max_events < 0;
    p->scan = p->scan && kn.sweep_scan;   // A/B and tests
    p->blk = p->fwm && p->bits && g->nw >= RQ_BLK_MIN_NW;
    p->blk = p->blk && kn.phasec_blk;   // A/B and tests
    // the mask rows' stride: the event-blocked phase C reads two words of a row at a time
    const int mstride = p->blk ? RQ_BLK_MSTRIDE(g->nw) : p->mstride;
    if (p->fw) {
        int best = -1;
        const int c16 = p->bits ? 1 : (g->n_sinks <= 65535 ? 1 : 0);
        if (pw && !c16) p->fw = false;   // OptPWSignificance fused instances: uint16 columns
        // BITS: sink bitsets [n_str + 1][mstride] (row n_str all zero: the mask of a
        // lane without a wall event) replace the columns
        const size_t colb = p->bits ? 4 * (size_t)(g->n_str + 1) * mstride
                                    : (c16 ? 2 * g->csr_col.size() : 0);
        size_t sh = 0;
        const size_t o_col = sh;  sh = align_up(sh + colb, 16);
        const size_t o_ptr = sh;  sh = align_up(sh + 4 * (g->n_str + 1), 16);
        const size_t o_odf = sh;  sh = align_up(sh + 4 * g->n_str, 16);
        const size_t o_cbf = sh;  sh = align_up(sh + 4 * g->n_str, 16);
        const size_t o_etab = sh; sh = align_up(sh + RQ_EXP_TAB_N * 8, 16);   // rq_exp's table
        const int only_w = kn.fw_w;   // tuning only
        for (int W : {32, 16, 8}) {
            if (!p->fw) break;
            if (only_w && W != only_w) continue;
            if (pw && W != 16) continue;
            if (W == 32 && !p->bits) continue;   // 32-deep rings: K = 1 bitset instance only
            const int H = W > 16 ? 8 : W / 2;    // register window
            const size_t r_off = align_up(8 * (size_t)g->n_str, 16);
            // per wave: BITS -> (F, T) word pairs [nw] (blk: of the four column blocks); else
            // int16 sink ranks
            const size_t ftw = p->blk ? 4 * (size_t)RQ_BLK_CB(g->nw) : (size_t)((g->nw + 1) & ~1);
            const size_t w_off = align_up(r_off + (p->bits ? 8 * ftw : 2 * (size_t)p->n_sinks_pad), 16);
            // merged streams: no arrival rings
            const size_t s_off = align_up(w_off + (p->fwm ? 0 : 8 * (size_t)g->n_str * (W + 1)), 16);
            size_t stride = align_up(s_off + 64 * 12, 16);
            // the sweep's own scan aliases the wave's area (dead after the tile loop)
            if (p->scan) stride = std::max(stride, align_up(RQ_FWS_LDS_BYTES(p->nK), 16));
            for (int wpb : {16, 12, 10, 8, 6, 5, 4, 3, 2, 1}) {
                const size_t tot = sh + wpb * stride;
                if (tot > kLdsMax) continue;
                int blocks = sweep_blocks_per_cu(sweep_inst(*p, b->ctrl_kind, true, W, c16, false, false), wpb, tot);
                if (blocks <= 0) blocks = (int)std::min<size_t>(kLdsMax / tot, 16 / wpb);
                const int waves = blocks * wpb;
                const int score = waves * 4 + (W == 16 ? 2 : W == 32 ? 1 : 0);
                if (score > best) {
                    best = score;
                    p->wpc = waves;
                    p->gwin = W; p->fw_h = H; p->gwpb = wpb; p->gcol_lds = c16; p->gcol16 = c16;
                    p->g_col = o_col; p->g_ptr = o_ptr; p->g_odf = o_odf; p->g_cbf = o_cbf;
                    p->g_wave = sh; p->g_wave_stride = stride; p->g_rank_off = r_off;
                    p->g_win_off = w_off; p->g_stage_off = s_off; p->g_x_off = 0; p->g_total = tot;
                    p->g_etab = o_etab;
                }
            }
        }
        if (best < 0) p->fw = false;
    }
    if (!p->fw) p->fwm = false;
    if (!p->fwm) p->pair = p->scan = p->blk = false;
    // the sweep's own rows as 16-byte records; the occupancy searches above score the array
    // instance (the records change no LDS byte and the instance is not heavier in registers)
    p->rows16 = p->scan && rows16_fits(p->nK, g->n_sinks, p->mrg_stride);
    p->rows16 = p->rows16 && kn.rows_packed;   // A/B and tests
    if (p->blk) p->mstride = mstride;
    if (p->fw) p->mrg = p->fwm;   // the merge kernel feeds the fused sweep too
}

}  // namespace

SweepInst sweep_inst(const Plan& p, int ctrl_kind)
{
    return sweep_inst(p, ctrl_kind, p.fw, p.gwin, p.gcol16, p.gs, p.gt);
}

void plan_info(const Plan& p, int ctrl_kind, int64_t info[9])
{
    info[0] = (p.log ? (p.gs ? 4 : 1) : (p.bits ? 2 : (p.bl ? 3 : 0))) + (p.fwm ? 20 : p.fw ? 10 : 0);
    info[1] = p.mrg ? 0 : p.spl;   // 0: merged streams (lanes own no sources)
    info[2] = p.gwin;
    info[3] = p.gwpb;
    info[4] = sweep_blocks_per_cu(sweep_inst(p, ctrl_kind), p.gwpb, p.g_total);
    info[5] = p.gcol_lds;
    info[6] = (int64_t)p.g_total;
    info[7] = p.chunk;
    info[8] = p.scan ? 1 : 0;
}

int make_plan(const GraphTopo& topo, const rq_batch_desc* b, const Knobs& kn, double budget, Plan* p)
{
    const GraphTopo* g = &topo;
    if (const int rc = plan_args(g, b, p)) return rc;
    if (const int rc = plan_capacities(g, b, kn, p)) return rc;
    const int ck = b->ctrl_kind;
    // Opt / OptPWSignificance with a duplicated controlled edge: the reference's follower
    // vectors (sqrt_s_by_q, old_ranks: one entry per edge) no longer match the ranks (one
    // per distinct follower) and its first non-own event raises ValueError
    if (g->ctrl_dup && (ck == RQ_SRC_OPT || ck == RQ_SRC_OPTPW)) return RQ_EINVAL;
    if (g->n_str > RQ_MAX_STREAMS_MRG) return RQ_EUNSUPPORTED;
    p->spl = g->n_str <= 64 ? 1 : g->n_str <= 128 ? 2 : g->n_str <= 256 ? 4 : 8;
    p->n_sinks_pad = (g->n_sinks + 1) | 1;   // odd stride: spreads replicas over LDS banks
    const size_t per_wave = (size_t)p->n_sinks_pad * 4;
    p->wpb = per_wave * 4 <= 64 * 1024 ? 4 : per_wave * 2 <= 80 * 1024 ? 2 : 1;

    // the sequential exact variant when equal event times are certain: the graph's own
    // RealData times (every replica plays them) repeat a time; otherwise RealData and
    // the per-replica plugin streams play on the fast sweeps, which flag RQ_ST_TIE on any
    // equal-time pair, and the caller reruns the flagged replicas on the exact sequential
    // sweep (rq_batch_desc.rep_idx).  max_events cuts the fast sweeps' tiles
    // (truncate_tile); the fast sweeps write the event log themselves.
    const bool rd_ties = ck == RQ_SRC_REALDATA ? g->rd_ties_ctrl : g->rd_ties;
    p->log = b->sweep_mode == 2 || (rd_ties && b->sweep_mode != 1 && b->sweep_mode != 5);
    for (int q = 0; q < b->nK; ++q) p->log = p->log || b->Ks[q] > 32767;   // int16 ranks
    // a multigraph (duplicate edges make fractional pivot cells, the exact sequential
    // sweep's business); > 512 sources: the fast general sweep plays the two-level merged
    // sequence (rq_merge_streams per group of 512, then over the groups), the windowed
    // sweep (mode 6) owns <= 8 sources per lane
    p->log = p->log || g->multi || (g->n_str > 512 && b->sweep_mode == 6);

    // a graph no fast instance takes goes to the exact sequential sweep: one further pass
    // with p->log set; a sequential pass that fits nothing ends the loop
    for (;;) {
        plan_variant(g, b, kn, p);
        // without the merged streams the windowed sweep owns <= 8 sources per lane
        const bool too_wide = !p->mrg && !p->log && g->n_str > 512;
        if (!too_wide && plan_general_lds(g, b, kn, p)) break;
        if (p->log) return RQ_EUNSUPPORTED;
        p->log = true;
    }
    // stream ids past 16 bits are read (mrg_jh) by the GT instances only; such graphs'
    // tables never fit LDS, so they always get one
    if (p->mrg && g->n_str > 65535 && !p->gt) return RQ_EUNSUPPORTED;
    plan_fused_lds(g, b, kn, p);

    // pipelined chunks for the merged-stream sweeps (not the sequential LOG sweep, whose
    // global per-sink slots are sized for one grid): the batch in an even number of
    // chunks of <= 131072 replicas on two streams, so the two streams' generation, merge,
    // sweep and scan run side by side and one chunk's sweep tail is the other's work.
    // C3, 10k replicas (profiles/r04_pipe_ab.txt): one stream 3.02 ms per step; two
    // streams x 2 chunks of 5000 2.82 ms; 3 x 3334 3.36; 5 x 2000 4.15; 10 x 1000 5.98
    // (the sweep is latency-bound per replica: a chunk much below the resident wave
    // slots leaves them empty)
    p->nbuf = 1;
    p->order = false;
    if (p->mrg && !p->log) {
        const int nb = kn.pipe;   // 2 unless RQ_PIPE (A/B only)
        if (b->chunk <= 0) {
            // two chunks (one per stream) up to 2^17 replicas each: C4's 256k replicas of
            // the README graph 16 x 16000 -> 2 x 128000: 7.1 -> 9.2 M replicas/s (a
            // generator launch of 16000 x 3 streams is ~0.7 waves per SIMD)
            int64_t nch = (p->R + 131071) / 131072;
            if (nb > 1) nch = std::max<int64_t>(2, (nch + 1) & ~(int64_t)1);   // even: both streams busy
            if (kn.pipe_chunk.set)   // A/B only
                nch = (p->R + kn.pipe_chunk.v - 1) / kn.pipe_chunk.v;
            nch = std::max<int64_t>(1, std::min(nch, p->R));
            p->chunk = (p->R + nch - 1) / nch;
        }
        const int64_t nch = (p->R + p->chunk - 1) / p->chunk;
        p->nbuf = (int)std::min<int64_t>(nb, nch);
    }

    // the workspace within the device-memory budget (C5: ~20 MB per replica in flight):
    // with the library's chunking, smaller chunks (an even count when pipelined) until the
    // nbuf buffer sets in flight fit; a caller-fixed chunk is the caller's business
    plan_layout(g, b, p);
    if (b->chunk <= 0 && budget > 0.0) {
        while ((double)p->total > budget) {
            if (p->chunk <= 1) return RQ_ENOMEM;
            int64_t c = (int64_t)((double)p->chunk * budget / (double)p->total * 0.97);
            c = std::max<int64_t>(1, std::min<int64_t>(c, p->chunk - 1));
            int64_t nch = (p->R + c - 1) / c;
            if (p->nbuf > 1) nch = (nch + 1) & ~(int64_t)1;
            p->chunk = (p->R + nch - 1) / nch;
            plan_layout(g, b, p);
        }
    }

    // longest-first order (rq_order_replicas) of the replicas the sweep's work queue hands
    // out (a chunk larger than the resident wave slots): measured neutral on C3 (3.01 vs
    // 3.02 ms per step) and slower on C5 (8192 replicas in one chunk: sweep 424 ms against
    // 400 ms in index order, profiles/r04_c5_ab.txt) -- off unless RQ_ORDER=1 (A/B)
    if (kn.order) {
        p->order = p->mrg && !p->log && p->chunk > (int64_t)std::max(1, p->wpc) * rq_cu_count() &&
                   p->chunk <= 65536;   // rq_order_replicas sorts <= 65536 replicas per launch
        if (p->order) plan_layout(g, b, p);
    }
    return RQ_OK;
}

namespace {

void plan_layout(const GraphTopo* g, const rq_batch_desc* b, Plan* p)
{
    // the sequential sweep's global per-sink slots: no more than the chunk's replicas
    if (p->gs) p->gs_slots = std::min<int64_t>(p->gs_slots, (int64_t)align_up((size_t)p->chunk, (size_t)p->gwpb));
    const size_t A = 256;
    const int64_t C = p->chunk;
    size_t o = 0;
    p->off_invc = o;    o = o + sizeof(double) * (size_t)b->n_grid * g->n_str;
    p->off_stoff = o;   o = o + sizeof(int64_t) * g->n_str;
    p->off_cap = o;     o = o + sizeof(int) * g->n_str;
    p->off_rdk = o;     o = o + sizeof(int) * g->n_str;
    o = align_up(o, 8);
    p->off_repidx = o;  o = o + sizeof(int64_t) * (b->rep_idx ? (size_t)p->R : 0);
    const size_t nseg = b->ctrl_kind == RQ_SRC_OPTPW ? (size_t)b->n_seg : 0;
    o = align_up(o, 8);
    p->off_pwc = o;     o = o + sizeof(double) * (size_t)b->n_grid * g->n_str * nseg;
    p->off_pwmax = o;   o = o + sizeof(double) * (nseg ? (size_t)b->n_grid * g->n_str : 0);
    p->tables_bytes = o;
    o = align_up(o, A);
    // one buffer set per pipelined stream; offsets relative to the set's base
    p->off_set0 = o;
    const size_t o_set = o;
    o = 0;
    const int64_t strm = p->fw && !p->fwm ? 0 : C;   // the generating fused sweep keeps its arrivals in LDS
    const size_t strm_bytes = sizeof(double) * (size_t)strm * p->capsum;
    p->off_slen = o;    o = align_up(o + sizeof(int) * (size_t)strm * g->n_str, A);
    // two-level merge: per (replica, group) the first level's sequences
    p->sub_stride = 0;
    if (p->mrg && p->n_grp > 1)
        for (int gq = 0; gq < p->n_grp; ++gq) {
            int64_t c = 0;
            for (int j = gq * p->grp_sz; j < std::min(g->n_str, (gq + 1) * p->grp_sz); ++j) c += p->cap[j];
            p->sub_stride = std::max(p->sub_stride, (c + 15) & ~(int64_t)15);
        }
    const int64_t subc = p->sub_stride > 0 ? C * p->n_grp : 0;
    p->off_sub_t = o;   o = align_up(o + sizeof(double) * (size_t)subc * p->sub_stride, A);
    p->off_sub_j = o;   o = align_up(o + sizeof(uint16_t) * (size_t)subc * p->sub_stride, A);
    p->off_sub_len = o; o = align_up(o + sizeof(int) * (size_t)subc, A);
    const int64_t mrgc = p->mrg ? C : 0;   // merged sequences: t f64, stream u16, length
    p->off_mt = o;      o = align_up(o + sizeof(double) * (size_t)mrgc * p->mrg_stride, A);
    p->off_mj = o;      o = align_up(o + sizeof(uint16_t) * (size_t)mrgc * p->mrg_stride, A);
    // > 65535 streams: each entry's stream bits 16-23
    p->off_mjh = o;     o = align_up(o + (g->n_str > 65535 ? (size_t)mrgc * p->mrg_stride : 0), A);
    p->off_mlen = o;    o = align_up(o + sizeof(int) * (size_t)mrgc, A);
    p->off_ord = o;     o = align_up(o + sizeof(int) * (size_t)(p->order ? C : 0), A);
    const size_t o_rows = o;
    p->off_rt = o;      o = align_up(o + sizeof(double) * (size_t)C * p->cap_rows, A);
    p->off_rs = o;      o = align_up(o + sizeof(double) * (size_t)C * p->cap_rows, A);
    p->off_rv = o;      o = align_up(o + sizeof(uint32_t) * (size_t)C * p->cap_rows, A);
    p->off_rc = o;      o = align_up(o + sizeof(uint32_t) * (size_t)C * p->cap_rows * p->nK, A);
    // the per-source streams are dead once merged (rq_merge_streams runs before the sweep
    // writes its first row, in the same stream's order): they share the pivot rows' bytes
    if (p->mrg && strm_bytes <= o - o_rows) {
        p->off_streams = o_rows;
    } else {
        p->off_streams = o;
        o = align_up(o + strm_bytes, A);
    }
    p->off_sall = o;    o = align_up(o + sizeof(int) * (size_t)C, A);
    p->off_wq = o;      o = align_up(o + 2 * sizeof(int), A);   // [0] sweep, [1] scan queue
    p->set_stride = o;
    o = o_set + (size_t)p->nbuf * p->set_stride;
    // LOG + gs: per resident wave, rank int + gtag/gcnt/gsum int per sink
    p->gs_stride = p->gs ? (int64_t)align_up(16 * (size_t)p->n_sinks_pad, A) : 0;
    p->off_gs = o;      o = align_up(o + (size_t)(p->gs ? p->gs_slots : 0) * p->gs_stride, A);
    p->total = o;
}

}  // namespace

}  // namespace rqh
